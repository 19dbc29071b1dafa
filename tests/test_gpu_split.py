"""The three-pass narrow sort (csrc/radix_split.hpp) at its sub-bucket, bin, tie, staging-row and tile edges (cases and model:
tests/split_cases.py).  Every fallback of this plan repairs the array -- a staging row that overflows repeats the flags work
as its own pass, a sub-bucket over the cap moves the sort to the large form or to the LSD passes, a tied pair that is never
staged stays in (key, suffix) order -- so every build is compared four ways: the array with the oracle (and verify()), the
queries with the oracle (they go through the directory the local pass writes, the entries of empty sub-buckets and the end
marker included), BuildStats' plan fields with the model (split_plan, split_max, lite_flags, radix_passes and the records and bytes they count), and its
refinement counts with refine_cases.simulate on the tied groups read off the oracle's array, exactly: a tied slot that is
not staged, or staged with the wrong head bit, changes tiny_resolved / finisher_* / rounds / active_total.

Forms per case: default (persistent local pass), SA_HIP_LOCAL_PERSIST=0 (one workgroup per sub-bucket), SA_HIP_LOCAL_GRID=1
(one workgroup walks every sub-bucket) and SA_HIP_SPLIT_FLAGS=0 (the flags work as a pass of its own).  A fresh DeviceIndex
per form: the switches are read at init.  Mismatches are collected per test function and reported together."""
import itertools

import numpy as np
import pytest

import refine_cases as rc
import split_cases as sc

pytestmark = pytest.mark.gpu

SWITCHES = ("SA_HIP_SPLIT", "SA_HIP_INITIAL_CHARS", "SA_HIP_LOCAL_PERSIST", "SA_HIP_LOCAL_GRID", "SA_HIP_SPLIT_FLAGS", "SA_HIP_LOCAL_BIG",
            "SA_HIP_LOCAL_BINS", "SA_HIP_SPLIT_ITEMS", "SA_HIP_DIR_BITS", "SA_HIP_SPLIT_CAP", "SA_HIP_LITE_FLAGS",
            "SA_HIP_TINY", "SA_HIP_GROUP_FINISH", "SA_HIP_PERIOD_FINISH")
COUNTS = ("tiny_resolved", "finisher_runs", "finisher_records", "finisher_resolved", "period_resolved")
_memo = {}


@pytest.fixture(autouse=True)
def _drop_memo():
    """text, expected array, groups and patterns are shared by the cases and forms inside one test function only"""
    yield
    _memo.clear()


def patterns(T, sa, m):
    """every string of 1, 2 and 3 symbols over the text's alphabet, the planted words cut at every length, the keys of tied slots"""
    A = T.A.tolist()
    pats = [bytes(p) for r in (1, 2, 3) for p in itertools.product(A, repeat=r)]
    for w in T.words:
        pats += [bytes(T.t[w:w + j]) for j in range(1, T.k + 2)]
    pats += [bytes(T.t[-j:]) for j in range(1, T.k + 1)]                       # what ends the text
    if m.get("tied") is not None:
        slots = m["tied"][m["head"]]
        if m.get("rb") and T.words:
            lo = int(m["sub_starts"][sc.sub_of(m, T.words[0])])
            mine = slots[(slots >= lo) & (slots < lo + 1200)]
            slots = np.concatenate([mine[:300], slots[:100]])
        pats += [bytes(T.t[p:p + T.k]) for p in sa[slots[:400]]]
    return pats


def prepared(oracle, text):
    if text not in _memo:
        T = sc.make(text)
        sa = oracle.sais(T.t).astype(np.int64)
        g = rc.groups_after_keys(T.t, sa, T.k)
        sim = rc.simulate(g, int(T.t.size), T.k, 5, t=T.t, sa=sa)
        _memo[text] = (T, sa, g, sim)
    return _memo[text]


def run_case(gpu, oracle, monkeypatch, name, errors):
    case = sc.CASES[name]
    T, want, g, sim = prepared(oracle, case.text)
    mkey = ("m", case.text, tuple(sorted(case.env.items())))
    if mkey not in _memo:
        m = sc.measure(T.t, T.k, case.env)
        pats = patterns(T, want, m)
        _memo[mkey] = (m, pats, oracle.query_batch(T.t, want.astype(np.uint32), 0xFFFFFFFF, pats))
    m, pats, exp_q = _memo[mkey]
    c = case.claim
    taken = c["form"] is not None
    forms = sc.FORMS if taken else sc.FORMS[:1]
    for fi, (tag, fenv) in enumerate(forms):
        env = dict(case.env, SA_HIP_SPLIT="1", SA_HIP_INITIAL_CHARS=str(T.k), **fenv)
        wide = fi == (sum(map(ord, name)) % len(forms))        # one form per case, not always the same one
        who = "%s%s" % (name, tag)

        def err(msg, *a):
            errors.append("%s: %s" % (who, msg % a))
        t = T.t
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with gpu.DeviceIndex(t.size, 0) as idx:
            idx.build(t)
            if wide:
                import torch
                out = torch.full((t.size + 2,), -7, dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                idx.build_device64(idx.text_dev, t.size, out.data_ptr(), 0)
                idx.sync()
            st = idx.build_stats()
            bad = idx.verify()
            sa = idx.sa_u32().astype(np.int64)
            got_q = idx.query_batch(pats)
            if wide:
                got = out.cpu().numpy()
                if not np.array_equal(got[:t.size], sa):
                    err("int64 copy differs from the array, first at slot %d", int(np.flatnonzero(got[:t.size] != sa)[0]))
                if not (got[t.size:] == -7).all():
                    err("guard words behind the int64 copy written: %s", got[t.size:].tolist())
                if taken and st["widen_fused"] != 1:
                    err("widen_fused = %d with the plan taken", st["widen_fused"])
        print(who, {x: st[x] for x in ("split_plan", "split_max", "lite_flags", "narrow_k", "radix_passes", "rounds", "active_total") + COUNTS})
        # 1. the array
        if bad != 0:
            err("verify() = %d", bad)
        if not np.array_equal(sa, want):
            slot = int(np.flatnonzero(sa != want)[0])
            sub = int(np.searchsorted(m["sub_starts"], slot, side="right") - 1) if m.get("rb") else -1
            err("array differs from the oracle, first at slot %d (sub-bucket %d, its slot %d)", slot, sub,
                slot - int(m["sub_starts"][sub]) if sub >= 0 else -1)
        # 3. the queries
        if not np.array_equal(got_q, exp_q):
            i = int(np.flatnonzero(got_q != exp_q)[0])
            err("query %r: %s, oracle %s (%d of %d differ)", pats[i], got_q[i], exp_q[i], int((got_q != exp_q).sum()), len(pats))
        # 4. the plan: the claim for the default form; the model, which the CPU test holds against the claims, for the others
        lite = c["lite"] if not fenv.get("SA_HIP_SPLIT_FLAGS") else m["lite_unfused"]
        expect = dict(split_plan=c["plan"], split_max=c["split_max"], lite_flags=lite, narrow_k=c.get("narrow_k", 1), initial_chars=T.k,
                      bits_per_symbol=5)
        if taken:
            # top digit from the text 9 bytes per record, split pass 16, local pass 16 (24 when it stores the int64 array too:
            # the wide form's stats are those of the 64-bit build)
            expect.update(radix_passes=3, radix_records=3 * t.size, radix_bytes=(49 if wide else 41) * t.size)
        if (m["plan"], m["split_max"], m["lite"]) != (c["plan"], c["split_max"], c["lite"]):
            err("model and claim disagree: %s", (m["plan"], m["split_max"], m["lite"]))
        for x, v in expect.items():
            if st[x] != v:
                err("%s = %s, expected %s", x, st[x], v)
        # 5. the staged slots, through the refinement counts (refine_cases.simulate; test_gpu_refine.check's rule)
        for x in COUNTS:
            if st[x] != sim[x]:
                err("%s = %d, model %d", x, st[x], sim[x])
        if sim["exact"]:
            for x in ("rounds", "chunk_rounds", "active_total"):
                if st[x] != sim[x]:
                    err("%s = %d, model %d", x, st[x], sim[x])
            if st["doubling_rounds"] != 0:
                err("doubling_rounds = %d", st["doubling_rounds"])
        elif not (st["doubling_rounds"] > 0 and st["chunk_rounds"] == sim["chunk_rounds"] and st["rounds"] > sim["rounds"]
                  and st["active_total"] >= sim["active_total"] + sim["handover"] > sim["active_total"]):
            err("rounds %s against the model's lower bounds %s", {x: st[x] for x in ("rounds", "chunk_rounds", "doubling_rounds", "active_total")},
                {x: sim[x] for x in ("rounds", "chunk_rounds", "active_total", "handover")})
    return g, sim


def run_family(gpu, oracle, monkeypatch, names):
    errors = []
    out = [run_case(gpu, oracle, monkeypatch, n, errors) for n in names]
    assert not errors, "%d mismatches:\n%s" % (len(errors), "\n".join(errors[:40]))
    return out


def _by_text(family):
    groups = {}
    for n in sc.FAMILIES[family]:
        groups.setdefault(sc.CASES[n].text, []).append(n)
    return [pytest.param(v, id=k) for k, v in groups.items()]


@pytest.mark.parametrize("names", _by_text("caps"))
def test_sub_bucket_against_the_caps(gpu, oracle, monkeypatch, names):
    """8191 / 8192 records: the small form; 8193 / 16384: the large one; 16385: declined, the LSD passes sort"""
    run_family(gpu, oracle, monkeypatch, names)


@pytest.mark.parametrize("names", _by_text("sizes"))
def test_sub_bucket_against_the_item_loop(gpu, oracle, monkeypatch, names):
    """1, 2, 511, 512, 513, 1023, 1024, 1025 records between empty sub-buckets, 512 threads and (SA_HIP_LOCAL_BIG=1) 1024"""
    run_family(gpu, oracle, monkeypatch, names)


@pytest.mark.parametrize("names", _by_text("bins"))
def test_bins(gpu, oracle, monkeypatch, names):
    """a full sub-bucket in one even / odd bin; bin 0, bins of two and three, an odd last bin that ends the sub-bucket; 12 and
    11 bin bits"""
    run_family(gpu, oracle, monkeypatch, names)


@pytest.mark.parametrize("names", _by_text("ties"))
def test_tied_slots(gpu, oracle, monkeypatch, names):
    """pairs at the row edge, next to it, at the item edge, at slot 0 and at slot m - 1; a run over a row edge; adjacent groups"""
    for g, sim in run_family(gpu, oracle, monkeypatch, names):
        assert g.M >= 5 and sim["tiny_resolved"] > 0


@pytest.mark.parametrize("names", _by_text("staging"))
def test_staging_row(gpu, oracle, monkeypatch, names):
    """256 staged entries in one row: lite_flags == 2; 257: the overflow path, lite_flags == 0 -- in the table's first and last
    non-empty sub-bucket"""
    run_family(gpu, oracle, monkeypatch, names)


@pytest.mark.parametrize("names", _by_text("tiles"))
def test_split_pass_tiles(gpu, oracle, monkeypatch, names):
    """buckets of T - 1, T, T + 1, 2 T and 1 records at T = 512 x 24 / 28 / 32"""
    run_family(gpu, oracle, monkeypatch, names)


@pytest.mark.parametrize("names", _by_text("length"))
def test_text_length_against_the_top_digit_pass(gpu, oracle, monkeypatch, names):
    """n = 2^22 - 1 (no narrow-record sort), 2^22, 2^22 + 1, 2^22 + 8191; a planted word ends the text"""
    run_family(gpu, oracle, monkeypatch, names)


def test_directory_slice(gpu, oracle, monkeypatch):
    """one directory entry per sub-bucket, one per bin, and one bit more: the fused flags work is declined (lite_flags == 1)"""
    run_family(gpu, oracle, monkeypatch, sc.FAMILIES["directory"])


@pytest.mark.parametrize("names", _by_text("short_key"))
def test_key_of_seven_symbols(gpu, oracle, monkeypatch, names):
    """SA_HIP_INITIAL_CHARS=7: 27 narrow bits, 15 below the bins"""
    run_family(gpu, oracle, monkeypatch, names)
