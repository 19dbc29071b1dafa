"""The two device arrays every byte-pattern query starts from -- K, the sorted packed keys, and dir, the bucket directory
(csrc/sa_query.hpp: query_one searches only [dir[bl], dir[bl + 1])) -- read back through replica_layout / replica_buffers and
compared with the NumPy model of tests/query_struct_cases.py, every slot and every entry, exactly.  A wrong directory entry
neither faults nor touches the suffix array: it narrows the search of the patterns of one bucket, and the other tests ask a
few thousand patterns of 2^17 .. 2^20 entries.

Five code paths write the arrays (query_struct_cases.WRITERS); every (text, form) is a fresh DeviceIndex -- the switches are
read at init -- and is judged five ways: verify() and the array against the oracle; the layout against what the form implies;
K against the model; dir against the model, the first bad entry reported with the run of the owner decomposition that holds it
(owner slot, span, inline / queued / piece i of m); queries tied to the structure (every 1- and 2-symbol string, the prefixes
on both sides of the longest and of the planted runs, cases.edge_patterns) against the oracle under SA_HIP_SECTOR_SEARCH 2 and
0.  The writer is read off BuildStats and the form and noted in COVER; the last test asserts that every writer ran with the
directory forced to 14 and to 21 bits on the crafted text, on every planted span, and that the local pass of the three-pass plan
met empty sub-buckets inside the planted runs.  Text, arrays and models are shared by the forms of one test."""
import time

import numpy as np
import pytest

import query_struct_cases as qs

pytestmark = pytest.mark.gpu

COVER = {}      # (writer, forced dbits or None) -> runs
REACHED = {}    # (writer, what) -> runs; what: a planted span, "pieces>=3", "leading>1", "empty_subs"
_memo = {}


def _text(name, n):
    if _memo.get("text") != (name, n):
        _memo.clear()
        _memo["text"] = (name, n)
        _memo["t"] = qs.make(name, n)
    return _memo["t"]


def _cached(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _read(ptr, nbytes, dtype):
    import torch
    from suffixarray_amd.distributed import device_view
    return device_view(ptr, nbytes, torch.uint8, torch.device("cuda", 0)).cpu().numpy().view(dtype)


def _open(gpu, monkeypatch, t, sa, form, sector):
    for k in qs.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in form.env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SA_HIP_SECTOR_SEARCH", str(sector))
    idx = gpu.DeviceIndex(t.size, 0)
    if form.adopted:
        idx.load(t, sa, form.L)
    else:
        idx.build(t, form.L)
    return idx


def run_form(gpu, oracle, monkeypatch, case, form, errors):
    who = "%s/%s" % (case.id, form.tag)

    def err(msg, *a):
        errors.append("%s: %s" % (who, msg % a))
    t0 = time.time()
    t = _text(case.text, case.n)
    n, L, env = int(t.size), form.L, form.env
    want_sa = _cached(("sa", L), lambda: (oracle.sais(t) if L == 0 else oracle.truncated_sa(t, L)).astype(np.uint32))
    code, sigma, b = _cached("code", lambda: qs.code_map(t))
    idx = _open(gpu, monkeypatch, t, want_sa, form, 2)
    try:
        st = idx.build_stats() if not form.adopted else {}
        # 1. the array
        bad = idx.verify()
        if bad != 0:
            err("verify() = %d", bad)
        sa = idx.sa_u32()
        if not np.array_equal(sa, want_sa):
            err("array differs from the oracle, first at slot %d", int(np.flatnonzero(sa != want_sa)[0]))
        # 2. the layout
        lay = idx.replica_layout()
        buf = idx.replica_buffers()
        k0, dbits, kb = int(lay.initial_chars), int(lay.dir_bits), int(lay.key_bytes)
        forced_d = int(env["SA_HIP_DIR_BITS"]) if "SA_HIP_DIR_BITS" in env else None
        cap = qs.kmax(b, n, env.get("SA_HIP_NARROW48") != "0")
        if "SA_HIP_INITIAL_CHARS" in env:
            want_k0 = min(int(env["SA_HIP_INITIAL_CHARS"]), cap, L if L else 64)
        else:
            want_k0 = st["initial_chars"] if st else k0
            if not 1 <= k0 <= min(cap, L if L else 64):
                err("initial_chars = %d beyond %d", k0, min(cap, L if L else 64))
        expect = dict(n=n, max_suffix_length=L, bits_per_symbol=b, initial_chars=want_k0, dir_bits=forced_d if forced_d else qs.default_dir_bits(n),
                      key_bytes=qs.expected_key_bytes(b, k0, n, env, form.adopted), dir_entries=(1 << dbits) + 1)
        if kb == 4:
            expect["lo_shift"] = 64 - b * k0
        for x, v in expect.items():
            if int(getattr(lay, x)) != v:
                err("layout.%s = %d, expected %d", x, int(getattr(lay, x)), v)
        if list(lay.code) != code.tolist():
            err("layout.code differs from the code map of the text")
        if st and (st["bits_per_symbol"], st["sigma"]) != (b, sigma):
            err("stats: b = %d, sigma = %d", st["bits_per_symbol"], st["sigma"])
        if (int(buf.keys_bytes), int(buf.dir_bytes)) != (n * kb, ((1 << dbits) + 1) * 4) or kb not in (4, 8) or not buf.keys or not buf.dir:
            err("buffers: %d key bytes, %d directory bytes, key_bytes = %d", buf.keys_bytes, buf.dir_bytes, kb)
            return
        partial = bool(st) and qs.partial_applies(b, k0, L, st["narrow48"])
        # 3. K, every slot (the model is made over the oracle's array)
        got_k = _read(buf.keys, n * kb, np.uint64 if kb == 8 else np.uint32)
        got_d = _read(buf.dir, ((1 << dbits) + 1) * 4, np.uint32)
        kkey = ("K", L, k0, kb, int(lay.lo_shift) if kb == 4 else 0, partial)
        want_k, dkeys = _cached(kkey, lambda: qs.stored_keys(t, want_sa, code, b, k0, kb, int(lay.lo_shift), partial))
        if not np.array_equal(got_k, want_k):
            d = np.flatnonzero(got_k != want_k)
            j = int(d[0])
            err("K[%d] = %#x, model %#x (suffix %d; %d of %d slots differ)", j, int(got_k[j]), int(want_k[j]), int(want_sa[j]), d.size, n)
        # 4. dir, every entry
        want_d, own = _cached(("dir", kkey, dbits), lambda: (qs.directory(dkeys, dbits), qs.owners(dkeys, dbits)))
        why = qs.dir_mismatch(got_d, want_d, own)
        if why:
            err("%s", why)
        # 5. who wrote it, and what it met
        w = qs.writer_of(st, env, form.adopted)
        tag = "%s [%s]" % (who, "" if not st else "plan %d lite %d" % (st["split_plan"], st["lite_flags"]))
        COVER.setdefault((w, forced_d), []).append(tag)
        spans = _cached(("spans", kkey, dbits), lambda: set(own.span.tolist()))
        if case.text == "markov" and forced_d in qs.PLANTED_SPANS:
            for s in qs.PLANTED_SPANS[forced_d]:
                if s in spans:
                    REACHED.setdefault((w, s), []).append(tag)
            if own.pieces.max() >= 3:
                REACHED.setdefault((w, "pieces>=3"), []).append(tag)
            if own.span[0] > 1:
                REACHED.setdefault((w, "leading>1"), []).append(tag)
            if w == 4:   # sub-buckets of the local pass (the top 8 + split_plan key bits) that the planted symbol X leaves empty
                rb = st["split_plan"]
                subs = np.unique(dkeys >> np.uint64(56 - rb)).astype(np.int64)
                lo, hi = qs.X << (1 + rb), (qs.X + 1) << (1 + rb)
                empty = (hi - lo) - int(((subs >= lo) & (subs < hi)).sum())
                if empty > 0 and int(((subs >= lo) & (subs < hi)).sum()) > 0:
                    REACHED.setdefault((w, "empty_subs", forced_d), []).append("%s: %d of %d" % (tag, empty, hi - lo))
        # 6. queries tied to the structure
        pats, exp_q = _cached(("q", kkey, dbits), lambda: _patterns(oracle, t, want_sa, dkeys, dbits, b, k0, L))
        _ask(idx, pats, exp_q, err, 2)
    finally:
        idx.close()
    idx = _open(gpu, monkeypatch, t, want_sa, form, 0)
    try:
        _ask(idx, pats, exp_q, err, 0)
    finally:
        idx.close()
    print("%-44s writer %s  k0 %d  %d-byte keys  dbits %d  %d patterns  %.2f s  %s" % (
        who, w, k0, kb, dbits, len(pats), time.time() - t0,
        {x: st[x] for x in ("split_plan", "lite_flags", "narrow_k", "narrow48", "text_top_pass")} if st else "adopted"))


def _patterns(oracle, t, sa, dkeys, dbits, b, k0, L):
    rng = np.random.default_rng(dbits * 100 + k0)
    pats = qs.structure_patterns(t, dkeys, dbits, b, rng, k0, L)
    return pats, oracle.query_batch(t, sa, L if L else 0xFFFFFFFF, pats)


def _ask(idx, pats, exp_q, err, sector):
    got_q = idx.query_batch(pats)
    if not np.array_equal(got_q, exp_q):
        d = np.flatnonzero(got_q != exp_q)
        i = int(d[0])
        err("SA_HIP_SECTOR_SEARCH=%d: query %r: %s, oracle %s (%d of %d differ)", sector, pats[i][:40], got_q[i], exp_q[i], d.size, len(pats))


@pytest.mark.parametrize("cid", [c.id for c in qs.CASES])
def test_key_array_and_directory(gpu, oracle, monkeypatch, cid):
    """K and dir of every form of the case, slot by slot and entry by entry, against the model"""
    case = qs.CASE_BY_ID[cid]
    errors = []
    for form in case.forms:
        run_form(gpu, oracle, monkeypatch, case, form, errors)
    assert not errors, "%d mismatches:\n%s" % (len(errors), "\n".join(errors[:40]))


def test_writer_coverage_matrix():
    """After the cases above: each of the five writers ran with the directory forced to 14 and to 21 bits, on runs of exactly 40,
    41, 16384 and 16385 buckets, on a run of three pieces and more and a leading run; the local pass filled entries of empty
    sub-buckets inside the planted runs at both widths -- a change of a plan predicate cannot quietly empty a cell."""
    for key in sorted(COVER, key=str):
        print("writer %s, dbits %s: %s" % (key[0], key[1], "; ".join(COVER[key][:4])))
    for key in sorted(REACHED, key=str):
        print("reached %s: %s" % (key, "; ".join(REACHED[key][:2])))
    assert COVER, "run the whole module: the table is filled by test_key_array_and_directory"
    missing = [(w, d) for w in qs.WRITERS for d in (14, 21) if (w, d) not in COVER]
    missing += [(w, s) for w in qs.WRITERS for d, ss in qs.PLANTED_SPANS.items() for s in ss if (w, s) not in REACHED]
    missing += [(w, x) for w in qs.WRITERS for x in ("pieces>=3", "leading>1") if (w, x) not in REACHED]
    missing += [(4, "empty_subs", d) for d in (14, 21) if (4, "empty_subs", d) not in REACHED]
    assert not missing, missing
    assert any(w is not None and d is None for w, d in COVER)          # ... and at the default width
