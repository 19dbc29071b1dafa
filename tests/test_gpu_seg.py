"""The bucketed LSD sorts -- csrc/radix_narrow.hpp (8-byte records) and csrc/radix_narrow48.hpp (10-byte records), with the
stable top-digit pass in front of them -- at their bucket, tile and part edges (cases and model: tests/seg_cases.py; what every
case contains is asserted by tests/test_seg_cases_cpu.py).

Every (case, form, key length) is built twice, each time on a fresh DeviceIndex with the form's switches (they are read at
init):

  max_suffix_length = k0   The sort's output with nothing behind it.  Builder::build keeps the key length (choose_initial_chars
                           only shortens a key LONGER than L) and the plan (narrow_sort_applies / narrow48_applies look at n and
                           the key's bits), and with h = k0 = L no refinement round runs: the suffix array is what the last
                           pass stored.  The project keeps ties in text order, so the array must equal one stable argsort of the
                           keys (seg_cases.lsd_model) slot by slot, and oracle.truncated_sa.  One thing does change with L = k0:
                           the 10-byte plan takes no partial character (b = 5, k0 = 11: 55-bit keys, a last digit of 7 bits,
                           where the full build sorts the first 56 bits of 12 symbols); seg_cases.passes(b, k0, L) models both.
  max_suffix_length = 0    The full build: verify(), the array against oracle.sais, and the two arrays the sort leaves for the
                           queries -- K (u32 narrow keys, u64 keys rebuilt from the bucket, or the 56-bit form of the 10-byte
                           plan) read back through replica_buffers and compared with query_struct_cases.stored_keys slot by
                           slot, dir with query_struct_cases.directory entry by entry.

BuildStats must show that the path under test ran: narrow48, narrow_k, text_top_pass, split_plan == 0, one launch of the
top-digit pass (two on the declined path: claim form, then stable form), and as many launches of the LSD pass kernels as
seg_cases.passes() lists; for the L = k0 build, where the sort is all that counts, also the passes, records and algorithmic
bytes, total and per kind, that the host drivers add up (_accounting).  One run per plan also asks for the int64 array (build_device64) and expects it from the sort's last
store (widen_fused).  All comparisons are exact; a mismatch names the first bad slot, its bucket, its flat tile and whether
that tile is full or partial.  Text, oracle arrays and models are shared by the runs of one case."""
import time

import numpy as np
import pytest

import query_struct_cases as qs
import seg_cases as sg
from pipeline_model import split_levels

pytestmark = pytest.mark.gpu

_memo = {}


def _case_memo(name):
    if _memo.get("case") != name:
        _memo.clear()
        _memo["case"] = name
    return _memo


def _cached(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _read(ptr, nbytes, dtype):
    import torch
    from suffixarray_amd.distributed import device_view
    return device_view(ptr, nbytes, torch.uint8, torch.device("cuda", 0)).cpu().numpy().view(dtype)


def _accounting(st, T, form, k0, spec, err):
    """The L = k0 build runs one sort and nothing else that counts: passes, records and algorithmic bytes per pass kind
    (EventTimer's kinds: 0 12-byte passes, 1 top digit, 2 LSD passes but the last, 3 the last) as the host drivers count them,
    in units of n.  Every counted pass moves n records."""
    plan_, _, expect = sg.FORMS[form]
    n = int(T.t.size)
    if plan_ == 12:      # pass 0 reads the text (13 bytes per record), every other pass 8 + 4 bytes in and out
        np12 = -(-T.b * k0 // 8)
        per_kind = [13 + 24 * (np12 - 1), 0, 0, 0]
        count = np12
    else:
        mid = len(spec["passes"]) - 1
        if plan_ == 10:  # the top-digit pass writes k16 too; the last pass rebuilds the u64 keys
            per_kind = [0, 11, 20 * mid, 22]
        else:            # from the text 9 bytes per record (twice on the declined path), from a u64 key array 16
            top = 9 * expect["top"] if expect["text_top_pass"] else 16
            per_kind = [0, top, 16 * mid, 16 if expect["narrow_k"] else 20]
        count = expect["top"] + mid + 1
    want = dict(radix_passes=count, radix_records=count * n, radix_bytes=sum(per_kind) * n, pass_bytes=[x * n for x in per_kind])
    for x, v in want.items():
        got = list(st[x]) if isinstance(v, list) else st[x]
        if got != v:
            err("L=%d: %s = %s, the drivers' model counts %s (n = %d)", k0, x, st[x], v, n)


def _stats(st, T, form, k0, spec, err, L):
    plan_, env, expect = sg.FORMS[form]
    want = dict(initial_chars=k0, bits_per_symbol=T.b, sigma=T.sigma, narrow48=expect["narrow48"], narrow_k=expect["narrow_k"],
                text_top_pass=expect["text_top_pass"], split_plan=0)
    for x, v in want.items():
        if st[x] != v:
            err("L=%d: %s = %s, expected %s", L, x, st[x], v)
    launches = st["pass_launches"]
    if L == k0:
        _accounting(st, T, form, k0, spec, err)
    if plan_ == 12:
        if launches[0] == 0 or launches[1:] != [0, 0, 0]:
            err("L=%d: the 12-byte control launched %s", L, launches)
        return
    if launches[2] + launches[3] != len(spec["passes"]) or launches[3] != 1:
        err("L=%d: %d + %d launches of the LSD pass kernels, the model has %d passes", L, launches[2], launches[3], len(spec["passes"]))
    if launches[1] != expect["top"]:
        err("L=%d: %d launches of the top-digit pass, expected %d", L, launches[1], expect["top"])


def run(gpu, oracle, monkeypatch, name, form, errors):
    case = sg.CASES[name]
    _case_memo(name)
    T = _cached("text", lambda: sg.make(case.text))
    t, n = T.t, int(T.t.size)
    plan_, fenv, expect = sg.FORMS[form]
    tile = sg.tile_of(plan_)
    code = _cached("code", lambda: qs.code_map(t)[0])
    want_full = _cached("sais", lambda: oracle.sais(t).astype(np.uint32))
    for k0 in dict(case.runs)[form]:
        who = "%s/%s/k0=%d" % (name, form, k0)
        t0 = time.time()

        def err(msg, *a):
            errors.append("%s: %s" % (who, msg % a))
        env = dict(fenv, SA_HIP_INITIAL_CHARS=str(k0))
        for k in sg.SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pl = _cached(("plan", tile, k0), lambda: sg.plan(np.bincount(sg.top_digit(t, T.b, k0), minlength=256), tile))

        # 1. the sort's output with nothing behind it: L = k0
        spec = sg.spec_of(T, form, k0, k0)
        keys = _cached(("keys", spec["chars"], spec["bits"]), lambda: sg.sort_keys(t, spec))
        want = _cached(("lsd", spec["chars"], spec["bits"]), lambda: sg.lsd_model(keys).astype(np.uint32))
        want_tr = _cached(("trunc", k0), lambda: oracle.truncated_sa(t, k0))
        with gpu.DeviceIndex(n, 0) as idx:
            idx.build(t, k0)
            st = idx.build_stats()
            bad = idx.verify()
            sa = idx.sa_u32()
        _stats(st, T, form, k0, spec, err, k0)
        if bad != 0:
            err("L=%d: verify() = %d", k0, bad)
        why = sg.mismatch(sa, want, pl, tile)
        if why:
            err("L=%d: the array is not the stable sort of the keys: %s", k0, why)
        why = sg.mismatch(sa, want_tr, pl, tile)
        if why:
            err("L=%d: the array differs from oracle.truncated_sa: %s", k0, why)
        if form == "declined":
            levels = _cached("levels", lambda: split_levels(keys, spec["lo_bits"], 10))
            if st["split_max"] != levels[10] or levels[10] <= 16384:
                err("split_max = %d, the model's largest group at the finest level is %d", st["split_max"], levels[10])
        elif st["split_max"] != 0:
            err("split_max = %d: the three-pass plan was considered", st["split_max"])

        # 2. the full build
        spec0 = sg.spec_of(T, form, k0, 0)
        wide = case.sa64 == (form, k0)
        with gpu.DeviceIndex(n, 0) as idx:
            idx.build(t)
            if wide:
                import torch
                out = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                idx.build_device64(idx.text_dev, n, out.data_ptr(), 0)
                idx.sync()
            st0 = idx.build_stats()
            bad = idx.verify()
            sa = idx.sa_u32()
            lay = idx.replica_layout()
            buf = idx.replica_buffers()
            dbits, kb = int(lay.dir_bits), int(lay.key_bytes)
            got_k = got_d = None
            if kb in (4, 8) and buf.keys and buf.dir and int(buf.keys_bytes) == n * kb and int(buf.dir_bytes) == ((1 << dbits) + 1) * 4:
                got_k = _read(buf.keys, n * kb, np.uint64 if kb == 8 else np.uint32)
                got_d = _read(buf.dir, ((1 << dbits) + 1) * 4, np.uint32)
            if wide:
                got64 = out.cpu().numpy()
        _stats(st0, T, form, k0, spec0, err, 0)
        if bad != 0:
            err("L=0: verify() = %d", bad)
        why = sg.mismatch(sa, want_full, pl, tile)
        if why:
            err("L=0: the array differs from oracle.sais: %s", why)
        if wide:
            if st0["widen_fused"] != 1:
                err("widen_fused = %d", st0["widen_fused"])
            why = sg.mismatch(got64[:n], sa.astype(np.int64), pl, tile)
            if why:
                err("the int64 array differs from the u32 one: %s", why)
            if not (got64[n:] == -7).all():
                err("guard words behind the int64 array written: %s", got64[n:].tolist())
        # K and dir
        want_kb = qs.expected_key_bytes(T.b, k0, n, env, False)
        if got_k is None or kb != want_kb or int(lay.initial_chars) != k0 or dbits != qs.default_dir_bits(n):
            err("layout: key_bytes %d (expected %d), initial_chars %d, dir_bits %d, %d key bytes, %d directory bytes", kb, want_kb,
                int(lay.initial_chars), dbits, int(buf.keys_bytes), int(buf.dir_bytes))
        else:
            partial = qs.partial_applies(T.b, k0, 0, st0["narrow48"])
            if partial != (spec0["chars"] == k0 + 1):
                err("partial character: query_struct_cases says %s, seg_cases.passes %d characters", partial, spec0["chars"])
            lo_shift = int(lay.lo_shift) if kb == 4 else 0
            if kb == 4 and lo_shift != 64 - T.b * k0:
                err("layout.lo_shift = %d", lo_shift)
            want_k, dkeys = _cached(("K", k0, kb, lo_shift, partial), lambda: qs.stored_keys(t, want_full, code, T.b, k0, kb, lo_shift, partial))
            why = sg.mismatch(got_k, want_k, pl, tile)
            if why:
                err("K (%d-byte keys%s): %s", kb, ", 56-bit form" if partial else "", why)
            want_d = _cached(("dir", k0, partial, dbits), lambda: qs.directory(dkeys, dbits))
            if not np.array_equal(got_d, want_d):
                d = np.flatnonzero(got_d != want_d)
                j = int(d[0])
                err("dir[%d] = %d, model %d (%d of %d entries differ; top digit %d)", j, int(got_d[j]), int(want_d[j]), d.size, want_d.size, j >> (dbits - 8))
        print("%-40s %d passes  L=k0 %s  L=0 %s  %d-byte keys  %.2f s" % (
            who, len(spec["passes"]), st["pass_launches"], st0["pass_launches"], kb, time.time() - t0))


RUNS = [pytest.param(name, form, id="%s-%s" % (name, form)) for name, case in sg.CASES.items() for form, _ in case.runs]


@pytest.mark.parametrize("name,form", RUNS)
def test_bucketed_lsd_sort(gpu, oracle, monkeypatch, name, form):
    """every key length of the (case, form): the truncated build against the stable sort of the keys, the full build against
    the oracle, K and dir against the model, BuildStats against the path the form is there to reach"""
    errors = []
    run(gpu, oracle, monkeypatch, name, form, errors)
    assert not errors, "%d mismatches:\n%s" % (len(errors), "\n".join(errors[:40]))

