"""Top-k next symbols and draws over a shard set without a GPU: the entry points are declared, exported and bound and the class
methods exist; the two new structs match the C compiler's view of the header; every argument error that needs no live set is
answered with -1 before the handle or a device is touched; the top-k, the budget and the sample model of token_shard_top_cases.py
agree with a brute-force count of the windows of all shards on every set and configuration; and the planted sets hold what their
names promise."""
import ctypes as C
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import token_shard_cases as sc
import token_shard_top_cases as stc
import token_top_cases as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_shards_top_batch_device", "sa_hip_token_shards_top_batch", "sa_hip_token_shards_sample_batch_device",
       "sa_hip_token_shards_sample_batch", "sa_hip_token_shards_top_info"]


def test_shard_top_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    for name in ("top_batch", "top_batch_device", "sample_batch", "sample_batch_device", "top_info"):
        assert callable(getattr(capi.TokenShards, name)), name
    from suffixarray_amd import token_shards
    for name in ("top_next_tokens", "sample_next"):
        assert callable(getattr(token_shards.ShardedTokenIndex, name)), name
    assert capi.SHARDS_TOP_DTYPE.itemsize == C.sizeof(capi.TokenShardsTop) == 32
    assert capi.SHARDS_TOP_DTYPE.names == tuple(f for f, _ in capi.TokenShardsTop._fields_)
    assert [capi.SHARDS_TOP_DTYPE.fields[f][1] for f in capi.SHARDS_TOP_DTYPE.names] == [0, 4, 8, 12, 16, 24]     # no implicit padding


@pytest.mark.parametrize("struct, cls, fields", [
    ("sa_hip_token_shards_top", "TokenShardsTop", ["written", "distinct", "length", "shards", "covered", "total"]),
    ("sa_hip_token_shards_top_stats", "TokenShardsTopStats", ["q", "spans_ms", "top_ms", "sample_ms"]),
])
def test_shard_top_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields):
    S = getattr(capi, cls)
    assert [f for f, _ in S._fields_] == fields
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sa_hip.h"\nint main(void) { printf("%zu'
                   + "".join(" %zu" for _ in fields) + '\\n", sizeof(' + struct + ")"
                   + "".join(", offsetof(%s, %s)" % (struct, f) for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields], got


def test_shard_top_argument_errors_that_need_no_live_set(capi):
    """a NULL set is refused under the entry point's name whatever else is wrong with the call; behind an address that holds
    nothing, k, m, mode, need_next, the products, NULL pointers and descending offsets are refused before the set is touched"""
    lib = capi.lib()
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    spans = np.zeros(2 * 64, capi.SPAN_DTYPE)
    sym, cnt, heads = np.zeros(128, np.int32), np.zeros(128, np.uint64), np.zeros(2, capi.SHARDS_TOP_DTYPE)
    draws, sh, rk = np.zeros(8, np.uint64), np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    p, o, s, y, c, hd, dr, a, r = (x.ctypes.data for x in (pat, off, spans, sym, cnt, heads, draws, sh, rk))
    D = 1 << 20                                                    # "device pointers": never touched
    # NULL set: with good arguments and with a bad k / m / mode -- the set's refusal stands in the last error
    for k, m, mode in ((4, 1, 0), (0, 0, 2), (65, 0, -1)):
        assert lib.sa_hip_token_shards_top_batch_device(None, D, 2, k, 0, D, D, D) == -1
        assert b"sa_hip_token_shards_top_batch_device: NULL handle" in lib.sa_hip_last_error(), lib.sa_hip_last_error()
        assert lib.sa_hip_token_shards_top_batch(None, p, o, 2, mode, 0, 1, k, 0, s, y, c, hd) == -1
        assert b"sa_hip_token_shards_top_batch: NULL handle" in lib.sa_hip_last_error(), lib.sa_hip_last_error()
        assert lib.sa_hip_token_shards_sample_batch_device(None, D, 2, D, m, D, D, D) == -1
        assert b"sa_hip_token_shards_sample_batch_device: NULL handle" in lib.sa_hip_last_error(), lib.sa_hip_last_error()
        assert lib.sa_hip_token_shards_sample_batch(None, p, o, 2, mode, 0, 1, dr, m, s, y, a, r) == -1
        assert b"sa_hip_token_shards_sample_batch: NULL handle" in lib.sa_hip_last_error(), lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_top_info(None, C.byref(capi.TokenShardsTopStats())) == -1
    assert b"sa_hip_token_shards_top_info" in lib.sa_hip_last_error()
    h = 0x1234                                                     # a handle that holds nothing: never dereferenced below
    assert lib.sa_hip_token_shards_top_info(h, None) == -1
    # mode and need_next are 0 or 1 (also with Q == 0)
    for mode, need in ((2, 1), (-1, 1), (0, 2), (1, -1)):
        for q in (2, 0):
            assert lib.sa_hip_token_shards_top_batch(h, p, o, q, mode, 0, need, 4, 0, s, y, c, hd) == -1, (mode, need, q)
            assert b"sa_hip_token_shards_top_batch" in lib.sa_hip_last_error()
            assert lib.sa_hip_token_shards_sample_batch(h, p, o, q, mode, 0, need, dr, 1, s, y, a, r) == -1, (mode, need, q)
            assert b"sa_hip_token_shards_sample_batch" in lib.sa_hip_last_error()
    # k == 0, k > 64, Q * k >= 2^31 (also with Q == 0)
    for q, k in ((2, 0), (0, 0), (2, 65), (0, 65), (2, 0xFFFFFFFF), (1 << 31, 1), (1 << 25, 64), (1 << 58, 64), (0x80000000 // 3 + 1, 3)):
        assert lib.sa_hip_token_shards_top_batch_device(h, D, q, k, 0, D, D, D) == -1, (q, k)
        assert lib.sa_hip_token_shards_top_batch(h, p, o, q, 0, 0, 1, k, 0, s, y, c, hd) == -1, (q, k)
    assert lib.sa_hip_token_shards_top_batch_device(h, D, 2, 65, 0, D, D, D) == -1 and b"64" in lib.sa_hip_last_error()
    # m == 0, Q * m >= 2^31
    for q, m in ((2, 0), (0, 0), (1 << 31, 1), (1 << 20, 1 << 11), (1, 0xFFFFFFFF), (1 << 40, 1 << 30)):
        assert lib.sa_hip_token_shards_sample_batch_device(h, D, q, D, m, D, D, D) == -1, (q, m)
        assert lib.sa_hip_token_shards_sample_batch(h, p, o, q, 0, 0, 1, dr, m, s, y, a, r) == -1, (q, m)
    assert b"2^31" in lib.sa_hip_last_error()
    # NULL arguments (spans of the host forms, shards_out and ranks may be NULL: not among them)
    for args in ((None, D, D, D), (D, None, D, D), (D, D, None, D), (D, D, D, None)):
        assert lib.sa_hip_token_shards_top_batch_device(h, args[0], 2, 4, 0, *args[1:]) == -1, args
    for args in ((None, c, hd), (y, None, hd), (y, c, None)):
        assert lib.sa_hip_token_shards_top_batch(h, p, o, 2, 0, 0, 1, 4, 0, s, *args) == -1, args
    assert lib.sa_hip_token_shards_top_batch(h, p, None, 2, 0, 0, 1, 4, 0, s, y, c, hd) == -1
    assert lib.sa_hip_token_shards_top_batch(h, None, o, 2, 0, 0, 1, 4, 0, s, y, c, hd) == -1           # symbols without a buffer
    for args in ((None, D, D), (D, None, D), (D, D, None)):
        assert lib.sa_hip_token_shards_sample_batch_device(h, args[0], 2, args[1], 1, args[2], D, D) == -1, args
    assert lib.sa_hip_token_shards_sample_batch(h, p, None, 2, 0, 0, 1, dr, 1, s, y, a, r) == -1
    assert lib.sa_hip_token_shards_sample_batch(h, p, o, 2, 0, 0, 1, None, 1, s, y, a, r) == -1
    assert lib.sa_hip_token_shards_sample_batch(h, p, o, 2, 0, 0, 1, dr, 1, s, None, a, r) == -1
    assert b"NULL" in lib.sa_hip_last_error()
    # descending offsets
    assert lib.sa_hip_token_shards_top_batch(h, p, down.ctypes.data, 2, 1, 0, 1, 4, 0, s, y, c, hd) == -1
    assert b"descend" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_sample_batch(h, p, down.ctypes.data, 2, 1, 0, 1, dr, 1, s, y, a, r) == -1
    # Q == 0 with good arguments: a no-op that touches nothing
    assert lib.sa_hip_token_shards_top_batch_device(h, None, 0, 64, 7, None, None, None) == 0
    assert lib.sa_hip_token_shards_top_batch(h, None, None, 0, 1, 0, 1, 1, 0, None, None, None, None) == 0
    assert lib.sa_hip_token_shards_sample_batch_device(h, None, 0, None, 3, None, None, None) == 0
    assert lib.sa_hip_token_shards_sample_batch(h, None, None, 0, 1, 0, 1, None, 3, None, None, None, None) == 0


def test_shard_top_no_device_is_minus_three(capi):
    lib = capi.lib()
    if lib.sa_hip_device_count() >= 1:
        return                                                     # (with a device: test_gpu_token_shard_top.py)
    import suffixarray_amd
    with pytest.raises(capi.SaHipError) as e:
        suffixarray_amd.ShardedTokenIndex([[5, 1, 5, 1, 5], [5, 2]]).top_next_tokens([[5]])
    assert e.value.code == -3


@pytest.mark.parametrize("name", stc.SETS)
def test_models_against_window_counts_of_all_shards(name):
    """per distinct (configuration, matched tail) of the set: the merged entries are the brute-force window counts over all shards;
    the top-k model is their k largest under (-count, symbol); the budget model is a brute-force cut of the continuations in
    ascending symbol order; every edge draw of the sample model lands where the shard-major list of continuations says"""
    e = stc.expected(name)
    seen = set()
    for cfg in stc.CONFIGS:
        L, totals, spans, entries = e[cfg]
        for i, c in enumerate(e["ctx"]):
            tail = c[len(c) - L[i]:]
            if (cfg[2], tuple(tail)) in seen:
                continue
            seen.add((cfg[2], tuple(tail)))
            _, with_next, want = sc.brute(e["shards"], tail)
            sym, cnt = entries[i]
            assert dict(zip(sym, cnt)) == want, (name, cfg, i)
            total, d = sum(cnt), len(want)
            assert total == with_next == sc.next_total(spans)[i], (name, cfg, i)
            brute = sorted(want.items(), key=lambda p: (-p[1], p[0]))
            for k in {1, max(d - 1, 1), max(d, 1), d + 1, 8, 64}:
                assert stc.top_of((sym, cnt), k) == brute[:k], (name, cfg, i, k)
            flat = np.repeat(np.array(sym, np.int64), np.array(cnt, np.int64))
            for budget in {1, 63, 64, 65, max(total - 1, 1), total, total + 1}:
                ws, wc = stc.cut_entries((sym, cnt), budget)
                assert dict(zip(ws, wc)) == dict(Counter(flat[:budget].tolist())), (name, cfg, i, budget)
                assert sum(wc) == min(total, budget), (name, cfg, i, budget)
            assert stc.cut_entries((sym, cnt), 0) == (list(sym), list(cnt))
            # the sample model against the shard-major list of continuations
            major = stc.shard_major_flat(e, spans, i)
            assert len(major) == total and Counter(major) == Counter(want), (name, cfg, i)
            if total == 0:
                assert stc.sample_of(e, spans, i, 2 ** 64 - 1) == (-1, 0xFFFFFFFF, 0xFFFFFFFF), (name, cfg, i)
                continue
            hit = set()
            for dr in tt.edge_draws(stc.shard_major_runs(e, spans, i)):
                s, shard, rank = stc.sample_of(e, spans, i, dr)
                r = (dr * total) >> 64
                assert r * 2 ** 64 <= dr * total < (r + 1) * 2 ** 64 and s == major[r], (name, cfg, i, dr)
                sp = spans[shard, i]
                before = sum(int(spans[t, i, 1]) - int(spans[t, i, 3]) for t in range(shard))
                assert rank == int(sp[0]) + int(sp[3]) + r - before and int(sp[0]) + int(sp[3]) <= rank < int(sp[0]) + int(sp[1]), (name, cfg, i, dr)
                hit.add(s)
            assert hit == set(want), (name, cfg, i)
    assert seen


def test_planted_sets_hold_what_their_names_promise():
    for name in stc.PLANTED:
        e = stc.expected(name)
        i = e["ctx"].index([stc.A])
        sym, cnt = e[(0, 0, 1)][3][i]
        assert list(zip(sym, cnt)) == stc.merged_runs(name), name
        for s, runs in enumerate(stc.RUNS[name]):
            sp = e[(0, 0, 1)][2][s, i]
            assert (int(sp[1]), int(sp[3])) == ((sum(c for _, c in runs) + 1, 1) if runs else (0, 0)), (name, s)   # an ended suffix first
            assert [r[0] for r in runs] == sorted(r[0] for r in runs), (name, s)
    # sum_beats: the common symbol is third in every shard and first overall; merging the shards' own top-2 lists misses it
    runs = stc.RUNS["sum_beats"]
    assert len(runs) == 4 and all(sorted(c for _, c in r) == [9, 10, 10] for r in runs)
    assert stc.top_of(tuple(zip(*stc.merged_runs("sum_beats"))), 2) == [(50, 36), (100, 10)]
    own = {}
    for r in runs:
        for s, c in sorted(r, key=lambda p: (-p[1], p[0]))[:2]:
            own[s] = own.get(s, 0) + c
    assert 50 not in own
    # ties3: 130 symbols of count 1 dealt round-robin
    m = stc.merged_runs("ties3")
    assert len(m) == 130 > 2 * tt.WINDOW and {c for _, c in m} == {1} and [len(r) for r in stc.RUNS["ties3"]] == [44, 43, 43]
    assert stc.top_of(tuple(zip(*m)), 8) == [(7 * j, 1) for j in range(8)]
    # queue_edge
    q = stc.RUNS["queue_edge"]
    S = len(q)
    assert S == 17 and stc.depth(S) == 32 and stc.depth(16) == 64 and stc.depth(33) == 16 and all(S * stc.depth(S) <= stc.QUEUE for S in range(1, 65))
    assert len(q[0]) == 70 > 64 > stc.depth(S) and {c for _, c in q[0]} == {1}
    assert [c for _, c in q[1]] == [5, 70, 3] and tt.WINDOW < 70 <= stc.JUMP_MIN
    assert [c for _, c in q[2]] == [5, 4097, 2] and q[1][1][0] == q[2][1][0]
    assert q[3][0][1] == tt.WINDOW and len(q[3]) == 2 and q[4] == []
    assert all(len(r) == 2 and max(c for _, c in r) <= 3 for r in q[5:])
    assert len(sc.expected("one_next64")["shards"]) == 64 and stc.depth(64) == 16                       # 64 counts into one entry, D = 16
    assert any(len(t) == 0 for t in sc.expected("s3")["shards"])                                     # an empty shard in a reused set
    # all_shared: every merge step sums all shards; last_wins: the largest sum is the last merged run
    a = stc.RUNS["all_shared"]
    assert len(a) == 5 and all([s for s, _ in r] == [3 * j for j in range(40)] for r in a) and len({tuple(c for _, c in r) for r in a}) == 5
    lw = stc.merged_runs("last_wins")
    assert lw[-1] == (900, 60) and max(c for _, c in lw[:-1]) < 60
