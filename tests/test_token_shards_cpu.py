"""The shard set without a GPU: every new entry point is declared, exported and bound and the classes exist; the two new structs
match the C compiler's view of the header; every argument error is answered with -1 before a handle or a device is touched, and
without a device nothing is created; the combine model that test_gpu_token_shards.py measures the device against
(token_shard_cases.py) agrees with a brute-force window count over the shards."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_cases as tc
import token_shard_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_shards_create", "sa_hip_token_shards_sync", "sa_hip_token_shards_info", "sa_hip_token_shards_query_batch",
       "sa_hip_token_shards_query_batch_device", "sa_hip_token_shards_spans_batch", "sa_hip_token_shards_spans_batch_device",
       "sa_hip_token_shards_next_batch", "sa_hip_token_shards_next_batch_device", "sa_hip_token_shards_merge_device"]


def test_shard_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW + ["sa_hip_token_shards_destroy", "sa_hip_token_shards_shard"]:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    for name in NEW:
        assert getattr(lib, name).restype is C.c_int, name
    for name in ("create", "build", "shard", "sync", "info", "query_batch", "query_batch_device", "spans_batch", "spans_batch_device",
                 "next_batch", "next_batch_device", "merge_device", "close"):
        assert callable(getattr(capi.TokenShards, name)), name
    import suffixarray_amd
    from suffixarray_amd import token_shards
    assert suffixarray_amd.ShardedTokenIndex is token_shards.ShardedTokenIndex
    for name in ("count", "ranges", "positions", "longest_suffix", "next_tokens", "next_token_counts", "shard_sizes", "info", "close",
                 "__enter__", "__exit__"):
        assert callable(getattr(token_shards.ShardedTokenIndex, name)), name
    assert capi.SHARDS_NEXT_DTYPE.itemsize == C.sizeof(capi.TokenShardsNext) == 24
    assert capi.SHARDS_NEXT_DTYPE.names == tuple(f for f, _ in capi.TokenShardsNext._fields_)
    assert [capi.SHARDS_NEXT_DTYPE.fields[f][1] for f in capi.SHARDS_NEXT_DTYPE.names] == [getattr(capi.TokenShardsNext, f).offset for f in capi.SHARDS_NEXT_DTYPE.names]
    assert capi.SHARDS_MAX == 64


@pytest.mark.parametrize("struct, cls, fields", [
    ("sa_hip_token_shards_next", "TokenShardsNext", ["written", "length", "covered", "total"]),
    ("sa_hip_token_shards_stats", "TokenShardsStats", ["shards", "chunk", "tokens", "q", "ranges_ms", "spans_ms", "next_ms", "merge_ms"]),
])
def test_shard_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields):
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
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
    assert [f for f in re.findall(r"^\s*\w+\s+(\w+);", body, re.M)] == fields


def test_shard_create_refusals_before_any_device_call(capi):
    """the list is looked at, the handles in it are not: they are addresses that hold nothing"""
    lib = capi.lib()
    out = C.c_void_p(0x77)
    two = (C.c_void_p * 2)(0x1000, 0x2000)
    assert lib.sa_hip_token_shards_create(None, two, 2) == -1
    assert lib.sa_hip_token_shards_create(C.byref(out), None, 2) == -1 and not out.value
    assert b"sa_hip_token_shards_create" in lib.sa_hip_last_error()
    out = C.c_void_p(0x77)
    assert lib.sa_hip_token_shards_create(C.byref(out), two, 0) == -1 and not out.value
    many = (C.c_void_p * 65)(*[0x1000 + 64 * j for j in range(65)])
    assert lib.sa_hip_token_shards_create(C.byref(out), many, 65) == -1                               # S = 65 is refused
    assert b"64" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_create(C.byref(out), many, 0xFFFFFFFF) == -1
    hole = (C.c_void_p * 3)(0x1000, None, 0x3000)
    assert lib.sa_hip_token_shards_create(C.byref(out), hole, 3) == -1
    assert b"NULL" in lib.sa_hip_last_error()
    twice = (C.c_void_p * 3)(0x1000, 0x2000, 0x1000)
    assert lib.sa_hip_token_shards_create(C.byref(out), twice, 3) == -1
    assert b"twice" in lib.sa_hip_last_error()
    lib.sa_hip_token_shards_destroy(None)
    assert lib.sa_hip_token_shards_shard(None, 0) is None
    with pytest.raises(ValueError):
        from suffixarray_amd import token_shards
        token_shards.ShardedTokenIndex([])
    with pytest.raises(ValueError):
        token_shards.ShardedTokenIndex([[1]] * 65)


def test_shard_argument_errors_before_any_device_call(capi):
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    tot, per, ln = np.zeros(2, np.uint64), np.zeros(4, capi.PAIR_DTYPE), np.zeros(2, np.uint32)
    spans = np.zeros(4, capi.SPAN_DTYPE)
    sym, cnt, heads = np.zeros(8, np.int32), np.zeros(8, np.uint64), np.zeros(2, capi.SHARDS_NEXT_DTYPE)
    p, o, t, r, l, s, y, c, hd = (a.ctypes.data for a in (pat, off, tot, per, ln, spans, sym, cnt, heads))
    D = 1 << 20                                                    # "device pointers": never touched
    # NULL handle
    assert lib.sa_hip_token_shards_query_batch(None, p, o, 2, t, r) == -1
    assert b"sa_hip_token_shards_query_batch" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_query_batch_device(None, D, D, 2, D, D) == -1
    assert lib.sa_hip_token_shards_spans_batch(None, p, o, 2, 0, 0, 1, l, t, s) == -1
    assert lib.sa_hip_token_shards_spans_batch_device(None, D, D, 2, 0, 0, 1, D, D, D) == -1
    assert lib.sa_hip_token_shards_next_batch(None, p, o, 2, 0, 0, 1, 4, s, y, c, hd) == -1
    assert lib.sa_hip_token_shards_next_batch_device(None, D, 2, 4, D, D, D) == -1
    assert lib.sa_hip_token_shards_merge_device(None, D, D, D, 2, 4, D, D, D) == -1
    assert lib.sa_hip_token_shards_sync(None) == -1
    assert lib.sa_hip_token_shards_info(None, C.byref(capi.TokenShardsStats())) == -1
    assert lib.sa_hip_token_shards_info(h, None) == -1
    # mode and need_next are 0 or 1
    for mode, need in ((2, 1), (-1, 1), (0, 2), (1, -1)):
        assert lib.sa_hip_token_shards_spans_batch(h, p, o, 2, mode, 0, need, l, t, s) == -1, (mode, need)
        assert lib.sa_hip_token_shards_spans_batch_device(h, D, D, 2, mode, 0, need, D, D, D) == -1, (mode, need)
        assert lib.sa_hip_token_shards_next_batch(h, p, o, 2, mode, 0, need, 4, s, y, c, hd) == -1, (mode, need)
        assert lib.sa_hip_token_shards_spans_batch(h, p, o, 0, mode, 0, need, l, t, s) == -1, (mode, need)   # also with Q == 0
    # cap == 0, Q * cap >= 2^31
    for q, cap in ((2, 0), (0, 0), (1 << 31, 1), (1 << 20, 1 << 11), (1, 0xFFFFFFFF), (3, 0x80000000 // 3 + 1)):
        assert lib.sa_hip_token_shards_next_batch_device(h, D, q, cap, D, D, D) == -1, (q, cap)
        assert lib.sa_hip_token_shards_next_batch(h, p, o, q, 0, 0, 1, cap, s, y, c, hd) == -1, (q, cap)
        assert lib.sa_hip_token_shards_merge_device(h, D, D, D, q, cap, D, D, D) == -1, (q, cap)
    assert b"2^31" in lib.sa_hip_last_error()
    # NULL arguments (per_shard of the ranges and spans of next_batch may be NULL: not among them)
    assert lib.sa_hip_token_shards_query_batch(h, p, None, 2, t, r) == -1
    assert lib.sa_hip_token_shards_query_batch(h, p, o, 2, None, r) == -1
    assert lib.sa_hip_token_shards_query_batch(h, None, o, 2, t, r) == -1                              # symbols without a buffer
    assert lib.sa_hip_token_shards_query_batch_device(h, D, None, 2, D, D) == -1
    assert lib.sa_hip_token_shards_query_batch_device(h, D, D, 2, None, D) == -1
    for args in ((None, t, s), (l, None, s), (l, t, None)):
        assert lib.sa_hip_token_shards_spans_batch(h, p, o, 2, 1, 0, 1, *args) == -1, args
        assert lib.sa_hip_token_shards_spans_batch_device(h, D, D, 2, 1, 0, 1, *(a and D for a in args)) == -1, args
    assert lib.sa_hip_token_shards_spans_batch(h, p, None, 2, 1, 0, 1, l, t, s) == -1
    assert lib.sa_hip_token_shards_spans_batch(h, None, o, 2, 1, 0, 1, l, t, s) == -1
    assert lib.sa_hip_token_shards_spans_batch_device(h, D, None, 2, 1, 0, 1, D, D, D) == -1
    for args in ((None, c, hd), (y, None, hd), (y, c, None)):
        assert lib.sa_hip_token_shards_next_batch(h, p, o, 2, 0, 0, 1, 4, s, *args) == -1, args
    assert lib.sa_hip_token_shards_next_batch(h, p, None, 2, 0, 0, 1, 4, s, y, c, hd) == -1
    for args in ((None, D, D, D), (D, None, D, D), (D, D, None, D), (D, D, D, None)):
        assert lib.sa_hip_token_shards_next_batch_device(h, args[0], 2, 4, *args[1:]) == -1, args
    for k in range(6):
        a = [D] * 6
        a[k] = None
        assert lib.sa_hip_token_shards_merge_device(h, a[0], a[1], a[2], 2, 4, a[3], a[4], a[5]) == -1, k
    # descending offsets
    assert lib.sa_hip_token_shards_query_batch(h, p, down.ctypes.data, 2, t, r) == -1
    assert b"descend" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_spans_batch(h, p, down.ctypes.data, 2, 1, 0, 1, l, t, s) == -1
    assert lib.sa_hip_token_shards_next_batch(h, p, down.ctypes.data, 2, 1, 0, 1, 4, s, y, c, hd) == -1
    # Q == 0 with good arguments: a no-op that touches nothing
    assert lib.sa_hip_token_shards_query_batch(h, None, None, 0, None, None) == 0
    assert lib.sa_hip_token_shards_query_batch_device(h, None, None, 0, None, None) == 0
    assert lib.sa_hip_token_shards_spans_batch(h, None, None, 0, 1, 0, 1, None, None, None) == 0
    assert lib.sa_hip_token_shards_spans_batch_device(h, None, None, 0, 0, 0, 0, None, None, None) == 0
    assert lib.sa_hip_token_shards_next_batch(h, None, None, 0, 1, 0, 1, 4, None, None, None, None) == 0
    assert lib.sa_hip_token_shards_next_batch_device(h, None, 0, 4, None, None, None) == 0
    assert lib.sa_hip_token_shards_merge_device(h, None, None, None, 0, 4, None, None, None) == 0


def test_shards_without_a_device_fail_loudly(capi):
    """no shard handle without a device, hence no set, and no answer from anywhere else"""
    if capi.lib().sa_hip_device_count() >= 1:
        with pytest.raises(capi.SaHipError) as e:
            capi.TokenShards.build([[1, 2, 3], [2, 3]], device=1 << 20)
        assert e.value.code == -3
        return
    import suffixarray_amd
    with pytest.raises(capi.SaHipError) as e:
        suffixarray_amd.ShardedTokenIndex([[5, 1, 5], [1, 5]])
    assert e.value.code == -3
    with pytest.raises(capi.SaHipError) as e:
        capi.TokenShards.build([[1, 2, 3]])
    assert e.value.code == -3


@pytest.mark.parametrize("name", sc.SETS)
def test_combine_model_against_brute_force(name):
    e = sc.expected(name)
    shards, ctx = e["shards"], e["ctx"]
    S, Q = len(shards), len(ctx)
    assert e["first"].shape == e["count"].shape == (S, Q) and all(len(t) < 30000 for t in shards)
    windows = np.array([tc.model_b(t, ctx) for t in shards], np.int64)                                # no suffix array involved
    assert np.array_equal(windows, e["count"])
    small = sum(len(t) for t in shards) < 10000                                                       # brute force is O(tokens * Q) in Python
    backed = differs = 0
    for cfg in sc.CONFIGS:
        mode, max_length, need_next = cfg
        L, totals, spans, entries = e[cfg]
        assert spans.shape == (S, Q, 4)
        for i, c in enumerate(ctx):
            limit = len(c) if mode == 0 else min(len(c), max_length or len(c))
            assert L[i] <= limit and (mode == 1 or L[i] == len(c)), (name, cfg, i)
            assert all(int(spans[s, i, 2]) == (L[i] if len(shards[s]) else 0) for s in range(S)), (name, cfg, i)
            sym, cnt = entries[i]
            assert sym == sorted(set(sym)) and sum(cnt) == sum(int(spans[s, i, 1]) - int(spans[s, i, 3]) for s in range(S)), (name, cfg, i)
            backed += L[i] < len(c)
            if not small:
                continue
            hits, with_next, nxt = sc.brute(shards, c[len(c) - L[i]:])
            assert totals[i] == (with_next if need_next else hits), (name, cfg, i, c[:8])
            assert dict(zip(sym, cnt)) == nxt and int(spans[:, i, 1].sum()) == hits, (name, cfg, i, c[:8])
            if mode == 1:
                assert totals[i] >= 1 or L[i] == 0, (name, cfg, i)
                if L[i] < limit:                                                                      # one symbol more qualifies nowhere
                    h1, w1, _ = sc.brute(shards, c[len(c) - L[i] - 1:])
                    assert (w1 if need_next else h1) == 0, (name, cfg, i, c[:8])
        if mode == 1 and need_next:
            differs += int((np.array(L) != np.array(e[(1, 0, 0)][0])).sum()) if cfg == (1, 0, 1) else 0
    assert backed > 10, name
    if name == "ls":
        i = ctx.index([7, 3, 4, 5])
        assert e[(1, 0, 0)][0][i] == 4 and e[(1, 0, 1)][0][i] == 3 and differs >= 2
        assert e[(1, 0, 1)][2][:, i].tolist() == [[2, 1, 3, 0], [0, 1, 3, 1], [1, 1, 3, 0]]            # shard 1: it only ends the text
        assert e[(1, 0, 0)][2][:, i].tolist() == [[5, 0, 4, 0], [3, 1, 4, 1], [5, 0, 4, 0]]            # misses keep the lower bound
        j = ctx.index([3, 4, 5])
        assert e[(1, 0, 1)][1][j] == 2 and e[(1, 0, 0)][1][j] == 3 and e[(1, 0, 1)][3][j] == ([6, 9], [1, 1])
        k = ctx.index([0, 2, 3, 4, 5, 6])
        assert e[(1, 0, 1)][0][k] == 0 and e[(1, 0, 0)][0][k] == 5 and e[(1, 0, 0)][2][:, k, 1].tolist() == [0, 0, 1]
        k = ctx.index([0, 8, 2, 3, 4])
        assert e[(1, 0, 1)][0][k] == 4 and e[(1, 0, 1)][2][:, k, 1].tolist() == [0, 0, 1] and e[(1, 0, 1)][3][k] == ([5], [1])
        k = ctx.index([0, 1, 2, 3, 4, 5])
        assert e[(1, 0, 1)][0][k] == 5 and e[(1, 0, 1)][2][:, k, 1].tolist() == [1, 0, 0]
    if name == "mod_deal":
        i = ctx.index([sc.A])
        sym, cnt = e[(0, 0, 1)][3][i]
        assert sym == list(range(sc.MOD_D)) and cnt == [x + 1 for x in range(sc.MOD_D)]
    if name == "one_next64":
        i = ctx.index([sc.A])
        sym, cnt = e[(0, 0, 1)][3][i]
        assert sym[0] == 7 and cnt[0] == 64 * 65 // 2 and len(sym) == 65
