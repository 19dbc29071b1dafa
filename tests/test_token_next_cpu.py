"""Spans and next symbols of the token index without a GPU: the new entry points are declared, exported and bound and the class
methods exist; the three new structs match the C compiler's view of the header; every argument error is answered with -1 before
the handle or a device is touched, and a missing device is -3; the two CPU models that test_gpu_token_next.py measures the device
against (token_next_cases.py) agree on the whole case list; and a hand-worked example pins what the words of the contract mean."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_next_cases as nc
from test_int_cpu import model_sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_index_spans_batch", "sa_hip_token_index_spans_batch_device", "sa_hip_token_index_next_batch_device",
       "sa_hip_token_index_next_batch", "sa_hip_token_index_next_of_spans", "sa_hip_token_index_next_info"]


def test_next_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    for name in ("spans_batch", "spans_batch_device", "next_batch_device", "next_batch", "next_of_spans", "next_info"):
        assert callable(getattr(capi.TokenIndex, name)), name
    from suffixarray_amd import token_index
    for name in ("longest_suffix", "next_tokens", "next_token_counts"):
        assert callable(getattr(token_index.TokenIndex, name)), name
    assert capi.SPAN_DTYPE.itemsize == C.sizeof(capi.TokenSpan) == 16 and capi.NEXT_DTYPE.itemsize == C.sizeof(capi.TokenNext) == 16
    assert capi.SPAN_DTYPE.names == tuple(f for f, _ in capi.TokenSpan._fields_)
    assert capi.NEXT_DTYPE.names == tuple(f for f, _ in capi.TokenNext._fields_)


@pytest.mark.parametrize("struct, cls, fields", [
    ("sa_hip_token_span", "TokenSpan", ["first", "count", "length", "ended"]),
    ("sa_hip_token_next", "TokenNext", ["written", "covered", "total", "reserved"]),
    ("sa_hip_token_next_info", "TokenNextInfo", ["q", "spans_ms", "next_ms", "lane_spans", "wave_spans"]),
])
def test_next_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields):
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


def test_next_argument_errors_before_any_device_call(capi):
    """every refusal comes before the handle is touched: the handle of these calls is an address that holds nothing"""
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    spans = np.zeros(2, capi.SPAN_DTYPE)
    sym, cnt, heads = np.zeros(8, np.int32), np.zeros(8, np.uint32), np.zeros(2, capi.NEXT_DTYPE)
    p, o, s, y, c, hd = (a.ctypes.data for a in (pat, off, spans, sym, cnt, heads))
    D = 1 << 20                                                    # "device pointers": never touched
    # NULL handle
    assert lib.sa_hip_token_index_spans_batch(None, p, o, 2, 0, 0, 1, s) == -1
    assert b"sa_hip_token_index_spans_batch" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_spans_batch_device(None, D, D, 2, 0, 0, 1, D) == -1
    assert lib.sa_hip_token_index_next_batch_device(None, D, 2, 4, D, D, D) == -1
    assert lib.sa_hip_token_index_next_batch(None, p, o, 2, 0, 0, 1, 4, s, y, c, hd) == -1
    assert lib.sa_hip_token_index_next_of_spans(None, s, 2, 4, y, c, hd) == -1
    assert lib.sa_hip_token_index_next_info(None, C.byref(capi.TokenNextInfo())) == -1
    assert lib.sa_hip_token_index_next_info(h, None) == -1
    # mode and need_next are 0 or 1
    for mode, need in ((2, 1), (-1, 1), (0, 2), (1, -1)):
        assert lib.sa_hip_token_index_spans_batch(h, p, o, 2, mode, 0, need, s) == -1, (mode, need)
        assert lib.sa_hip_token_index_spans_batch_device(h, D, D, 2, mode, 0, need, D) == -1, (mode, need)
        assert lib.sa_hip_token_index_next_batch(h, p, o, 2, mode, 0, need, 4, s, y, c, hd) == -1, (mode, need)
        assert lib.sa_hip_token_index_spans_batch(h, p, o, 0, mode, 0, need, s) == -1, (mode, need)     # also with Q == 0
    # cap == 0, Q * cap >= 2^31
    for q, cap in ((2, 0), (0, 0), (1 << 31, 1), (1 << 20, 1 << 11), (1, 0xFFFFFFFF), (3, 0x80000000 // 3 + 1)):
        assert lib.sa_hip_token_index_next_batch_device(h, D, q, cap, D, D, D) == -1, (q, cap)
        assert lib.sa_hip_token_index_next_batch(h, p, o, q, 0, 0, 1, cap, s, y, c, hd) == -1, (q, cap)
        assert lib.sa_hip_token_index_next_of_spans(h, s, q, cap, y, c, hd) == -1, (q, cap)
    assert b"2^31" in lib.sa_hip_last_error()
    # NULL arguments (spans of next_batch may be NULL: not among them)
    assert lib.sa_hip_token_index_spans_batch(h, p, None, 2, 0, 0, 1, s) == -1
    assert lib.sa_hip_token_index_spans_batch(h, p, o, 2, 0, 0, 1, None) == -1
    assert lib.sa_hip_token_index_spans_batch(h, None, o, 2, 0, 0, 1, s) == -1                         # symbols without a buffer
    assert lib.sa_hip_token_index_spans_batch_device(h, D, None, 2, 0, 0, 1, D) == -1
    assert lib.sa_hip_token_index_spans_batch_device(h, D, D, 2, 0, 0, 1, None) == -1
    for args in ((None, D, D, D), (D, None, D, D), (D, D, None, D), (D, D, D, None)):
        assert lib.sa_hip_token_index_next_batch_device(h, args[0], 2, 4, *args[1:]) == -1, args
    for args in ((None, c, hd), (y, None, hd), (y, c, None)):
        assert lib.sa_hip_token_index_next_batch(h, p, o, 2, 0, 0, 1, 4, s, *args) == -1, args
        assert lib.sa_hip_token_index_next_of_spans(h, s, 2, 4, *args) == -1, args
    assert lib.sa_hip_token_index_next_batch(h, p, None, 2, 0, 0, 1, 4, s, y, c, hd) == -1
    assert lib.sa_hip_token_index_next_of_spans(h, None, 2, 4, y, c, hd) == -1
    # descending offsets
    assert lib.sa_hip_token_index_spans_batch(h, p, down.ctypes.data, 2, 1, 0, 1, s) == -1
    assert b"descend" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_next_batch(h, p, down.ctypes.data, 2, 1, 0, 1, 4, s, y, c, hd) == -1
    # Q == 0 with good arguments: a no-op that touches nothing
    assert lib.sa_hip_token_index_spans_batch(h, None, None, 0, 1, 0, 1, None) == 0
    assert lib.sa_hip_token_index_spans_batch_device(h, None, None, 0, 0, 0, 0, None) == 0
    assert lib.sa_hip_token_index_next_batch_device(h, None, 0, 4, None, None, None) == 0
    assert lib.sa_hip_token_index_next_batch(h, None, None, 0, 1, 0, 1, 4, None, None, None, None) == 0
    assert lib.sa_hip_token_index_next_of_spans(h, None, 0, 4, None, None, None) == 0


def test_next_no_device_is_minus_three(capi):
    """no handle without a device, so no answer from anywhere else: the class raises -3 before next_tokens can be asked"""
    lib = capi.lib()
    if lib.sa_hip_device_count() >= 1:
        h = C.c_void_p(0x1234)
        t = np.array([3, 1, 2, 1], np.int32)
        assert lib.sa_hip_token_index_build(C.byref(h), t.ctypes.data, 4, 4, 1 << 20) == -3 and not h.value
        return
    import suffixarray_amd
    with pytest.raises(capi.SaHipError) as e:
        suffixarray_amd.TokenIndex([5, 1, 5, 1, 5]).next_tokens([[5]])
    assert e.value.code == -3
    with pytest.raises(capi.SaHipError) as e:
        capi.TokenIndex.build([1, 2, 3]).next_batch([[1]])
    assert e.value.code == -3


def test_next_models_agree_on_the_case_list():
    total, lane, wave, ended, backed = 0, 0, 0, 0, 0
    for name in nc.TEXTS:
        e = nc.expected(name)
        for cfg in nc.CONFIGS:
            sp = e["spans"][cfg]
            b = nc.model_b(e["t"], e["ctx"], *cfg)
            for i, (count, length, end, ctr) in enumerate(b):
                where = (name, cfg, i, e["ctx"][i][:6], len(e["ctx"][i]))
                assert (count, length, end) == tuple(sp[i, 1:]), where
                sym, cnt = e["entries"][cfg][i]
                assert dict(zip(sym.tolist(), cnt.tolist())) == dict(ctr), where
                assert np.all(np.diff(sym) > 0) and int(cnt.sum()) == count - end, where
            total += len(b)
            lane += int((sp[:, 1] <= nc.LANE_MAX).sum())
            wave += int((sp[:, 1] > nc.LANE_MAX).sum())
            ended += int(sp[:, 3].sum())
            if cfg[0] == 1:
                backed += int((sp[:, 2] < np.array([len(c) for c in e["ctx"]])).sum())
    assert total > 2500 and lane > 500 and wave > 500 and ended > 50 and backed > 500
    # the planted runs are the entries of [A]
    e = nc.expected("planted")
    i = e["ctx"].index([nc.PLANT_A])
    sym, cnt = e["entries"][(0, 0, 1)][i]
    assert sym.tolist() == list(nc.PLANT_S) and cnt.tolist() == list(nc.RUNS) and e["spans"][(0, 0, 1)][i, 3] == 1


def test_next_hand_worked_banana():
    """"banana" as tokens (b = 1, a = 0, n = 2); suffixes in order: a, ana, anana, banana, na, nana = SA [5, 3, 1, 0, 4, 2]"""
    t = np.array([1, 0, 2, 0, 2, 0], np.int32)
    sa = model_sa(t)
    assert sa.tolist() == [5, 3, 1, 0, 4, 2]
    tl, sl = t.tolist(), sa.tolist()
    ctx = [[0], [0, 2], [2, 0], [7, 2, 0], [0, 2, 0, 2, 0], [7], [], [1, 0, 2, 0, 2, 0], [9, 1]]
    exact = nc.spans_a(tl, sl, ctx, 0, 0, 1)
    assert exact.tolist() == [[0, 3, 1, 1], [1, 2, 2, 0], [4, 2, 2, 1], [6, 0, 3, 0], [2, 1, 5, 1], [6, 0, 1, 0], [0, 6, 0, 0],
                              [3, 1, 6, 1], [6, 0, 2, 0]]
    nxt = [dict(zip(*(a.tolist() for a in nc.entries_a(t, sa, s)))) for s in exact]
    assert nxt == [{2: 2}, {0: 2}, {2: 1}, {}, {}, {}, {0: 3, 1: 1, 2: 2}, {}, {}]
    # longest suffix that has a next symbol: [7, 2, 0] -> [2, 0]; "anana" ends the text -> "nana" too -> ... -> [2, 0] (na + n)
    back = nc.spans_a(tl, sl, ctx, 1, 0, 1)
    assert back.tolist() == [[0, 3, 1, 1], [1, 2, 2, 0], [4, 2, 2, 1], [4, 2, 2, 1], [1, 2, 3, 1], [0, 6, 0, 0], [0, 6, 0, 0],
                             [1, 2, 3, 1], [3, 1, 1, 0]]
    # ... and without that demand the ended suffix counts: the whole of "anana" and of the text
    stay = nc.spans_a(tl, sl, ctx, 1, 0, 0)
    assert stay[4].tolist() == [2, 1, 5, 1] and stay[7].tolist() == [3, 1, 6, 1] and stay[3].tolist() == [4, 2, 2, 1]
    # max_length caps L
    assert nc.spans_a(tl, sl, ctx, 1, 1, 1)[:, 2].tolist() == [1, 1, 1, 1, 1, 0, 0, 1, 1]
    assert nc.spans_a(tl, sl, ctx, 1, 2, 1)[4].tolist() == [4, 2, 2, 1]
    for cfg in ((0, 0, 1), (1, 0, 1), (1, 0, 0), (1, 1, 1), (1, 2, 1)):
        a = nc.spans_a(tl, sl, ctx, *cfg)
        b = nc.model_b(t, ctx, *cfg)
        assert [tuple(r[1:]) for r in a.tolist()] == [x[:3] for x in b], cfg
    # cap: the smallest symbols, exact counts, covered < total
    sym, cnt, heads = nc.capped([nc.entries_a(t, sa, exact[6])], 2, -7, 7)
    assert sym.tolist() == [[0, 1]] and cnt.tolist() == [[3, 1]] and heads.tolist() == [[2, 4, 6, 0]]
