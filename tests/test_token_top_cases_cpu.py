"""Top-k next symbols and draws from a span without a GPU: the entry points are declared, exported and bound and the class methods
exist; the two new structs match the C compiler's view of the header; every argument error is answered with -1 before the handle
or a device is touched; the top-k and the sample model of token_top_cases.py agree with a brute-force count of the text's windows on
every text; and the planted texts hold the runs their names promise."""
import ctypes as C
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import token_next_cases as nc
import token_top_cases as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_index_top_batch_device", "sa_hip_token_index_top_batch", "sa_hip_token_index_sample_batch_device",
       "sa_hip_token_index_sample_batch", "sa_hip_token_index_top_info"]


def test_top_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    for name in ("top_batch", "top_batch_device", "sample_batch", "sample_batch_device", "top_info"):
        assert callable(getattr(capi.TokenIndex, name)), name
    from suffixarray_amd import token_index
    for name in ("top_next_tokens", "sample_next"):
        assert callable(getattr(token_index.TokenIndex, name)), name
    assert capi.TOP_DTYPE.itemsize == C.sizeof(capi.TokenTop) == 16
    assert capi.TOP_DTYPE.names == tuple(f for f, _ in capi.TokenTop._fields_)


@pytest.mark.parametrize("struct, cls, fields", [
    ("sa_hip_token_top", "TokenTop", ["written", "distinct", "covered", "total"]),
    ("sa_hip_token_top_info", "TokenTopInfo", ["q", "spans_ms", "top_ms", "sample_ms"]),
])
def test_top_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields):
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


def test_top_argument_errors_before_any_device_call(capi):
    """every refusal comes before the handle is touched: the handle of these calls is an address that holds nothing"""
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    spans = np.zeros(2, capi.SPAN_DTYPE)
    sym, cnt, heads = np.zeros(128, np.int32), np.zeros(128, np.uint32), np.zeros(2, capi.TOP_DTYPE)
    draws = np.zeros(8, np.uint64)
    p, o, s, y, c, hd, dr = (a.ctypes.data for a in (pat, off, spans, sym, cnt, heads, draws))
    D = 1 << 20                                                    # "device pointers": never touched
    # NULL handle
    assert lib.sa_hip_token_index_top_batch_device(None, D, 2, 4, 0, D, D, D) == -1
    assert b"sa_hip_token_index_top_batch_device" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_top_batch(None, p, o, 2, 0, 0, 1, 4, 0, s, y, c, hd) == -1
    assert lib.sa_hip_token_index_sample_batch_device(None, D, 2, D, 1, D, D) == -1
    assert lib.sa_hip_token_index_sample_batch(None, p, o, 2, 0, 0, 1, dr, 1, s, y, c) == -1
    assert lib.sa_hip_token_index_top_info(None, C.byref(capi.TokenTopInfo())) == -1
    assert lib.sa_hip_token_index_top_info(h, None) == -1
    # mode and need_next are 0 or 1 (also with Q == 0)
    for mode, need in ((2, 1), (-1, 1), (0, 2), (1, -1)):
        for q in (2, 0):
            assert lib.sa_hip_token_index_top_batch(h, p, o, q, mode, 0, need, 4, 0, s, y, c, hd) == -1, (mode, need, q)
            assert lib.sa_hip_token_index_sample_batch(h, p, o, q, mode, 0, need, dr, 1, s, y, c) == -1, (mode, need, q)
    # k == 0, k > 64, Q * k >= 2^31 (also with Q == 0)
    for q, k in ((2, 0), (0, 0), (2, 65), (0, 65), (2, 0xFFFFFFFF), (1 << 31, 1), (1 << 25, 64), (1 << 58, 64), (0x80000000 // 3 + 1, 3)):
        assert lib.sa_hip_token_index_top_batch_device(h, D, q, k, 0, D, D, D) == -1, (q, k)
        assert lib.sa_hip_token_index_top_batch(h, p, o, q, 0, 0, 1, k, 0, s, y, c, hd) == -1, (q, k)
    assert lib.sa_hip_token_index_top_batch_device(h, D, 2, 65, 0, D, D, D) == -1 and b"64" in lib.sa_hip_last_error()
    # m == 0, Q * m >= 2^31
    for q, m in ((2, 0), (0, 0), (1 << 31, 1), (1 << 20, 1 << 11), (1, 0xFFFFFFFF), (1 << 40, 1 << 30)):
        assert lib.sa_hip_token_index_sample_batch_device(h, D, q, D, m, D, D) == -1, (q, m)
        assert lib.sa_hip_token_index_sample_batch(h, p, o, q, 0, 0, 1, dr, m, s, y, c) == -1, (q, m)
    assert b"2^31" in lib.sa_hip_last_error()
    # NULL arguments (spans of the host forms and ranks may be NULL: not among them)
    for args in ((None, D, D, D), (D, None, D, D), (D, D, None, D), (D, D, D, None)):
        assert lib.sa_hip_token_index_top_batch_device(h, args[0], 2, 4, 0, *args[1:]) == -1, args
    for args in ((None, c, hd), (y, None, hd), (y, c, None)):
        assert lib.sa_hip_token_index_top_batch(h, p, o, 2, 0, 0, 1, 4, 0, s, *args) == -1, args
    assert lib.sa_hip_token_index_top_batch(h, p, None, 2, 0, 0, 1, 4, 0, s, y, c, hd) == -1
    assert lib.sa_hip_token_index_top_batch(h, None, o, 2, 0, 0, 1, 4, 0, s, y, c, hd) == -1            # symbols without a buffer
    for args in ((None, D, D), (D, None, D), (D, D, None)):
        assert lib.sa_hip_token_index_sample_batch_device(h, args[0], 2, args[1], 1, args[2], D) == -1, args
    assert lib.sa_hip_token_index_sample_batch(h, p, None, 2, 0, 0, 1, dr, 1, s, y, c) == -1
    assert lib.sa_hip_token_index_sample_batch(h, p, o, 2, 0, 0, 1, None, 1, s, y, c) == -1
    assert lib.sa_hip_token_index_sample_batch(h, p, o, 2, 0, 0, 1, dr, 1, s, None, c) == -1
    assert b"NULL" in lib.sa_hip_last_error()
    # descending offsets
    assert lib.sa_hip_token_index_top_batch(h, p, down.ctypes.data, 2, 1, 0, 1, 4, 0, s, y, c, hd) == -1
    assert b"descend" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_sample_batch(h, p, down.ctypes.data, 2, 1, 0, 1, dr, 1, s, y, c) == -1
    # Q == 0 with good arguments: a no-op that touches nothing
    assert lib.sa_hip_token_index_top_batch_device(h, None, 0, 64, 7, None, None, None) == 0
    assert lib.sa_hip_token_index_top_batch(h, None, None, 0, 1, 0, 1, 1, 0, None, None, None, None) == 0
    assert lib.sa_hip_token_index_sample_batch_device(h, None, 0, None, 3, None, None) == 0
    assert lib.sa_hip_token_index_sample_batch(h, None, None, 0, 1, 0, 1, None, 3, None, None, None) == 0


def test_top_no_device_is_minus_three(capi):
    lib = capi.lib()
    if lib.sa_hip_device_count() >= 1:
        return                                                     # (with a device: test_gpu_token_top.py)
    import suffixarray_amd
    with pytest.raises(capi.SaHipError) as e:
        suffixarray_amd.TokenIndex([5, 1, 5, 1, 5]).top_next_tokens([[5]])
    assert e.value.code == -3


def _pattern(e, cfg, i):
    c, length = e["ctx"][i], int(e["spans"][cfg][i, 2])
    return c[len(c) - length:]


@pytest.mark.parametrize("name", tt.TEXTS)
def test_top_and_sample_models_against_window_counts(name):
    """per distinct span of the text: the entries are the brute-force window counts; the top-k model is their k largest under
    (-count, symbol) for k below, at and above their number, with and without a budget; every edge draw of the sample model lands
    on the symbol that the cumulative window counts give, and the draws of a span hit every symbol"""
    e = tt.expected(name)
    t, sa = e["t"], e["sa"]
    seen = set()
    for cfg in nc.CONFIGS:
        for i, span in enumerate(e["spans"][cfg].tolist()):
            if tuple(span[:3]) in seen:
                continue
            seen.add(tuple(span[:3]))
            want = tt.window_counter(t, _pattern(e, cfg, i)) if span[1] else {}
            sym, cnt = e["entries"][cfg][i]
            assert dict(zip(sym.tolist(), cnt.tolist())) == want, (name, cfg, i)
            total, d = span[1] - span[3], len(want)
            assert total == sum(want.values()), (name, cfg, i)
            brute = sorted(want.items(), key=lambda p: (-p[1], p[0]))
            for k in {1, max(d - 1, 1), max(d, 1), d + 1, 8, 64}:
                assert tt.top_of((sym, cnt), k) == brute[:k], (name, cfg, i, k)
            # a budget keeps the smallest symbols: the first `budget` of the ranks in ascending symbol order
            flat = np.repeat(sym, cnt)
            for budget in {1, 63, 64, 65, max(total - 1, 1), total + 1}:
                ws, wc = tt.walked_entries(t, sa, span, budget)
                cut = Counter(flat[:budget].tolist())
                assert dict(zip(ws.tolist(), wc.tolist())) == dict(cut), (name, cfg, i, budget)
            assert tt.sample_of(t, sa, span, 0)[0] == (int(flat[0]) if total else -1), (name, cfg, i)
            if total == 0:
                assert tt.sample_of(t, sa, span, 2 ** 64 - 1) == (-1, 0xFFFFFFFF), (name, cfg, i)
                continue
            draws = tt.edge_draws(cnt)
            assert len(draws) == 2 * d
            hit = []
            for dr in draws:
                s, rank = tt.sample_of(t, sa, span, dr)
                # exact rational arithmetic: the rank inside the span is floor(draw * total / 2^64)
                r = rank - span[0] - span[3]
                assert 0 <= r < total and r * 2 ** 64 <= dr * total < (r + 1) * 2 ** 64, (name, cfg, i, dr)
                assert s == int(flat[r]), (name, cfg, i, dr)
                hit.append((r, s))
            assert hit[0][0] == 0 and hit[1][0] == total - 1, (name, cfg, i)
            edges = np.cumsum(cnt)[:-1].tolist()
            assert [h[0] for h in hit[2::2]] == edges and [h[0] for h in hit[3::2]] == [j - 1 for j in edges], (name, cfg, i)
            assert {s for _, s in hit} == set(want), (name, cfg, i)
    assert seen


def test_top_planted_texts_hold_their_runs():
    for name in tt.NEW_TEXTS:
        i, span = tt.run_span(name)
        e = tt.expected(name)
        sym, cnt = e["entries"][(0, 0, 1)][i]
        assert sym.tolist() == tt.run_symbols(name) and cnt.tolist() == list(tt.RUN_TEXTS[name]), name
        assert span[3] == 1 and span[1] == sum(tt.RUN_TEXTS[name]) + 1 and 200 < e["t"].size < 10000, name
    i, span = tt.run_span("planted")
    assert tt.expected("planted")["entries"][(0, 0, 1)][i][1].tolist() == list(nc.RUNS)           # the ascending runs
    desc, ties, many = tt.RUN_TEXTS["top_desc"], tt.RUN_TEXTS["top_ties"], tt.RUN_TEXTS["top_many"]
    assert list(desc) == sorted(desc, reverse=True) and len(set(desc)) == len(desc) > 8
    assert list(nc.RUNS) == sorted(nc.RUNS) and len(nc.RUNS) > 8
    assert len(ties) == 130 > 2 * tt.WINDOW and set(ties) == {1}
    for name, at in (("top_edge64", 64), ("top_edge128", 128)):
        r = tt.RUN_TEXTS[name]
        assert r[0] + r[1] == at and r[1] == max(r) and r[0] < tt.WINDOW                           # starts in window 0, ends at the edge
    assert tt.RUN_TEXTS["top_last"][-1] == max(tt.RUN_TEXTS["top_last"])
    j = tt.RUN_TEXTS["top_jump"]
    assert j[2] == 4097 and 0 < sum(j[:2]) and sum(j[3:]) > 0
    assert len(many) >= 65 and len(set(many)) == len(many)
    # the tie-break at the k-th place: 130 runs of one rank each give the k smallest symbols
    e = tt.expected("top_ties")
    i, _ = tt.run_span("top_ties")
    assert tt.top_of(e["entries"][(0, 0, 1)][i], 8) == [(7 * j, 1) for j in range(8)]


def test_top_hand_worked_banana():
    """"banana" as tokens (b = 1, a = 0, n = 2), SA [5, 3, 1, 0, 4, 2]: the empty context is followed by a x3, n x2, b x1"""
    from test_int_cpu import model_sa
    t = np.array([1, 0, 2, 0, 2, 0], np.int32)
    sa = model_sa(t)
    span = (0, 6, 0, 0)
    ent = nc.entries_a(t, sa, span)
    assert tt.top_of(ent, 2) == [(0, 3), (2, 2)] and tt.top_of(ent, 64) == [(0, 3), (2, 2), (1, 1)]
    assert tt.top_of(tt.walked_entries(t, sa, span, 4), 1) == [(0, 3)] and tt.top_of(tt.walked_entries(t, sa, span, 5), 3) == [(0, 3), (1, 1), (2, 1)]
    # ranks 0..2 are a, 3 is b, 4..5 are n: a draw below 2^63 lands in the first three ranks
    assert [tt.sample_of(t, sa, span, d) for d in (0, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1)] == [(0, 0), (0, 2), (1, 3), (2, 5)]
    assert tt.edge_draws([3, 1, 2]) == [0, 2 ** 64 - 1, 2 ** 63, 2 ** 63 - 1, -((-4 << 64) // 6), -((-4 << 64) // 6) - 1]
    # [0] = "a": the ended suffix stands first and is stepped over; n n follow
    assert tt.sample_of(t, sa, (0, 3, 1, 1), 0) == (2, 1) and tt.sample_of(t, sa, (0, 3, 1, 1), 2 ** 64 - 1) == (2, 2)
    assert tt.sample_of(t, sa, (0, 1, 1, 1), 5) == (-1, 0xFFFFFFFF)
