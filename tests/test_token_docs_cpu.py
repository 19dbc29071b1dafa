"""Documents of a token index without a GPU: every new entry point is declared, exported and bound; the three new structs match the
C compiler's view of the header; every argument error that is answered before a HIP call is answered with -1 on a handle that is
only an address; the two CPU models that test_gpu_token_docs.py measures the device against (token_doc_cases.py) agree with each
other, with hand-counted cases and with the closed forms of the all-equal text; the case lists hold every edge they are there for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_cases as tc
import token_doc_cases as dc
import token_next_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_index_set_documents", "sa_hip_token_index_get_doc_range", "sa_hip_token_index_docs_info",
       "sa_hip_token_index_locate_batch_device", "sa_hip_token_index_locate_batch", "sa_hip_token_index_docs_batch_device",
       "sa_hip_token_index_docs_batch"]


def test_doc_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int, name
    for name in ("set_documents", "doc_range", "docs_info", "locate_batch", "locate_batch_device", "docs_batch", "docs_batch_device"):
        assert callable(getattr(capi.TokenIndex, name)), name
    from suffixarray_amd import token_index
    for name in ("set_documents", "locate", "documents", "document_counts"):
        assert callable(getattr(token_index.TokenIndex, name)), name
    import inspect
    assert list(inspect.signature(token_index.TokenIndex.__init__).parameters) == ["self", "tokens", "k", "device", "doc_starts"]
    for dt, cls, size in ((capi.LOCATE_DTYPE, capi.TokenLocate, 8), (capi.DOCS_DTYPE, capi.TokenDocs, 16)):
        assert dt.itemsize == C.sizeof(cls) == size
        assert dt.names == tuple(f for f, _ in cls._fields_)
        assert [dt.fields[f][1] for f in dt.names] == [getattr(cls, f).offset for f in dt.names]
    assert os.path.exists(os.path.join(ROOT, "suffixarray_amd", "csrc", "token_docs.hpp"))
    unroll = int(re.search(r"constexpr int DOC_UNROLL = (\d+);", open(os.path.join(ROOT, "suffixarray_amd", "csrc", "token_docs.hpp")).read()).group(1))
    assert unroll == dc.UNROLL


@pytest.mark.parametrize("struct, cls, fields", [
    ("sa_hip_token_locate", "TokenLocate", ["written", "count"]),
    ("sa_hip_token_docs", "TokenDocs", ["written", "examined", "distinct", "count"]),
    ("sa_hip_token_docs_info", "TokenDocsInfo", ["documents", "bytes", "prepare_ms", "da_ms", "sort_ms", "pv_ms", "sort_passes", "reserved",
                                                 "locate_q", "locate_ms", "docs_q", "docs_ms", "examined"]),
])
def test_doc_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields):
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


def test_doc_argument_errors_before_any_device_call(capi):
    """the handle is an address that holds nothing: every call below must return before it is looked at"""
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    spans = np.zeros(2, capi.SPAN_DTYPE)
    docs, offs = np.zeros(8, np.int32), np.zeros(8, np.int32)
    lh, dh = np.zeros(2, capi.LOCATE_DTYPE), np.zeros(2, capi.DOCS_DTYPE)
    p, o, s, d, f, l, g = (a.ctypes.data for a in (pat, off, spans, docs, offs, lh, dh))
    D = 1 << 20                                                    # "device pointers": never touched
    # NULL handle
    tab = np.array([0, 2], np.int32)
    assert lib.sa_hip_token_index_set_documents(None, tab.ctypes.data, 2) == -1
    assert b"sa_hip_token_index_set_documents" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_get_doc_range(None, 0, 1, d, f) == -1
    assert lib.sa_hip_token_index_docs_info(None, C.byref(capi.TokenDocsInfo())) == -1
    assert lib.sa_hip_token_index_docs_info(h, None) == -1
    assert lib.sa_hip_token_index_locate_batch_device(None, D, 2, 4, D, D, D) == -1
    assert lib.sa_hip_token_index_locate_batch(None, p, o, 2, 4, s, d, f, l) == -1
    assert lib.sa_hip_token_index_docs_batch_device(None, D, 2, 4, 0, D, D, D) == -1
    assert lib.sa_hip_token_index_docs_batch(None, p, o, 2, 0, 0, 0, 4, 0, s, d, f, g) == -1
    assert b"sa_hip_token_index_docs_batch" in lib.sa_hip_last_error()
    # the table: what can be told without the handle's n
    assert lib.sa_hip_token_index_set_documents(h, None, 3) == -1                                     # D >= 1 without a table
    assert lib.sa_hip_token_index_set_documents(h, tab.ctypes.data, 0) == -1                          # a table with D == 0
    for bad, word in (([1, 2], b"[0]"), ([-1, 2], b"[0]"), ([0, 5, 4], b"descend"), ([0, 3, 3, 2], b"descend"), ([0, -1], b"descend")):
        b = np.array(bad, np.int32)
        assert lib.sa_hip_token_index_set_documents(h, b.ctypes.data, b.size) == -1, bad
        assert word in lib.sa_hip_last_error(), (bad, lib.sa_hip_last_error())
    # mode and need_next are 0 or 1
    for mode, need in ((2, 1), (-1, 1), (0, 2), (1, -1)):
        assert lib.sa_hip_token_index_docs_batch(h, p, o, 2, mode, 0, need, 4, 0, s, d, f, g) == -1, (mode, need)
        assert lib.sa_hip_token_index_docs_batch(h, p, o, 0, mode, 0, need, 4, 0, s, d, f, g) == -1, (mode, need)   # also with Q == 0
    # cap == 0 in locate (the documents calls allow it); Q * cap >= 2^31 in all four
    assert lib.sa_hip_token_index_locate_batch_device(h, D, 2, 0, D, D, D) == -1
    assert b"cap" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_locate_batch(h, p, o, 2, 0, s, d, f, l) == -1
    assert lib.sa_hip_token_index_locate_batch(h, p, o, 0, 0, s, d, f, l) == -1                      # also with Q == 0
    for q, cap in ((1 << 31, 1), (1 << 20, 1 << 11), (1, 0xFFFFFFFF), (3, 0x80000000 // 3 + 1)):
        assert lib.sa_hip_token_index_locate_batch_device(h, D, q, cap, D, D, D) == -1, (q, cap)
        assert lib.sa_hip_token_index_locate_batch(h, p, o, q, cap, s, d, f, l) == -1, (q, cap)
        assert lib.sa_hip_token_index_docs_batch_device(h, D, q, cap, 0, D, D, D) == -1, (q, cap)
        assert lib.sa_hip_token_index_docs_batch(h, p, o, q, 0, 0, 0, cap, 0, s, d, f, g) == -1, (q, cap)
    assert b"2^31" in lib.sa_hip_last_error()
    # NULL required pointers (spans of the host forms may be NULL: not among them)
    for args in ((None, D, D, D), (D, None, D, D), (D, D, None, D), (D, D, D, None)):
        assert lib.sa_hip_token_index_locate_batch_device(h, args[0], 2, 4, *args[1:]) == -1, args
        assert lib.sa_hip_token_index_docs_batch_device(h, args[0], 2, 4, 0, *args[1:]) == -1, args
    assert lib.sa_hip_token_index_docs_batch_device(h, None, 2, 0, 0, None, None, D) == -1           # cap 0: spans and heads still
    assert lib.sa_hip_token_index_docs_batch_device(h, D, 2, 0, 0, None, None, None) == -1
    for args in ((None, f, l), (d, None, l), (d, f, None)):
        assert lib.sa_hip_token_index_locate_batch(h, p, o, 2, 4, s, *args) == -1, args
    for args in ((None, f, g), (d, None, g), (d, f, None)):
        assert lib.sa_hip_token_index_docs_batch(h, p, o, 2, 0, 0, 0, 4, 0, s, *args) == -1, args
    assert lib.sa_hip_token_index_docs_batch(h, p, o, 2, 0, 0, 0, 0, 0, s, None, None, None) == -1   # cap 0: heads still
    assert lib.sa_hip_token_index_locate_batch(h, p, None, 2, 4, s, d, f, l) == -1
    assert lib.sa_hip_token_index_docs_batch(h, p, None, 2, 0, 0, 0, 4, 0, s, d, f, g) == -1
    assert lib.sa_hip_token_index_locate_batch(h, None, o, 2, 4, s, d, f, l) == -1                   # symbols without a buffer
    assert lib.sa_hip_token_index_docs_batch(h, None, o, 2, 0, 0, 0, 4, 0, s, d, f, g) == -1
    # descending offsets
    assert lib.sa_hip_token_index_locate_batch(h, p, down.ctypes.data, 2, 4, s, d, f, l) == -1
    assert b"descend" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_docs_batch(h, p, down.ctypes.data, 2, 1, 0, 0, 4, 0, s, d, f, g) == -1
    assert b"descend" in lib.sa_hip_last_error()
    # Q == 0 with good arguments: a no-op that touches nothing
    assert lib.sa_hip_token_index_locate_batch_device(h, None, 0, 4, None, None, None) == 0
    assert lib.sa_hip_token_index_locate_batch(h, None, None, 0, 4, None, None, None, None) == 0
    assert lib.sa_hip_token_index_docs_batch_device(h, None, 0, 4, 0, None, None, None) == 0
    assert lib.sa_hip_token_index_docs_batch_device(h, None, 0, 0, 7, None, None, None) == 0
    assert lib.sa_hip_token_index_docs_batch(h, None, None, 0, 1, 0, 1, 0, 0, None, None, None, None) == 0


def test_docs_without_a_device_fail_loudly(capi):
    """no handle without a device, hence no documents, and no answer from anywhere else"""
    import suffixarray_amd
    if capi.lib().sa_hip_device_count() >= 1:
        with pytest.raises(capi.SaHipError) as e:
            suffixarray_amd.TokenIndex([5, 1, 5], device=1 << 20, doc_starts=[0, 2])
        assert e.value.code == -3
        return
    with pytest.raises(capi.SaHipError) as e:
        suffixarray_amd.TokenIndex([5, 1, 5], doc_starts=[0, 2])
    assert e.value.code == -3


# ---- the models ----------------------------------------------------------------------------------------------------------------

HAND_T = [1, 2, 1, 2, 3, 1, 2]
HAND_STARTS = [0, 0, 2, 5, 5, 7]          # 0 empty at the front, 1 = [1 2], 2 = [1 2 3], 3 empty in the middle, 4 = [1 2], 5 empty at the end


def test_models_on_a_hand_counted_text():
    t, starts = np.array(HAND_T, np.int32), np.array(HAND_STARTS, np.int32)
    sa = dc.model_sa(t)
    assert sa.tolist() == [5, 0, 2, 6, 1, 3, 4]
    assert dc.doc_of(starts, np.arange(7)).tolist() == [1, 1, 2, 2, 2, 4, 4]                          # an empty document owns nothing
    da, pv = dc.model_da_pv(sa, starts)
    assert da.tolist() == [4, 1, 2, 4, 1, 2, 2] and pv.tolist() == [-1, -1, -1, 0, 1, 2, 5]
    # [1, 2]: ranks 0 .. 2, one occurrence in each of three documents
    assert dc.docs_a(sa, da, starts, 0, 3, 16, 0) == ((3, 3, 3, 3), [(4, 0), (1, 0), (2, 0)])
    assert dc.docs_a(sa, da, starts, 0, 3, 2, 0) == ((2, 3, 3, 3), [(4, 0), (1, 0)])
    assert dc.docs_a(sa, da, starts, 0, 3, 0, 0) == ((0, 3, 3, 3), [])
    assert dc.docs_a(sa, da, starts, 0, 3, 16, 2) == ((2, 2, 2, 3), [(4, 0), (1, 0)])
    assert dc.model_b(t, starts, [1, 2]) == (3, 3, [(1, 0), (2, 0), (4, 0)])
    # the whole array: 7 ranks, 3 documents; [2]: ranks 3 .. 5; [2, 1] runs over the boundary of document 1 and stays its hit
    assert dc.docs_a(sa, da, starts, 0, 7, 16, 0) == ((3, 7, 3, 7), [(4, 0), (1, 0), (2, 0)])
    assert dc.docs_a(sa, da, starts, 3, 3, 16, 0) == ((3, 3, 3, 3), [(4, 1), (1, 1), (2, 1)])
    assert dc.docs_a(sa, da, starts, 5, 2, 16, 0) == ((1, 2, 1, 2), [(2, 1)])                         # ranks 5, 6: document 2 twice
    assert dc.model_b(t, starts, [2, 1]) == (1, 1, [(1, 1)])
    assert dc.model_b(t, starts, [3]) == (1, 1, [(2, 2)]) and dc.model_b(t, starts, []) [:2] == (7, 3)
    assert dc.locate_a(sa, da, starts, 3, 3, 2) == ((2, 3), [(4, 1), (1, 1)])
    # D == 1, and one token per document
    da1, pv1 = dc.model_da_pv(sa, [0])
    assert da1.tolist() == [0] * 7 and pv1.tolist() == [-1, 0, 1, 2, 3, 4, 5]
    dan, pvn = dc.model_da_pv(sa, dc.one_token_each(7))
    assert dan.tolist() == sa.tolist() and pvn.tolist() == [-1] * 7
    assert dc.docs_a(sa, dan, dc.one_token_each(7), 0, 7, 4, 0) == ((4, 7, 7, 7), [(5, 0), (0, 0), (2, 0), (6, 0)])
    # the criterion the device counts by: r is a head of [a, a + e) iff PV[r] < a
    for a in range(7):
        for e in range(8 - a):
            assert dc.docs_a(sa, da, starts, a, e, 0, 0)[0][2] == int((pv[a:a + e] < a).sum()), (a, e)


@pytest.mark.parametrize("name", list(dc.RANDOM))
def test_models_agree_on_the_random_texts(name):
    c = dc.random_case(name)
    e = nc.expected(name)
    t, sa, starts, da, pv = c["t"], c["sa"], c["starts"], c["da"], c["pv"]
    assert np.array_equal(sa, e["sa"]) and t.size <= 70000
    assert (np.diff(starts) == 0).any() and starts[0] == 0 and starts[-1] == t.size - 1              # empty documents; the last one owns a token
    assert int(da.max()) == starts.size - 1
    for r in range(0, sa.size, 997):                                                                  # PV by its definition, sampled
        same = np.flatnonzero(da[:r] == da[r])
        assert pv[r] == (same[-1] if same.size else -1), r
    for cfg in ((0, 0, 1), (1, 0, 0)):
        for ctx, sp in zip(e["ctx"], e["spans"][cfg].tolist()):
            first, count, length = sp[0], sp[1], sp[2]
            head, ent = dc.docs_a(sa, da, starts, first, count, 16, 0)
            cnt, distinct, occ = dc.model_b(t, starts, ctx[len(ctx) - length:])
            assert (cnt, distinct) == (count, head[2]), (name, cfg, ctx[:6])
            assert head[2] == int((pv[first:first + count] < first).sum()), (name, cfg, ctx[:6])
            assert set(ent) <= set(occ), (name, cfg, ctx[:6])
            lh, loc = dc.locate_a(sa, da, starts, first, count, 1 << 20)
            assert sorted(loc) == occ, (name, cfg, ctx[:6])


def test_all_equal_text_closed_forms_and_edges():
    assert np.array_equal(dc.equal_sa(), dc.model_sa(dc.equal_text()))
    assert dc.N_EQ <= 70000 and max(dc.COUNTS) <= dc.N_EQ
    step = 64 * dc.UNROLL
    assert {0, 1, 63, 64, 65, 127, 128, 129, step - 1, step, step + 1} <= set(dc.COUNTS) and max(dc.COUNTS) > 4 * step
    assert {0, 1, 16, 64} == set(dc.CAPS)
    assert {0, 1, 64, 65} <= set(dc.BUDGETS) and all({c - 1, c, c + 1} - {0, -1} <= set(dc.BUDGETS) | {0} for c in dc.COUNTS if c)
    for Ld in dc.LDS:
        c = dc.equal_case(Ld)
        sa, starts, da, pv = c["sa"], c["starts"], c["da"], c["pv"]
        assert np.array_equal(da, (dc.N_EQ - 1 - np.arange(dc.N_EQ)) // Ld)
        assert np.array_equal(pv, np.where(np.concatenate([[True], da[1:] != da[:-1]]), -1, np.arange(dc.N_EQ) - 1))
        spans = dc.equal_spans(Ld)
        assert {(0, k) for k in dc.COUNTS} <= set(spans) and {(dc.N_EQ - k, k) for k in dc.COUNTS} <= set(spans)
        assert all(f + k <= dc.N_EQ for f, k in spans)
        mid = dc.equal_mid(Ld)
        if Ld >= 3:
            assert pv[mid] == mid - 1 and pv[mid + 1] == mid                                         # just outside: a head; inside: none
            assert dc.docs_a(sa, da, starts, mid, 2, 16, 0)[0][2] == 1
        for budget in (0, 1, 64, 65, 256, 1024, 1026):
            for f, k in spans:
                head, ent = dc.docs_a(sa, da, starts, f, k, 16, budget)
                assert head[2] == dc.equal_distinct(Ld, f, head[1]) and head[1] == (min(k, budget) if budget else k), (Ld, f, k, budget)
                if k:                                                                                 # the documents descend with the rank
                    assert [d for d, _ in ent] == list(range(int(da[f]), int(da[f]) - head[0], -1)), (Ld, f, k, budget)
    # a list that fills exactly at a window's last lane, and one that fills one head later
    c = dc.equal_case(1)
    assert dc.docs_a(c["sa"], c["da"], c["starts"], 0, 64, 64, 0)[0] == (64, 64, 64, 64)
    assert dc.docs_a(c["sa"], c["da"], c["starts"], 0, 65, 64, 0)[0] == (64, 65, 65, 65)
    c = dc.equal_case(64)                                                                             # ... and with one head per window
    assert dc.docs_a(c["sa"], c["da"], c["starts"], 0, 1025, 16, 0)[0] == (16, 1025, 17, 1025)


def test_tables_hold_their_edges():
    n = 5000
    w = dc.with_empties(n)
    assert w[0] == w[1] == w[2] == 0 and (w[3] == w[4] == w[5]) and w[-1] == w[-2] == n               # front, middle, end
    own = set(dc.doc_of(w, np.arange(n)).tolist())
    assert own == {2, 5, 6}                                                                           # the LARGEST d with starts[d] <= p
    for D in (2, 255, 256, 257, 65536, 65537):
        s = dc.rand_table(n, D, 1)
        assert s.size == D and s[0] == 0 and (np.diff(s) >= 0).all() and s.max() < n
        assert int(dc.doc_of(s, np.arange(n)).max()) == D - 1                                         # the sort sees its top key bit
    assert tc.pack([[1], [2, 3]])[1].tolist() == [0, 1, 3]
