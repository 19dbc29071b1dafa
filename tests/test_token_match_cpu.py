"""Matching statistics of the token index without a GPU: the five entry points are declared, exported and bound and the class
methods exist; the two new structs match the C compiler's view of the header; every argument error is answered with -1 before the
handle or a device is touched, and a missing device is -3; the two CPU models that test_gpu_token_match.py measures the device
against (token_match_cases.py) agree on the whole case list; end(j) never decreases; and a hand-worked example pins what the words
of the contract mean."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_match_cases as mc
from test_int_cpu import model_sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_index_match_batch_device", "sa_hip_token_index_match_docs_batch_device", "sa_hip_token_index_match_batch",
       "sa_hip_token_index_match_docs_batch", "sa_hip_token_index_match_info"]


def test_match_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    for name in ("match_batch", "match_batch_device", "match_docs_batch", "match_docs_batch_device", "match_info"):
        assert callable(getattr(capi.TokenIndex, name)), name
    from suffixarray_amd import token_index
    for name in ("matching_statistics", "matched_spans", "coverage"):
        assert callable(getattr(token_index.TokenIndex, name)), name
    assert capi.MATCH_HEAD_DTYPE.itemsize == C.sizeof(capi.TokenMatchHead) == 16
    assert capi.MATCH_HEAD_DTYPE.names == tuple(f for f, _ in capi.TokenMatchHead._fields_)


@pytest.mark.parametrize("struct, cls, fields", [
    ("sa_hip_token_match_head", "TokenMatchHead", ["written", "maximal", "longest", "covered"]),
    ("sa_hip_token_match_info", "TokenMatchInfo", ["q", "positions", "match_ms", "docs_ms"]),
])
def test_match_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields):
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


def test_match_argument_errors_before_any_device_call(capi):
    """every refusal comes before the handle is touched: the handle of these calls is an address that holds nothing"""
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    huge = np.array([0, 2, 1 << 31], np.uint64)                    # total >= 2^31: refused before a symbol is read
    spans, outs = np.zeros(4, capi.SPAN_DTYPE), np.zeros(8, capi.SPAN_DTYPE)
    pos, heads = np.zeros(8, np.uint32), np.zeros(2, capi.MATCH_HEAD_DTYPE)
    p, o, s, ps, os_, hd = (a.ctypes.data for a in (pat, off, spans, pos, outs, heads))
    D = 1 << 20                                                    # "device pointers": never touched
    # NULL handle
    assert lib.sa_hip_token_index_match_batch(None, p, o, 2, 0, s) == -1
    assert b"sa_hip_token_index_match_batch" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_match_batch_device(None, D, D, 2, 4, 0, D) == -1
    assert lib.sa_hip_token_index_match_docs_batch_device(None, D, D, 2, 1, 4, D, D, D) == -1
    assert lib.sa_hip_token_index_match_docs_batch(None, p, o, 2, 0, 1, 4, s, ps, os_, hd) == -1
    assert lib.sa_hip_token_index_match_info(None, C.byref(capi.TokenMatchInfo())) == -1
    assert lib.sa_hip_token_index_match_info(h, None) == -1
    # min_length == 0
    assert lib.sa_hip_token_index_match_docs_batch_device(h, D, D, 2, 0, 4, D, D, D) == -1
    assert b"min_length" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_match_docs_batch(h, p, o, 2, 0, 0, 4, s, ps, os_, hd) == -1
    assert lib.sa_hip_token_index_match_docs_batch(h, p, o, 0, 0, 0, 4, s, ps, os_, hd) == -1                 # also with Q == 0
    # total >= 2^31
    for total in (1 << 31, (1 << 31) + 5, 1 << 40, (1 << 64) - 1):
        assert lib.sa_hip_token_index_match_batch_device(h, D, D, 2, total, 0, D) == -1, total
    assert b"2^31" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_match_batch(h, p, huge.ctypes.data, 2, 0, s) == -1
    assert b"2^31" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_match_docs_batch(h, p, huge.ctypes.data, 2, 0, 1, 4, s, ps, os_, hd) == -1
    # Q * cap >= 2^31
    for q, cap in ((1 << 31, 1), (1 << 20, 1 << 11), (1, 0xFFFFFFFF), (3, 0x80000000 // 3 + 1)):
        assert lib.sa_hip_token_index_match_docs_batch_device(h, D, D, q, 1, cap, D, D, D) == -1, (q, cap)
        assert lib.sa_hip_token_index_match_docs_batch(h, p, o, q, 0, 1, cap, s, ps, os_, hd) == -1, (q, cap)
    assert b"2^31" in lib.sa_hip_last_error()
    # NULL arguments (spans of match_docs_batch may be NULL, positions and out_spans with cap == 0: not among them)
    assert lib.sa_hip_token_index_match_batch(h, p, None, 2, 0, s) == -1
    assert lib.sa_hip_token_index_match_batch(h, p, o, 2, 0, None) == -1
    assert lib.sa_hip_token_index_match_batch(h, None, o, 2, 0, s) == -1                                        # symbols without a buffer
    for args in ((None, D, D), (D, None, D), (D, D, None)):
        assert lib.sa_hip_token_index_match_batch_device(h, args[0], args[1], 2, 4, 0, args[2]) == -1, args
    for args in ((None, D, D, D), (D, None, D, D), (D, D, None, D), (D, D, D, None)):
        assert lib.sa_hip_token_index_match_docs_batch_device(h, D, args[0], 2, 1, 4, *args[1:]) == -1, args
    assert lib.sa_hip_token_index_match_docs_batch_device(h, D, D, 2, 1, 0, None, None, None) == -1             # heads, also with cap == 0
    for args in ((None, os_, hd), (ps, None, hd), (ps, os_, None)):
        assert lib.sa_hip_token_index_match_docs_batch(h, p, o, 2, 0, 1, 4, s, *args) == -1, args
    assert lib.sa_hip_token_index_match_docs_batch(h, p, None, 2, 0, 1, 4, s, ps, os_, hd) == -1
    assert lib.sa_hip_token_index_match_docs_batch(h, None, o, 2, 0, 1, 4, s, ps, os_, hd) == -1
    assert lib.sa_hip_token_index_match_docs_batch(h, p, o, 2, 0, 1, 0, None, None, None, None) == -1
    # descending offsets
    assert lib.sa_hip_token_index_match_batch(h, p, down.ctypes.data, 2, 0, s) == -1
    assert b"descend" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_match_docs_batch(h, p, down.ctypes.data, 2, 0, 1, 4, s, ps, os_, hd) == -1
    assert b"descend" in lib.sa_hip_last_error()
    # Q == 0 with good arguments: a no-op that touches nothing
    assert lib.sa_hip_token_index_match_batch(h, None, None, 0, 0, None) == 0
    assert lib.sa_hip_token_index_match_batch_device(h, None, None, 0, 0, 0, None) == 0
    assert lib.sa_hip_token_index_match_docs_batch_device(h, None, None, 0, 1, 4, None, None, None) == 0
    assert lib.sa_hip_token_index_match_docs_batch(h, None, None, 0, 7, 1, 4, None, None, None, None) == 0


def test_match_no_device_is_minus_three(capi):
    """no handle without a device, so no answer from anywhere else: the class raises -3 before a match can be asked"""
    lib = capi.lib()
    if lib.sa_hip_device_count() >= 1:
        h = C.c_void_p(0x1234)
        t = np.array([3, 1, 2, 1], np.int32)
        assert lib.sa_hip_token_index_build(C.byref(h), t.ctypes.data, 4, 4, 1 << 20) == -3 and not h.value
        return
    import suffixarray_amd
    for call in (lambda ti: ti.matching_statistics([[5, 1]]), lambda ti: ti.matched_spans([[5, 1]], 1), lambda ti: ti.coverage([[5, 1]], 1)):
        with pytest.raises(capi.SaHipError) as e:
            call(suffixarray_amd.TokenIndex([5, 1, 5, 1, 5]))
        assert e.value.code == -3
    with pytest.raises(capi.SaHipError) as e:
        capi.TokenIndex.build([1, 2, 3]).match_docs_batch([[1]])
    assert e.value.code == -3


def test_match_models_agree_on_the_case_list():
    positions, docs, hits, partial, capped, several = 0, 0, 0, 0, 0, 0
    for name in mc.TEXTS:
        e, b = mc.expected(name), mc.expected_b(name)
        n = len(e["t"])
        for (batch, M), sp in e["spans"].items():
            where = (name, batch, M)
            dl = e["batches"][batch]
            bad = np.flatnonzero((sp[:, 1:].astype(np.int64) != b[batch, M]).any(axis=1))
            assert bad.size == 0, (where, bad[:5], sp[bad[:5]].tolist(), b[batch, M][bad[:5]].tolist())
            # end(j) never decreases, never passes its document's end, and the length respects the three caps
            base = np.concatenate([[0], np.cumsum([len(d) for d in dl])]).astype(np.int64)
            doc_end = np.repeat(base[1:], np.diff(base))
            j = np.arange(sp.shape[0], dtype=np.int64)
            end = j + sp[:, 2]
            assert (np.diff(end) >= 0).all() and (end <= doc_end).all(), where
            assert (sp[:, 2] <= min(M or n, n)).all(), where
            for mlen in mc.MIN_LENGTHS:
                ha, hb = mc.heads_a(sp[:, 2], dl, mlen), mc.heads_b(sp[:, 2], dl, mlen)
                assert ha == hb, (where, mlen, [(x, y) for x, y in zip(ha, hb) if x != y][:2])
                several += sum(h[1][0] > 1 for h in ha)
            positions += sp.shape[0]
            docs += len(dl)
            hits += int((sp[:, 2] > 0).sum())
            partial += int(((sp[:, 2] > 0) & (end < doc_end) & (sp[:, 2] < (M or n))).sum())
            capped += int((M > 0) and (sp[:, 2] == M).sum())
    assert positions > 100000 and docs > 2000 and hits > 50000 and partial > 10000 and capped > 10000 and several > 1000


def test_end_is_non_decreasing_under_the_cap_and_across_documents():
    """fact 2 where it could fail: a cap that cuts a long match, and a document that ends inside one"""
    e = mc.expected("rand_k1000")
    tl = [int(v) for v in e["t"]]
    docs = [tl[100:140], tl[130:131], [], tl[500:530] + [mc.NONE] + tl[505:520]]
    sl = [int(v) for v in e["sa"]]
    for M in (0, 1, 2, 5, 29, 30, 31):
        sp = mc.spans_a(tl, sl, docs, M)
        end = np.arange(sp.shape[0]) + sp[:, 2]
        assert (np.diff(end.astype(np.int64)) >= 0).all(), M
        assert sp[0, 2] == min(M or 40, 40) and sp[39, 2] == 1 and sp[40, 2] == 1 and sp[41, 2] == min(M or 30, 30), (M, sp[:, 2])


def test_match_hand_worked():
    """"banana" as tokens (b = 1, a = 0, n = 2); suffixes in order: a, ana, anana, banana, na, nana = SA [5, 3, 1, 0, 4, 2].
    The query document is "anan?ba" (? = 7 occurs nowhere)"""
    t = np.array([1, 0, 2, 0, 2, 0], np.int32)
    sa = model_sa(t)
    assert sa.tolist() == [5, 3, 1, 0, 4, 2]
    tl, sl = t.tolist(), sa.tolist()
    docs = [[0, 2, 0, 2, 7, 1, 0]]
    sp = mc.spans_a(tl, sl, docs, 0)
    # "anan" is in anana alone; "nan" in nana; "an" in ana, anana; "n" in na, nana; "?" nowhere: {0, n}; "ba" in banana; "a" ends the text
    assert sp.tolist() == [[2, 1, 4, 0], [5, 1, 3, 0], [1, 2, 2, 0], [4, 2, 1, 0], [0, 6, 0, 0], [3, 1, 2, 0], [0, 3, 1, 1]]
    assert (np.arange(7) + sp[:, 2]).tolist() == [4, 4, 4, 4, 4, 7, 7]                    # end(j)
    # maximal: "anan" at 0 and "ba" at 5; the "a" at 6 ends where "ba" ends and lies inside it
    assert mc.heads_a(sp[:, 2], docs, 1) == [([(0, 0), (5, 5)], (2, 4, 6))]
    assert mc.heads_a(sp[:, 2], docs, 2) == [([(0, 0), (5, 5)], (2, 4, 6))]
    assert mc.heads_a(sp[:, 2], docs, 3) == [([(0, 0)], (1, 4, 4))]                       # longest stays 4, covered drops to "anan"
    assert mc.heads_a(sp[:, 2], docs, 5) == [([], (0, 4, 0))]
    # max_length 2: "an", "na" (which ends the text), "an", "n", nothing, "ba", "a"
    sp2 = mc.spans_a(tl, sl, docs, 2)
    assert sp2.tolist() == [[1, 2, 2, 0], [4, 2, 2, 1], [1, 2, 2, 0], [4, 2, 1, 0], [0, 6, 0, 0], [3, 1, 2, 0], [0, 3, 1, 1]]
    assert mc.heads_a(sp2[:, 2], docs, 1) == [([(0, 0), (1, 1), (2, 2), (5, 5)], (4, 2, 6))]
    # a document boundary cuts a match: "ana" | "na" -- the first document's matches end at its end
    two = [[0, 2, 0], [2, 0]]
    sp3 = mc.spans_a(tl, sl, two, 0)
    assert sp3[:, 2].tolist() == [3, 2, 1, 2, 1] and sp3[0].tolist() == [1, 2, 3, 1] and sp3[1].tolist() == [4, 2, 2, 1]
    assert mc.heads_a(sp3[:, 2], two, 1) == [([(0, 0)], (1, 3, 3)), ([(0, 3)], (1, 2, 2))]
    for d, M in ((docs, 0), (docs, 2), (two, 0), (docs, 1), (docs, 3)):
        a, b = mc.spans_a(tl, sl, d, M), mc.spans_b(t, d, M)
        assert np.array_equal(a[:, 1:].astype(np.int64), b), M
        for mlen in (1, 2, 3, 5):
            assert mc.heads_a(a[:, 2], d, mlen) == mc.heads_b(a[:, 2], d, mlen), (M, mlen)
    # the all-equal text: ms(j) = min(avail(j), M, n); 7^L is a prefix of the n - L + 1 longest suffixes, the shortest of them ends
    t5 = np.full(5, 7, np.int32)
    s5 = model_sa(t5)
    assert s5.tolist() == [4, 3, 2, 1, 0]
    eq = [[7] * 8]
    a = mc.spans_a(t5.tolist(), s5.tolist(), eq, 0)
    assert a[:, 2].tolist() == [5, 5, 5, 5, 4, 3, 2, 1] and a[:, 1].tolist() == [1, 1, 1, 1, 2, 3, 4, 5]
    assert a[:, 0].tolist() == [4, 4, 4, 4, 3, 2, 1, 0] and a[:, 3].tolist() == [1] * 8
    assert mc.heads_a(a[:, 2], eq, 1) == [([(0, 0), (1, 1), (2, 2), (3, 3)], (4, 5, 8))]
    assert mc.spans_a(t5.tolist(), s5.tolist(), eq, 3)[:, 2].tolist() == [3, 3, 3, 3, 3, 3, 2, 1]
    assert np.array_equal(mc.spans_b(t5, eq, 3), mc.spans_a(t5.tolist(), s5.tolist(), eq, 3)[:, 1:].astype(np.int64))
    # rows: what a launch with cap 1 leaves of two maximal matches
    pos, outs, hd = mc.rows([f for f, _ in mc.heads_a(sp[:, 2], docs, 1)], [h for _, h in mc.heads_a(sp[:, 2], docs, 1)], sp, 1, -7)
    assert pos.tolist() == [[0]] and outs.tolist() == [[[2, 1, 4, 0]]] and hd.tolist() == [[1, 2, 4, 6]]
