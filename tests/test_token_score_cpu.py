"""Infinity-gram scores of the token index without a GPU: the four entry points are declared, exported and bound and the class
methods exist; the three new structs match the C compiler's view of the header; every argument error is answered with -1 before the
handle or a device is touched, and a missing device is -3; the two CPU models that test_gpu_token_score.py measures the device
against (token_score_cases.py) agree on the whole case list, with and without the matching statistics; model A's own trace shows
that the case list holds every edge it was written for; the invariants hold; and a hand-worked example pins what the words of the
contract mean."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_score_cases as sc
from test_int_cpu import model_sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_index_score_batch_device", "sa_hip_token_index_score_docs_batch_device", "sa_hip_token_index_score_batch",
       "sa_hip_token_index_score_info"]


def test_score_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    for name in ("score_batch", "score_batch_device", "score_docs_batch_device", "score_info"):
        assert callable(getattr(capi.TokenIndex, name)), name
    from suffixarray_amd import token_index
    for name in ("infgram", "infgram_probs", "infgram_summary"):
        assert callable(getattr(token_index.TokenIndex, name)), name
    assert capi.SCORE_DTYPE.itemsize == C.sizeof(capi.TokenScore) == 16
    assert capi.SCORE_HEAD_DTYPE.itemsize == C.sizeof(capi.TokenScoreHead) == 24
    assert capi.SCORE_DTYPE.names == tuple(f for f, _ in capi.TokenScore._fields_)
    assert capi.SCORE_HEAD_DTYPE.names == tuple(f for f, _ in capi.TokenScoreHead._fields_)
    assert [capi.SCORE_HEAD_DTYPE.fields[f][1] for f in capi.SCORE_HEAD_DTYPE.names] == [getattr(capi.TokenScoreHead, f).offset for f in capi.SCORE_HEAD_DTYPE.names]


@pytest.mark.parametrize("struct, cls, fields, size", [
    ("sa_hip_token_score", "TokenScore", ["length", "context_count", "token_count", "first"], 16),
    ("sa_hip_token_score_head", "TokenScoreHead", ["scored", "seen", "certain", "longest", "length_sum"], 24),
    ("sa_hip_token_score_info", "TokenScoreInfo", ["q", "positions", "match_ms", "score_ms", "docs_ms"], 40),
])
def test_score_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields, size):
    S = getattr(capi, cls)
    assert [f for f, _ in S._fields_] == fields and C.sizeof(S) == size
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


def test_score_argument_errors_before_any_device_call(capi):
    """every refusal comes before the handle is touched: the handle of these calls is an address that holds nothing"""
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    huge = np.array([0, 2, 1 << 31], np.uint64)                    # total >= 2^31: refused before a symbol is read
    scores, heads = np.zeros(4, capi.SCORE_DTYPE), np.zeros(2, capi.SCORE_HEAD_DTYPE)
    p, o, s, hd = (a.ctypes.data for a in (pat, off, scores, heads))
    D = 1 << 20                                                    # "device pointers": never touched
    # NULL handle
    assert lib.sa_hip_token_index_score_batch(None, p, o, 2, 0, s, hd) == -1
    assert b"sa_hip_token_index_score_batch" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_score_batch_device(None, D, D, 2, 4, 0, D, D) == -1
    assert lib.sa_hip_token_index_score_batch_device(None, D, D, 2, 4, 0, None, D) == -1
    assert lib.sa_hip_token_index_score_docs_batch_device(None, D, D, 2, D) == -1
    assert lib.sa_hip_token_index_score_info(None, C.byref(capi.TokenScoreInfo())) == -1
    assert lib.sa_hip_token_index_score_info(h, None) == -1
    # total >= 2^31
    for total in (1 << 31, (1 << 31) + 5, 1 << 40, (1 << 64) - 1):
        assert lib.sa_hip_token_index_score_batch_device(h, D, D, 2, total, 0, D, D) == -1, total
        assert lib.sa_hip_token_index_score_batch_device(h, D, D, 2, total, 0, None, D) == -1, total
    assert b"2^31" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_score_batch(h, p, huge.ctypes.data, 2, 0, s, hd) == -1
    assert b"2^31" in lib.sa_hip_last_error()
    # NULL arguments (spans of the device form may be NULL, one of scores and heads of the host form: not among them)
    for args in ((None, D, D), (D, None, D), (D, D, None)):
        assert lib.sa_hip_token_index_score_batch_device(h, args[0], args[1], 2, 4, 0, D, args[2]) == -1, args
        assert lib.sa_hip_token_index_score_batch_device(h, args[0], args[1], 2, 4, 0, None, args[2]) == -1, args
    assert lib.sa_hip_token_index_score_docs_batch_device(h, D, None, 2, D) == -1
    assert lib.sa_hip_token_index_score_docs_batch_device(h, D, D, 2, None) == -1
    assert lib.sa_hip_token_index_score_batch(h, p, None, 2, 0, s, hd) == -1
    assert lib.sa_hip_token_index_score_batch(h, None, o, 2, 0, s, hd) == -1                                    # symbols without a buffer
    assert lib.sa_hip_token_index_score_batch(h, p, o, 2, 0, None, None) == -1                                  # both outputs
    assert b"NULL" in lib.sa_hip_last_error()
    # descending offsets
    for a, b in ((s, hd), (s, None), (None, hd)):
        assert lib.sa_hip_token_index_score_batch(h, p, down.ctypes.data, 2, 0, a, b) == -1
        assert b"descend" in lib.sa_hip_last_error()
    # Q == 0 with good arguments: a no-op that touches nothing
    assert lib.sa_hip_token_index_score_batch(h, None, None, 0, 0, None, None) == 0
    assert lib.sa_hip_token_index_score_batch_device(h, None, None, 0, 0, 0, None, None) == 0
    assert lib.sa_hip_token_index_score_docs_batch_device(h, None, None, 0, None) == 0


def test_score_no_device_is_minus_three(capi):
    """no handle without a device, so no answer from anywhere else: the class raises -3 before a score can be asked"""
    lib = capi.lib()
    if lib.sa_hip_device_count() >= 1:
        h = C.c_void_p(0x1234)
        t = np.array([3, 1, 2, 1], np.int32)
        assert lib.sa_hip_token_index_build(C.byref(h), t.ctypes.data, 4, 4, 1 << 20) == -3 and not h.value
        return
    import suffixarray_amd
    for call in (lambda ti: ti.infgram([[5, 1]]), lambda ti: ti.infgram_probs([[5, 1]]), lambda ti: ti.infgram_summary([[5, 1]])):
        with pytest.raises(capi.SaHipError) as e:
            call(suffixarray_amd.TokenIndex([5, 1, 5, 1, 5]))
        assert e.value.code == -3
    with pytest.raises(capi.SaHipError) as e:
        capi.TokenIndex.build([1, 2, 3]).score_batch([[1]])
    assert e.value.code == -3


def test_score_models_agree_on_the_case_list():
    """model A == model B for every max_length, the invariants of the contract, and -- on model A's own trace -- every edge the
    case list was written for"""
    positions = shift1 = shift3 = by_cap = by_start = missed = certain = unseen = 0
    for name in sc.names():
        e, b = sc.expected(name), sc.expected_b(name)
        n = len(e["t"])
        for M in sc.MAX_LENGTHS:
            where = (name, M)
            a, tr = e["scores"][M], e["trace"][M]
            bad = np.flatnonzero((a[:, :3].astype(np.int64) != b[M]).any(axis=1))
            assert bad.size == 0, (where, bad[:5], a[bad[:5]].tolist(), b[M][bad[:5]].tolist())
            L, cc, tc = (a[:, k].astype(np.int64) for k in range(3))
            assert (tc <= cc).all() and (L <= tr[:, 1]).all() and (L <= tr[:, 0]).all(), where
            assert ((cc >= 1) if n else (a == 0)).all(), where
            assert (cc[L == 0] == n).all(), where
            shift = tr[:, 0] - L                                    # how far the fallback moved the start
            shift1 += int((shift == 1).sum())
            shift3 += int((shift >= 3).sum())
            by_cap += int(((M > 0) & (L == M) & (tr[:, 2] > M)).sum())
            by_start += int(((L == tr[:, 2]) & (L > 0) & ((M == 0) | (L < M))).sum())
            missed += int(((tc == 0) & (L > 0)).sum())
            unseen += int(((tc == 0) & (L == 0)).sum())
            certain += int(((tc == cc) & (n > 0)).sum())
            positions += a.shape[0]
    assert positions > 100000 and shift1 >= 1 and shift3 >= 1, (positions, shift1, shift3)
    assert by_cap > 1000 and by_start > 1000 and missed > 1000 and unseen > 100 and certain > 1000, (by_cap, by_start, missed, unseen, certain)


def test_score_way_two_gives_the_same_records():
    """the bisection over L alone (no matching statistics) against the way through them, on the cases the fallback is about and one
    text of every kind of repeat"""
    for name in ("equal20", "unique_tail", "tail_twice", "never_followed", "all_equal/doc_sizes", "period2/tails", "rand_k2/total257",
                 "planted/carried", "zero_and_max/odd_tokens", "n1/windows", "n0/q3"):
        e = sc.expected(name)
        tl, sl = [int(v) for v in e["t"]], [int(v) for v in e["sa"]]
        for M in sc.MAX_LENGTHS:
            assert np.array_equal(sc.score_a(tl, sl, e["docs"], M, None)[0], e["scores"][M]), (name, M)


def test_score_named_cases():
    """what the issue's words say of the cases the fallback and the numerator are about"""
    e = sc.expected("equal20")
    a, tr = e["scores"][0], e["trace"][0]
    assert a[19:30].tolist() == [[19, 1, 1, 19]] * 11                                   # L = 19 and counts (1, 1) from position 19 on
    assert (tr[:, 0] - a[:, 0])[:30].tolist() == [0] * 20 + [1] * 10                    # ... the fallback moves the start by one
    e = sc.expected("unique_tail")
    a, tr = e["scores"][0], e["trace"][0]
    assert a[:5].tolist() == [[0, 403, 77, 0], [1, 77, 0, 77], [1, 1, 1, 400], [2, 1, 1, 400], [0, 403, 78, 77]]
    assert (tr[:5, 0] - a[:5, 0]).tolist() == [0, 0, 0, 0, 3]                           # by 3, down to L = 0
    assert sorted(set((tr[:, 0] - a[:, 0]).tolist())) == [0, 1, 2, 3, 13]
    e = sc.expected("tail_twice")
    a, tr = e["scores"][0], e["trace"][0]
    assert e["ms"][0][1].tolist()[1:] == [2, 3, 1]                                      # the tail: count 2, one of them ended
    assert a[4].tolist() == [3, 1, 0, 401] and a[8].tolist() == [3, 1, 1, 401]          # effective count 1
    assert not (tr[:, 0] - a[:, 0]).any()                                               # and no fallback
    e = sc.expected("never_followed")
    assert e["scores"][0][2].tolist() == [2, 3, 0, 3]                                   # "1 2" stands three times, never before a 9


def test_score_hand_worked():
    """corpus 7 8 9 1 2 3, text 5 1 2 3 4.  5 and 4 occur nowhere: the empty context (6 tokens have a token: themselves) and a token
    count of 0.  1 after "5": no context occurs, 1 stands once among 6.  2 after "1": "1" stands once with a token behind it, a 2.
    3 after "1 2": once, a 3.  4 after "1 2 3": that is the corpus's tail and nothing follows it anywhere; so are "2 3" and "3": L = 0."""
    t = np.array([7, 8, 9, 1, 2, 3], np.int32)
    sa = model_sa(t)
    assert sa.tolist() == [3, 4, 5, 0, 1, 2]
    tl, sl = t.tolist(), sa.tolist()
    docs = [[5, 1, 2, 3, 4]]
    ms = sc.mc.spans_a(tl, sl, docs, 0)
    assert ms[:, 2].tolist() == [0, 3, 2, 1, 0]
    a, tr = sc.score_a(tl, sl, docs, 0, ms[:, 2])
    assert a[:, :3].tolist() == [[0, 6, 0], [0, 6, 1], [1, 1, 1], [2, 1, 1], [0, 6, 0]]
    assert a[:, 3].tolist() == [3, 0, 0, 0, 3]                      # suffixes before "5", "1", "1 2", "1 2 3", "4"
    assert (tr[:, 0] - a[:, 0]).tolist() == [0, 0, 0, 0, 3]         # fact 1 finds "1 2 3"; the fallback goes down to nothing
    assert np.array_equal(sc.score_a(tl, sl, docs, 0, None)[0], a)
    assert sc.score_b(t, docs, 0).tolist() == [[0, 6, 0], [0, 6, 1], [1, 1, 1], [2, 1, 1], [0, 6, 0]]
    assert sc.heads_of(a, docs).tolist() == [[5, 3, 2, 2, 3]]       # seen: 1, 2, 3; certain: the 2 and the 3
    # max_length 1: the 3 is scored behind "2" alone
    a1 = sc.score_a(tl, sl, docs, 1, sc.mc.spans_a(tl, sl, docs, 1)[:, 2])[0]
    assert a1[:, :3].tolist() == [[0, 6, 0], [0, 6, 1], [1, 1, 1], [1, 1, 1], [0, 6, 0]] and sc.score_b(t, docs, 1).tolist() == a1[:, :3].tolist()
    # a document boundary cuts the context: "1 2" | "3"
    two = [[1, 2], [3], []]
    a2 = sc.score_a(tl, sl, two, 0, sc.mc.spans_a(tl, sl, two, 0)[:, 2])[0]
    assert a2.tolist() == [[0, 6, 1, 0], [1, 1, 1, 0], [0, 6, 1, 2]]
    assert sc.heads_of(a2, two).tolist() == [[2, 2, 1, 1, 1], [1, 1, 0, 0, 0], [0, 0, 0, 0, 0]]
