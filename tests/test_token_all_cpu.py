"""Per-document counts and AND groups of a token index without a GPU: every new entry point is declared, exported and bound; the
new structs match the C compiler's view of the header; every argument error that is answered before a HIP call is answered with -1
on a handle that is only an address; the two CPU models that test_gpu_token_all.py measures the device against (token_all_cases.py)
agree with each other, with hand-counted tables and with the closed forms of the all-equal text; the case lists hold every edge they
are there for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_all_cases as ac
import token_doc_cases as dc
import token_next_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_index_prepare_doc_ranks", "sa_hip_token_index_get_doc_ranks", "sa_hip_token_index_doc_ranks_info",
       "sa_hip_token_index_doc_counts_batch_device", "sa_hip_token_index_doc_counts_batch", "sa_hip_token_index_all_batch_device",
       "sa_hip_token_index_all_batch"]


def test_all_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int, name
    for name in ("prepare_doc_ranks", "doc_ranks", "doc_ranks_info", "doc_counts_batch", "doc_counts_batch_device", "all_batch",
                 "all_batch_device"):
        assert callable(getattr(capi.TokenIndex, name)), name
    from suffixarray_amd import token_index
    for name in ("prepare_document_ranks", "term_counts", "documents_with_all", "count_documents_with_all"):
        assert callable(getattr(token_index.TokenIndex, name)), name
    assert capi.ALL_DTYPE.itemsize == C.sizeof(capi.TokenAll) == 32
    assert capi.ALL_DTYPE.names == tuple(f for f, _ in capi.TokenAll._fields_)
    assert [capi.ALL_DTYPE.fields[f][1] for f in capi.ALL_DTYPE.names] == [getattr(capi.TokenAll, f).offset for f in capi.ALL_DTYPE.names]
    assert int(re.search(r"#define SA_HIP_TOKEN_ALL_MAX (\d+)", header).group(1)) == capi.TOKEN_ALL_MAX == ac.ALL_MAX == 16
    for f in ("token_all.hpp", "capi_token_all.hpp"):
        assert os.path.exists(os.path.join(ROOT, "suffixarray_amd", "csrc", f)), f


@pytest.mark.parametrize("struct, cls, fields", [
    ("sa_hip_token_all", "TokenAll", ["written", "examined", "matched", "candidates", "driver", "count", "reserved"]),
    ("sa_hip_token_doc_ranks_info", "TokenDocRanksInfo", ["present", "sort_passes", "bytes", "prepare_ms", "counts_q", "counts_ms", "all_q",
                                                          "all_ms"]),
])
def test_all_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields):
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
    assert C.sizeof(S) == {"TokenAll": 32, "TokenDocRanksInfo": 56}[cls]
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
    assert [f for f in re.findall(r"^\s*\w+\s+(\w+)(?:\[\d+\])?;", body, re.M)] == fields


def test_all_argument_errors_before_any_device_call(capi):
    """the handle is an address that holds nothing: every call below must return before it is looked at"""
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    spans = np.zeros(2, capi.SPAN_DTYPE)
    docs, offs, cnt = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, np.uint32)
    wr = np.zeros(2, np.uint32)
    heads = np.zeros(2, capi.ALL_DTYPE)
    go1 = np.array([0, 2], np.uint64)                              # one group of both spans
    go2 = np.array([0, 1, 2], np.uint64)                           # two groups of one
    p, o, s, d, f, c, w, a = (x.ctypes.data for x in (pat, off, spans, docs, offs, cnt, wr, heads))
    g1, g2 = go1.ctypes.data, go2.ctypes.data
    D = 1 << 20                                                    # "device pointers": never touched

    def counts_dev(t=h, sp=D, q=2, cap=4, dd=D, ww=D, stride=16, cc=D):
        return lib.sa_hip_token_index_doc_counts_batch_device(t, sp, q, cap, dd, ww, stride, cc)

    def counts_host(t=h, pp=p, oo=o, q=2, mode=0, need=0, cap=4, dd=d, ww=w, cc=c, ss=s):
        return lib.sa_hip_token_index_doc_counts_batch(t, pp, oo, q, mode, 0, need, cap, dd, ww, cc, ss)

    def all_dev(t=h, sp=D, S=2, go=g1, G=1, cap=4, dd=D, ff=D, hh=D):
        return lib.sa_hip_token_index_all_batch_device(t, sp, S, go, G, cap, 0, dd, ff, hh)

    def all_host(t=h, pp=p, oo=o, S=2, go=g1, G=1, mode=0, need=0, cap=4, ss=s, dd=d, ff=f, hh=a):
        return lib.sa_hip_token_index_all_batch(t, pp, oo, S, go, G, mode, 0, need, cap, 0, ss, dd, ff, hh)

    # NULL handle
    assert lib.sa_hip_token_index_prepare_doc_ranks(None, 1) == -1
    assert b"sa_hip_token_index_prepare_doc_ranks" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_prepare_doc_ranks(None, 0) == -1
    assert lib.sa_hip_token_index_prepare_doc_ranks(h, 2) == -1 and lib.sa_hip_token_index_prepare_doc_ranks(h, -1) == -1
    assert lib.sa_hip_token_index_get_doc_ranks(None, 0, 1, d) == -1
    assert lib.sa_hip_token_index_get_doc_ranks(h, 0, 1, None) == -1
    assert lib.sa_hip_token_index_doc_ranks_info(None, C.byref(capi.TokenDocRanksInfo())) == -1
    assert lib.sa_hip_token_index_doc_ranks_info(h, None) == -1
    for call in (counts_dev, counts_host, all_dev, all_host):
        assert call(t=None) == -1, call.__name__
    assert b"sa_hip_token_index_all_batch" in lib.sa_hip_last_error()
    # mode and need_next are 0 or 1, also with Q == 0 / G == 0
    for mode, need in ((2, 1), (-1, 1), (0, 2), (1, -1)):
        assert counts_host(mode=mode, need=need) == -1 and counts_host(mode=mode, need=need, q=0) == -1, (mode, need)
        assert all_host(mode=mode, need=need) == -1 and all_host(mode=mode, need=need, G=0, S=0) == -1, (mode, need)
    # cap == 0 in doc_counts (the all calls allow it); the stride of written
    assert counts_dev(cap=0) == -1 and b"cap" in lib.sa_hip_last_error()
    assert counts_host(cap=0) == -1 and counts_host(cap=0, q=0) == -1
    for stride in (0, 1, 2, 3, 5, 6, 7, 18):
        assert counts_dev(stride=stride) == -1 and b"stride" in lib.sa_hip_last_error(), stride
    # Q * cap, G * cap, S >= 2^31
    for q, cap in ((1 << 31, 1), (1 << 20, 1 << 11), (1, 0xFFFFFFFF), (3, 0x80000000 // 3 + 1)):
        assert counts_dev(q=q, cap=cap) == -1 and b"2^31" in lib.sa_hip_last_error(), (q, cap)
        assert counts_host(q=q, cap=cap) == -1, (q, cap)
        assert all_dev(G=q, cap=cap) == -1 and b"2^31" in lib.sa_hip_last_error(), (q, cap)
        assert all_host(G=q, cap=cap) == -1, (q, cap)
    assert all_dev(S=1 << 31) == -1 and b"2^31" in lib.sa_hip_last_error()
    assert all_host(S=1 << 31) == -1 and b"2^31" in lib.sa_hip_last_error()
    # the group table
    big = np.arange(0, 18, 17, dtype=np.uint64)                    # one group of 17
    for tab, S, G, word in (([1, 2], 2, 1, b"[0]"), ([0, 1], 2, 1, b"end at S"), ([0, 3], 2, 1, b"end at S"), ([0, 0, 2], 2, 2, b"empty"),
                            ([0, 2, 2], 2, 2, b"empty"), ([0, 2, 1, 2], 2, 3, b"empty"), (big.tolist(), 17, 1, b"SA_HIP_TOKEN_ALL_MAX")):
        t_ = np.array(tab, np.uint64)
        assert all_dev(S=S, go=t_.ctypes.data, G=G) == -1, tab
        assert word in lib.sa_hip_last_error(), (tab, lib.sa_hip_last_error())
        assert all_host(S=S, go=t_.ctypes.data, G=G) == -1 and word in lib.sa_hip_last_error(), tab
    assert all_dev(go=None) == -1 and all_host(go=None) == -1
    # NULL required pointers (written of doc_counts and spans of the host forms may be NULL: not among them)
    assert counts_dev(sp=None) == -1 and counts_dev(dd=None) == -1 and counts_dev(cc=None) == -1
    assert counts_host(oo=None) == -1 and counts_host(dd=None) == -1 and counts_host(cc=None) == -1 and counts_host(pp=None) == -1
    assert all_dev(sp=None) == -1 and all_dev(dd=None) == -1 and all_dev(ff=None) == -1 and all_dev(hh=None) == -1
    assert all_dev(cap=0, dd=None, ff=None, hh=None) == -1 and all_dev(cap=0, sp=None, dd=None, ff=None) == -1   # cap 0: spans and heads still
    assert all_host(oo=None) == -1 and all_host(dd=None) == -1 and all_host(ff=None) == -1 and all_host(hh=None) == -1
    assert all_host(pp=None) == -1 and all_host(cap=0, dd=None, ff=None, hh=None) == -1
    # descending offsets
    assert counts_host(oo=down.ctypes.data) == -1 and b"descend" in lib.sa_hip_last_error()
    assert all_host(oo=down.ctypes.data) == -1 and b"descend" in lib.sa_hip_last_error()
    assert all_host(oo=down.ctypes.data, go=g2, G=2) == -1 and b"descend" in lib.sa_hip_last_error()
    # Q == 0 / G == 0 with good arguments: no-ops that touch nothing
    assert counts_dev(sp=None, q=0, dd=None, ww=None, cc=None) == 0
    assert counts_host(pp=None, oo=None, q=0, dd=None, ww=None, cc=None, ss=None) == 0
    assert all_dev(sp=None, S=0, go=None, G=0, dd=None, ff=None, hh=None) == 0
    assert all_dev(sp=None, S=0, go=None, G=0, cap=0, dd=None, ff=None, hh=None) == 0
    assert all_host(pp=None, oo=None, S=0, go=None, G=0, ss=None, dd=None, ff=None, hh=None) == 0


def test_all_without_a_device_fails_loudly(capi):
    """no handle without a device, hence no rank-by-document array, and no answer from anywhere else"""
    import suffixarray_amd
    device = 1 << 20 if capi.lib().sa_hip_device_count() >= 1 else 0
    with pytest.raises(capi.SaHipError) as e:
        suffixarray_amd.TokenIndex([5, 1, 5], device=device, doc_starts=[0, 2]).term_counts([[5]], [0])
    assert e.value.code == -3


# ---- the models ----------------------------------------------------------------------------------------------------------------

HAND_T = [1, 2, 1, 2, 3, 1, 2]
HAND_STARTS = [0, 0, 2, 5, 5, 7]          # 0 empty at the front, 1 = [1 2], 2 = [1 2 3], 3 empty in the middle, 4 = [1 2], 5 empty at the end


def test_models_on_hand_counted_tables():
    t, starts = np.array(HAND_T, np.int32), np.array(HAND_STARTS, np.int32)
    n = t.size
    sa = dc.model_sa(t)
    da, pv = dc.model_da_pv(sa, starts)
    assert sa.tolist() == [5, 0, 2, 6, 1, 3, 4] and da.tolist() == [4, 1, 2, 4, 1, 2, 2]
    rk, cl = ac.model_rk(da), ac.closed(starts, n)
    assert rk.tolist() == [1, 4, 2, 5, 6, 0, 3]                    # documents 1 | 2 | 4 at the positions 0 | 2 | 5: empty ones own none
    assert cl.tolist() == [0, 0, 2, 5, 5, 7, 7]
    isa = np.argsort(sa)
    for d in range(starts.size):                                   # the segment-length identity and the ISA form
        seg = rk[cl[d]:cl[d + 1]]
        assert seg.size == int((da == d).sum()) and sorted(isa[cl[d]:cl[d + 1]].tolist()) == seg.tolist(), d
    # [1, 2] = ranks 0 .. 2 once in 1, 2, 4; [2] = ranks 3 .. 5; the whole array; [3] = rank 6
    assert [ac.count_a(rk, cl, 0, 3, d) for d in range(-1, 7)] == [0, 0, 1, 1, 0, 1, 0, 0]
    assert [ac.count_a(rk, cl, 0, 7, d) for d in range(6)] == [0, 2, 3, 0, 2, 0]
    assert [ac.count_a(rk, cl, 6, 7, d) for d in range(6)] == [0, 0, 1, 0, 0, 0] and ac.count_a(rk, cl, 3, 3, 2) == 0
    assert ac.tf_b(t, starts, [1, 2]) == {1: 1, 2: 1, 4: 1} and ac.tf_b(t, starts, [3]) == {2: 1} and ac.tf_b(t, starts, []) == {1: 2, 2: 3, 4: 2}
    # [1, 2] AND [3]: the driver is [3] (count 1, index 1), document 2 at offset 2
    w = ac.all_walk(sa, da, cl, n, [(0, 3), (6, 1)])
    assert w[:3] == (1, 1, [(6, 2, 2, True)])
    assert ac.all_a(w, 6, 0) == ((1, 1, 1, 1, 1, 1), [(2, 2)]) and ac.all_b(t, starts, [[1, 2], [3]])[0] == [2]
    # [1, 2] AND [2]: a tie in counts picks index 0; all three documents, in the rank order of [1, 2]
    w = ac.all_walk(sa, da, cl, n, [(0, 3), (3, 3)])
    assert w[:2] == (0, 3) and ac.all_a(w, 0, 0) == ((3, 3, 3, 3, 0, 3), [(4, 0), (1, 0), (2, 0)])
    assert ac.all_a(w, 0, 2) == ((2, 2, 2, 2, 0, 3), [(4, 0), (1, 0)]) and ac.all_a(w, 0, 0, most=1)[1] == [(4, 0)]
    w = ac.all_walk(sa, da, cl, n, [(3, 3), (0, 3)])                # swapped: the rank order of [2]
    assert ac.all_a(w, 3, 0) == ((3, 3, 3, 3, 0, 3), [(4, 1), (1, 1), (2, 1)])
    # an empty span: everything is 0; a span twice: matched == candidates
    assert ac.all_a(ac.all_walk(sa, da, cl, n, [(0, 7), (2, 0)]), 2, 0) == ((0, 0, 0, 0, 1, 0), [])
    assert ac.all_a(ac.all_walk(sa, da, cl, n, [(0, 7), (0, 7)]), 0, 0)[0] == (3, 7, 3, 3, 0, 7)
    # D == 1 and one token per document
    da1, _ = dc.model_da_pv(sa, [0])
    assert ac.model_rk(da1).tolist() == list(range(7)) and ac.count_a(ac.model_rk(da1), ac.closed([0], n), 2, 6, 0) == 4
    one = dc.one_token_each(n)
    dan, _ = dc.model_da_pv(sa, one)
    rkn, cln = ac.model_rk(dan), ac.closed(one, n)
    assert rkn.tolist() == isa.tolist() and [ac.count_a(rkn, cln, 0, 3, d) for d in range(7)] == [1, 0, 1, 0, 0, 1, 0]
    assert ac.all_a(ac.all_walk(sa, dan, cln, n, [(0, 3), (1, 4)]), 0, 0) == ((2, 3, 2, 3, 0, 3), [(0, 0), (2, 0)])


@pytest.mark.parametrize("name", list(dc.RANDOM))
def test_models_agree_on_the_random_texts(name):
    c, e = ac.random_case(name), nc.expected(name)
    t, sa, starts, da, rk, cl = c["t"], c["sa"], c["starts"], c["da"], c["rk"], c["cl"]
    n = t.size
    assert np.array_equal(np.sort(rk), np.arange(n)) and np.array_equal(da[rk], np.sort(da, kind="stable"))
    assert np.array_equal(np.bincount(da, minlength=starts.size), np.diff(cl))                         # the segment-length identity
    isa = np.argsort(sa)
    for d in range(0, starts.size, 17):
        assert np.array_equal(rk[cl[d]:cl[d + 1]], np.sort(isa[cl[d]:cl[d + 1]])), d
    for cfg in ((0, 0, 1), (1, 0, 0)):
        spans = e["spans"][cfg].tolist()
        pats = [ctx[len(ctx) - sp[2]:] for ctx, sp in zip(e["ctx"], spans)]
        for i in range(0, len(pats), 7):                                                              # counts: A against B
            tf = ac.tf_b(t, starts, pats[i])
            a, end = ac.clamp(n, spans[i][0], spans[i][1])
            for d in list(tf)[:5] + [0, starts.size - 1, -1, starts.size]:
                assert ac.count_a(rk, cl, a, end, d) == tf.get(d, 0), (name, cfg, i, d)
        for grp in ac.random_groups(len(pats)):                                                       # AND groups: A against B
            sp = [(spans[i][0], spans[i][1]) for i in grp]
            w = ac.all_walk(sa, da, cl, n, sp)
            head, ent = ac.all_a(w, ac.group_first(n, sp), 0, most=1 << 20)
            both, tfs = ac.all_b(t, starts, [pats[i] for i in grp])
            assert head[2] == len(both) and sorted(d for d, _ in ent) == both, (name, cfg, grp)
            assert head[4] == ac.driver_of([s[1] for s in sp]) and head[3] == len(tfs[head[4]]), (name, cfg, grp)


def test_all_equal_text_closed_forms_and_edges():
    assert ac.N_EQ <= 70000 and set(ac.TF_LDS) == {1, 2, 63, 64, 65}
    for Ld in ac.TF_LDS:
        c = dc.equal_case(Ld)
        rk, cl = ac.model_rk(c["da"]), ac.closed(c["starts"], ac.N_EQ)
        D = c["starts"].size
        for d in ac.tf_docs(Ld):
            s, e = ac.equal_segment(Ld, d)
            assert rk[cl[d]:cl[d + 1]].tolist() == list(range(s, e)), (Ld, d)
        spans, docs = ac.tf_cells(Ld)
        assert docs.shape == (len(spans), 8) and {-1, D, ac.I32_MAX} <= set(docs[0].tolist())
        assert any(f > ac.N_EQ for f, _ in spans) and any(f + k > ac.N_EQ and f <= ac.N_EQ for f, k in spans) and any(k == 0 for _, k in spans)
        s, e = ac.equal_segment(Ld, D // 2)
        assert {(s, e - s), (s - 1, e - s + 2), (s + 1, max(e - s - 2, 0)) if e - s >= 2 else (s, e - s)} <= set(spans), Ld
        want = ac.counts_rows(rk, cl, ac.N_EQ, spans, docs)
        for i, (f, k) in enumerate(spans):
            a, end = ac.clamp(ac.N_EQ, f, k)
            assert want[i].tolist() == [ac.equal_count(Ld, a, end, int(d)) for d in docs[i]], (Ld, i)
    # AND groups on the text cut every token
    c = dc.equal_case(1)
    cl = ac.closed(c["starts"], ac.N_EQ)
    assert {63, 64, 65, 255, 256, 257} <= set(ac.AND_COUNTS) and {63, 64, 65, 255, 256, 257} <= {lo for lo, _ in ac.AND_OTHERS}
    assert all(hi - lo > max(ac.AND_COUNTS) for lo, hi in ac.AND_OTHERS) and set(ac.AND_CAPS) == {0, 1, 16}
    assert all({k - 1, k, k + 1} - {0, -1} <= set(ac.AND_BUDGETS) | {0} for k in ac.AND_COUNTS if k)
    seen = set()
    for grp in ac.and_groups():
        (_, k), (lo, m) = grp
        w = ac.all_walk(c["sa"], c["da"], cl, ac.N_EQ, grp)
        head, ent = ac.all_a(w, 0, 0, most=1 << 20)
        assert head == (max(0, k - lo), k, max(0, k - lo), k, 0, k), grp
        assert [d for d, _ in ent] == [ac.N_EQ - 1 - r for r in range(lo, k)] and all(o == 0 for _, o in ent), grp
        seen.add(head[2])
    assert {0, 1, 2, 15, 16, 17} <= seen                                                              # below, at and above the caps


def test_planted_spans_reach_their_edges():
    c = ac.planted_case()
    n, da, rk, cl = c["t"].size, c["da"], c["rk"], c["cl"]
    assert len(c["groups"]) >= 16 and len(c["groups"]) == len(c["want"]) and set(c["want"]) == {True, False}
    for (A, B), want in zip(c["groups"], c["want"]):
        d = int(da[A[0]])
        w = ac.all_walk(c["sa"], da, cl, n, [A, B])
        assert w[0] == 0 and w[2][0][:2] == (A[0], d) and w[2][0][3] is want, (A, B)
        assert (ac.count_a(rk, cl, B[0], B[0] + B[1], d) == 1) is want, (A, B)
    D = c["starts"].size
    assert c["last_size"] >= 3 and c["top"] + 4 <= n and int(da[c["top"]]) == D - 1 and cl[D] == n
    (A, B), (A2, B2), (A3, B3) = c["last"]
    assert ac.all_walk(c["sa"], da, cl, n, [A, B])[2][0][1:] == (D - 1, int(c["sa"][A[0]]) - int(cl[D - 1]), False)
    assert ac.all_walk(c["sa"], da, cl, n, [A2, B2])[2][0][3] is True
    assert ac.all_walk(c["sa"], da, cl, n, [A3, B3]) [2] == [(c["top"], D - 1, int(c["sa"][c["top"]]) - int(cl[D - 1]), False)]
    assert int(np.searchsorted(rk[cl[D - 1]:n], B[0])) == c["last_size"]                               # the lower bound is the segment's end: RK[n]
