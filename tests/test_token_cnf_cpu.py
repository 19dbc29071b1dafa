"""CNF document queries of a token index without a GPU: the three entry points are declared, exported and bound; the two structs match
the C compiler's view of the header; every argument error that is answered before a HIP call is answered with -1 on a handle that is
only an address; the two CPU models that test_gpu_token_cnf.py measures the device against (token_cnf_cases.py) agree with each
other, with the hand-counted 7-token table of test_token_all_cpu.py and on the random texts; the case lists hold every edge they are
there for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_all_cases as ac
import token_cnf_cases as cc
import token_doc_cases as dc
import token_next_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_index_cnf_batch_device", "sa_hip_token_index_cnf_batch", "sa_hip_token_index_cnf_info"]
CNF_FIELDS = ["written", "matched", "candidates", "duplicates", "driver", "literals", "examined", "count", "reserved"]


def test_cnf_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int, name
    for name in ("cnf_batch", "cnf_batch_device", "cnf_info"):
        assert callable(getattr(capi.TokenIndex, name)), name
    from suffixarray_amd import token_index
    for name in ("documents_with_cnf", "count_documents_with_cnf"):
        assert callable(getattr(token_index.TokenIndex, name)), name
    assert capi.CNF_DTYPE.itemsize == C.sizeof(capi.TokenCnf) == 48
    assert capi.CNF_DTYPE.names == tuple(f for f, _ in capi.TokenCnf._fields_) == tuple(CNF_FIELDS)
    assert [capi.CNF_DTYPE.fields[f][1] for f in capi.CNF_DTYPE.names] == [getattr(capi.TokenCnf, f).offset for f in capi.CNF_DTYPE.names]
    assert capi.CNF_DTYPE.names[0] == "written" and capi.CNF_DTYPE.fields["written"][1] == 0         # chains as written_dev, stride 48
    assert int(re.search(r"#define SA_HIP_TOKEN_CNF_MAX_CLAUSES (\d+)", header).group(1)) == capi.TOKEN_CNF_MAX_CLAUSES == cc.MAX_CLAUSES == 16
    assert int(re.search(r"#define SA_HIP_TOKEN_CNF_MAX_LITERALS (\d+)", header).group(1)) == capi.TOKEN_CNF_MAX_LITERALS == cc.MAX_LITERALS == 64
    assert cc.HEAD == tuple(CNF_FIELDS[:8])
    for f in ("token_cnf.hpp", "capi_token_cnf.hpp"):
        assert os.path.exists(os.path.join(ROOT, "suffixarray_amd", "csrc", f)), f


@pytest.mark.parametrize("struct, cls, fields, size", [
    ("sa_hip_token_cnf", "TokenCnf", CNF_FIELDS, 48),
    ("sa_hip_token_cnf_info", "TokenCnfInfo", ["q", "ms"], 16),
])
def test_cnf_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields, size):
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
    assert C.sizeof(S) == size
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
    assert [f for f in re.findall(r"^\s*\w+\s+(\w+)(?:\[\d+\])?;", body, re.M)] == fields


def test_cnf_argument_errors_before_any_device_call(capi):
    """the handle is an address that holds nothing: every call below must return before it is looked at"""
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1, 5], np.int32)
    off = np.array([0, 2, 4, 5], np.uint64)                        # three literals
    down = np.array([0, 3, 2, 5], np.uint64)
    spans = np.zeros(3, capi.SPAN_DTYPE)
    docs, offs = np.zeros(8, np.int32), np.zeros(8, np.int32)
    heads = np.zeros(2, capi.CNF_DTYPE)
    co = np.array([0, 2, 3], np.uint64)                            # two clauses: literals 0 1 | 2
    go = np.array([0, 2], np.uint64)                               # one group of both
    go2 = np.array([0, 1, 2], np.uint64)                           # two groups of one
    ng = np.array([0, 1], np.uint8)
    p, o, s, d, f, a = (x.ctypes.data for x in (pat, off, spans, docs, offs, heads))
    D = 1 << 20                                                    # "device pointers": never touched

    def dev(t=h, sp=D, S=3, cl=co, C=2, neg=ng, gr=go, G=1, cap=4, dd=D, ff=D, hh=D):
        return lib.sa_hip_token_index_cnf_batch_device(t, sp, S, None if cl is None else cl.ctypes.data, C,
                                                       None if neg is None else neg.ctypes.data, None if gr is None else gr.ctypes.data, G,
                                                       cap, 0, dd, ff, hh)

    def host(t=h, pp=p, oo=o, S=3, cl=co, C=2, neg=ng, gr=go, G=1, mode=0, need=0, cap=4, ss=s, dd=d, ff=f, hh=a):
        return lib.sa_hip_token_index_cnf_batch(t, pp, oo, S, None if cl is None else cl.ctypes.data, C, None if neg is None else neg.ctypes.data,
                                                None if gr is None else gr.ctypes.data, G, mode, 0, need, cap, 0, ss, dd, ff, hh)

    # NULL handle: the message names the call
    assert dev(t=None) == -1 and b"sa_hip_token_index_cnf_batch_device" in lib.sa_hip_last_error()
    assert host(t=None) == -1 and b"sa_hip_token_index_cnf_batch" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_cnf_info(None, C.byref(capi.TokenCnfInfo())) == -1 and b"sa_hip_token_index_cnf_info" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_cnf_info(h, None) == -1
    # mode and need_next are 0 or 1, also with G == 0 and with C == 0
    for mode, need in ((2, 1), (-1, 1), (0, 2), (1, -1)):
        assert host(mode=mode, need=need) == -1 and b"sa_hip_token_index_cnf_batch" in lib.sa_hip_last_error(), (mode, need)
        assert host(mode=mode, need=need, G=0) == -1 and host(mode=mode, need=need, G=0, C=0, S=0) == -1, (mode, need)
    # G * cap, S, C, G >= 2^31
    for q, cap in ((1 << 31, 1), (1 << 20, 1 << 11), (1, 0xFFFFFFFF), (3, 0x80000000 // 3 + 1)):
        assert dev(G=q, cap=cap) == -1 and b"2^31" in lib.sa_hip_last_error(), (q, cap)
        assert host(G=q, cap=cap) == -1 and b"2^31" in lib.sa_hip_last_error(), (q, cap)
    for kw in ({"S": 1 << 31}, {"C": 1 << 31}, {"G": 1 << 31, "cap": 0}):
        assert dev(**kw) == -1 and b"2^31" in lib.sa_hip_last_error(), kw
        assert host(**kw) == -1 and b"2^31" in lib.sa_hip_last_error(), kw
    # the clause table
    for tab, S, word in (([1, 2, 3], 3, b"clause_offsets[0]"), ([0, 2, 2], 2, b"empty clause"), ([0, 0, 3], 3, b"empty clause"),
                         ([0, 2, 1], 1, b"empty clause"), ([0, 2, 3], 4, b"end at S"), ([0, 1, 2], 3, b"end at S")):
        t_ = np.array(tab, np.uint64)
        assert dev(cl=t_, S=S) == -1 and word in lib.sa_hip_last_error(), (tab, lib.sa_hip_last_error())
        assert host(cl=t_, S=S) == -1 and word in lib.sa_hip_last_error(), tab
    # the group table
    for tab, G, word in (([1, 2], 1, b"group_offsets[0]"), ([0, 1], 1, b"end at C"), ([0, 3], 1, b"end at C"), ([0, 0, 2], 2, b"empty group"),
                         ([0, 2, 2], 2, b"empty group"), ([0, 2, 1, 2], 3, b"empty group")):
        t_ = np.array(tab, np.uint64)
        assert dev(gr=t_, G=G) == -1 and word in lib.sa_hip_last_error(), (tab, lib.sa_hip_last_error())
        assert host(gr=t_, G=G) == -1 and word in lib.sa_hip_last_error(), tab
    # more than 16 clauses; more than 64 literals (in 2 clauses); both at their limits pass the tables and stop at the NULL spans
    c17, g17, o17 = np.arange(18, dtype=np.uint64), np.array([0, 17], np.uint64), np.arange(18, dtype=np.uint64)
    assert dev(S=17, cl=c17, C=17, neg=None, gr=g17) == -1 and b"SA_HIP_TOKEN_CNF_MAX_CLAUSES" in lib.sa_hip_last_error()
    assert host(S=17, oo=o17.ctypes.data, cl=c17, C=17, neg=None, gr=g17) == -1 and b"SA_HIP_TOKEN_CNF_MAX_CLAUSES" in lib.sa_hip_last_error()
    c65, o65 = np.array([0, 1, 65], np.uint64), np.arange(66, dtype=np.uint64)
    assert dev(S=65, cl=c65, neg=None) == -1 and b"SA_HIP_TOKEN_CNF_MAX_LITERALS" in lib.sa_hip_last_error()
    assert host(S=65, oo=o65.ctypes.data, cl=c65, neg=None) == -1 and b"SA_HIP_TOKEN_CNF_MAX_LITERALS" in lib.sa_hip_last_error()
    c16, g16, c64 = np.arange(17, dtype=np.uint64), np.array([0, 16], np.uint64), np.array([0, 1, 64], np.uint64)
    assert dev(sp=None, S=16, cl=c16, C=16, neg=None, gr=g16) == -1 and b"NULL argument" in lib.sa_hip_last_error()
    assert dev(sp=None, S=64, cl=c64, neg=None) == -1 and b"NULL argument" in lib.sa_hip_last_error()
    # no positive clause; a negated byte other than 0 / 1
    for neg, gr, G in (([1, 1], go, 1), ([0, 1], go2, 2), ([1, 0], go2, 2)):
        n_ = np.array(neg, np.uint8)
        assert dev(neg=n_, gr=gr, G=G) == -1 and b"no positive clause" in lib.sa_hip_last_error(), neg
        assert host(neg=n_, gr=gr, G=G) == -1 and b"no positive clause" in lib.sa_hip_last_error(), neg
    for neg in ([2, 0], [0, 255]):
        n_ = np.array(neg, np.uint8)
        assert dev(neg=n_) == -1 and b"negated" in lib.sa_hip_last_error(), neg
        assert host(neg=n_) == -1 and b"negated" in lib.sa_hip_last_error(), neg
    # NULL required pointers (negated and the spans of the host form may be NULL: not among them)
    assert dev(cl=None) == -1 and dev(gr=None) == -1 and host(cl=None) == -1 and host(gr=None) == -1
    assert dev(sp=None) == -1 and dev(dd=None) == -1 and dev(ff=None) == -1 and dev(hh=None) == -1
    assert dev(cap=0, dd=None, ff=None, hh=None) == -1 and dev(cap=0, sp=None, dd=None, ff=None) == -1   # cap 0: spans and heads still
    assert host(oo=None) == -1 and host(dd=None) == -1 and host(ff=None) == -1 and host(hh=None) == -1
    assert host(pp=None) == -1 and host(cap=0, dd=None, ff=None, hh=None) == -1
    # descending offsets
    assert host(oo=down.ctypes.data) == -1 and b"descend" in lib.sa_hip_last_error()
    # G == 0 with good arguments: no-ops that touch nothing
    assert dev(sp=None, S=0, cl=None, C=0, neg=None, gr=None, G=0, dd=None, ff=None, hh=None) == 0
    assert dev(sp=None, S=0, cl=None, C=0, neg=None, gr=None, G=0, cap=0, dd=None, ff=None, hh=None) == 0
    assert host(pp=None, oo=None, S=0, cl=None, C=0, neg=None, gr=None, G=0, ss=None, dd=None, ff=None, hh=None) == 0


def test_cnf_without_a_device_fails_loudly(capi):
    """no handle without a device, and no answer from anywhere else"""
    import suffixarray_amd
    device = 1 << 20 if capi.lib().sa_hip_device_count() >= 1 else 0
    with pytest.raises(capi.SaHipError) as e:
        suffixarray_amd.TokenIndex([5, 1, 5], device=device, doc_starts=[0, 2]).documents_with_cnf([[[[5]]]])
    assert e.value.code == -3


def test_python_tables_and_limits():
    from suffixarray_amd.token_index import TokenIndex
    flat, coff, neg, goff = TokenIndex._cnf_tables([[[[1, 2], [3]], [[4]]], [[[5]]]], [[[6], [7, 8]], None])
    assert flat == [[1, 2], [3], [4], [6], [7, 8], [5]] and coff.tolist() == [0, 2, 3, 5, 6] and neg.tolist() == [0, 0, 1, 0]
    assert goff.tolist() == [0, 3, 4] and coff.dtype == goff.dtype == np.uint64 and neg.dtype == np.uint8
    assert TokenIndex._cnf_tables([[[[5]]]], [[]])[2].tolist() == [0]                                  # an empty exclusion: none
    one = [[1]]
    for bad, ex in (([[]], None), ([[[]]], None), ([[one] * 17], None), ([[one] * 16], [[[2]]]), ([[[[1]] * 65]], None),
                    ([[[[1]] * 60]], [[[2]] * 5]), ([[one]], [[[1]], [[2]]])):
        with pytest.raises(ValueError):
            TokenIndex._cnf_tables(bad, ex)
    assert TokenIndex._cnf_tables([[one] * 15], [[[2]]])[3].tolist() == [0, 16] and len(TokenIndex._cnf_tables([[[[1]] * 64]], None)[0]) == 64


# ---- the models ----------------------------------------------------------------------------------------------------------------

HAND_T = [1, 2, 1, 2, 3, 1, 2]
HAND_STARTS = [0, 0, 2, 5, 5, 7]          # documents 1 = [1 2], 2 = [1 2 3], 4 = [1 2]; 0, 3 and 5 are empty


def _hand():
    t, starts = np.array(HAND_T, np.int32), np.array(HAND_STARTS, np.int32)
    sa = dc.model_sa(t)
    da, pv = dc.model_da_pv(sa, starts)
    return {"t": t, "starts": starts, "sa": sa, "da": da, "pv": pv, "rk": ac.model_rk(da), "cl": ac.closed(starts, t.size)}


def test_models_on_the_hand_counted_table():
    c = _hand()
    t, starts = c["t"], c["starts"]
    assert c["sa"].tolist() == [5, 0, 2, 6, 1, 3, 4] and c["da"].tolist() == [4, 1, 2, 4, 1, 2, 2]
    # literals as rank ranges: [1 2] = 0 .. 2, [2] = 3 .. 5, [3] = 6, [2 3] = rank 5, [1] = 0 .. 2, [1 2 3] = rank 2
    P12, P2, P3, P23, P123 = (0, 3), (3, 3), (6, 1), (5, 1), (2, 1)

    def a(group, budget=0):
        return cc.cnf_a(cc.walk_of(c, group), budget)

    # ([3] OR [1 2 3]) AND [2]: the driver is clause 0 (sum 2 < 3); document 2 once, at [3], and a duplicate at [1 2 3]
    assert a(cc.positive([[P3, P123], [P2]])) == ((1, 1, 1, 1, 0, 2, 2, 2), [(2, 2)])
    assert cc.cnf_b(t, starts, [[[3], [1, 2, 3]], [[2]]], [0, 0]) == ([2], [2, 3])
    # a driver chosen by its sum, not by its smallest literal: {[3], [1 2]} sums 4, {[2]} sums 3
    head, ent = a(cc.positive([[P3, P12], [P2]]))
    assert head == (3, 3, 3, 0, 1, 1, 3, 3) and ent == [(4, 1), (1, 1), (2, 1)]
    assert cc.cnf_b(t, starts, [[[3], [1, 2]], [[2]]], [0, 0]) == ([1, 2, 4], [4, 3])
    # a tie of sums goes to the lower clause index: the rank order of [1 2], then swapped that of [2]
    assert a(cc.positive([[P12], [P2]])) == ((3, 3, 3, 0, 0, 1, 3, 3), [(4, 0), (1, 0), (2, 0)])
    assert a(cc.positive([[P2], [P12]])) == ((3, 3, 3, 0, 0, 1, 3, 3), [(4, 1), (1, 1), (2, 1)])
    assert a(cc.positive([[P23, P3], [P12], [P123, P123]]))[0][4:] == (0, 2, 2, 2)                     # 2, 3, 2: clause 0, not 2
    # a negated clause with the smallest sum is not the driver: [1 2] but not [3] -> documents 4 and 1
    assert a(([[P3], [P12]], [1, 0])) == ((2, 2, 3, 0, 1, 1, 3, 3), [(4, 0), (1, 0)])
    assert cc.cnf_b(t, starts, [[[3]], [[1, 2]]], [1, 0]) == ([1, 4], [1, 3])
    # an exclusion that removes one document; an exclusion of two literals that removes all; an empty exclusion literal removes none
    assert a(([[P2], [P23]], [0, 1]))[1] == [(4, 1), (1, 1)] and a(([[P2], [P23, P12]], [0, 1]))[0][:3] == (0, 0, 3)
    assert a(([[P2], [(3, 0)]], [0, 1]))[0][:3] == (3, 3, 3)
    # OR inside the driver: [3] OR [2] walks rank 6 and then 3 .. 5; document 2 is a duplicate under [2]
    head, ent = a(cc.positive([[P3, P2]]))
    assert head == (3, 3, 3, 1, 0, 2, 4, 4) and ent == [(2, 2), (4, 1), (1, 1)]
    # the budget is consumed in literal order: 1 rank = [3] alone, 2 = one rank of [2], then 3, then all
    assert [a(cc.positive([[P3, P2]]), b)[0] for b in (1, 2, 3, 4, 5)] == [(1, 1, 1, 0, 0, 2, 1, 4), (2, 2, 2, 0, 0, 2, 2, 4),
                                                                          (3, 3, 3, 0, 0, 2, 3, 4), (3, 3, 3, 1, 0, 2, 4, 4), (3, 3, 3, 1, 0, 2, 4, 4)]
    # a positive all-empty clause is the driver: everything is 0 but the clause's index and size
    assert a(cc.positive([[P12], [(2, 0), (9, 4)]])) == ((0, 0, 0, 0, 1, 2, 0, 0), [])
    assert cc.cnf_b(t, starts, [[[1, 2]], [[9], [8, 8]]], [0, 0]) == ([], [3, 0])
    # rows: the 64-bit fields as low and high words, written cut to the cap
    docs, offs, heads = cc.cnf_rows([a(cc.positive([[P3, P2]]))], 2)
    assert heads[0].tolist() == [2, 3, 3, 1, 0, 2, 4, 0, 4, 0, 0, 0] and docs[0].tolist() == [2, 4] and offs[0].tolist() == [2, 1]
    flat, coff, neg, goff = cc.tables([cc.positive([[P3, P2], [P12]]), ([[P2], [P23]], [0, 1])])
    assert flat == [P3, P2, P12, P2, P23] and coff.tolist() == [0, 2, 3, 4, 5] and neg.tolist() == [0, 0, 0, 1] and goff.tolist() == [0, 2, 4]


def test_driver_sum_is_formed_in_64_bits():
    big = 2 ** 31 - 1
    assert 3 * big > 2 ** 32 and (3 * big) % 2 ** 32 < big                                            # a 32-bit sum would pick clause 0
    assert cc.driver_of([3 * big, big], [0, 0]) == 1 and cc.driver_of([64 * big, 64 * big], [0, 0]) == 0
    assert cc.driver_of([0, 5, 3], [1, 0, 0]) == 2 and cc.driver_of([5, 5, 5], [1, 0, 0]) == 1
    head = cc.cnf_a((0, 64, 64 * big, []), 0)[0]
    docs, offs, heads = cc.cnf_rows([(head, [])], 1)
    assert head[6] == head[7] == 64 * big and int(heads[0, 8]) | int(heads[0, 9]) << 32 == 64 * big and heads[0, 9] == 31


@pytest.mark.parametrize("name", list(dc.RANDOM))
def test_models_agree_on_the_random_texts(name):
    c, e = ac.random_case(name), nc.expected(name)
    t, starts = c["t"], c["starts"]
    drivers, negs, dups = set(), 0, 0
    for cfg in ((0, 0, 1), (1, 0, 0)):
        spans = e["spans"][cfg].tolist()
        pats = [ctx[len(ctx) - sp[2]:] for ctx, sp in zip(e["ctx"], spans)]
        for clauses, neg in cc.random_queries(len(pats)):
            group = ([[(spans[i][0], spans[i][1]) for i in cla] for cla in clauses], neg)
            head, ent = cc.cnf_a(cc.walk_of(c, group), 0, most=1 << 20)
            both, sums = cc.cnf_b(t, starts, [[pats[i] for i in cla] for cla in clauses], neg)
            assert head[1] == len(both) and sorted(d for d, _ in ent) == both and len({d for d, _ in ent}) == len(ent), (name, cfg, clauses)
            assert head[4] == cc.driver_of(sums, neg) and head[7] == sums[head[4]] == head[6], (name, cfg, clauses)
            union = set().union(*[set(dc.doc_of(starts, dc.occurrences(t, pats[i])).tolist()) for i in clauses[head[4]]])
            assert head[2] == len(union), (name, cfg, clauses)                                         # candidates: the distinct documents
            drivers.add(head[4] > 0)
            negs += any(neg) and head[1] < head[2]
            dups += head[3] > 0
    assert drivers == {True, False} and negs and dups


def test_the_row_loop_is_run_past_the_launch_cap():
    """tq_cnf_kernel strides over the groups beyond the launch cap; its launch-cap test is in test_gpu_token_cnf.py"""
    import token_walk_cases as wc
    src = open(os.path.join(ROOT, "suffixarray_amd", "csrc", "token_cnf.hpp")).read()
    assert len(re.findall(r"w < g\.G; w \+= stride\)", src)) == 1 and "wave_row_grid(g.G)" in src and src.count("__global__") == 1
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_token_cnf.py")).read()
    rows = (wc.CAP_ROWS, wc.CAP_ROWS + 1, 2 * wc.CAP_ROWS + 1)
    assert rows == (16384, 16385, 32769) and "def test_launch_cap" in gpu_tests and "for G in %r:" % (rows,) in gpu_tests


def test_case_lists_reach_their_edges():
    assert cc.N_EQ <= 70000
    # de-duplication: the second literal's first candidate at lanes 63, 0 and 1 of the next window, across a 256-rank trip, nested
    assert {0, 1, 63, 64, 65, 255, 256, 257, cc.DEDUP_K2} == set(cc.DEDUP_OVERLAPS) and cc.DEDUP_K1 >= cc.DEDUP_K2 > 257 + 64
    assert all((cc.DEDUP_K1 - o) % 64 for o in cc.DEDUP_OVERLAPS if o)                                 # a start on no window boundary
    for Ld in (1, 2):
        c = cc.equal_case(Ld)
        for group in cc.dedup_groups():
            lits = group[0][0]
            w = cc.walk_of(c, group)
            assert w[0] == 0, group
            head = cc.cnf_a(w, 0, most=1 << 20)[0]
            union = set()
            for f, k in lits:
                union |= set(c["da"][f:f + k].tolist())
            assert head[2] == len(union) and head[6] == head[7] == sum(k for _, k in lits), (Ld, group)
            if Ld == 1 and len(lits) == 2 and lits[0] != lits[1]:
                o = cc.DEDUP_K1 - lits[1][0]
                assert head[3] == o and (o == cc.DEDUP_K2 or w[3][cc.DEDUP_K1 + o][:2] == (cc.DEDUP_K1 + o, cc.DEDUP_K1)), group
        assert any(cc.cnf_a(cc.walk_of(c, g), 0)[0][3] == cc.DEDUP_K1 // Ld + (Ld == 2) for g in cc.dedup_groups()[-2:-1]), Ld
    c = cc.equal_case(1)
    # budgets either side of the first literal and of the sum; caps either side of 16 with the 16th match from the second literal
    g = cc.dedup_groups()[1]
    assert cc.budgets_of(g) == [0, 400, 401, 402, 733, 734, 735]
    assert set(cc.CAPS) == {0, 1, 16}
    got = [cc.cnf_a(cc.walk_of(c, g), 0) for g in cc.cap_groups()]
    assert [h[1] for h, _ in got] == [0, 1, 15, 16, 17] and all(h[4] == 0 and h[5] == 2 for h, _ in got)
    assert [d for d, _ in got[4][1][15:]] == [cc.N_EQ - 1 - 100, cc.N_EQ - 1 - 101]
    # the limits
    lim = cc.limit_groups()
    assert len(lim[0][0][0]) == 64 and [len(x) for x in lim[2][0]] == [4] * 16 and len(lim[3][0]) == 16 and sum(lim[3][1]) == 1
    assert sum(len(x) for x in lim[1][0]) == 64
    heads = [cc.cnf_a(cc.walk_of(c, g), 0)[0] for g in lim]
    assert heads[0][2:6] == (20 * 63 + 25, 5 * 63, 0, 64) and heads[2][4:6] == (15, 4) and heads[3][4:6] == (15, 1) and heads[3][1] == 40
    assert heads[2][1] and heads[2][3] and heads[1][1] < heads[1][2]
    # the driver rule and the probes on the planted text
    p = cc.planted_case()
    n = p["t"].size
    dg = cc.driver_groups(n)
    heads = [cc.cnf_a(cc.walk_of(p, g), 0)[0] for g in dg]
    assert [h[4] for h in heads] == [1, 0, 0, 0, 0, 1, 0, 1, 0, 1, 1, 0, 0] and [h[7] for h in heads][:4] == [8, 8, 5, 5]
    assert all(h[:4] == (0, 0, 0, 0) and h[6:] == (0, 0) for h in heads[8:11]) and heads[9][5] == 2 and heads[11][5] == 2 and heads[11][7] == 5
    probes = cc.probe_groups(p)
    assert len(probes) >= 200 and {w for _, w in probes} == {True, False}
    sizes = set()
    for group, want in probes:
        A = group[0][0][0]
        w = cc.walk_of(p, group)
        assert w[0] == 0 and w[3][0][1] == A[0] and (w[3][0][4] == 2) is want, (group, w[3][:2])
        sizes |= {(len(cla), ng) for cla, ng in zip(group[0][1:], group[1][1:])}
    assert {(1, 0), (2, 0), (16, 0), (1, 1), (2, 1), (16, 1)} <= sizes
    D = p["starts"].size
    assert any(int(p["da"][g[0][0][0][0]]) == D - 1 for g, _ in probes)                                # the last document: RK[n]
    # random queries: both limits, exclusions, 1, 2 and 4 literals
    rq = cc.random_queries(500)
    assert any(len(c_) == 16 for c_, _ in rq) and any(sum(map(len, c_)) == 64 for c_, _ in rq) and any(any(ng) for _, ng in rq)
    assert {len(x) for c_, _ in rq[:48] for x in c_} >= {1, 2, 4}
