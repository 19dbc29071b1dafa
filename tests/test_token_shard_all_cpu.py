"""Per-document counts and AND groups over a shard set without a GPU: the combine model that test_gpu_token_shard_all.py measures
the device against (token_shard_all_cases.py, model A) agrees with a window scan of the shards (model B) on the planted and the
random sets and with hand-counted tables; every new entry point is declared, exported and bound; the two new structs match the C
compiler's view of the header; every argument error is answered with -1 before a set or a device is touched; the case lists hold
the edges they are there for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_all_cases as ta
import token_doc_cases as td
import token_shard_all_cases as sa
import token_shard_doc_cases as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_shards_prepare_doc_ranks", "sa_hip_token_shards_doc_ranks_info", "sa_hip_token_shards_doc_counts_batch_device",
       "sa_hip_token_shards_doc_counts_batch", "sa_hip_token_shards_all_batch_device", "sa_hip_token_shards_all_batch",
       "sa_hip_token_shards_all_merge_device"]


# ---- model A against model B ---------------------------------------------------------------------------------------------------

def _a_against_b(cases, pats, groups, where):
    """groups: index groups over pats.  -> (groups with a match, groups whose driver is not every shard's rarest span)"""
    sa.ranked(cases)
    spans = sd.spans_of(cases, pats)
    base = sd.bases(cases)
    held = other = 0
    for members in groups:
        gs = sa.group_spans(spans, members)
        both, tfs = sa.all_b_set(cases, [pats[p] for p in members])
        head, ent, parts = sa.all_set(cases, gs, sa.MOST, 0)
        drv, C, cd, es = sa.plan_set(cases, gs, 0)
        assert C == [sum(f.values()) for f in tfs], (where, members)                                   # the sums the driver rule is applied to
        assert head[1] == drv == min(range(len(C)), key=lambda j: (C[j], j)) and head[5] == head[2] == C[drv], (where, members)
        assert head[3] == len(both) == len(ent) and sorted(d for d, _ in ent) == both, (where, members, head, both[:8])
        assert head[4] == len(tfs[drv]) >= head[3], (where, members)                                   # candidates: the documents of the driver
        shard_of = [int(np.searchsorted(base, d, "right")) - 1 for d, _ in ent]
        assert shard_of == sorted(shard_of), (where, members)                                          # the shards' lists one after another
        for j, p in enumerate(members):                                                                # the counts in the matched documents
            sp = sd.context(spans, p)
            for d in both[:6] + [base[-1] - 1, base[-1], 2 ** 63]:
                assert sa.count_set(cases, sp, d) == tfs[j].get(d, 0), (where, members, j, d)
        for cap in (0, 1, 3):
            h2, e2, _ = sa.all_set(cases, gs, cap, 0)
            assert h2 == (min(head[3], cap),) + head[1:] and e2 == ent[:cap]
        for budget in sd.budget_edges(cd):                                                             # a prefix of the driver's hits, shard by shard
            h3, e3, p3 = sa.all_set(cases, gs, sa.MOST, budget)
            ex = min(C[drv], budget) if budget else C[drv]
            assert h3[2] == ex == sum(e for e, _, _ in p3) and h3[1] == drv and h3[5] == C[drv], (where, members, budget)
            in3 = set(e3)
            assert e3 == [x for x in ent if x in in3] and h3[3] <= head[3] and h3[4] <= head[4], (where, members, budget)
            assert (h3[3], h3[4]) == (head[3], head[4]) or ex < C[drv], (where, members, budget)
        held += head[3] > 0
        rarest = [min(range(len(members)), key=lambda j: (row[j][1], j)) for row in gs]
        other += any(r != drv for r in rarest)
    return held, other


def test_models_agree_on_the_driver_plants():
    cases = sa.driver_set()
    pats = [sa.X, sa.Y, sa.Z, sa.W, [5, 5], [1], [2, 3], []]
    spans = sd.spans_of(cases, pats)
    for name, j in (("X", 0), ("Y", 1), ("Z", 2), ("W", 3)):
        assert tuple(c for _, c in sd.context(spans, j)) == sa.DRIVER_TOTALS[name], name
    groups = [[0, 1], [2, 3], [3, 2], [0, 1, 2], [1], [0, 4], [3, 0], [5, 6], [7, 0], [5, 6, 7, 1], list(range(8)) * 2]
    held, other = _a_against_b(cases, pats, groups, "driver")
    assert held >= 6 and other >= 3


@pytest.mark.parametrize("Ld", td.LDS)
def test_models_agree_on_the_all_equal_shards(Ld):
    cases = sd.equal_set(Ld)
    pats = [[sd.A] * m for m in (1, 2, 64, 1100, 1101, 1300, 1301, 1500, 1501)] + [[sd.A + 1], []]
    groups = [[0, 1], [2, 0], [3, 4], [5, 6, 0], [7, 0], [8, 0], [9, 0], [10, 2], [4, 4], [6], list(range(9))]
    held, _ = _a_against_b(cases, pats, groups, ("eq", Ld))
    assert held == 8


@pytest.mark.parametrize("name", sorted(sd.RANDOM))
def test_models_agree_on_the_random_sets(name):
    cases = sd.random_set(name)
    pats = sa.frequent_patterns(cases) + sd.random_patterns(cases)[:20]
    groups = sa.random_groups(len(pats))
    held, other = _a_against_b(cases, pats, groups, name)
    assert held > len(groups) // 4 and other >= 1, (held, other)                   # some group whose driver is not a shard's rarest span


def test_hand_counted_tables():
    cases = sa.driver_set()
    assert sd.bases(cases) == [0, 9, 16, 20]
    flat = [p for g in sa.DRIVER_GROUPS for p in g]
    spans = sd.spans_of(cases, flat)
    at = 0
    for g, want in zip(sa.DRIVER_GROUPS, sa.DRIVER_WANT):
        head, ent, parts = sa.all_set(cases, sa.group_spans(spans, range(at, at + len(g))), sa.MOST, 0)
        at += len(g)
        assert (head[1], head[5], head[3], head[4]) == want and head[2] == head[5], (g, head, want)
    # {X, Y}: the driver Y has 10, 1 and 3 ranks; shard 0 matches its documents 0 and 1, shard 1 its document 1 (global 10), shard 2
    # its documents 0 and 2 (global 16 and 18)
    gs = sa.group_spans(spans, [0, 1])
    head, ent, parts = sa.all_set(cases, gs, sa.MOST, 0)
    assert sorted(d for d, _ in ent) == [0, 1, 10, 16, 18] and parts == [(10, 2, 6), (1, 1, 1), (3, 2, 2)]
    assert [d for d, _ in ent][2] == 10                                                               # shard order
    assert sa.all_set(cases, gs, 8, 10)[2] == [(10, 2, 6), (0, 0, 0), (0, 0, 0)]                       # the budget ends with shard 0
    assert sa.all_set(cases, gs, 8, 11)[2] == [(10, 2, 6), (1, 1, 1), (0, 0, 0)]
    assert sa.all_set(cases, gs, 8, 12)[0][2:5] == (12, sa.all_set(cases, gs, 8, 12)[0][3], 8)
    assert sa.all_set(cases, gs, 2, 0)[0] == (2, 1, 14, 5, 9, 14) and len(sa.all_set(cases, gs, 2, 0)[1]) == 2
    assert sa.all_set(cases, gs, 0, 0)[0] == (0, 1, 14, 5, 9, 14) and sa.all_set(cases, gs, 0, 0)[1] == []
    # counts: X in document 0 of shard 1 (global 9) three times, in its document 2 (global 11) four times
    x = sd.context(spans, 0)
    assert [sa.count_set(cases, x, d) for d in (0, 1, 2, 8, 9, 10, 11, 12, 16, 17, 18, 19, 20, 2 ** 63)] == [1, 1, 0, 0, 3, 2, 4, 3, 1, 1, 1, 0, 0, 0]
    y = sd.context(spans, 1)
    assert [sa.count_set(cases, y, d) for d in (0, 1, 5, 10, 18)] == [1, 2, 3, 1, 2]
    rows = sa.counts_rows(cases, [[s] for s in x], [[9, 11, 0]], written=[2])
    assert rows.tolist() == [[3, 4, sa.FILL32]]
    # the edge plants: what the middle shard matches is what was planted
    ecases, groups, want, last_at = sa.edge_set()
    assert len(want) == len(groups) == last_at + 3 and last_at >= 40 and [w for _, w in want[last_at:]] == [False, True, False]
    assert sum(w for _, w in want[:last_at]) * 2 == last_at                                            # a_B - 1 and end_B miss, a_B and end_B - 1 hit
    for g, (doc, hit) in zip(groups, want):
        head, ent, parts = sa.all_set(ecases, g, sa.MOST, 0)
        assert head[1] == 0 and parts[1][0] in (1, 2) and ((doc in [d for d, _ in ent]) == hit), (g, parts, doc, hit)
    assert want[-1][0] == sd.bases(ecases)[2] - 1                                                     # the last document of the middle shard


# ---- the case lists hold their edges -------------------------------------------------------------------------------------------

def test_case_lists_contain_their_edges():
    spans = sd.equal_contexts()
    groups = sa.equal_groups()
    sizes = {len(g) for g in groups}
    assert {1, 2, 3, ta.ALL_MAX} <= sizes and any(len(set(g)) < len(g) for g in groups)
    for Ld in (1, 64, 257):
        cases = sa.ranked(sd.equal_set(Ld))
        drivers, empty, over, last, cands = set(), 0, 0, 0, set()
        for members in groups:
            gs = sa.group_spans(spans, members)
            drv, C, cd, es = sa.plan_set(cases, gs, 0)
            drivers.add(drv)
            empty += C[drv] == 0
            b = sd.budget_edges(cd)
            run = 0
            for c in cd:
                assert {x for x in (run - 1, run, run + 1) if x >= 0} <= set(b)
                run += c
            assert {0, run, run + 1} <= set(b) and max(b) > run
            parts = sa.all_set(cases, gs, sa.MOST, 0)[2]
            caps = sd.cap_edges([m for _, m, _ in parts])
            assert set(td.CAPS) <= set(caps)
            over += any(m > c for _, m, _ in parts for c in caps if c)                                # a shard alone beyond the cap
            last += parts[-1][1] > 0 and sum(m for _, m, _ in parts) in caps                          # the cap reached exactly at the last shard
            cands |= {e for e, _, _ in parts}
        assert len(drivers) >= 2 and empty and over and last, Ld
        assert {63, 64, 65, 255, 256, 257, 1025} <= cands, Ld                                         # the walk's lanes and trips inside one shard
    cases = sa.driver_set()
    assert all(len(c["t"]) < 4000 for c in cases) and all(len(c["t"]) <= 4000 for c in sa.edge_set()[0])
    ids = sa.count_ids(cases)
    base = sd.bases(cases)
    assert {0, base[1] - 1, base[1], base[-1] - 1, base[-1], 2 ** 63} <= set(ids)
    for name in sd.RANDOM:                                                                            # empty documents at the end of a shard
        text, lens, Ds, empties = sd.RANDOM[name]
        assert any(empties)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------

def test_shard_all_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int, name
    for name in ("prepare_doc_ranks", "doc_ranks_info", "doc_counts_batch", "doc_counts_batch_device", "all_batch", "all_batch_device",
                 "all_merge_device"):
        assert callable(getattr(capi.TokenShards, name)), name
    from suffixarray_amd import token_shards
    for name in ("prepare_document_ranks", "term_counts", "documents_with_all", "count_documents_with_all"):
        assert callable(getattr(token_shards.ShardedTokenIndex, name)), name
    dt, cls = capi.SHARDS_ALL_DTYPE, capi.TokenShardsAll
    assert dt.itemsize == C.sizeof(cls) == 40
    assert dt.names == tuple(f for f, _ in cls._fields_)
    assert [dt.fields[f][1] for f in dt.names] == [getattr(cls, f).offset for f in dt.names]
    assert capi.SHARDS_ALL_PAIR_DTYPE.itemsize == 16 and capi.SHARDS_ALL_PLAN_DTYPE.itemsize == 16
    assert "Per-document counts and AND groups (6e) over a set\n * are not built" not in header
    assert "(6h)" in header


@pytest.mark.parametrize("struct, cls, fields", [
    ("sa_hip_token_shards_all", "TokenShardsAll", ["written", "driver", "examined", "matched", "candidates", "count"]),
    ("sa_hip_token_shards_ranks_stats", "TokenShardsRanksStats", ["present", "chunk", "bytes", "prepare_ms", "counts_q", "counts_ms",
                                                                  "plan_q", "plan_ms", "pairs_q", "pairs_ms", "merge_q", "merge_ms",
                                                                  "streamed"]),
])
def test_shard_all_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields):
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


def test_shard_all_argument_errors_before_any_device_call(capi):
    """the set is an address that holds nothing: every refusal below comes before it is looked at"""
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    goff = np.array([0, 2], np.uint64)
    spans = np.zeros(4, capi.SPAN_DTYPE)
    docs, offs, cnt, wr = np.zeros(8, np.uint64), np.zeros(8, np.int32), np.zeros(8, np.uint32), np.zeros(2, np.uint32)
    ah = np.zeros(2, capi.SHARDS_ALL_DTYPE)
    p, o, go, s, d, f, c, w, k = (a.ctypes.data for a in (pat, off, goff, spans, docs, offs, cnt, wr, ah))
    D = 1 << 20                                                    # "device pointers": never touched
    err = lib.sa_hip_last_error

    def counts_dev(set_=h, sp=D, q=2, cap=4, dd=D, wd=None, stride=4, cd=D):
        return lib.sa_hip_token_shards_doc_counts_batch_device(set_, sp, q, cap, dd, wd, stride, cd)

    def counts_host(set_=h, pp=p, oo=o, q=2, mode=0, need=0, cap=4, dd=d, ww=w, cc=c, ss=s):
        return lib.sa_hip_token_shards_doc_counts_batch(set_, pp, oo, q, mode, 0, need, cap, dd, ww, cc, ss)

    def all_dev(set_=h, sp=D, P=2, gg=go, G=1, cap=4, budget=0, dd=D, ff=D, hh=D):
        return lib.sa_hip_token_shards_all_batch_device(set_, sp, P, gg, G, cap, budget, dd, ff, hh)

    def all_host(set_=h, pp=p, oo=o, P=2, gg=go, G=1, mode=0, need=0, cap=4, budget=0, ss=s, dd=d, ff=f, hh=k):
        return lib.sa_hip_token_shards_all_batch(set_, pp, oo, P, gg, G, mode, 0, need, cap, budget, ss, dd, ff, hh)

    def merge(set_=h, dd=D, ff=D, hh=D, pl=D, bb=D, G=2, cap=4, od=D, of=D, oh=D):
        return lib.sa_hip_token_shards_all_merge_device(set_, dd, ff, hh, pl, bb, G, cap, od, of, oh)

    # NULL set
    assert lib.sa_hip_token_shards_prepare_doc_ranks(None, 1) == -1
    assert b"sa_hip_token_shards_prepare_doc_ranks" in err()
    assert lib.sa_hip_token_shards_prepare_doc_ranks(None, 0) == -1
    assert lib.sa_hip_token_shards_doc_ranks_info(None, C.byref(capi.TokenShardsRanksStats())) == -1
    assert lib.sa_hip_token_shards_doc_ranks_info(h, None) == -1
    for call in (counts_dev, counts_host, all_dev, all_host, merge):
        assert call(set_=None) == -1, call.__name__
        assert b"NULL handle" in err(), call.__name__
    # on is 0 or 1
    for on in (2, -1):
        assert lib.sa_hip_token_shards_prepare_doc_ranks(h, on) == -1
    assert b"0 or 1" in err()
    # mode and need_next are 0 or 1, also with Q == 0 / G == 0
    for mode, need in ((2, 0), (-1, 0), (0, 2), (1, -1)):
        assert counts_host(mode=mode, need=need) == -1 and counts_host(mode=mode, need=need, q=0) == -1, (mode, need)
        assert all_host(mode=mode, need=need) == -1 and all_host(mode=mode, need=need, G=0) == -1, (mode, need)
    # cap == 0 in doc_counts
    for q in (2, 0):
        assert counts_dev(q=q, cap=0) == -1 and counts_host(q=q, cap=0) == -1
    assert b"cap == 0" in err()
    # the stride of written
    for stride in (0, 2, 3, 5, 6, 41):
        assert counts_dev(wd=D, stride=stride) == -1, stride
        assert b"written_stride" in err()
    # Q * cap, G * cap, P >= 2^31
    for q, cap in ((1 << 31, 1), (1 << 20, 1 << 11), (1, 0xFFFFFFFF), (3, 0x80000000 // 3 + 1)):
        assert counts_dev(q=q, cap=cap) == -1 and counts_host(q=q, cap=cap) == -1, (q, cap)
        assert all_dev(G=q, cap=cap) == -1 and all_host(G=q, cap=cap) == -1 and merge(G=q, cap=cap) == -1, (q, cap)
        assert b"2^31" in err()
    assert all_dev(P=1 << 31) == -1 and b"P >= 2^31" in err()
    assert all_host(P=1 << 31) == -1 and b"P >= 2^31" in err()
    assert all_dev(P=1 << 31, G=0) == -1
    # the group table
    for tab, what in (([1, 2], b"group_offsets[0]"), ([0, 0], b"empty group"), ([0, 1], b"end at"), ([0, 3], b"end at")):
        t = np.array(tab, np.uint64)
        assert all_dev(gg=t.ctypes.data) == -1 and what in err(), tab
        assert all_host(gg=t.ctypes.data) == -1 and what in err(), tab
    big = np.array([0, 17], np.uint64)
    assert all_dev(P=17, gg=big.ctypes.data) == -1 and b"SA_HIP_TOKEN_ALL_MAX" in err()
    assert all_dev(gg=None) == -1 and all_host(gg=None) == -1
    # NULL arguments (written, and the spans of the host forms, may be NULL: not among them; bases of the merge may be NULL)
    assert counts_dev(sp=None) == -1 and counts_dev(dd=None) == -1 and counts_dev(cd=None) == -1
    assert counts_host(oo=None) == -1 and counts_host(dd=None) == -1 and counts_host(cc=None) == -1
    assert counts_host(pp=None) == -1                                                                 # symbols without a buffer
    assert all_dev(sp=None) == -1 and all_dev(dd=None) == -1 and all_dev(ff=None) == -1 and all_dev(hh=None) == -1
    assert all_dev(cap=0, dd=None, ff=None, hh=None) == -1 and all_dev(cap=0, sp=None, dd=None, ff=None) == -1
    assert all_host(oo=None) == -1 and all_host(dd=None) == -1 and all_host(ff=None) == -1 and all_host(hh=None) == -1
    assert all_host(cap=0, dd=None, ff=None, hh=None) == -1 and all_host(pp=None) == -1
    for name in ("dd", "ff", "hh", "pl", "od", "of", "oh"):
        assert merge(**{name: None}) == -1, name
    assert merge(cap=0, dd=None, ff=None, od=None, of=None, hh=None) == -1 and merge(cap=0, dd=None, ff=None, od=None, of=None, oh=None) == -1
    assert merge(cap=0, dd=None, ff=None, od=None, of=None, pl=None) == -1
    # descending offsets
    assert counts_host(oo=down.ctypes.data) == -1 and b"descend" in err()
    assert all_host(oo=down.ctypes.data) == -1 and b"descend" in err()
    # Q == 0 and G == 0 with good arguments: no-ops that touch nothing
    assert counts_dev(sp=None, q=0, dd=None, cd=None) == 0
    assert counts_dev(sp=None, q=0, dd=None, wd=D, stride=40, cd=None) == 0
    assert lib.sa_hip_token_shards_doc_counts_batch(h, None, None, 0, 1, 0, 1, 4, None, None, None, None) == 0
    assert all_dev(sp=None, P=0, gg=None, G=0, dd=None, ff=None, hh=None) == 0
    assert all_dev(sp=None, P=5, gg=None, G=0, cap=0, budget=7, dd=None, ff=None, hh=None) == 0
    assert lib.sa_hip_token_shards_all_batch(h, None, None, 0, None, 0, 1, 0, 1, 4, 0, None, None, None, None) == 0
    assert merge(dd=None, ff=None, hh=None, pl=None, bb=None, G=0, od=None, of=None, oh=None) == 0
    with pytest.raises(ValueError):
        capi.TokenShards(C.c_void_p(), 2).doc_counts_batch([[1], [2]], [[0, 1]])                       # refused before the library is asked
    with pytest.raises(ValueError):
        capi.TokenShards(C.c_void_p(), 2).doc_counts_batch([[1], [2]], [[0], [1]], written=[1])
