"""Documents over a shard set without a GPU: the combine model that test_gpu_token_shard_docs.py measures the device against
(token_shard_doc_cases.py, model A) agrees with a window scan of the shards (model B) on the planted and the random sets and with
hand-counted tables; every new entry point is declared, exported and bound; the three new structs match the C compiler's view of
the header; every argument error is answered with -1 before a set or a device is touched; the case lists hold the edges they are
there for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_doc_cases as td
import token_shard_doc_cases as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_shards_set_documents", "sa_hip_token_shards_adopt_documents", "sa_hip_token_shards_doc_bases",
       "sa_hip_token_shards_docs_info", "sa_hip_token_shards_locate_batch_device", "sa_hip_token_shards_locate_batch",
       "sa_hip_token_shards_docs_batch_device", "sa_hip_token_shards_docs_batch", "sa_hip_token_shards_docs_merge_device"]


# ---- model A against model B ---------------------------------------------------------------------------------------------------

def _a_against_b(cases, pats, where):
    spans = sd.spans_of(cases, pats)
    base = sd.bases(cases)
    assert base[-1] == sum(len(c["starts"]) for c in cases)
    held = 0
    for i, p in enumerate(pats):
        sp = sd.context(spans, i)
        count, distinct, hits = sd.model_b(cases, p)
        head, ent = sd.docs_set(cases, sp, sd.MOST, 0)
        assert head == (distinct, count, distinct, count), (where, p[:6], head, count, distinct)
        assert len({d for d, _ in ent}) == len(ent) == distinct and set(ent) <= set(hits), (where, p[:6])
        assert {d for d, _ in ent} == {d for d, _ in hits}, (where, p[:6])
        shard_of = [int(np.searchsorted(base, d, "right")) - 1 for d, _ in ent]
        assert shard_of == sorted(shard_of), (where, p[:6])                                           # the shards' lists one after another
        lhead, lent = sd.locate_set(cases, sp, sd.MOST)
        assert lhead == (count, count) and sorted(lent) == hits, (where, p[:6])
        for cap in (1, 3):
            h2, e2 = sd.docs_set(cases, sp, cap, 0)
            assert h2 == (min(distinct, cap), count, distinct, count) and e2 == ent[:cap]
            assert sd.locate_set(cases, sp, cap) == ((min(count, cap), count), lent[:cap])
        for budget in sd.budget_edges([c for _, c in sp]):                                            # a prefix of the hits, shard by shard
            h3, e3 = sd.docs_set(cases, sp, sd.MOST, budget)
            ex = min(count, budget) if budget else count
            front = lent[:ex]
            seen = list(dict.fromkeys(d for d, _ in front))
            assert h3 == (len(seen), ex, len(seen), count) and [d for d, _ in e3] == seen, (where, p[:6], budget)
            assert sum(sd.split_budget([c for _, c in sp], budget)) == ex
        held += count > 0
    return held


@pytest.mark.parametrize("Ld", td.LDS)
def test_models_agree_on_the_planted_sets(Ld):
    cases = sd.equal_set(Ld)
    assert [len(c["t"]) for c in cases] == list(sd.EQ_N) and len(set(sd.EQ_N)) == 3
    for c, n in zip(cases, sd.EQ_N):
        assert c["sa"].tolist() == list(range(n - 1, -1, -1)) and len(c["starts"]) == -(-n // Ld)
    pats = [[sd.A] * m for m in (1, 2, 64, 1100, 1101, 1300, 1301, 1500, 1501)] + [[sd.A + 1], []]
    assert _a_against_b(cases, pats, ("eq", Ld)) == 9
    spans = sd.equal_contexts()                                                                       # the closed form beside the model
    for i in range(len(spans[0])):
        head, _ = sd.docs_set(cases, sd.context(spans, i), sd.MOST, 0)
        assert head[2] == sum(_distinct(n, Ld, f, c) for n, (f, c) in zip(sd.EQ_N, sd.context(spans, i))), (Ld, i)
    assert all(_distinct(td.N_EQ, Ld, f, c) == td.equal_distinct(Ld, f, c) for f, c in spans[0])


def _distinct(n, Ld, first, examined):
    """token_doc_cases.equal_distinct for a shard of n tokens"""
    return 0 if examined == 0 else (n - 1 - first) // Ld - (n - first - examined) // Ld + 1


@pytest.mark.parametrize("name", sorted(sd.RANDOM))
def test_models_agree_on_the_random_sets(name):
    cases = sd.random_set(name)
    text, lens, Ds, empties = sd.RANDOM[name]
    assert [len(c["t"]) for c in cases] == list(lens) and all(n <= 3000 for n in lens)
    for c, D, e in zip(cases, Ds, empties):
        assert len(c["starts"]) == D + e and (c["starts"][D:] == len(c["t"])).all()                   # empty documents at the end ...
        assert int(c["da"].max()) < D or e == 0
    base = sd.bases(cases)
    assert base == [0] + list(np.cumsum([D + e for D, e in zip(Ds, empties)]))                        # ... and the bases count them
    assert any(empties[:-1])
    pats = sd.random_patterns(cases)
    assert _a_against_b(cases, pats, name) > len(pats) // 2
    counts = np.array([[c for _, c in row] for row in sd.spans_of(cases, pats)])
    assert ((counts > 0).any(axis=0) & (counts == 0).any(axis=0)).sum() >= 4                          # held by some shards, missed by others


def test_hand_counted_tables():
    cases = [sd.shard_case([1, 2, 1, 2, 3], [0, 2]), sd.shard_case([1, 2, 9, 1, 2], [0, 0, 3, 5])]
    assert sd.bases(cases) == [0, 2, 6]                                                               # documents 2 and 5 are empty
    spans = sd.spans_of(cases, [[1, 2], [2], [9], [3, 1]])
    assert spans == [[(0, 2), (2, 2), (5, 0), (5, 0)], [(0, 2), (2, 2), (4, 1), (4, 0)]]
    c12 = sd.context(spans, 0)
    # shard 0: [1 2 1 2 3] < [1 2 3]: positions 0 (document 0), 2 (document 1); shard 1: [1 2] < [1 2 9 1 2]: positions 3 (its
    # document 2, global 4), 0 (its document 1, global 3)
    assert sd.locate_set(cases, c12, 8) == ((4, 4), [(0, 0), (1, 0), (4, 0), (3, 0)])
    assert sd.locate_set(cases, c12, 3) == ((3, 4), [(0, 0), (1, 0), (4, 0)])
    assert sd.locate_set(cases, c12, 2) == ((2, 4), [(0, 0), (1, 0)])
    assert sd.docs_set(cases, c12, 8, 0) == ((4, 4, 4, 4), [(0, 0), (1, 0), (4, 0), (3, 0)])
    assert sd.docs_set(cases, c12, 8, 3) == ((3, 3, 3, 4), [(0, 0), (1, 0), (4, 0)])
    assert sd.docs_set(cases, c12, 8, 2) == ((2, 2, 2, 4), [(0, 0), (1, 0)])
    assert sd.docs_set(cases, c12, 1, 9) == ((1, 4, 4, 4), [(0, 0)])
    assert sd.docs_set(cases, c12, 0, 1) == ((0, 1, 1, 4), [])
    # [2]: shard 0 positions 1 (document 0), 3 (document 1); shard 1: [2] < [2 9 1 2]: positions 4 (global 4), 1 (global 3)
    assert sd.docs_set(cases, sd.context(spans, 1), 8, 0) == ((4, 4, 4, 4), [(0, 1), (1, 1), (4, 1), (3, 1)])
    assert sd.docs_set(cases, sd.context(spans, 2), 8, 0) == ((1, 1, 1, 1), [(3, 2)])                 # only shard 1 holds it
    assert sd.docs_set(cases, sd.context(spans, 3), 8, 0) == ((0, 0, 0, 0), [])                       # [3 1] would span the cut
    one = [sd.shard_case([5, 5, 5, 5], [0, 2])]                                                       # two ranks of a document in one span
    assert sd.docs_set(one, [(0, 4)], 8, 0) == ((2, 4, 2, 4), [(1, 1), (0, 1)])
    assert sd.split_budget([3, 0, 5], 0) == [3, 0, 5] and sd.split_budget([3, 0, 5], 3) == [3, 0, 0]
    assert sd.split_budget([3, 0, 5], 4) == [3, 0, 1] and sd.split_budget([3, 0, 5], 2) == [2, 0, 0] and sd.split_budget([3, 0, 5], 99) == [3, 0, 5]


# ---- the case lists hold their edges -------------------------------------------------------------------------------------------

def test_case_lists_contain_their_edges():
    spans = sd.equal_contexts()
    S, Q = len(spans), len(spans[0])
    assert S == 3
    for s in range(S):
        assert {c for _, c in spans[s]} >= set(td.COUNTS), s                                          # window edges, the step +- 1, in every shard
        assert all(f + c <= sd.EQ_N[s] for f, c in spans[s])
        assert {0, 1, 255, 256, 257} <= set(td.COUNTS) and td.UNROLL * 64 == 256
        kinds = {(f == 0, f + c == sd.EQ_N[s]) for f, c in spans[s] if c}
        assert {(True, False), (False, True), (False, False)} <= kinds, s
    triples = [tuple(sd.counts_of(spans, i)) for i in range(Q)]
    assert any(a and not b and c for a, b, c in triples)                                              # the middle shard misses
    assert (0, 0, 0) in triples and any(not a and not b and c for a, b, c in triples) and any(a and not b and not c for a, b, c in triples)
    for i, tr in enumerate(triples):
        b = sd.budget_edges(list(tr))
        run = 0
        for c in tr:
            assert {x for x in (run - 1, run, run + 1) if x >= 0} <= set(b), (i, run)
            assert c < 2 or any(run < x < run + c for x in b), (i, run)                               # inside the span
            run += c
        assert {0, run, run + 1} <= set(b) and max(b) > run
    assert set(sd.all_budgets(spans)) >= set(sd.budget_edges(list(triples[0])))
    for Ld in td.LDS:
        cases = sd.equal_set(Ld)
        over = last = 0
        for i in range(Q):
            sp = sd.context(spans, i)
            d = [sd.docs_set([cases[s]], [sp[s]], sd.MOST, 0)[0][2] for s in range(S)]
            caps = sd.cap_edges(d)
            assert set(td.CAPS) <= set(caps)
            run = 0
            for x in d:
                run += x
                assert {y for y in (run - 1, run, run + 1) if y >= 0} <= set(caps), (Ld, i)
            over += any(x > c for x in d for c in caps if c)                                          # a shard alone beyond the cap
            last += d[-1] > 0 and sum(d) in caps                                                      # the cap reached exactly at the last shard
        assert over and last, Ld


# ---- the ABI -------------------------------------------------------------------------------------------------------------------

def test_shard_docs_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int, name
    for name in ("set_documents", "adopt_documents", "doc_bases", "docs_info", "locate_batch", "locate_batch_device", "docs_batch",
                 "docs_batch_device", "docs_merge_device"):
        assert callable(getattr(capi.TokenShards, name)), name
    from suffixarray_amd import token_shards
    for name in ("set_documents", "document_bases", "locate", "documents", "document_counts"):
        assert callable(getattr(token_shards.ShardedTokenIndex, name)), name
    for dt, cls, size in ((capi.SHARDS_LOCATE_DTYPE, capi.TokenShardsLocate, 16), (capi.SHARDS_DOCS_DTYPE, capi.TokenShardsDocs, 32)):
        assert dt.itemsize == C.sizeof(cls) == size
        assert dt.names == tuple(f for f, _ in cls._fields_)
        assert [dt.fields[f][1] for f in dt.names] == [getattr(cls, f).offset for f in dt.names]
    assert "Documents (locate, document counts) over a set are not built" not in header
    assert "(6g)" in header


@pytest.mark.parametrize("struct, cls, fields", [
    ("sa_hip_token_shards_locate", "TokenShardsLocate", ["written", "reserved", "count"]),
    ("sa_hip_token_shards_docs", "TokenShardsDocs", ["written", "reserved", "examined", "distinct", "count"]),
    ("sa_hip_token_shards_docs_stats", "TokenShardsDocsStats", ["documents", "chunk", "reserved", "locate_q", "locate_ms", "pairs_q",
                                                                "pairs_ms", "merge_q", "merge_ms", "streamed"]),
])
def test_shard_docs_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields):
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


def test_shard_docs_argument_errors_before_any_device_call(capi):
    """the set is an address that holds nothing: every refusal below comes before it is looked at"""
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    spans = np.zeros(4, capi.SPAN_DTYPE)
    docs, offs = np.zeros(8, np.uint64), np.zeros(8, np.int32)
    lh, dh = np.zeros(2, capi.SHARDS_LOCATE_DTYPE), np.zeros(2, capi.SHARDS_DOCS_DTYPE)
    p, o, s, d, f, l, k = (a.ctypes.data for a in (pat, off, spans, docs, offs, lh, dh))
    D = 1 << 20                                                    # "device pointers": never touched
    tabs = (C.c_void_p * 2)(p, p)
    sizes = (C.c_uint32 * 2)(1, 1)
    # NULL set
    assert lib.sa_hip_token_shards_set_documents(None, tabs, sizes) == -1
    assert b"sa_hip_token_shards_set_documents" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_set_documents(None, None, None) == -1
    assert lib.sa_hip_token_shards_adopt_documents(None) == -1
    assert lib.sa_hip_token_shards_doc_bases(None, d) == -1
    assert lib.sa_hip_token_shards_docs_info(None, C.byref(capi.TokenShardsDocsStats())) == -1
    assert lib.sa_hip_token_shards_locate_batch_device(None, D, 2, 4, D, D, D) == -1
    assert lib.sa_hip_token_shards_locate_batch(None, p, o, 2, 4, s, d, f, l) == -1
    assert lib.sa_hip_token_shards_docs_batch_device(None, D, 2, 4, 0, D, D, D) == -1
    assert lib.sa_hip_token_shards_docs_batch(None, p, o, 2, 0, 0, 0, 4, 0, s, d, f, k) == -1
    assert lib.sa_hip_token_shards_docs_merge_device(None, D, D, D, D, 2, 4, D, D, D) == -1
    # one of starts and D without the other; NULL outputs
    assert lib.sa_hip_token_shards_set_documents(h, tabs, None) == -1
    assert lib.sa_hip_token_shards_set_documents(h, None, sizes) == -1
    assert b"both" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_doc_bases(h, None) == -1
    assert lib.sa_hip_token_shards_docs_info(h, None) == -1
    # mode and need_next are 0 or 1
    for mode, need in ((2, 0), (-1, 0), (0, 2), (1, -1)):
        assert lib.sa_hip_token_shards_docs_batch(h, p, o, 2, mode, 0, need, 4, 0, s, d, f, k) == -1, (mode, need)
        assert lib.sa_hip_token_shards_docs_batch(h, p, o, 0, mode, 0, need, 4, 0, s, d, f, k) == -1, (mode, need)   # also with Q == 0
    # cap == 0 in locate
    for q in (2, 0):
        assert lib.sa_hip_token_shards_locate_batch_device(h, D, q, 0, D, D, D) == -1
        assert lib.sa_hip_token_shards_locate_batch(h, p, o, q, 0, s, d, f, l) == -1
    assert b"cap == 0" in lib.sa_hip_last_error()
    # Q * cap >= 2^31
    for q, cap in ((1 << 31, 1), (1 << 20, 1 << 11), (1, 0xFFFFFFFF), (3, 0x80000000 // 3 + 1)):
        assert lib.sa_hip_token_shards_locate_batch_device(h, D, q, cap, D, D, D) == -1, (q, cap)
        assert lib.sa_hip_token_shards_locate_batch(h, p, o, q, cap, s, d, f, l) == -1, (q, cap)
        assert lib.sa_hip_token_shards_docs_batch_device(h, D, q, cap, 0, D, D, D) == -1, (q, cap)
        assert lib.sa_hip_token_shards_docs_batch(h, p, o, q, 0, 0, 0, cap, 0, s, d, f, k) == -1, (q, cap)
        assert lib.sa_hip_token_shards_docs_merge_device(h, D, D, D, D, q, cap, D, D, D) == -1, (q, cap)
    assert b"2^31" in lib.sa_hip_last_error()
    # NULL arguments (spans of the host forms may be NULL: not among them; bases of the merge may be NULL: the set's own)
    for a in ((None, D, D, D), (D, None, D, D), (D, D, None, D), (D, D, D, None)):
        assert lib.sa_hip_token_shards_locate_batch_device(h, a[0], 2, 4, *a[1:]) == -1, a
        assert lib.sa_hip_token_shards_docs_batch_device(h, a[0], 2, 4, 0, *a[1:]) == -1, a
    assert lib.sa_hip_token_shards_docs_batch_device(h, None, 2, 0, 0, None, None, D) == -1           # counts only still needs spans and heads
    assert lib.sa_hip_token_shards_docs_batch_device(h, D, 2, 0, 0, None, None, None) == -1
    for a in ((None, f, l), (d, None, l), (d, f, None)):
        assert lib.sa_hip_token_shards_locate_batch(h, p, o, 2, 4, s, *a) == -1, a
    for a in ((None, f, k), (d, None, k), (d, f, None)):
        assert lib.sa_hip_token_shards_docs_batch(h, p, o, 2, 0, 0, 0, 4, 0, s, *a) == -1, a
    assert lib.sa_hip_token_shards_docs_batch(h, p, o, 2, 0, 0, 0, 0, 0, s, None, None, None) == -1
    assert lib.sa_hip_token_shards_locate_batch(h, p, None, 2, 4, s, d, f, l) == -1
    assert lib.sa_hip_token_shards_docs_batch(h, p, None, 2, 0, 0, 0, 4, 0, s, d, f, k) == -1
    assert lib.sa_hip_token_shards_locate_batch(h, None, o, 2, 4, s, d, f, l) == -1                    # symbols without a buffer
    assert lib.sa_hip_token_shards_docs_batch(h, None, o, 2, 0, 0, 0, 4, 0, s, d, f, k) == -1
    for j in (0, 1, 2, 3, 4, 5):
        a = [D] * 6                                                # docs, offsets, heads, out docs, out offsets, out heads
        a[j] = None
        assert lib.sa_hip_token_shards_docs_merge_device(h, a[0], a[1], a[2], D, 2, 4, a[3], a[4], a[5]) == -1, j
    assert lib.sa_hip_token_shards_docs_merge_device(h, None, None, None, D, 2, 0, None, None, D) == -1
    assert lib.sa_hip_token_shards_docs_merge_device(h, None, None, D, D, 2, 0, None, None, None) == -1
    # descending offsets
    assert lib.sa_hip_token_shards_locate_batch(h, p, down.ctypes.data, 2, 4, s, d, f, l) == -1
    assert b"descend" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_docs_batch(h, p, down.ctypes.data, 2, 1, 0, 0, 4, 0, s, d, f, k) == -1
    # Q == 0 with good arguments: a no-op that touches nothing
    assert lib.sa_hip_token_shards_locate_batch_device(h, None, 0, 4, None, None, None) == 0
    assert lib.sa_hip_token_shards_locate_batch(h, None, None, 0, 4, None, None, None, None) == 0
    assert lib.sa_hip_token_shards_docs_batch_device(h, None, 0, 4, 7, None, None, None) == 0
    assert lib.sa_hip_token_shards_docs_batch_device(h, None, 0, 0, 0, None, None, None) == 0
    assert lib.sa_hip_token_shards_docs_batch(h, None, None, 0, 1, 0, 1, 4, 0, None, None, None, None) == 0
    assert lib.sa_hip_token_shards_docs_merge_device(h, None, None, None, None, 0, 4, None, None, None) == 0
    with pytest.raises(ValueError):
        capi.TokenShards(C.c_void_p(), 2).set_documents([[0], [[0]]])                                  # refused before the library is asked
    with pytest.raises(ValueError):
        capi.TokenShards(C.c_void_p(), 2).set_documents([[0]])
