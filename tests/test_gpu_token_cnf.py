"""CNF document queries of a token index on the device against the two CPU models of token_cnf_cases.py: single-literal clauses
against the AND launch of token_all.hpp byte for byte; the driver rule; de-duplication inside the driver clause at the lane, window
and trip edges; budgets and caps across a literal boundary; OR probes and exclusions on planted literals, the last document included;
the limits of 16 clauses and 64 literals; the launch cap; random texts in both span modes against both models; the device chain
against the host form and into the per-document counts; the Python class."""
import numpy as np
import pytest

import token_all_cases as ac
import token_cases as tc
import token_cnf_cases as cc
import token_doc_cases as dc
import token_next_cases as nc
from test_gpu_token_all import _all_device
from test_gpu_token_docs import _dev, _span_array

pytestmark = pytest.mark.gpu

FILL = cc.FILL
UFILL = FILL & 0xFFFFFFFF


def _cnf_device(gpu, ti, groups, cap, budget, negated=True):
    """one cnf launch over groups (clauses of (first, count) literals, neg) -> (docs[G, max(cap, 1)], offsets, heads uint32[G, 12]);
    a guard row either side of every output"""
    import torch
    flat, coff, neg, goff = cc.tables(groups)
    sp_d = _dev(_span_array(gpu, flat).view(np.int32).reshape(-1, 4))
    G = len(groups)
    d_d = torch.full((G + 2, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
    o_d = torch.full((G + 2, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
    h_d = torch.full((G + 2, 12), FILL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ti.cnf_batch_device(sp_d.data_ptr(), len(flat), coff, neg if negated else None, goff, cap, budget, d_d[1:].data_ptr() if cap else None,
                        o_d[1:].data_ptr() if cap else None, h_d[1:].data_ptr())
    coff[:] = 0                                                                                       # the tables were copied by the call
    goff[:] = 0
    neg[:] = 1
    ti.sync()
    out = []
    for t in (d_d, o_d, h_d):
        a = t.cpu().numpy()
        assert (a[0] == FILL).all() and (a[-1] == FILL).all(), "a guard row was written"
        out.append(a[1:-1])
    assert ti.cnf_info()["q"] == G and ti.cnf_info()["ms"] > 0
    return out[0], out[1], out[2].view(np.uint32)


def _check(gpu, ti, c, groups, caps, budgets, tag):
    """the device against model A for every cap and budget -> the walks"""
    walks = [cc.walk_of(c, g) for g in groups]
    for budget in budgets:
        full = [cc.cnf_a(w, budget) for w in walks]
        for cap in caps:
            docs, offs, heads = cc.cnf_rows(full, cap)
            gd, go, gh = _cnf_device(gpu, ti, groups, cap, budget)
            bad = np.flatnonzero((gh != heads).any(axis=1))
            assert bad.size == 0, (tag, cap, budget, [(groups[i], gh[i].tolist(), heads[i].tolist()) for i in bad[:3]])
            if cap:
                bad = np.flatnonzero((gd != docs).any(axis=1) | (go != offs).any(axis=1))                 # the guard pattern beyond written too
                assert bad.size == 0, (tag, cap, budget, [(groups[i], gd[i, :4].tolist(), docs[i, :4].tolist(), go[i, :4].tolist(),
                                                          offs[i, :4].tolist()) for i in bad[:3]])
            else:
                assert (gd == FILL).all() and (go == FILL).all(), (tag, budget)
    return walks


def _index(gpu, c, k=None):
    ti = gpu.TokenIndex.build(c["t"]) if k is None else gpu.TokenIndex.build(c["t"], k)
    ti.set_documents(c["starts"])
    ti.prepare_doc_ranks()
    return ti


# ---- one literal per clause: the AND launch ------------------------------------------------------------------------------------

@pytest.mark.parametrize("text", ["equal", "planted", "random"])
def test_single_literal_clauses_equal_the_all_launch(gpu, text):
    if text == "equal":
        c, groups, settings = cc.equal_case(1), ac.and_groups(), [(16, 0), (1, 0), (0, 0), (16, 64), (16, 65), (1, 255), (16, 257), (0, 80)]
    elif text == "planted":
        c = cc.planted_case()
        n = c["t"].size
        groups = list(c["groups"]) + list(c["last"]) + [[(0, n), (7, 0)], [(7, 0), (0, n)], [(100, 5), (200, 5), (300, 4)], [(0, n)] * 16]
        settings = [(16, 0), (1, 2), (0, 0)]
    else:
        c, e = ac.random_case("rand_k1000"), nc.expected("rand_k1000")
        spans = [(int(s[0]), int(s[1])) for s in e["spans"][(1, 0, 0)]]
        groups = [[spans[i] for i in g] for g in ac.random_groups(len(spans))]
        settings = [(16, 0), (3, 40), (0, 0)]
    cnf = [cc.positive([[s] for s in g]) for g in groups]
    with _index(gpu, c, 1000 if text == "random" else None) as ti:
        for cap, budget in settings:
            ad, ao, ah = _all_device(gpu, ti, groups, cap, budget)
            gd, go, gh = _cnf_device(gpu, ti, cnf, cap, budget, negated=(budget == 0))
            assert gd.tobytes() == ad.tobytes() and go.tobytes() == ao.tobytes(), (text, cap, budget)     # the guard pattern behind written too
            # all: written, examined, matched, candidates, driver, count; cnf: written, matched, candidates, duplicates, driver, literals
            for x, y in ((0, 0), (1, 2), (2, 3), (4, 4)):
                assert np.array_equal(gh[:, x], ah[:, y]), (text, cap, budget, x)
            assert np.array_equal(gh[:, 6], ah[:, 1]) and np.array_equal(gh[:, 8], ah[:, 5]) and not gh[:, (7, 9, 10, 11)].any(), (text, cap, budget)
            assert not gh[:, 3].any() and (gh[:, 5] == 1).all(), (text, cap, budget)


# ---- the driver rule -----------------------------------------------------------------------------------------------------------

def test_driver_rule(gpu):
    c = cc.planted_case()
    n = c["t"].size
    groups = cc.driver_groups(n)
    with _index(gpu, c) as ti:
        assert np.array_equal(ti.doc_ranks(0, n), c["rk"])
        walks = _check(gpu, ti, c, groups, (16, 1, 0), (0, 1, 6, 9), "driver")
        assert [w[0] for w in walks] == [1, 0, 0, 0, 0, 1, 0, 1, 0, 1, 1, 0, 0]
        gd, go, gh = _cnf_device(gpu, ti, groups[8:11], 4, 0)                                         # a positive all-empty clause
        assert not gh[:, (0, 1, 2, 3, 6, 7, 8, 9, 10, 11)].any() and gh[:, 4].tolist() == [0, 1, 1] and gh[:, 5].tolist() == [1, 2, 2]
        assert (gd == FILL).all() and (go == FILL).all()


# ---- de-duplication, budgets, caps, limits: the all-equal text -----------------------------------------------------------------

@pytest.mark.parametrize("Ld", [1, 2])
def test_deduplication_inside_the_driver_clause(gpu, Ld):
    c = cc.equal_case(Ld)
    groups = cc.dedup_groups()
    budgets = sorted({b for g in groups[:8] + groups[-2:] for b in cc.budgets_of(g)})
    with _index(gpu, c) as ti:
        walks = _check(gpu, ti, c, groups, (16, 0), budgets, ("dedup", Ld))
        gd, go, gh = _cnf_device(gpu, ti, groups, 1024, 0)                                            # every list whole
        for i, (g, w) in enumerate(zip(groups, walks)):
            head, ent = cc.cnf_a(w, 0, most=1024)
            lits = g[0][0]
            union = set()
            for f, k in lits:
                union |= set(c["da"][f:f + k].tolist())
            firsts = sum(len(set(c["da"][f:f + k].tolist())) for f, k in lits)
            assert int(gh[i, 2]) == len(union) and int(gh[i, 3]) == firsts - len(union), (Ld, g)         # candidates and duplicates: exact
            listed = gd[i, :int(gh[i, 0])].tolist()
            assert len(set(listed)) == len(listed) and listed == [d for d, _ in ent], (Ld, g)         # each document once
            if len(g[0]) == 1:                                                                        # ... at its first literal
                want, seen = [], set()
                for f, k in lits:
                    for d in c["da"][f:f + k].tolist():
                        if d not in seen:
                            seen.add(d)
                            want.append(d)
                assert listed == want, (Ld, g)


def test_budgets_and_caps_across_a_literal_boundary(gpu):
    c = cc.equal_case(1)
    groups = cc.cap_groups()
    with _index(gpu, c) as ti:
        walks = _check(gpu, ti, c, groups, cc.CAPS, (0, 14, 15, 16, 17, 34, 35, 36), "caps")
        assert [cc.cnf_a(w, 0)[0][1] for w in walks] == [0, 1, 15, 16, 17]
        for g in (cc.dedup_groups()[1], cc.dedup_groups()[6]):                                        # count_0 and count, one either side
            assert len(cc.budgets_of(g)) == 7
            _check(gpu, ti, c, [g], (16,), cc.budgets_of(g), "budget")


def test_limits(gpu):
    c = cc.equal_case(1)
    groups = cc.limit_groups()
    with _index(gpu, c) as ti:
        walks = _check(gpu, ti, c, groups, (16, 0), (0, 30, 1000), "limits")
        assert [w[1] for w in walks] == [64, 63, 4, 1] and [w[0] for w in walks] == [0, 0, 15, 15]
        lib = gpu.lib()
        sp = _dev(np.zeros((65, 4), np.int32))
        for coff, goff in ((np.arange(18), [0, 17]), ([0, 65], [0, 1]), ([0, 1, 65], [0, 2])):       # 17 clauses, 65 literals: refused
            co, go = np.array(coff, np.uint64), np.array(goff, np.uint64)
            assert lib.sa_hip_token_index_cnf_batch_device(ti._h, sp.data_ptr(), int(co[-1]), co.ctypes.data, co.size - 1, None, go.ctypes.data,
                                                           go.size - 1, 0, 0, None, None, sp.data_ptr()) == -1
            assert b"SA_HIP_TOKEN_CNF_MAX" in lib.sa_hip_last_error()


# ---- OR probes and exclusions on planted literals ------------------------------------------------------------------------------

def test_or_probes_and_exclusions(gpu):
    c = cc.planted_case()
    probes = cc.probe_groups(c)
    groups = [g for g, _ in probes]
    with _index(gpu, c) as ti:
        _check(gpu, ti, c, groups, (4,), (0, 1), "probes")
        gd, go, gh = _cnf_device(gpu, ti, groups, 4, 1)                                               # one rank: A's first, its document alone
        for i, (g, want) in enumerate(probes):
            d = int(c["da"][g[0][0][0][0]])
            assert gh[i, :3].tolist() == [int(want), int(want), 1] and (not want or gd[i, 0] == d), (g, want, gh[i].tolist())


# ---- the launch cap ------------------------------------------------------------------------------------------------------------

def test_launch_cap(gpu):
    c = cc.equal_case(2)
    base = cc.cap_groups() + cc.dedup_groups()[:9] + cc.limit_groups()[2:]
    budget, cap = 300, 4
    docs, offs, heads = cc.cnf_rows([cc.cnf_a(cc.walk_of(c, g), budget) for g in base], cap)
    assert (heads[:, 0] == cap).any() and (heads[:, 0] < cap).any()
    with _index(gpu, c) as ti:
        for G in (16384, 16385, 32769):
            idx = np.arange(G) % len(base)
            gd, go, gh = _cnf_device(gpu, ti, [base[i] for i in idx], cap, budget)
            for got, want, what in ((gd, docs, "docs"), (go, offs, "offsets"), (gh, heads, "heads")):
                bad = np.flatnonzero((got != want[idx]).any(axis=1))
                assert bad.size == 0, (G, what, bad[:5].tolist(), got[bad[:2]].tolist(), want[idx][bad[:2]].tolist())


# ---- random texts, both span modes, both models --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model_b():
    """model B once per text and mode: per query the documents that satisfy it"""
    out = {}
    for name in dc.RANDOM:
        c, e = ac.random_case(name), nc.expected(name)
        for cfg in ((0, 0, 1), (1, 0, 0)):
            pats = [ctx[len(ctx) - int(sp[2]):] for ctx, sp in zip(e["ctx"], e["spans"][cfg])]
            out[name, cfg] = [cc.cnf_b(c["t"], c["starts"], [[pats[i] for i in cla] for cla in clauses], neg)
                              for clauses, neg in cc.random_queries(len(pats))]
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(dc.RANDOM))
def test_random_texts_against_both_models(gpu, model_b, name, mode):
    c, e = ac.random_case(name), nc.expected(name)
    cfg = (1, 0, 0) if mode else (0, 0, 1)
    spans = [(int(s[0]), int(s[1])) for s in e["spans"][cfg]]
    queries = cc.random_queries(len(spans))
    order = [i for clauses, _ in queries for cla in clauses for i in cla]
    flat = [e["ctx"][i] for i in order]
    groups = [([[spans[i] for i in cla] for cla in clauses], neg) for clauses, neg in queries]
    _, coff, neg, goff = cc.tables(groups)
    walks = [cc.walk_of(c, g) for g in groups]
    with _index(gpu, c) as ti:
        for cap, budget in ((16, 0), (0, 0), (1, 1), (16, 100)):
            docs, offs, heads = cc.cnf_rows([cc.cnf_a(w, budget) for w in walks], cap)
            got = ti.cnf_batch(flat, coff, neg, goff, cap=cap, budget=budget, mode=mode, need_next=False, fill=FILL)
            assert np.array_equal(got["spans"].view(np.uint32).reshape(-1, 4), e["spans"][cfg][order]), (name, mode)
            gh = got["heads"].view(np.uint32).reshape(-1, 12)
            bad = np.flatnonzero((gh != heads).any(axis=1) | (got["docs"] != docs).any(axis=1) | (got["offsets"] != offs).any(axis=1))
            assert bad.size == 0, (name, mode, cap, budget, [(queries[i], gh[i].tolist(), heads[i].tolist()) for i in bad[:3]])
            if budget == 0:                                                                           # model B: no suffix array behind it
                for i, (both, sums) in enumerate(model_b[name, cfg]):
                    assert int(got["heads"]["matched"][i]) == len(both) and got["heads"]["examined"][i] == got["heads"]["count"][i], (name, mode, i)
                    assert int(got["heads"]["count"][i]) == sums[int(got["heads"]["driver"][i])], (name, mode, i)
                    assert set(got["docs"][i, :int(gh[i, 0])].tolist()) <= set(both), (name, mode, i)


# ---- the device chain ----------------------------------------------------------------------------------------------------------

def test_device_chain_equals_the_host_form_and_feeds_the_counts(gpu):
    import torch
    c, e = ac.random_case("rand_k1000"), nc.expected("rand_k1000")
    n = c["t"].size
    cap, budget = 5, 60
    with _index(gpu, c, 1000) as ti:
        assert ti.cnf_batch([], [0], None, [0], cap=cap)["docs"].shape == (0, cap)                    # G == 0
        for mode in (0, 1):
            cfg = (1, 0, 0) if mode else (0, 0, 1)
            queries = cc.random_queries(len(e["ctx"]), seed=12 + mode)
            order = [i for clauses, _ in queries for cla in clauses for i in cla]
            flat = [e["ctx"][i] for i in order]
            spans = [(int(s[0]), int(s[1])) for s in e["spans"][cfg]]
            _, coff, neg, goff = cc.tables([([[spans[i] for i in cla] for cla in clauses], ng) for clauses, ng in queries])
            S, G = len(flat), len(queries)
            host = ti.cnf_batch(flat, coff, neg, goff, cap=cap, budget=budget, mode=mode, need_next=False, fill=FILL)
            buf, off = tc.pack(flat)
            pd, od = _dev(buf), _dev(off.view(np.int64))
            sp_d = torch.zeros((S, 4), dtype=torch.int32, device="cuda:0")
            d_d, o_d, n_d = (torch.full((G, cap), FILL, dtype=torch.int32, device="cuda:0") for _ in range(3))
            h_d = torch.zeros((G, 12), dtype=torch.int32, device="cuda:0")
            firsts = [int(coff[int(goff[i])]) for i in range(G)]                                      # per query: its first literal
            first_d = _dev(np.array(firsts, np.int64))
            torch.cuda.synchronize()
            ti.spans_batch_device(pd.data_ptr(), od.data_ptr(), S, mode, 0, 0, sp_d.data_ptr())       # three launches, one sync
            ti.cnf_batch_device(sp_d.data_ptr(), S, coff, neg, goff, cap, budget, d_d.data_ptr(), o_d.data_ptr(), h_d.data_ptr())
            ti.sync()
            assert sp_d.cpu().numpy().tobytes() == host["spans"].tobytes(), mode
            assert d_d.cpu().numpy().tobytes() == host["docs"].tobytes() and o_d.cpu().numpy().tobytes() == host["offsets"].tobytes(), mode
            assert h_d.cpu().numpy().tobytes() == host["heads"].tobytes(), mode
            # heads.written chains into the per-document counts with the head's size as the stride
            lit_d = sp_d[first_d].contiguous()
            torch.cuda.synchronize()
            ti.doc_counts_batch_device(lit_d.data_ptr(), G, cap, d_d.data_ptr(), h_d.data_ptr(), 48, n_d.data_ptr())
            ti.sync()
            want = ac.counts_rows(c["rk"], c["cl"], n, [spans[order[f]] for f in firsts], host["docs"], host["heads"]["written"])
            assert np.array_equal(n_d.cpu().numpy().view(np.uint32), want), mode
            assert ti.cnf_info()["q"] == G and ti.doc_ranks_info()["counts_q"] == G


# ---- the Python class ----------------------------------------------------------------------------------------------------------

def test_python_class(gpu):
    import suffixarray_amd
    rng = np.random.default_rng(9)
    tokens = rng.integers(0, 5, 400).astype(np.int32)
    starts = np.array(sorted({0} | set(rng.integers(1, 400, 14).tolist())) + [400], np.int32)        # the last document is empty
    tl = tokens.tolist()
    ngrams = [list(g) for g in sorted({tuple(tl[p:p + m]) for m in (2, 3) for p in range(400 - m + 1)})] + [[9], [4, 4, 4, 4, 4, 4, 4]]
    N = len(ngrams)
    queries = [[[ngrams[i], ngrams[(5 * i + 2) % N]], [ngrams[(3 * i + 1) % N]]] for i in range(N)]
    exclude = [[ngrams[(7 * i + 3) % N]] if i % 2 else None for i in range(N)]
    queries += [[[ngrams[0]]], [[[9]], [ngrams[0]]], [[ngrams[1]]] * 15, [[[9], ngrams[2]]]]
    exclude += [None, None, [ngrams[3]], []]
    with suffixarray_amd.TokenIndex(tokens, doc_starts=starts) as ti, suffixarray_amd.TokenIndex(tokens) as bare:
        assert ti._idx.doc_ranks_info()["present"] == 0
        res = ti.documents_with_cnf(queries, exclude, cap=16)                                         # prepares on first use
        assert ti._idx.doc_ranks_info()["present"] == 1 and ti._idx.cnf_info()["q"] == len(queries)
        matched, exact = ti.count_documents_with_cnf(queries, exclude)
        assert matched.dtype == np.uint32 and exact.dtype == np.bool_ and exact.all() and len(res) == len(queries)
        for q, ex, r, m in zip(queries, exclude, res, matched.tolist()):
            clauses, neg = list(q) + ([ex] if ex else []), [0] * len(q) + ([1] if ex else [])
            both, sums = cc.cnf_b(tokens, starts, clauses, neg)
            assert sorted(r) == ["documents", "driver", "duplicates", "exact", "matched", "offsets"] and r["matched"] == m == len(both) and r["exact"], q
            assert r["driver"] == cc.driver_of(sums, neg), q
            assert r["documents"].size == min(m, 16) and set(r["documents"].tolist()) <= set(both), q
            for d, o in zip(r["documents"].tolist(), r["offsets"].tolist()):                          # the round trip: a literal of the driver
                assert any(tl[starts[d] + o:starts[d] + o + len(p)] == p for p in q[r["driver"]]), (q, d, o)
        same = ti.documents_with_all([[c_[0] for c_ in q] for q in queries[-4:-2]])                  # one literal per clause: the AND query
        for r, a in zip(ti.documents_with_cnf(queries[-4:-2]), same):
            assert r["matched"] == a["matched"] and r["documents"].tolist() == a["documents"].tolist() and r["duplicates"] == 0
        m1, e1 = ti.count_documents_with_cnf(queries, exclude, budget=1)
        assert (m1 <= 1).all() and not e1.all()
        assert ti.documents_with_cnf([]) == [] and ti.count_documents_with_cnf([])[0].size == 0
        for bad, ex in (([[]], None), ([[[]]], None), ([[[ngrams[0]]] * 17], None), ([[[ngrams[0]]] * 16], [[ngrams[1]]]),
                        ([[[ngrams[0]] * 65]], None), (queries[:2], [None])):
            with pytest.raises(ValueError):
                ti.documents_with_cnf(bad, ex)
        for call in (lambda: bare.documents_with_cnf([[[[1]]]]), lambda: bare.count_documents_with_cnf([[[[1]]]])):
            with pytest.raises(gpu.SaHipError) as err:
                call()
            assert err.value.code == -1
