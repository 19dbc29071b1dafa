"""Per-document counts and AND groups of a token index on the device against the two CPU models of token_all_cases.py: the
rank-by-document array at the sort's pass and tile edges and across set_documents; counts on the all-equal text at the segment edges,
with foreign document ids, shortened rows and a guard pattern; AND groups against docs_batch_device, at the driver rule, on planted
spans, at the lane, trip, cap and budget edges; random texts with random tables in exact and longest-suffix mode; the device chain
against the host forms; the Python class."""
import numpy as np
import pytest

import token_all_cases as ac
import token_cases as tc
import token_doc_cases as dc
import token_next_cases as nc
from test_gpu_token_docs import _dev, _passes, _sort_tile, _span_array

pytestmark = pytest.mark.gpu

FILL = ac.FILL
UFILL = FILL & 0xFFFFFFFF


def _all_device(gpu, ti, groups, cap, budget):
    """one all launch over groups of (first, count) spans -> (docs[G, max(cap, 1)], offsets, heads uint32[G, 8])"""
    import torch
    flat = [s for g in groups for s in g]
    goff = np.cumsum([0] + [len(g) for g in groups]).astype(np.uint64)
    sp_d = _dev(_span_array(gpu, flat).view(np.int32).reshape(-1, 4))
    G = len(groups)
    d_d = torch.full((G, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
    o_d = torch.full((G, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
    h_d = torch.full((G, 8), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ti.all_batch_device(sp_d.data_ptr(), len(flat), goff, cap, budget, d_d.data_ptr() if cap else None, o_d.data_ptr() if cap else None,
                        h_d.data_ptr())
    ti.sync()
    return d_d.cpu().numpy(), o_d.cpu().numpy(), h_d.cpu().numpy().view(np.uint32)


def _check_all(gpu, ti, c, groups, caps, budgets, tag):
    n = c["sa"].size
    walks = [ac.all_walk(c["sa"], c["da"], c["cl"], n, g) for g in groups]
    firsts = [ac.group_first(n, g) for g in groups]
    for budget in budgets:
        full = [ac.all_a(w, f, budget) for w, f in zip(walks, firsts)]
        for cap in caps:
            docs, offs, heads = ac.all_rows(full, cap)
            gd, go, gh = _all_device(gpu, ti, groups, cap, budget)
            bad = np.flatnonzero((gh != heads).any(axis=1))
            assert bad.size == 0, (tag, cap, budget, [(groups[i], gh[i].tolist(), heads[i].tolist()) for i in bad[:5]])
            if cap:
                bad = np.flatnonzero((gd != docs).any(axis=1) | (go != offs).any(axis=1))                 # the guard pattern beyond written too
                assert bad.size == 0, (tag, cap, budget, [(groups[i], gd[i, :4].tolist(), docs[i, :4].tolist(), go[i, :4].tolist(),
                                                          offs[i, :4].tolist()) for i in bad[:5]])
            else:
                assert (gd == FILL).all() and (go == FILL).all(), (tag, budget)
    return walks


# ---- the rank-by-document array ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["tile-1", "tile", "tile+1", "2tile-1", "2tile", "2tile+1"])
def test_rank_by_document_array(gpu, where):
    tile = _sort_tile()
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2tile-1": 2 * tile - 1, "2tile": 2 * tile, "2tile+1": 2 * tile + 1}[where]
    assert n <= 140000
    t = np.random.default_rng(n).integers(0, 4, n).astype(np.int32)
    sa = dc.model_sa(t).astype(np.int32)
    tables = [(D, dc.rand_table(n, D, 100 + D)) for D in (1, 2, 256, 257)] + [(n, dc.one_token_each(n)), (9, dc.with_empties(n))]
    lib = gpu.lib()
    pats = [[0], [1, 2]]
    with gpu.TokenIndex.build(t) as ti:
        with pytest.raises(gpu.SaHipError) as err:                                                    # no documents yet
            ti.prepare_doc_ranks()
        assert err.value.code == -1 and "no documents" in str(err.value)
        assert ti.doc_ranks_info()["present"] == 0
        for D, starts in tables:                                                                      # every call replaces the table before it
            ti.set_documents(starts)
            before = ti.docs_info()
            assert ti.doc_ranks_info()["present"] == 0 and ti.doc_ranks_info()["bytes"] == 0, D       # gone with the table it was built for
            for call in (lambda: ti.doc_ranks(0, 1), lambda: ti.all_batch(pats, [0, 2], cap=4),
                         lambda: ti.doc_counts_batch(pats, np.zeros((2, 3), np.int32))):
                with pytest.raises(gpu.SaHipError) as err:
                    call()
                assert err.value.code == -1 and "prepare_doc_ranks" in str(err.value), D
            ti.prepare_doc_ranks()
            ti.prepare_doc_ranks()                                                                    # a no-op
            da, _ = dc.model_da_pv(sa, starts)
            got = ti.doc_ranks(0, n)
            want = ac.model_rk(da)
            assert np.array_equal(got, want), (where, D, np.flatnonzero(got != want)[:5])
            info = ti.doc_ranks_info()
            assert info["present"] == 1 and info["bytes"] == 4 * n and info["sort_passes"] == _passes(D) and info["prepare_ms"] > 0, (D, info)
            assert ti.docs_info() == before, D                                                        # set_documents' figures stay
        assert np.array_equal(ti.doc_ranks(n - 3, 3), want[n - 3:]) and ti.doc_ranks(n, 0).size == 0
        one = np.zeros(2, np.int32)
        assert lib.sa_hip_token_index_get_doc_ranks(ti._h, n - 1, 2, one.ctypes.data) == -1 and b"beyond" in lib.sa_hip_last_error()
        ti.prepare_doc_ranks(False)                                                                   # freed, and freed again
        ti.prepare_doc_ranks(False)
        assert ti.doc_ranks_info()["present"] == 0 and ti.docs_info()["documents"] == 9
        ti.prepare_doc_ranks()
        assert np.array_equal(ti.doc_ranks(0, n), want)
        ti.set_documents(None)                                                                        # removed with the documents
        assert ti.doc_ranks_info()["present"] == 0
        with pytest.raises(gpu.SaHipError):
            ti.doc_ranks(0, 1)


# ---- counts: the all-equal text ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ld", ac.TF_LDS)
def test_counts_at_segment_edges(gpu, Ld):
    import torch
    c = dc.equal_case(Ld)
    n = ac.N_EQ
    rk, cl = ac.model_rk(c["da"]), ac.closed(c["starts"], n)
    spans, docs = ac.tf_cells(Ld)
    q, cap = docs.shape
    with gpu.TokenIndex.build(c["t"]) as ti:
        ti.set_documents(c["starts"])
        ti.prepare_doc_ranks()
        assert np.array_equal(ti.doc_ranks(0, n), rk)
        sp_d = _dev(_span_array(gpu, spans).view(np.int32).reshape(-1, 4))
        d_d = _dev(docs)
        rows = (np.arange(q) * 5 % (cap + 3)).astype(np.uint32)                                       # lengths 0 .. cap + 2: some beyond cap
        for stride, written in ((0, None), (4, rows), (16, rows)):
            want = ac.counts_rows(rk, cl, n, spans, docs, written)
            buf = torch.full((q + 2, cap), FILL, dtype=torch.int32, device="cuda:0")                  # a guard row either side
            w_d = None
            if written is not None:
                w = np.full((q, stride // 4), 0x7FFFFFFF, np.uint32)                                  # the heads of another launch: written first
                w[:, 0] = written
                w_d = _dev(w.view(np.int32))
            torch.cuda.synchronize()
            ti.doc_counts_batch_device(sp_d.data_ptr(), q, cap, d_d.data_ptr(), w_d.data_ptr() if w_d is not None else None, stride,
                                       buf[1:].data_ptr())
            ti.sync()
            got = buf.cpu().numpy().view(np.uint32)
            assert (got[0] == UFILL).all() and (got[-1] == UFILL).all(), (Ld, stride)
            bad = np.flatnonzero((got[1:-1] != want).any(axis=1))
            assert bad.size == 0, (Ld, stride, [(spans[i], docs[i].tolist(), got[1 + i].tolist(), want[i].tolist()) for i in bad[:5]])
            info = ti.doc_ranks_info()
            assert info["counts_q"] == q and info["counts_ms"] > 0, info
        # the host form: [A] * m is the ranks [m - 1, n); rows through `written`, cells beyond them keep the fill
        ks = [k for k in dc.COUNTS if k]
        pats = [[dc.A] * (n - k + 1) for k in ks]
        hdocs = np.tile(np.array(ac.tf_docs(Ld) + [-1, len(c["starts"])], np.int32), (len(ks), 1))
        hrows = (np.arange(len(ks)) % (hdocs.shape[1] + 1)).astype(np.uint32)
        for written in (None, hrows):
            got = ti.doc_counts_batch(pats, hdocs, written, fill=FILL)
            assert [(int(s["first"]), int(s["count"])) for s in got["spans"]] == [(n - k, k) for k in ks]
            assert np.array_equal(got["counts"], ac.counts_rows(rk, cl, n, [(n - k, k) for k in ks], hdocs, written)), (Ld, written is None)


# ---- AND groups ----------------------------------------------------------------------------------------------------------------

def test_groups_of_one_equal_the_documents_launch(gpu):
    import torch
    c, e = ac.random_case("rand_k1000"), nc.expected("rand_k1000")
    spans = [(int(s[0]), int(s[1])) for s in e["spans"][(1, 0, 0)]] + [(0, c["t"].size), (5, 0)]
    q = len(spans)
    with gpu.TokenIndex.build(c["t"], 1000) as ti:
        ti.set_documents(c["starts"])
        ti.prepare_doc_ranks()
        sp_d = _dev(_span_array(gpu, spans).view(np.int32).reshape(-1, 4))
        for cap, budget in ((16, 0), (3, 40), (0, 0)):
            d_d = torch.full((q, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
            o_d = torch.full((q, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
            h_d = torch.full((q, 4), -1, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            ti.docs_batch_device(sp_d.data_ptr(), q, cap, budget, d_d.data_ptr() if cap else None, o_d.data_ptr() if cap else None, h_d.data_ptr())
            ti.sync()
            gd, go, gh = _all_device(gpu, ti, [[s] for s in spans], cap, budget)
            assert gd.tobytes() == d_d.cpu().numpy().tobytes() and go.tobytes() == o_d.cpu().numpy().tobytes(), (cap, budget)
            dh = h_d.cpu().numpy().view(np.uint32)                                                    # written, examined, distinct, count
            assert np.array_equal(gh[:, 0], dh[:, 0]) and np.array_equal(gh[:, 1], dh[:, 1]) and np.array_equal(gh[:, 5], dh[:, 3])
            assert np.array_equal(gh[:, 2], dh[:, 2]) and np.array_equal(gh[:, 3], dh[:, 2]) and not gh[:, 4].any() and not gh[:, 6:].any()
            assert ti.doc_ranks_info()["all_q"] == q and ti.doc_ranks_info()["all_ms"] > 0


def test_driver_rule_planted_spans_and_the_last_document(gpu):
    c = ac.planted_case()
    n = c["t"].size
    A, B = c["groups"][0]
    big = (0, n)
    groups = list(c["groups"]) + list(c["last"])
    groups += [[big, big], [B, B], [A, A, A]]                                                         # twice the same span
    groups += [[(100, 5), (200, 5)], [(200, 5), (100, 5)], [(100, 5), (200, 5), (300, 4)]]            # ties, and a later smaller one
    groups += [[big, (7, 0)], [(7, 0), big], [big, A, (n, 3)], [(n + 9, 9)]]                          # an empty span: all zero
    groups += [[big] * ac.ALL_MAX, [A] + [big] * (ac.ALL_MAX - 1), [big] * (ac.ALL_MAX - 1) + [A]]    # 16 spans
    with gpu.TokenIndex.build(c["t"]) as ti:
        ti.set_documents(c["starts"])
        ti.prepare_doc_ranks()
        assert np.array_equal(ti.doc_ranks(0, n), c["rk"])
        walks = _check_all(gpu, ti, c, groups, (16, 1, 0), (0, 1, 2, 3), "planted")
        by = {str(g): w for g, w in zip(groups, walks)}
        for g in ([big, big], [B, B], [A, A, A]):
            assert all(m for _, _, _, m in by[str(g)][2]), g                                          # matched == candidates
        assert by[str([(100, 5), (200, 5)])][0] == 0 and by[str([(200, 5), (100, 5)])][0] == 0 and by[str(groups[-1])][0] == ac.ALL_MAX - 1
        assert by[str([(100, 5), (200, 5), (300, 4)])][0] == 2
        gd, go, gh = _all_device(gpu, ti, [[big, (7, 0)], [(7, 0), big], [(n + 9, 9)]], 4, 0)
        assert gh[:, (0, 1, 2, 3, 5, 6, 7)].sum() == 0 and gh[:, 4].tolist() == [1, 0, 0] and (gd == FILL).all()
        lib = gpu.lib()
        sp = _dev(np.zeros((17, 4), np.int32))                                                        # 17 spans are refused
        go17 = np.array([0, 17], np.uint64)
        assert lib.sa_hip_token_index_all_batch_device(ti._h, sp.data_ptr(), 17, go17.ctypes.data, 1, 0, 0, None, None, sp.data_ptr()) == -1


def test_lane_trip_cap_and_budget_edges(gpu):
    c = dict(dc.equal_case(1))
    c["cl"] = ac.closed(c["starts"], ac.N_EQ)
    with gpu.TokenIndex.build(c["t"]) as ti:
        ti.set_documents(c["starts"])
        ti.prepare_doc_ranks()
        _check_all(gpu, ti, c, ac.and_groups(), ac.AND_CAPS, ac.AND_BUDGETS, "equal")


@pytest.fixture(scope="module")
def model_b():
    """model B once per text and mode: per group the documents that hold all of its matched patterns"""
    out = {}
    for name in dc.RANDOM:
        c, e = ac.random_case(name), nc.expected(name)
        for cfg in ((0, 0, 1), (1, 0, 0)):
            pats = [ctx[len(ctx) - int(sp[2]):] for ctx, sp in zip(e["ctx"], e["spans"][cfg])]
            out[name, cfg] = [ac.all_b(c["t"], c["starts"], [pats[i] for i in grp]) for grp in ac.random_groups(len(pats))]
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(dc.RANDOM))
def test_random_texts_against_both_models(gpu, model_b, name, mode):
    c, e = ac.random_case(name), nc.expected(name)
    cfg = (1, 0, 0) if mode else (0, 0, 1)
    n = c["t"].size
    spans = [(int(s[0]), int(s[1])) for s in e["spans"][cfg]]
    groups = ac.random_groups(len(spans))
    flat = [e["ctx"][i] for g in groups for i in g]
    goff = np.cumsum([0] + [len(g) for g in groups]).astype(np.uint64)
    sgroups = [[spans[i] for i in g] for g in groups]
    walks = [ac.all_walk(c["sa"], c["da"], c["cl"], n, g) for g in sgroups]
    with gpu.TokenIndex.build(c["t"]) as ti:
        ti.set_documents(c["starts"])
        ti.prepare_doc_ranks()
        assert np.array_equal(ti.doc_ranks(0, n), c["rk"])
        for cap, budget in ((16, 0), (0, 0), (1, 1), (16, 100)):
            docs, offs, heads = ac.all_rows([ac.all_a(w, ac.group_first(n, g), budget) for w, g in zip(walks, sgroups)], cap)
            got = ti.all_batch(flat, goff, cap=cap, budget=budget, mode=mode, need_next=False, fill=FILL)
            assert np.array_equal(got["spans"].view(np.uint32).reshape(-1, 4), e["spans"][cfg][[i for g in groups for i in g]]), (name, mode)
            gh = got["heads"].view(np.uint32).reshape(-1, 8)
            bad = np.flatnonzero((gh != heads).any(axis=1) | (got["docs"] != docs).any(axis=1) | (got["offsets"] != offs).any(axis=1))
            assert bad.size == 0, (name, mode, cap, budget, [(groups[i], gh[i].tolist(), heads[i].tolist()) for i in bad[:5]])
            if budget == 0:                                                                           # model B: no suffix array behind it
                for i, (both, tfs) in enumerate(model_b[name, cfg]):
                    assert int(gh[i, 2]) == len(both) and int(gh[i, 1]) == int(gh[i, 5]), (name, mode, i)
                    assert set(got["docs"][i, :int(gh[i, 0])].tolist()) <= set(both), (name, mode, i)
        # counts of the listed documents, chained on the host: every one is the model's, and none is 0
        ctx = e["ctx"][::3]
        r = ti.docs_batch(ctx, cap=8, mode=mode, need_next=False, fill=FILL)
        tf = ti.doc_counts_batch(ctx, r["docs"], r["heads"]["written"], mode=mode, fill=FILL)
        sub = [spans[i] for i in range(0, len(spans), 3)]
        assert np.array_equal(tf["counts"], ac.counts_rows(c["rk"], c["cl"], n, sub, r["docs"], r["heads"]["written"])), (name, mode)
        for i, p in enumerate(ctx[:40]):
            length = int(r["spans"]["length"][i])
            b = ac.tf_b(c["t"], c["starts"], p[len(p) - length:])
            w = int(r["heads"]["written"][i])
            assert tf["counts"][i, :w].tolist() == [b[d] for d in r["docs"][i, :w].tolist()], (name, mode, i)


# ---- the device chain ----------------------------------------------------------------------------------------------------------

def test_device_chain_equals_the_host_forms(gpu):
    import torch
    c, e = ac.random_case("rand_k1000"), nc.expected("rand_k1000")
    nctx = len(e["ctx"])
    cap, budget = 5, 40
    with gpu.TokenIndex.build(c["t"], 1000) as ti:
        ti.set_documents(c["starts"])
        ti.prepare_doc_ranks()
        assert ti.all_batch([], [0], cap=cap)["docs"].shape == (0, cap)                               # G == 0
        assert ti.doc_counts_batch([], np.zeros((0, 3), np.int32))["counts"].shape == (0, 3)          # Q == 0
        kept = []
        for q in (1, 3, 4, 5, 255, 256, 257):
            sub = [e["ctx"][(7 * k + q) % nctx] if k % 5 else [] for k in range(q)]                   # empty contexts inside
            cuts = sorted({0, q} | set(range(0, q, 3)) | set(range(1, q, 7)))                         # groups of 1 .. 3
            goff = np.array(cuts, np.uint64)
            G = goff.size - 1
            for mode in (0, 1):
                hall = ti.all_batch(sub, goff, cap=cap, budget=budget, mode=mode, need_next=False, fill=FILL)
                hdocs = ti.docs_batch(sub, cap=cap, budget=budget, mode=mode, need_next=False, fill=FILL)
                htf = ti.doc_counts_batch(sub, hdocs["docs"], hdocs["heads"]["written"], mode=mode, fill=FILL)
                buf, off = tc.pack(sub)
                pd, od = _dev(buf if buf.size else np.zeros(1, np.int32)), _dev(off.view(np.int64))
                sp_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
                outs = [torch.full((max(q, G), cap), FILL, dtype=torch.int32, device="cuda:0") for _ in range(5)]
                h_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
                a_d = torch.zeros((G, 8), dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()
                ti.spans_batch_device(pd.data_ptr(), od.data_ptr(), q, mode, 0, 0, sp_d.data_ptr())   # four launches, one sync
                ti.all_batch_device(sp_d.data_ptr(), q, goff, cap, budget, outs[0].data_ptr(), outs[1].data_ptr(), a_d.data_ptr())
                ti.docs_batch_device(sp_d.data_ptr(), q, cap, budget, outs[2].data_ptr(), outs[3].data_ptr(), h_d.data_ptr())
                ti.doc_counts_batch_device(sp_d.data_ptr(), q, cap, outs[2].data_ptr(), h_d.data_ptr(), 16, outs[4].data_ptr())
                goff[:] = 0                                                                           # the table was copied by the call
                ti.sync()
                goff[:] = cuts
                assert sp_d.cpu().numpy().tobytes() == hall["spans"].tobytes() == hdocs["spans"].tobytes() == htf["spans"].tobytes(), (q, mode)
                assert outs[0][:G].cpu().numpy().tobytes() == hall["docs"].tobytes(), (q, mode)
                assert outs[1][:G].cpu().numpy().tobytes() == hall["offsets"].tobytes(), (q, mode)
                assert a_d.cpu().numpy().tobytes() == hall["heads"].tobytes(), (q, mode)
                assert outs[2][:q].cpu().numpy().tobytes() == hdocs["docs"].tobytes(), (q, mode)
                assert outs[4][:q].cpu().numpy().tobytes() == htf["counts"].tobytes(), (q, mode)
                info = ti.doc_ranks_info()
                assert info["all_q"] == G and info["counts_q"] == q and info["all_ms"] > 0 and info["counts_ms"] > 0, info
                kept.append((pd, od, sp_d, outs, h_d, a_d))


# ---- the Python class ----------------------------------------------------------------------------------------------------------

def test_python_class(gpu):
    import suffixarray_amd
    rng = np.random.default_rng(8)
    tokens = rng.integers(0, 5, 400).astype(np.int32)
    starts = np.array(sorted({0} | set(rng.integers(1, 400, 14).tolist())) + [400], np.int32)        # the last document is empty
    D = starts.size
    tl = tokens.tolist()
    ngrams = sorted({tuple(tl[p:p + m]) for m in (1, 2, 3) for p in range(400 - m + 1)}) + [(9,), (4, 4, 4, 4, 4, 4, 4)]
    ngrams = [list(g) for g in ngrams]
    docs = list(range(D)) + [-1, D, 2 ** 31 - 1]
    groups = [[ngrams[i], ngrams[(3 * i + 1) % len(ngrams)]] for i in range(len(ngrams))]
    groups += [[ngrams[0]], [ngrams[5], ngrams[6], ngrams[7]], [ngrams[1]] * 16, [[9], ngrams[0]]]
    with suffixarray_amd.TokenIndex(tokens, doc_starts=starts) as ti, suffixarray_amd.TokenIndex(tokens) as bare:
        assert ti._idx.doc_ranks_info()["present"] == 0
        tf = ti.term_counts(ngrams, docs)                                                             # prepares on first use
        assert ti._idx.doc_ranks_info()["present"] == 1 and tf.dtype == np.uint32 and tf.shape == (len(ngrams), len(docs))
        for i, g in enumerate(ngrams):
            b = ac.tf_b(tokens, starts, g)
            assert tf[i].tolist() == [b.get(d, 0) for d in docs], g
        assert np.array_equal(tf.sum(axis=1), ti.count(ngrams))                                       # every occurrence is in one document
        assert np.array_equal((tf > 0).sum(axis=1), ti.document_counts(ngrams)[0])
        assert ti.term_counts([], docs).shape == (0, len(docs)) and ti.term_counts(ngrams, []).shape == (len(ngrams), 0)
        res = ti.documents_with_all(groups, cap=16)
        matched, exact = ti.count_documents_with_all(groups)
        assert matched.dtype == np.uint32 and exact.dtype == np.bool_ and exact.all() and len(res) == len(groups)
        for g, r, m in zip(groups, res, matched.tolist()):
            both, tfs = ac.all_b(tokens, starts, g)
            assert sorted(r) == ["documents", "driver", "exact", "matched", "offsets"] and r["matched"] == m == len(both) and r["exact"], g
            assert r["driver"] == ac.driver_of([sum(f.values()) for f in tfs]), g
            assert r["documents"].size == min(m, 16) and set(r["documents"].tolist()) <= set(both), g
            p = g[r["driver"]]
            for d, o in zip(r["documents"].tolist(), r["offsets"].tolist()):                          # the round trip
                assert tl[starts[d] + o:starts[d] + o + len(p)] == p, (g, d, o)
        m1, e1 = ti.count_documents_with_all(groups, budget=1)
        assert (m1 <= 1).all() and e1.tolist() == [min(sum(f.values()) for f in ac.all_b(tokens, starts, g)[1]) <= 1 for g in groups]
        rs = ti.documents_with_all([[[1, 2, 9], [9]]], cap=4, longest_suffix=True)                    # both back off to []: every document
        assert rs[0]["matched"] == len(set(dc.doc_of(starts, np.arange(400)).tolist())) and rs[0]["documents"].size == 4
        assert ti.documents_with_all([]) == [] and ti.count_documents_with_all([])[0].size == 0
        for badg in ([[]], [[ngrams[0]] * 17]):
            with pytest.raises(ValueError):
                ti.documents_with_all(badg)
        ti.set_documents([0])                                                                         # replaced: one document, prepared again
        assert ti._idx.doc_ranks_info()["present"] == 0
        assert ti.term_counts(ngrams, [0])[:, 0].tolist() == ti.count(ngrams).tolist()
        assert ti.count_documents_with_all(groups)[0].tolist() == [int(all(len(ac.tf_b(tokens, starts, p)) for p in g)) for g in groups]
        for call in (lambda: bare.term_counts([[1]], [0]), lambda: bare.documents_with_all([[[1]]]), lambda: bare.count_documents_with_all([[[1]]]),
                     lambda: bare.prepare_document_ranks()):
            with pytest.raises(gpu.SaHipError) as err:
                call()
            assert err.value.code == -1
