"""Documents of a token index on the device against the two CPU models of token_doc_cases.py: the document array and the
previous-rank array at the sort's pass and tile edges; counting and listing at the window, step, cap and budget edges of the walk on
the all-equal text, whose expected values have closed forms; random texts with random tables in exact and longest-suffix mode; the
device chain against the host forms; locate against sa_range and searchsorted; the Python class."""
import os
import re

import numpy as np
import pytest

import token_cases as tc
import token_doc_cases as dc
import token_next_cases as nc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = dc.FILL


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _sort_tile():
    """records per tile of the sort behind set_documents: its workgroup size times tq's SORT_ITEMS"""
    csrc = os.path.join(ROOT, "suffixarray_amd", "csrc")
    items = int(re.search(r"constexpr int SORT_ITEMS = (\d+);", open(os.path.join(csrc, "radix_sort.hpp")).read()).group(1))
    block = int(re.search(r"ws\.init\(n, (\d+)\)", open(os.path.join(csrc, "token_docs.hpp")).read()).group(1))
    return items * block


def _span_array(gpu, spans):
    a = np.zeros(len(spans), gpu.SPAN_DTYPE)
    a["first"], a["count"] = [f for f, _ in spans], [c for _, c in spans]
    return a


def _passes(D):
    bits = 0
    while (1 << bits) < D:
        bits += 1
    return (bits + 7) // 8


# ---- structures ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["tile-1", "tile", "tile+1", "2tile-1", "2tile", "2tile+1"])
def test_document_and_previous_rank_arrays(gpu, where):
    tile = _sort_tile()
    assert tile >= 1024
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2tile-1": 2 * tile - 1, "2tile": 2 * tile, "2tile+1": 2 * tile + 1}[where]
    t = np.random.default_rng(n).integers(0, 4, n).astype(np.int32)
    sa = dc.model_sa(t).astype(np.int32)
    tables = [(D, dc.rand_table(n, D, 100 + D)) for D in (1, 2, 255, 256, 257, 65536, 65537)]
    tables += [(n, dc.one_token_each(n)), (9, dc.with_empties(n))]
    with gpu.TokenIndex.build(t) as ti:
        assert np.array_equal(ti.sa_range(0, n), sa)
        assert ti.docs_info()["documents"] == 0
        for D, starts in tables:                                                                      # every call replaces the table before it
            assert starts.size == D
            ti.set_documents(starts)
            da, pv = dc.model_da_pv(sa, starts)
            got_da, got_pv = ti.doc_range(0, n)
            assert np.array_equal(got_da, da), (where, D, np.flatnonzero(got_da != da)[:5])
            assert np.array_equal(got_pv, pv), (where, D, np.flatnonzero(got_pv != pv)[:5])
            info = ti.docs_info()
            assert info["documents"] == D and info["bytes"] == 8 * n + 4 * (D + 1) and info["sort_passes"] == _passes(D), (where, D, info)
            assert info["prepare_ms"] > 0 and info["da_ms"] > 0 and info["pv_ms"] > 0, info
        lib = gpu.lib()
        a, b = ti.doc_range(n - 3, 3)                                                                 # a part, and either output alone
        assert np.array_equal(a, da[n - 3:]) and np.array_equal(b, pv[n - 3:])
        one = np.zeros(2, np.int32)
        assert lib.sa_hip_token_index_get_doc_range(ti._h, 5, 2, one.ctypes.data, None) == 0 and one.tolist() == da[5:7].tolist()
        assert lib.sa_hip_token_index_get_doc_range(ti._h, 5, 2, None, one.ctypes.data) == 0 and one.tolist() == pv[5:7].tolist()
        assert lib.sa_hip_token_index_get_doc_range(ti._h, n - 1, 2, one.ctypes.data, None) == -1
        assert b"beyond" in lib.sa_hip_last_error()
        # a table beyond the text is refused and the documents stay as they were
        far = np.array([0, n + 1], np.int32)
        assert lib.sa_hip_token_index_set_documents(ti._h, far.ctypes.data, 2) == -1 and b"beyond" in lib.sa_hip_last_error()
        assert ti.docs_info()["documents"] == 9
        ends = np.array([0, n, n], np.int32)                                                          # == n is allowed: empty documents at the end
        ti.set_documents(ends)
        assert np.array_equal(ti.doc_range(0, n)[0], np.zeros(n, np.int32))


def test_removing_the_documents(gpu):
    t = tc.texts()["rand_k4"]
    pats = [[0], [1, 2]]
    with gpu.TokenIndex.build(t) as ti:
        for rep in range(2):
            with pytest.raises(gpu.SaHipError) as err:
                ti.docs_batch(pats, cap=4)
            assert err.value.code == -1 and "no documents" in str(err.value)
            for call in (lambda: ti.locate_batch(pats, cap=4), lambda: ti.doc_range(0, 1), lambda: ti.docs_batch(pats, cap=0)):
                with pytest.raises(gpu.SaHipError):
                    call()
            assert ti.docs_info()["documents"] == 0
            ti.set_documents(None)                                                                    # removing nothing: fine
            ti.set_documents([0, 100, 100, 4000])
            got = ti.docs_batch(pats, cap=4)
            assert (got["heads"]["distinct"] == 3).all() and (got["heads"]["examined"] == got["heads"]["count"]).all()
            assert ti.docs_info()["documents"] == 4
            ti.set_documents(None)


# ---- counting and listing: the all-equal text ----------------------------------------------------------------------------------

@pytest.mark.parametrize("Ld", dc.LDS)
def test_counts_and_lists_at_window_cap_and_budget_edges(gpu, Ld):
    import torch
    c = dc.equal_case(Ld)
    sa, starts, da = c["sa"], c["starts"], c["da"]
    spans = dc.equal_spans(Ld)
    q = len(spans)
    with gpu.TokenIndex.build(c["t"]) as ti:
        assert np.array_equal(ti.sa_range(0, dc.N_EQ), sa)
        ti.set_documents(starts)
        sp_d = _dev(_span_array(gpu, spans).view(np.int32).reshape(-1, 4))
        for budget in dc.BUDGETS:
            full = dc.docs_full(sa, da, starts, spans, budget)
            for (f, k), (head, _) in zip(spans, full):                                                # the closed form beside the model
                assert head[2] == dc.equal_distinct(Ld, f, head[1]), (Ld, budget, f, k)
            for cap in dc.CAPS:
                docs, offs, heads = dc.docs_rows(full, cap)
                d_d = torch.full((q, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
                o_d = torch.full((q, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
                h_d = torch.full((q, 4), -1, dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()
                ti.docs_batch_device(sp_d.data_ptr(), q, cap, budget, d_d.data_ptr() if cap else None, o_d.data_ptr() if cap else None,
                                     h_d.data_ptr())
                ti.sync()
                hd = h_d.cpu().numpy().view(np.uint32)
                bad = np.flatnonzero((hd != heads).any(axis=1))
                assert bad.size == 0, (Ld, cap, budget, [(spans[i], hd[i].tolist(), heads[i].tolist()) for i in bad[:5]])
                if cap:
                    gd, go = d_d.cpu().numpy(), o_d.cpu().numpy()
                    bad = np.flatnonzero((gd != docs).any(axis=1) | (go != offs).any(axis=1))             # the guard pattern beyond written too
                    assert bad.size == 0, (Ld, cap, budget, [(spans[i], gd[i, :4].tolist(), docs[i, :4].tolist(), go[i, :4].tolist(),
                                                              offs[i, :4].tolist()) for i in bad[:5]])
                else:
                    assert (d_d.cpu().numpy() == FILL).all() and (o_d.cpu().numpy() == FILL).all()
                info = ti.docs_info()
                assert info["docs_q"] == q and info["examined"] == int(heads[:, 1].sum()) and info["docs_ms"] > 0, (Ld, cap, budget, info)
        # the host form: [A] * m is the ranks [m - 1, n), its count n - m + 1 every count of the list
        pats = [[dc.A] * (dc.N_EQ - k + 1) for k in dc.COUNTS]
        hspans = [(dc.N_EQ - k, k) for k in dc.COUNTS]
        for cap, budget in ((16, 0), (0, 65), (64, 256)):
            docs, offs, heads = dc.docs_rows(dc.docs_full(sa, da, starts, hspans, budget), cap)
            got = ti.docs_batch(pats, cap=cap, budget=budget, fill=FILL)
            assert [(int(s["first"]), int(s["count"])) for s in got["spans"] if s["count"]] == [s for s in hspans if s[1]], (Ld, cap)
            assert np.array_equal(got["heads"].view(np.uint32).reshape(-1, 4), heads), (Ld, cap, budget)
            assert np.array_equal(got["docs"], docs) and np.array_equal(got["offsets"], offs), (Ld, cap, budget)


def test_spans_beyond_the_array_are_clamped(gpu):
    """the device forms trust nothing: first and count are clamped, the calls return with written <= cap"""
    import torch
    c = dc.equal_case(64)
    n, cap = dc.N_EQ, 3
    bad = np.array([(n - 2, 3, 1, 0), (n, 1, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 7, 1), (5, 0xFFFFFFFF, 0xFFFFFFFF, 0), (0, n, 0, 0)],
                   gpu.SPAN_DTYPE)
    want = [(n - 2, 2), (n, 0), (n, 0), (5, n - 5), (0, n)]
    with gpu.TokenIndex.build(c["t"]) as ti:
        ti.set_documents(c["starts"])
        sp_d = _dev(bad.view(np.int32).reshape(-1, 4))
        d_d = torch.full((5, cap), FILL, dtype=torch.int32, device="cuda:0")
        o_d = torch.full((5, cap), FILL, dtype=torch.int32, device="cuda:0")
        h_d = torch.full((5, 4), -1, dtype=torch.int32, device="cuda:0")
        l_d = torch.full((5, 2), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ti.docs_batch_device(sp_d.data_ptr(), 5, cap, 0, d_d.data_ptr(), o_d.data_ptr(), h_d.data_ptr())
        ti.sync()
        docs, offs, heads = dc.docs_rows(dc.docs_full(c["sa"], c["da"], c["starts"], want, 0), cap)
        assert np.array_equal(h_d.cpu().numpy().view(np.uint32), heads)
        assert np.array_equal(d_d.cpu().numpy(), docs) and np.array_equal(o_d.cpu().numpy(), offs)
        d_d.fill_(FILL)
        o_d.fill_(FILL)
        torch.cuda.synchronize()
        ti.locate_batch_device(sp_d.data_ptr(), 5, cap, d_d.data_ptr(), o_d.data_ptr(), l_d.data_ptr())
        ti.sync()
        docs, offs, heads = dc.locate_rows(c["sa"], c["da"], c["starts"], want, cap)
        assert np.array_equal(l_d.cpu().numpy().view(np.uint32), heads)
        assert np.array_equal(d_d.cpu().numpy(), docs) and np.array_equal(o_d.cpu().numpy(), offs)


# ---- random texts, random tables -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model_b():
    """model B once per text and mode: (count, distinct, sorted entries) of the matched part of every context"""
    out = {}
    for name in dc.RANDOM:
        c, e = dc.random_case(name), nc.expected(name)
        for cfg in ((0, 0, 1), (1, 0, 0)):
            out[name, cfg] = [dc.model_b(c["t"], c["starts"], ctx[len(ctx) - int(sp[2]):]) for ctx, sp in zip(e["ctx"], e["spans"][cfg])]
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(dc.RANDOM))
def test_random_texts_against_both_models(gpu, model_b, name, mode):
    c, e = dc.random_case(name), nc.expected(name)
    cfg = (1, 0, 0) if mode else (0, 0, 1)
    sa, starts, da = c["sa"], c["starts"], c["da"]
    want_spans = e["spans"][cfg]
    spans = [(int(s[0]), int(s[1])) for s in want_spans]
    with gpu.TokenIndex.build(c["t"]) as ti:
        ti.set_documents(starts)
        got_da, got_pv = ti.doc_range(0, sa.size)
        assert np.array_equal(got_da, da) and np.array_equal(got_pv, c["pv"])
        for cap, budget in ((16, 0), (0, 0), (64, 100), (1, 1)):
            docs, offs, heads = dc.docs_rows(dc.docs_full(sa, da, starts, spans, budget), cap)
            got = ti.docs_batch(e["ctx"], cap=cap, budget=budget, mode=mode, need_next=False, fill=FILL)
            assert np.array_equal(got["spans"].view(np.uint32).reshape(-1, 4), want_spans), (name, mode, cap, budget)
            hd = got["heads"].view(np.uint32).reshape(-1, 4)
            bad = np.flatnonzero((hd != heads).any(axis=1) | (got["docs"] != docs).any(axis=1) | (got["offsets"] != offs).any(axis=1))
            assert bad.size == 0, (name, mode, cap, budget, [(e["ctx"][i][:6], spans[i], hd[i].tolist(), heads[i].tolist()) for i in bad[:5]])
            if budget == 0:                                                                           # model B: no suffix array behind it
                for i, (count, distinct, occ) in enumerate(model_b[name, cfg]):
                    assert (int(hd[i, 3]), int(hd[i, 2]), int(hd[i, 1])) == (count, distinct, count), (name, mode, i)
                    w = int(hd[i, 0])
                    assert set(zip(got["docs"][i, :w].tolist(), got["offsets"][i, :w].tolist())) <= set(occ), (name, mode, i)
        if mode == 0:
            cap = 4096
            got = ti.locate_batch(e["ctx"], cap=cap, fill=FILL)
            docs, offs, heads = dc.locate_rows(sa, da, starts, spans, cap)
            assert np.array_equal(got["heads"].view(np.uint32).reshape(-1, 2), heads), name
            assert np.array_equal(got["docs"], docs) and np.array_equal(got["offsets"], offs), name
            for i, (count, distinct, occ) in enumerate(model_b[name, cfg]):                           # the entries as a multiset
                if count <= cap:
                    assert sorted(zip(got["docs"][i, :count].tolist(), got["offsets"][i, :count].tolist())) == occ, (name, i)


# ---- the device chain ----------------------------------------------------------------------------------------------------------

def test_device_chain_equals_the_host_forms(gpu):
    import torch
    c, e = dc.random_case("rand_k1000"), nc.expected("rand_k1000")
    nctx = len(e["ctx"])
    cap, budget = 5, 40
    with gpu.TokenIndex.build(c["t"], 1000) as ti:
        ti.set_documents(c["starts"])
        assert ti.docs_batch([], cap=cap)["docs"].shape == (0, cap) and ti.locate_batch([], cap=cap)["heads"].size == 0   # Q == 0
        kept = []
        for q in (1, 3, 4, 5, 255, 256, 257):
            sub = [e["ctx"][(7 * k + q) % nctx] if k % 5 else [] for k in range(q)]                       # empty contexts inside
            for mode in (0, 1):
                hdocs = ti.docs_batch(sub, cap=cap, budget=budget, mode=mode, need_next=False, fill=FILL)
                hloc = ti.locate_batch(sub, cap=cap, fill=FILL) if mode == 0 else None
                buf, off = tc.pack(sub)
                pd, od = _dev(buf if buf.size else np.zeros(1, np.int32)), _dev(off.view(np.int64))
                sp_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
                outs = [torch.full((q, cap), FILL, dtype=torch.int32, device="cuda:0") for _ in range(4)]
                h_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
                l_d = torch.zeros((q, 2), dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()
                ti.spans_batch_device(pd.data_ptr(), od.data_ptr(), q, mode, 0, 0, sp_d.data_ptr())   # three launches, one sync
                ti.docs_batch_device(sp_d.data_ptr(), q, cap, budget, outs[0].data_ptr(), outs[1].data_ptr(), h_d.data_ptr())
                ti.locate_batch_device(sp_d.data_ptr(), q, cap, outs[2].data_ptr(), outs[3].data_ptr(), l_d.data_ptr())
                ti.sync()
                assert sp_d.cpu().numpy().tobytes() == hdocs["spans"].tobytes(), (q, mode)
                assert outs[0].cpu().numpy().tobytes() == hdocs["docs"].tobytes(), (q, mode)
                assert outs[1].cpu().numpy().tobytes() == hdocs["offsets"].tobytes(), (q, mode)
                assert h_d.cpu().numpy().tobytes() == hdocs["heads"].tobytes(), (q, mode)
                if mode == 0:
                    assert outs[2].cpu().numpy().tobytes() == hloc["docs"].tobytes(), q
                    assert outs[3].cpu().numpy().tobytes() == hloc["offsets"].tobytes(), q
                    assert l_d.cpu().numpy().tobytes() == hloc["heads"].tobytes(), q
                    assert hloc["spans"].tobytes() == hdocs["spans"].tobytes(), q
                info = ti.docs_info()
                assert info["docs_q"] == q and info["locate_q"] == q and info["locate_ms"] > 0 and info["docs_ms"] > 0, info
                assert info["examined"] == int(hdocs["heads"]["examined"].sum()), (q, mode, info)
                kept.append((pd, od, sp_d, outs, h_d, l_d))


# ---- locate --------------------------------------------------------------------------------------------------------------------

def test_locate_against_sa_range_and_searchsorted(gpu):
    c = dc.equal_case(64)
    n, starts, cap = dc.N_EQ, c["starts"], 16
    counts = (0, 1, cap - 1, cap, cap + 1, n)
    pats = [[dc.A] * (n - k + 1) for k in counts]
    with gpu.TokenIndex.build(c["t"]) as ti:
        ti.set_documents(starts)
        got = ti.locate_batch(pats, cap=cap, fill=FILL)
        first, count = ti.query_batch(pats)["first"], ti.query_batch(pats)["second"]
        assert count.tolist() == list(counts)
        for i, k in enumerate(counts):
            w = min(k, cap)
            pos = ti.sa_range(int(first[i]), w).astype(np.int64)
            d = np.searchsorted(starts, pos, "right") - 1
            assert (int(got["heads"]["written"][i]), int(got["heads"]["count"][i])) == (w, k), (i, k)
            assert got["docs"][i, :w].tolist() == d.tolist() and got["offsets"][i, :w].tolist() == (pos - starts[d]).tolist(), (i, k)
            assert (got["docs"][i, w:] == FILL).all() and (got["offsets"][i, w:] == FILL).all(), (i, k)
        # [A] from rank 0: position n - 1, the last entry of the last document -- its end is starts[D] = n
        D = starts.size
        assert got["docs"][-1, 0] == D - 1 and got["offsets"][-1, 0] == n - 1 - starts[D - 1] and starts[D - 1] + got["offsets"][-1, 0] + 1 == n


# ---- the Python class ----------------------------------------------------------------------------------------------------------

def test_python_class(gpu):
    import suffixarray_amd
    rng = np.random.default_rng(8)
    tokens = rng.integers(0, 5, 400).astype(np.int32)
    starts = np.array(sorted({0} | set(rng.integers(1, 400, 14).tolist())) + [400], np.int32)        # the last document is empty
    tl = tokens.tolist()
    ngrams = sorted({tuple(tl[p:p + m]) for m in (1, 2, 3) for p in range(400 - m + 1)}) + [(9,), (4, 4, 4, 4, 4, 4, 4)]
    ngrams = [list(g) for g in ngrams]
    model = [dc.model_b(tokens, starts, g) for g in ngrams]
    with suffixarray_amd.TokenIndex(tokens, doc_starts=starts) as ti, suffixarray_amd.TokenIndex(tokens) as bare:
        distinct, exact = ti.document_counts(ngrams)
        assert distinct.dtype == np.uint32 and exact.dtype == np.bool_ and exact.all()
        assert distinct.tolist() == [m[1] for m in model]
        r = ti.documents(ngrams, cap=16)
        assert sorted(r) == ["count", "distinct", "docs", "exact", "examined", "offsets", "written"]
        assert r["count"].tolist() == [m[0] for m in model] and r["distinct"].tolist() == distinct.tolist() and r["exact"].all()
        assert r["docs"].shape == (len(ngrams), 16) and r["written"].tolist() == [min(m[1], 16) for m in model]
        for i, g in enumerate(ngrams):
            d, o = ti.locate(g, limit=1000)
            assert d.dtype == np.int32 and o.dtype == np.int32 and d.size == model[i][0], g
            assert sorted(zip(d.tolist(), o.tolist())) == model[i][2], g
            for dd, oo in zip(d.tolist(), o.tolist()):                                                # the round trip
                assert tl[starts[dd] + oo:starts[dd] + oo + len(g)] == g, (g, dd, oo)
            assert len(set(d.tolist())) == distinct[i], g
            w = int(r["written"][i])
            assert len(set(r["docs"][i, :w].tolist())) == w and set(zip(r["docs"][i, :w].tolist(), r["offsets"][i, :w].tolist())) <= set(model[i][2]), g
        assert ti.locate(ngrams[0], limit=2)[0].size == min(2, model[0][0]) and ti.locate([9], limit=5)[0].size == 0
        d1, e1 = ti.document_counts(ngrams, budget=1)
        assert d1.tolist() == [min(m[0], 1) for m in model] and e1.tolist() == [m[0] <= 1 for m in model]
        rs = ti.documents([[1, 2, 9], [9]], cap=4, longest_suffix=True)                               # backs off to [] : every rank
        assert rs["count"].tolist() == [400, 400] and rs["distinct"].tolist() == [len(set(dc.doc_of(starts, np.arange(400)).tolist()))] * 2
        ti.set_documents([0])                                                                         # replaced: one document
        assert ti.document_counts(ngrams)[0].tolist() == [min(m[0], 1) for m in model]
        # without documents: the new methods raise, the old ones answer as before
        for call in (lambda: bare.locate([1], 3), lambda: bare.documents([[1]]), lambda: bare.document_counts([[1]])):
            with pytest.raises(gpu.SaHipError) as err:
                call()
            assert err.value.code == -1
        assert np.array_equal(bare.count(ngrams), ti.count(ngrams)) and bare.count(ngrams).tolist() == [m[0] for m in model]
        assert all(np.array_equal(a, b) for a, b in zip(bare.ranges(ngrams), ti.ranges(ngrams)))
        uni = [tl[0]]
        assert np.array_equal(bare.positions(uni), ti.positions(uni)) and bare.positions(uni, limit=2).size == 2
        assert bare.next_token_counts(ngrams[1]) == ti.next_token_counts(ngrams[1])
        assert all(np.array_equal(a, b) for a, b in zip(bare.longest_suffix([[9, 1, 2], [1]]), ti.longest_suffix([[9, 1, 2], [1]])))
        assert bare.info()["n"] == 400 and bare.n == 400
    with pytest.raises(gpu.SaHipError):
        suffixarray_amd.TokenIndex(tokens, doc_starts=[0, 401])
    with pytest.raises(ValueError):
        suffixarray_amd.TokenIndex(tokens, doc_starts=[])
