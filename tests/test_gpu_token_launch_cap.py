"""Every wave-per-row kernel of the token index and the shard sets beyond the launch cap: wave_row_grid() caps a launch at
WAVE_GRID_MAX workgroups of NEXT_WAVES waves, and each kernel serves the rows beyond NEXT_WAVES * WAVE_GRID_MAX = 16384 by its
`for (row = ...; row < rows; row += waves)` loop.  One test per loop (token_walk_cases.ROW_LOOPS; tq_top_kernel and
tq_shard_top_kernel have theirs in test_gpu_token_top.py and test_gpu_token_shard_top.py) with 16384, 16385 and 32769 rows.

Row i is base[i % B] with B odd, so on its second trip every wave meets a row other than its first; the base rows come from the
existing case modules and the expected values are their CPU models over the base rows, tiled.  Each kernel is run through its host
form and through the device chain, whose outputs are tensors of a sentinel with one guard row in front of row 0 and one behind the
last row: guards and unwritten cells must be intact."""
import numpy as np
import pytest

import token_all_cases as ac
import token_cases as tc
import token_doc_cases as dc
import token_match_cases as mc
import token_next_cases as nc
import token_score_cases as sc
import token_shard_all_cases as sall
import token_shard_cases as ssh
import token_shard_doc_cases as sd
import token_shard_score_cases as ssc
import token_walk_cases as wc
from test_int_cpu import model_sa

pytestmark = pytest.mark.gpu

FILL = -7
UFILL = FILL & 0xFFFFFFFF
ROWS = (wc.CAP_ROWS, wc.CAP_ROWS + 1, 2 * wc.CAP_ROWS + 1)         # the last row of the first trip, one more, and a third trip
CAP = 4


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class _Guarded:
    """an int32 device output of `rows` rows of `width` cells filled with the sentinel, one guard row on either side"""

    def __init__(self, rows, width, dtype=None):
        import torch
        self.rows, self.width = rows, width
        self.t = torch.full((rows + 2, width), FILL, dtype=dtype or torch.int32, device="cuda:0")
        self.ptr = self.t[1:].data_ptr()

    def body(self):
        """the rows between the guards, after asserting that the guards still hold the sentinel"""
        a = self.t.cpu().numpy()
        assert (a[0] == FILL).all() and (a[-1] == FILL).all(), "a guard row was written"
        return a[1:-1]


def _odd(items, most=199):
    """an odd number of them, 50 .. 200"""
    items = list(items)[:most]
    items = items if len(items) % 2 else items[:-1]
    assert 50 <= len(items) <= 200 and len(items) % 2 == 1, len(items)
    return items


def _small(e):
    """the indices of the contexts of at most 8 symbols"""
    return [i for i, c in enumerate(e["ctx"]) if len(c) <= 8]


def _same(got, want, where):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.flatnonzero((got.reshape(got.shape[0], -1) != want.reshape(want.shape[0], -1)).any(axis=1))
    assert bad.size == 0, (where, bad[:5].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist())


# ---- tq_next_kernel (token_next.hpp) -------------------------------------------------------------------------------------------

def test_next_symbols(gpu, monkeypatch):
    import torch
    nc.set_plan(monkeypatch, "default")
    e = nc.expected("rand_k1000")
    cfg = (1, 0, 1)
    base = _odd(_small(e))
    B = len(base)
    sym, cnt, heads = nc.capped([e["entries"][cfg][i] for i in base], CAP, FILL, UFILL)
    spans = e["spans"][cfg][base]
    assert (heads[:, 0] == CAP).any() and (heads[:, 0] < CAP).any()                               # full rows and rows with unwritten cells
    with gpu.TokenIndex.build(e["t"], 1000) as ti:
        for Q in ROWS:
            idx = np.arange(Q) % B
            buf, off = tc.pack([e["ctx"][base[j]] for j in idx])
            host = ti.next_batch((buf, off), cap=CAP, mode=1, fill=FILL)
            _same(host["spans"].view(np.uint32).reshape(-1, 4), spans[idx], (Q, "spans"))
            _same(host["symbols"], sym[idx], (Q, "symbols"))
            _same(host["counts"], cnt[idx], (Q, "counts"))
            _same(host["heads"].view(np.uint32).reshape(-1, 4), heads[idx], (Q, "heads"))
            info = ti.next_info()
            assert info["q"] == Q and info["lane_spans"] == 0 and info["wave_spans"] == Q, info
            pd, od = _dev(buf), _dev(off.view(np.int64))
            sp_d, sy_d, ct_d, hd_d = _Guarded(Q, 4), _Guarded(Q, CAP), _Guarded(Q, CAP), _Guarded(Q, 4)
            torch.cuda.synchronize()
            ti.spans_batch_device(pd.data_ptr(), od.data_ptr(), Q, 1, 0, 1, sp_d.ptr)
            ti.next_batch_device(sp_d.ptr, Q, CAP, sy_d.ptr, ct_d.ptr, hd_d.ptr)
            ti.sync()
            _same(sp_d.body().view(np.uint32), spans[idx], (Q, "device spans"))
            _same(sy_d.body(), sym[idx], (Q, "device symbols"))
            _same(ct_d.body().view(np.uint32), cnt[idx], (Q, "device counts"))
            _same(hd_d.body().view(np.uint32), heads[idx], (Q, "device heads"))


def test_next_symbols_the_list_form_strides(gpu, monkeypatch):
    """plan `lanes`: the spans of more than NEXT_LANE_MAX suffixes go to a list that tq_next_kernel walks by list[w]; more than
    16384 of them, between spans that their lane answers"""
    nc.set_plan(monkeypatch, "lanes")
    e = nc.expected("rand_k2")
    cfg = (1, 0, 1)
    tl, sl = [int(v) for v in e["t"]], [int(v) for v in e["sa"]]
    rng = np.random.default_rng(19)
    ctx = []                                                       # windows of 1 .. 18 symbols: a window of 14 occurs about 3 times
    for j in range(101):
        p = int(rng.integers(0, len(tl) - 18))
        ctx.append(tl[p:p + 1 + j % 18])
    B = len(ctx)
    spans = nc.spans_a(tl, sl, ctx, *cfg)
    sym, cnt, heads = nc.capped([nc.entries_a(e["t"], e["sa"], s) for s in spans], CAP, FILL, UFILL)
    big = spans[:, 1] > wc.NEXT_LANE_MAX
    with gpu.TokenIndex.build(e["t"]) as ti:
        for Q in ROWS:
            idx = np.arange(Q) % B
            listed = int(big[idx].sum())
            assert (Q < ROWS[2] or listed > wc.CAP_ROWS) and 0 < listed < Q, (Q, listed)
            host = ti.next_batch(tc.pack([ctx[j] for j in idx]), cap=CAP, mode=1, fill=FILL)
            _same(host["spans"].view(np.uint32).reshape(-1, 4), spans[idx], (Q, "spans"))
            _same(host["symbols"], sym[idx], (Q, "symbols"))
            _same(host["counts"], cnt[idx], (Q, "counts"))
            _same(host["heads"].view(np.uint32).reshape(-1, 4), heads[idx], (Q, "heads"))
            info = ti.next_info()
            assert info["q"] == Q and info["wave_spans"] == listed and info["lane_spans"] + info["wave_spans"] == Q, info


# ---- tq_docs_kernel (token_docs.hpp) -------------------------------------------------------------------------------------------

def test_documents(gpu):
    import torch
    c, e = dc.random_case("rand_k1000"), nc.expected("rand_k1000")
    cfg, budget = (1, 0, 0), 40
    base = _odd(_small(e))
    B = len(base)
    spans = e["spans"][cfg][base]
    docs, offs, heads = dc.docs_rows(dc.docs_full(c["sa"], c["da"], c["starts"], [(int(s[0]), int(s[1])) for s in spans], budget), CAP)
    assert (heads[:, 0] == CAP).any() and (heads[:, 0] < CAP).any() and (heads[:, 1] == budget).any()
    with gpu.TokenIndex.build(c["t"], 1000) as ti:
        ti.set_documents(c["starts"])
        for Q in ROWS:
            idx = np.arange(Q) % B
            buf, off = tc.pack([e["ctx"][base[j]] for j in idx])
            host = ti.docs_batch((buf, off), cap=CAP, budget=budget, mode=1, need_next=False, fill=FILL)
            _same(host["spans"].view(np.uint32).reshape(-1, 4), spans[idx], (Q, "spans"))
            _same(host["docs"], docs[idx], (Q, "docs"))
            _same(host["offsets"], offs[idx], (Q, "offsets"))
            _same(host["heads"].view(np.uint32).reshape(-1, 4), heads[idx], (Q, "heads"))
            info = ti.docs_info()
            assert info["docs_q"] == Q and info["examined"] == int(heads[idx, 1].astype(np.int64).sum()), (Q, info)   # streamed ranks: per row
            pd, od = _dev(buf), _dev(off.view(np.int64))
            sp_d, d_d, o_d, h_d = _Guarded(Q, 4), _Guarded(Q, CAP), _Guarded(Q, CAP), _Guarded(Q, 4)
            torch.cuda.synchronize()
            ti.spans_batch_device(pd.data_ptr(), od.data_ptr(), Q, 1, 0, 0, sp_d.ptr)
            ti.docs_batch_device(sp_d.ptr, Q, CAP, budget, d_d.ptr, o_d.ptr, h_d.ptr)
            ti.sync()
            _same(d_d.body(), docs[idx], (Q, "device docs"))
            _same(o_d.body(), offs[idx], (Q, "device offsets"))
            _same(h_d.body().view(np.uint32), heads[idx], (Q, "device heads"))
            assert ti.docs_info()["examined"] == int(heads[idx, 1].astype(np.int64).sum()), Q


# ---- tq_all_kernel (token_all.hpp) ---------------------------------------------------------------------------------------------

def test_documents_holding_all(gpu):
    """a row is a group of 1 .. 3 patterns"""
    import torch
    c, e = ac.random_case("rand_k1000"), nc.expected("rand_k1000")
    cfg, budget = (1, 0, 0), 40
    n = c["t"].size
    small = _small(e)
    B = 101
    groups = [[small[(5 * g + 3 * j) % len(small)] for j in range(1 + g % 3)] for g in range(B)]
    spans = e["spans"][cfg]
    sgroups = [[(int(spans[i][0]), int(spans[i][1])) for i in g] for g in groups]
    full = [ac.all_a(ac.all_walk(c["sa"], c["da"], c["cl"], n, g), ac.group_first(n, g), budget) for g in sgroups]
    docs, offs, heads = ac.all_rows(full, CAP)
    assert (heads[:, 0] == CAP).any() and (heads[:, 0] < CAP).any()
    with gpu.TokenIndex.build(c["t"], 1000) as ti:
        ti.set_documents(c["starts"])
        ti.prepare_doc_ranks()
        for G in ROWS:
            idx = np.arange(G) % B
            flat = [e["ctx"][i] for g in idx for i in groups[g]]
            goff = np.cumsum([0] + [len(groups[g]) for g in idx]).astype(np.uint64)
            P = len(flat)
            buf, off = tc.pack(flat)
            host = ti.all_batch((buf, off), goff, cap=CAP, budget=budget, mode=1, need_next=False, fill=FILL)
            _same(host["docs"], docs[idx], (G, "docs"))
            _same(host["offsets"], offs[idx], (G, "offsets"))
            _same(host["heads"].view(np.uint32).reshape(-1, 8), heads[idx], (G, "heads"))
            pd, od = _dev(buf), _dev(off.view(np.int64))
            sp_d, d_d, o_d, h_d = _Guarded(P, 4), _Guarded(G, CAP), _Guarded(G, CAP), _Guarded(G, 8)
            torch.cuda.synchronize()
            ti.spans_batch_device(pd.data_ptr(), od.data_ptr(), P, 1, 0, 0, sp_d.ptr)
            ti.all_batch_device(sp_d.ptr, P, goff, CAP, budget, d_d.ptr, o_d.ptr, h_d.ptr)
            ti.sync()
            _same(d_d.body(), docs[idx], (G, "device docs"))
            _same(o_d.body(), offs[idx], (G, "device offsets"))
            _same(h_d.body().view(np.uint32), heads[idx], (G, "device heads"))
            assert ti.doc_ranks_info()["all_q"] == G


# ---- tq_match_docs_kernel (token_match.hpp), tq_score_docs_kernel (token_score.hpp) --------------------------------------------

def _query_docs(tl, B=101, seed=23):
    """B query documents of 1 .. 3 tokens: windows of the text, every fourth with a token that occurs nowhere"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(B):
        p = int(rng.integers(0, len(tl) - 3))
        doc = tl[p:p + 1 + j % 3]
        if j % 4 == 3:
            doc[len(doc) // 2] = mc.NONE                          # in the middle of three tokens: two maximal matches
        out.append(doc)
    return out


def _tiled_positions(base_docs, idx):
    """for the batch of documents base_docs[idx]: (documents, the flat positions of the base batch that its positions repeat)"""
    boff = np.cumsum([0] + [len(d) for d in base_docs])
    return [base_docs[j] for j in idx], np.concatenate([np.arange(boff[j], boff[j + 1]) for j in idx])


def test_matching_statistics_per_document(gpu, monkeypatch):
    """a row is a query document"""
    import torch
    mc.set_plan(monkeypatch, "default")
    t = mc.texts()["rand_k1000"]
    tl, sl = [int(v) for v in t], [int(v) for v in model_sa(t)]
    base = _query_docs(tl)
    B, mlen = len(base), 1
    spans = mc.spans_a(tl, sl, base, 0)
    ha = mc.heads_a(spans[:, 2], base, mlen)
    pos, outs, hd = mc.rows([f for f, _ in ha], [h for _, h in ha], spans, CAP, FILL)
    assert (hd[:, 0] == 0).any() and (hd[:, 0] > 1).any()
    with gpu.TokenIndex.build(t) as ti:
        for Q in ROWS:
            idx = np.arange(Q) % B
            docs, at = _tiled_positions(base, idx)
            buf, off = mc.pack(docs)
            total = int(off[-1])
            host = ti.match_docs_batch((buf, off), min_length=mlen, cap=CAP, fill=FILL)
            _same(host["spans"].view(np.uint32).reshape(-1, 4), spans[at], (Q, "spans"))
            _same(host["positions"], pos[idx], (Q, "positions"))
            _same(host["out_spans"].view(np.uint32).reshape(Q, CAP, 4), outs[idx], (Q, "out_spans"))
            _same(host["heads"].view(np.uint32).reshape(-1, 4), hd[idx], (Q, "heads"))
            pd, od = _dev(buf), _dev(off.view(np.int64))
            sp_d, ps_d, os_d, hd_d = _Guarded(total, 4), _Guarded(Q, CAP), _Guarded(Q, CAP * 4), _Guarded(Q, 4)
            torch.cuda.synchronize()
            ti.match_batch_device(pd.data_ptr(), od.data_ptr(), Q, total, 0, sp_d.ptr)
            ti.match_docs_batch_device(sp_d.ptr, od.data_ptr(), Q, mlen, CAP, ps_d.ptr, os_d.ptr, hd_d.ptr)
            ti.sync()
            _same(sp_d.body().view(np.uint32), spans[at], (Q, "device spans"))
            _same(ps_d.body().view(np.uint32), pos[idx], (Q, "device positions"))
            _same(os_d.body().view(np.uint32).reshape(Q, CAP, 4), outs[idx], (Q, "device out_spans"))
            _same(hd_d.body().view(np.uint32), hd[idx], (Q, "device heads"))
            info = ti.match_info()
            assert info["q"] == Q and info["positions"] == total, info


def _score_head_rows(h):
    return np.stack([h[k].astype(np.uint64) for k in ("scored", "seen", "certain", "longest", "length_sum")], axis=1)


def test_scores_per_document(gpu, monkeypatch):
    """a row is a query document"""
    import torch
    sc.set_plan(monkeypatch, "default")
    t = mc.texts()["rand_k1000"]
    tl, sl = [int(v) for v in t], [int(v) for v in model_sa(t)]
    base = _query_docs(tl)
    B = len(base)
    scores, _ = sc.score_a(tl, sl, base, 0)
    heads = sc.heads_of(scores, base)
    assert len({tuple(h) for h in heads.tolist()}) > 3
    with gpu.TokenIndex.build(t) as ti:
        for Q in ROWS:
            idx = np.arange(Q) % B
            docs, at = _tiled_positions(base, idx)
            buf, off = sc.pack(docs)
            total = int(off[-1])
            host = ti.score_batch((buf, off), max_length=0)
            _same(host["scores"].view(np.uint32).reshape(-1, 4), scores[at], (Q, "scores"))
            _same(_score_head_rows(host["heads"]), heads[idx], (Q, "heads"))
            pd, od = _dev(buf), _dev(off.view(np.int64))
            s_d, h_d = _Guarded(total, 4), _Guarded(Q, 6)
            torch.cuda.synchronize()
            ti.score_batch_device(pd.data_ptr(), od.data_ptr(), Q, total, 0, None, s_d.ptr)
            ti.score_docs_batch_device(s_d.ptr, od.data_ptr(), Q, h_d.ptr)
            ti.sync()
            _same(s_d.body().view(np.uint32), scores[at], (Q, "device scores"))
            assert h_d.body().tobytes() == host["heads"].tobytes(), (Q, "device heads")
            info = ti.score_info()
            assert info["q"] == Q and info["positions"] == total, info


# ---- shard sets, S = 3 -----------------------------------------------------------------------------------------------------------
# The pair kernels serve (row, shard) pairs, rows * S of them: 5461 rows are 16383 pairs, 5462 are 16386.  SA_HIP_TOKEN_SHARD_CHUNK is
# left alone: the default chunk is far above the cap, and every test asserts from the set's info that one chunk held all rows.

PAIR_ROWS = (5461, 5462, wc.CAP_ROWS + 1)
FILL64 = FILL & 0xFFFFFFFFFFFFFFFF


def _g64(rows, width):
    import torch
    return _Guarded(rows, width, torch.int64)


def _tuples(a):
    return [tuple(int(v) for v in r) for r in a.tolist()]


def _variants(cases, S, n, vary):
    """n synthetic rows from the hand-made `cases` of the merge tests: case i % len(cases), changed by vary(list of shard s, i // len)"""
    return [[vary(cases[i % len(cases)][s], i // len(cases)) for i in range(n)] for s in range(S)]


def test_shard_next_merge(gpu):
    """tq_next_merge_kernel (token_shards.hpp): the host form and the device chain over 16385 contexts, and the merge alone"""
    import torch
    from test_gpu_token_shards import _merge_model
    e = ssh.expected("s3")
    S, cfg = 3, (1, 0, 1)
    base = _odd([i for i, c in enumerate(e["ctx"]) if len(c) <= 8])
    B = len(base)
    L, totals, spans, entries = e[cfg]
    spans = spans[:, base]
    sym, cnt, heads = ssh.capped([ssh.span_length(spans)[j] for j in range(B)], [entries[i] for i in base], ssh.next_total(spans), CAP, FILL)
    assert {h[0] for h in heads} >= {1, CAP}
    with gpu.TokenShards.build(e["shards"]) as st:
        for Q in ROWS:
            idx = np.arange(Q) % B
            buf, off = tc.pack([e["ctx"][base[j]] for j in idx])
            host = st.next_batch((buf, off), cap=CAP, mode=1, fill=FILL)
            _same(host["spans"].view(np.uint32).reshape(S, Q, 4), spans[:, idx], (Q, "spans"))
            _same(host["symbols"], sym[idx], (Q, "symbols"))
            _same(host["counts"], cnt[idx], (Q, "counts"))
            assert _tuples(host["heads"]) == [heads[j] for j in idx], (Q, "heads")
            assert st.info()["chunk"] == Q and st.info()["q"] == Q, st.info()
            pd, od = _dev(buf), _dev(off.view(np.int64))
            sp_d, ln_d, tt_d = _Guarded(S * Q, 4), _Guarded(Q, 1), _g64(Q, 1)
            sy_d, ct_d, hd_d = _Guarded(Q, CAP), _g64(Q, CAP), _g64(Q, 3)
            torch.cuda.synchronize()
            st.spans_batch_device(pd.data_ptr(), od.data_ptr(), Q, 1, 0, 1, ln_d.ptr, tt_d.ptr, sp_d.ptr)
            st.next_batch_device(sp_d.ptr, Q, CAP, sy_d.ptr, ct_d.ptr, hd_d.ptr)
            st.sync()
            assert sp_d.body().tobytes() == host["spans"].tobytes(), (Q, "device spans")
            assert sy_d.body().tobytes() == host["symbols"].tobytes() and ct_d.body().tobytes() == host["counts"].tobytes(), (Q, "device lists")
            assert hd_d.body().tobytes() == host["heads"].tobytes(), (Q, "device heads")
            assert ln_d.body().view(np.uint32).ravel().tolist() == host["heads"]["length"].tolist(), (Q, "device lengths")
            assert tt_d.body().ravel().tolist() == host["heads"]["total"].tolist(), (Q, "device totals")
        # the merge alone, on synthetic lists
        M, Q = 0xFFFFFFFF, wc.CAP_ROWS + 1
        cases = [[([3, 9, nc.I32_MAX - 1, nc.I32_MAX], [M, M, M, M], CAP, M)] * S, [([], [], 0, 0)] * S,
                 [([10 * s, 10 * s + 1], [M, 1], 2, M) for s in range(S)], [([s % 3, 5 + s % 2, 100 + s], [M, 2, 3], 3, M) for s in range(S)],
                 [([7], [M], 1, M)] + [([], [], 0, 0)] * (S - 1), [([], [], 0, 0)] * (S - 1) + [([0, nc.I32_MAX], [1, M], 2, M)],
                 [([1, 2, 3, 4], [1, 1, 1, 1], 9, 4)] * S, [([4, 6], [2, 2], 1, 9) for s in range(S)], [([5], [1], 1, 1), ([], [], 0, 0), ([5], [2], 1, 2)]]
        B = 9 * 7
        lists = _variants(cases, S, B, lambda c, v: (c[0], [min(x, M - v) if x == M else x + v for x in c[1]], c[2], c[3]))
        model = _merge_model(S, lists, CAP)
        idx = np.arange(Q) % B
        sym = np.full((S, Q, CAP), 12345, np.int32)
        cnt = np.full((S, Q, CAP), 54321, np.uint32)
        hds = np.zeros((S, Q), gpu.NEXT_DTYPE)
        for s in range(S):
            for i, j in enumerate(idx):
                y, c, w, tot = lists[s][j]
                sym[s, i, :len(y)], cnt[s, i, :len(c)] = y, c
                hds[s, i] = (w, 0, tot, 0)
        sy_d, ct_d, hd_d = _dev(sym), _dev(cnt.view(np.int32)), _dev(hds.view(np.uint32).view(np.int32).reshape(S, Q, 4))
        o_sy, o_ct, o_hd = _Guarded(Q, CAP), _g64(Q, CAP), _g64(Q, 3)
        torch.cuda.synchronize()
        st.merge_device(sy_d.data_ptr(), ct_d.data_ptr(), hd_d.data_ptr(), Q, CAP, o_sy.ptr, o_ct.ptr, o_hd.ptr)
        st.sync()
        w_sy, w_ct = np.full((B, CAP), FILL, np.int32), np.full((B, CAP), FILL64, np.uint64)
        w_hd = []
        for j, (keys, counts, total) in enumerate(model):
            w_sy[j, :len(keys)], w_ct[j, :len(keys)] = keys, counts
            w_hd.append((len(keys), 0, sum(counts), total))
        _same(o_sy.body(), w_sy[idx], "merge symbols")
        _same(o_ct.body().view(np.uint64), w_ct[idx], "merge counts")
        assert _tuples(o_hd.body().view(gpu.SHARDS_NEXT_DTYPE).reshape(Q)) == [w_hd[j] for j in idx], "merge heads"


def _doc_lists(S, B):
    """B synthetic rows of per-shard document lists (docs, offsets, written, examined, distinct / matched, count / candidates): the
    hand-made cases of the merge tests of the shard documents and AND forms, their offsets varied"""
    M = 0xFFFFFFFF
    cases = [[([], [], 0, M, M, M)] * S, [([7], [s], 1, 1, 1, 1) for s in range(S)],
             [([1, 2, 3, 4, 5, 6], [9] * 6, 9, 9, 9, 9)] + [([8], [8], 1, 1, 1, 1)] * (S - 1),
             [([], [], 0, 0, 0, 0)] * (S - 1) + [([2 ** 31 - 1, 0], [5, 6], 2, 2, 2, 2)],
             [([4, 5], [1, 2], 2, 5, 2, 7)] + [([], [], 0, 0, 0, 0)] * (S - 2) + [([6, 7, 8, 9, 1], [3, 4, 5, 6, 7], 5, 5, 5, 5)],
             [([3], [3], 1, 2, M, M)] + [([4], [4], 1, 1, 1, 1)] * (S - 1), [([1, 2], [1, 2], 1, 4, 1, 4) for s in range(S)]]
    return _variants(cases, S, B, lambda c, v: (c[0], [x + v for x in c[1]]) + tuple(c[2:]))


def _doc_list_arrays(gpu, lists, idx, S, cap, head_dtype):
    Q = len(idx)
    docs = np.full((S, Q, cap), 12345, np.int32)
    offs = np.full((S, Q, cap), 54321, np.int32)
    heads = np.zeros((S, Q), head_dtype)
    for s in range(S):
        for i, j in enumerate(idx):
            d, o, w, a, b, c = lists[s][j]
            docs[s, i, :min(len(d), cap)], offs[s, i, :min(len(o), cap)] = d[:cap], o[:cap]
            heads[s, i] = (w, a, b, c)
    return _dev(docs), _dev(offs), _dev(heads.view(np.uint32).view(np.int32).reshape(S, Q, 4))


def _merged_rows(model, cap):
    B = len(model)
    docs, offs = np.full((B, cap), FILL64, np.uint64), np.full((B, cap), FILL, np.int32)
    for j, (ent, _) in enumerate(model):
        for at, (d, o) in ent.items():
            docs[j, at], offs[j, at] = d, o
    return docs, offs, [head for _, head in model]


def test_shard_documents(gpu):
    """tq_shard_docs_kernel over rows * S pairs and tq_shard_docs_merge_kernel over the rows (token_shard_docs.hpp): the host
    form and the device chain, and the merge alone on 16385 synthetic rows"""
    import torch
    from test_gpu_token_shard_docs import _merge_model
    cases = sd.random_set("r3")
    S, budget = 3, 40
    pats = _odd([p for p in sd.random_patterns(cases) if len(p) <= 8])
    B = len(pats)
    spans = sd.spans_of(cases, pats)
    docs, offs, heads = sd.docs_rows(sd.docs_full(cases, spans, budget), CAP)
    assert {h[0] for h in heads} >= {0, CAP} and any(h[1] == budget for h in heads)
    with gpu.TokenShards.build([c["t"] for c in cases]) as st:
        st.set_documents([c["starts"] for c in cases])
        for Q in PAIR_ROWS:
            idx = np.arange(Q) % B
            buf, off = tc.pack([pats[j] for j in idx])
            host = st.docs_batch((buf, off), cap=CAP, budget=budget, fill=FILL)
            want = np.array(spans, np.uint32)[:, idx]                                                 # [S, Q, 2]: (first, count)
            assert np.array_equal(host["spans"]["first"], want[:, :, 0]) and np.array_equal(host["spans"]["count"], want[:, :, 1]), (Q, "spans")
            _same(host["docs"], docs[idx], (Q, "docs"))
            _same(host["offsets"], offs[idx], (Q, "offsets"))
            got = [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(*(host["heads"][k] for k in ("written", "examined", "distinct", "count")))]
            assert got == [heads[j] for j in idx] and not host["heads"]["reserved"].any(), (Q, "heads")
            info = st.docs_info()
            assert info["chunk"] == Q and info["pairs_q"] == S * Q and info["merge_q"] == Q and info["streamed"] == sum(heads[j][1] for j in idx), (Q, info)
            pd, od = _dev(buf), _dev(off.view(np.int64))
            sp_d, ln_d, tt_d = _Guarded(S * Q, 4), _Guarded(Q, 1), _g64(Q, 1)
            d_d, o_d, h_d = _g64(Q, CAP), _Guarded(Q, CAP), _g64(Q, 4)
            torch.cuda.synchronize()
            st.spans_batch_device(pd.data_ptr(), od.data_ptr(), Q, 0, 0, 0, ln_d.ptr, tt_d.ptr, sp_d.ptr)
            st.docs_batch_device(sp_d.ptr, Q, CAP, budget, d_d.ptr, o_d.ptr, h_d.ptr)
            st.sync()
            assert sp_d.body().tobytes() == host["spans"].tobytes(), (Q, "device spans")
            assert d_d.body().tobytes() == host["docs"].tobytes() and o_d.body().tobytes() == host["offsets"].tobytes(), (Q, "device lists")
            assert h_d.body().tobytes() == host["heads"].tobytes(), (Q, "device heads")
        # the merge alone
        Q, B = wc.CAP_ROWS + 1, 63
        bases = [s * (2 ** 32 + 5) for s in range(S + 1)]
        lists = _doc_lists(S, B)
        w_d, w_o, w_h = _merged_rows(_merge_model(S, lists, bases, CAP), CAP)
        idx = np.arange(Q) % B
        dd, od, hd = _doc_list_arrays(gpu, lists, idx, S, CAP, gpu.DOCS_DTYPE)
        bd = _dev(np.array(bases, np.uint64).view(np.int64))
        o_d, o_o, o_h = _g64(Q, CAP), _Guarded(Q, CAP), _g64(Q, 4)
        torch.cuda.synchronize()
        st.docs_merge_device(dd.data_ptr(), od.data_ptr(), hd.data_ptr(), Q, CAP, o_d.ptr, o_o.ptr, o_h.ptr, bases_dev_ptr=bd.data_ptr())
        st.sync()
        _same(o_d.body().view(np.uint64), w_d[idx], "merge docs")
        _same(o_o.body(), w_o[idx], "merge offsets")
        h = o_h.body().view(gpu.SHARDS_DOCS_DTYPE).reshape(Q)
        got = [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(*(h[k] for k in ("written", "examined", "distinct", "count")))]
        assert got == [w_h[j] for j in idx] and not h["reserved"].any(), "merge heads"


def test_shard_documents_holding_all(gpu):
    """tq_shard_all_plan_kernel over the groups, tq_shard_all_kernel over groups * S pairs and tq_shard_all_merge_kernel over
    the groups (token_shard_all.hpp): the host form and the device chain, and the merge alone on 16385 synthetic rows"""
    import torch
    from test_gpu_token_shard_all import _merge_model
    cases = sall.ranked(sd.random_set("r3"))
    S, budget, B = 3, 40, 101
    pats = sall.frequent_patterns(cases) + [p for p in sd.random_patterns(cases) if len(p) <= 8][:20]
    groups = [[(5 * g + 3 * j) % len(pats) for j in range(1 + g % 3)] for g in range(B)]
    spans = sd.spans_of(cases, pats)
    gsp = [sall.group_spans(spans, g) for g in groups]
    docs, offs, heads = sall.all_rows(sall.all_full(cases, gsp, budget), CAP)
    assert {h[0] for h in heads} >= {0, CAP}
    keys = ("written", "driver", "examined", "matched", "candidates", "count")
    with gpu.TokenShards.build([c["t"] for c in cases]) as st:
        st.set_documents([c["starts"] for c in cases])
        st.prepare_doc_ranks()
        for G in PAIR_ROWS:
            idx = np.arange(G) % B
            flat = [pats[i] for g in idx for i in groups[g]]
            goff = np.cumsum([0] + [len(groups[g]) for g in idx]).astype(np.uint64)
            P = len(flat)
            buf, off = tc.pack(flat)
            host = st.all_batch((buf, off), goff, cap=CAP, budget=budget, fill=FILL)
            _same(host["docs"], docs[idx], (G, "docs"))
            _same(host["offsets"], offs[idx], (G, "offsets"))
            assert [tuple(int(host["heads"][k][i]) for k in keys) for i in range(G)] == [heads[g] for g in idx], (G, "heads")
            info = st.doc_ranks_info()
            assert info["chunk"] == G and info["plan_q"] == info["merge_q"] == G and info["pairs_q"] == S * G, (G, info)
            assert info["streamed"] == sum(heads[g][2] for g in idx), (G, info)
            pd, od = _dev(buf), _dev(off.view(np.int64))
            sp_d, ln_d, tt_d = _Guarded(S * P, 4), _Guarded(P, 1), _g64(P, 1)
            d_d, o_d, h_d = _g64(G, CAP), _Guarded(G, CAP), _g64(G, 5)
            torch.cuda.synchronize()
            st.spans_batch_device(pd.data_ptr(), od.data_ptr(), P, 0, 0, 0, ln_d.ptr, tt_d.ptr, sp_d.ptr)
            st.all_batch_device(sp_d.ptr, P, goff, CAP, budget, d_d.ptr, o_d.ptr, h_d.ptr)
            st.sync()
            assert sp_d.body().tobytes() == host["spans"].tobytes(), (G, "device spans")
            assert d_d.body().tobytes() == host["docs"].tobytes() and o_d.body().tobytes() == host["offsets"].tobytes(), (G, "device lists")
            assert h_d.body().tobytes() == host["heads"].tobytes(), (G, "device heads")
        # the merge alone
        G, B = wc.CAP_ROWS + 1, 63
        bases = [s * (2 ** 32 + 5) for s in range(S + 1)]
        lists = _doc_lists(S, B)
        plan = [((3 * j) % 16, 2 ** 36 + j) for j in range(B)]
        w_d, w_o, w_h = _merged_rows(_merge_model(S, lists, plan, bases, CAP), CAP)
        idx = np.arange(G) % B
        dd, od, hd = _doc_list_arrays(gpu, lists, idx, S, CAP, gpu.SHARDS_ALL_PAIR_DTYPE)
        pl = np.zeros(G, gpu.SHARDS_ALL_PLAN_DTYPE)
        for i, j in enumerate(idx):
            pl[i] = (plan[j][0], 0, plan[j][1])
        pl_d, bd = _dev(pl.view(np.int64).reshape(G, 2)), _dev(np.array(bases, np.uint64).view(np.int64))
        o_d, o_o, o_h = _g64(G, CAP), _Guarded(G, CAP), _g64(G, 5)
        torch.cuda.synchronize()
        st.all_merge_device(dd.data_ptr(), od.data_ptr(), hd.data_ptr(), pl_d.data_ptr(), G, CAP, o_d.ptr, o_o.ptr, o_h.ptr, bases_dev_ptr=bd.data_ptr())
        st.sync()
        _same(o_d.body().view(np.uint64), w_d[idx], "merge docs")
        _same(o_o.body(), w_o[idx], "merge offsets")
        h = o_h.body().view(gpu.SHARDS_ALL_DTYPE).reshape(G)
        assert [tuple(int(h[k][i]) for k in keys) for i in range(G)] == [w_h[j] for j in idx], "merge heads"


def test_shard_scores_per_document(gpu, monkeypatch):
    """tq_shard_score_docs_kernel (token_shard_score.hpp): a row is a query document"""
    import torch
    ssc.set_plan(monkeypatch, "default")
    shards = ssc.make("rand_k1000/3")[0]
    S = len(shards)
    sas = [model_sa(t).astype(np.int32) for t in shards]
    base = _query_docs([int(v) for t in shards for v in t])
    B = len(base)
    scores, per, _ = ssc.score_a(shards, sas, base, 0)
    heads = ssc.heads_of(scores, base)
    rows = ssc.score_bytes(scores)
    assert S == 3 and len({tuple(h) for h in heads.tolist()}) > 3
    with gpu.TokenShards.build(shards) as st:
        for Q in ROWS:
            idx = np.arange(Q) % B
            docs, at = _tiled_positions(base, idx)
            buf, off = ssc.pack(docs)
            total = int(off[-1])
            host = st.score_batch((buf, off), max_length=0)
            assert host["scores"].tobytes() == rows[at].tobytes(), (Q, "scores")
            _same(np.ascontiguousarray(host["per_shard"]).view(np.uint32).reshape(S, total, 4), per[:, at], (Q, "per shard"))
            _same(_score_head_rows(host["heads"]), heads[idx], (Q, "heads"))
            pd, od = _dev(buf), _dev(off.view(np.int64))
            s_d, p_d, h_d = _Guarded(total, 6), _Guarded(S * total, 4), _Guarded(Q, 6)
            torch.cuda.synchronize()
            st.score_batch_device(pd.data_ptr(), od.data_ptr(), Q, total, 0, None, s_d.ptr, p_d.ptr)
            st.score_docs_batch_device(s_d.ptr, od.data_ptr(), Q, h_d.ptr)
            st.sync()
            assert s_d.body().tobytes() == host["scores"].tobytes(), (Q, "device scores")
            assert p_d.body().tobytes() == np.ascontiguousarray(host["per_shard"]).tobytes(), (Q, "device per shard")
            assert h_d.body().tobytes() == host["heads"].tobytes(), (Q, "device heads")
            info = st.score_info()
            assert info["q"] == Q and info["positions"] == total, info
