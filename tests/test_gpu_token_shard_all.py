"""Per-document counts and AND groups over a shard set on the device against the CPU models of token_shard_all_cases.py: one shard
byte for byte against the shard's own handle; two, three and 64 shards; counts for ids at the shards' first and last documents, at
and beyond the end of the set, rows shortened through the `written` of two kinds of heads; the driver plants and the edge plants;
budgets at the sums of the driver's counts in front of every shard, caps at the sums of the shards' matches, on all-equal shards
whose per-shard counts sit on the edges of the walk; a guard pattern beyond `written` and in both lists when cap == 0; the device
chain against the host forms; chunks; the merge step alone beyond 2^32; stale, re-adopted and freed rank arrays; the Python class."""
import numpy as np
import pytest

import token_cases as tc
import token_doc_cases as td
import token_shard_all_cases as sa
import token_shard_doc_cases as sd

pytestmark = pytest.mark.gpu

FILL, FILL64, FILL32 = sa.FILL, sa.FILL64, sa.FILL32


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _build(gpu, cases):
    st = gpu.TokenShards.build([c["t"] for c in cases])
    st.set_documents([c["starts"] for c in cases])
    st.prepare_doc_ranks()
    return st


def _span_dev(spans):
    """[S][P] (first, count) -> the device array sa_hip_token_span[S * P]"""
    a = np.zeros((len(spans), len(spans[0]), 4), np.uint32)
    for s, row in enumerate(spans):
        a[s, :, 0], a[s, :, 1] = [f for f, _ in row], [c for _, c in row]
    return _dev(a.view(np.int32))


def _flat_spans(groups):
    """groups as gspans[s][j] -> (spans [S][P], uint64 group offsets)"""
    S = len(groups[0])
    spans, goff = [[] for _ in range(S)], [0]
    for gs in groups:
        for s in range(S):
            spans[s] += list(gs[s])
        goff.append(len(spans[0]))
    return spans, np.array(goff, np.uint64)


def _all_dev(gpu, st, sp_d, P, goff, cap, budget, lists=True):
    """-> (docs uint64, offsets int32, heads) of a device all call; the lists are given even when cap == 0 unless lists is False"""
    import torch
    g = len(goff) - 1
    d_d = torch.full((g, max(cap, 1)), FILL, dtype=torch.int64, device="cuda:0")
    o_d = torch.full((g, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
    h_d = torch.full((g, 5), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st.all_batch_device(sp_d.data_ptr(), P, goff, cap, budget, d_d.data_ptr() if lists else None, o_d.data_ptr() if lists else None,
                        h_d.data_ptr())
    st.sync()
    return d_d.cpu().numpy().view(np.uint64), o_d.cpu().numpy(), h_d.cpu().numpy().view(gpu.SHARDS_ALL_DTYPE).reshape(g)


def _heads(h):
    return [tuple(int(h[k][i]) for k in ("written", "driver", "examined", "matched", "candidates", "count")) for i in range(len(h))]


def _same_rows(got, want, cap, heads, where):
    """the lists cell by cell, the guard pattern beyond `written` included; with cap == 0 nothing was touched"""
    gd, go = got
    wd, wo = want
    if cap == 0:
        assert (gd == FILL64).all() and (go == FILL).all(), where
        return
    bad = np.flatnonzero((gd != wd).any(axis=1) | (go != wo).any(axis=1))
    assert bad.size == 0, (where, [(int(i), heads[i], gd[i, :4].tolist(), wd[i, :4].tolist(), go[i, :4].tolist(), wo[i, :4].tolist()) for i in bad[:4]])


def _check_all(gpu, st, cases, groups, sp_d, P, goff, cap, budget, where, full=None):
    full = full if full is not None else sa.all_full(cases, groups, budget)
    docs, offs, heads = sa.all_rows(full, cap)
    gd, go, gh = _all_dev(gpu, st, sp_d, P, goff, cap, budget)
    got = _heads(gh)
    bad = [i for i in range(len(groups)) if got[i] != heads[i]]
    assert not bad, (where, [(i, groups[i], got[i], heads[i]) for i in bad[:4]])
    _same_rows((gd, go), (docs, offs), cap, heads, where)


# ---- the all-equal shards: budget and cap edges, candidates at the lanes and trips of the walk ---------------------------------

@pytest.fixture(scope="module")
def planted(gpu):
    built = {}

    def get(Ld):
        if Ld not in built:
            built[Ld] = _build(gpu, sd.equal_set(Ld))
        return built[Ld]
    yield get
    for st in built.values():
        st.close()


def _equal(Ld):
    cases = sa.ranked(sd.equal_set(Ld))
    spans = sd.equal_contexts()
    groups = [sa.group_spans(spans, m) for m in sa.equal_groups()]
    flat, goff = _flat_spans(groups)
    return cases, groups, flat, goff


@pytest.mark.parametrize("Ld", td.LDS)
def test_budget_edges(gpu, planted, Ld):
    """budgets at the sum of the driver's counts in front of every shard - 1, at it and one above, inside a span, at 0, at C and
    beyond, for per-shard counts at the window and step edges of the walk; counts only (guards in both lists) and a list"""
    cases, groups, flat, goff = _equal(Ld)
    st = planted(Ld)
    sp_d, P = _span_dev(flat), len(flat[0])
    budgets = set()
    for gs in groups:
        budgets |= set(sd.budget_edges(sa.plan_set(cases, gs, 0)[2]))
    assert len(budgets) > 40
    for budget in sorted(budgets):
        full = sa.all_full(cases, groups, budget)
        for cap in (0, 16):
            _check_all(gpu, st, cases, groups, sp_d, P, goff, cap, budget, (Ld, cap, budget), full)
    info = st.doc_ranks_info()
    assert info["present"] == 1 and info["bytes"] == 4 * sum(sd.EQ_N) and info["prepare_ms"] > 0, info
    assert info["plan_q"] == info["merge_q"] == len(groups) and info["pairs_q"] == 3 * len(groups) and info["chunk"] == len(groups), info
    assert info["plan_ms"] > 0 and info["pairs_ms"] > 0 and info["merge_ms"] > 0, info
    assert info["streamed"] == sum(h[2] for h, _, _ in full), info                                    # the last call's examined ranks


@pytest.mark.parametrize("Ld", td.LDS)
def test_cap_edges(gpu, planted, Ld):
    """caps 0, 1, 16, 64 and at the sum of the shards' matches - 1, at it and one above: a shard alone beyond the cap, the cap
    reached exactly at the last shard; without a budget and with one that ends inside a shard"""
    cases, groups, flat, goff = _equal(Ld)
    st = planted(Ld)
    sp_d, P = _span_dev(flat), len(flat[0])
    for budget in (0, 300):
        full = sa.all_full(cases, groups, budget)
        caps = set()
        for gs in groups:
            caps |= set(sd.cap_edges([m for _, m, _ in sa.all_set(cases, gs, sa.MOST, budget)[2]]))
        assert set(td.CAPS) < caps
        for cap in sorted(caps):
            _check_all(gpu, st, cases, groups, sp_d, P, goff, cap, budget, (Ld, cap, budget), full)
    gd, go, gh = _all_dev(gpu, st, sp_d, P, goff, 0, 0, lists=False)                                   # counts only: NULL lists are fine
    assert _heads(gh) == sa.all_rows(sa.all_full(cases, groups, 0), 0)[2]


# ---- the plants ----------------------------------------------------------------------------------------------------------------

def test_driver_plants(gpu):
    """(a) a driver that is not shard 0's rarest span, (b) a tie on C, (c) a shard without the driver, (d) a shard with candidates
    and no match: the host form against the hand-counted table and both models"""
    cases = sa.driver_set()
    flat = [p for g in sa.DRIVER_GROUPS for p in g]
    goff = np.cumsum([0] + [len(g) for g in sa.DRIVER_GROUPS]).astype(np.uint64)
    spans = sd.spans_of(cases, flat)
    groups = [sa.group_spans(spans, range(int(a), int(b))) for a, b in zip(goff[:-1], goff[1:])]
    with _build(gpu, cases) as st:
        for budget in (0, 1, 10, 11, 12, 14, 15):
            full = sa.all_full(cases, groups, budget)
            for cap in (0, 1, 4, 16):
                got = st.all_batch(flat, goff, cap=cap, budget=budget, fill=FILL)
                docs, offs, heads = sa.all_rows(full, cap)
                assert _heads(got["heads"]) == heads, (cap, budget)
                assert got["docs"].shape == (len(groups), cap) and np.array_equal(got["docs"], docs) and np.array_equal(got["offsets"], offs), (cap, budget)
        got = st.all_batch(flat, goff, cap=16)
        for h, want in zip(_heads(got["heads"]), sa.DRIVER_WANT):
            assert (h[1], h[5], h[3], h[4]) == want and h[2] == h[5], (h, want)
        assert sorted(got["docs"][0, :5].tolist()) == [0, 1, 10, 16, 18] and got["docs"][0, 2] == 10
        for g, row, h in zip(sa.DRIVER_GROUPS, got["docs"], got["heads"]):
            assert sorted(row[:int(h["written"])].tolist()) == sa.all_b_set(cases, g)[0], g
        ids = sa.count_ids(cases)
        pats = [sa.X, sa.Y, sa.Z, sa.W, [5, 5], [1], []]
        rows = np.broadcast_to(np.array(ids, np.uint64), (len(pats), len(ids)))
        cnt = st.doc_counts_batch(pats, rows)["counts"]
        assert np.array_equal(cnt, sa.counts_rows(cases, sd.spans_of(cases, pats), rows))
        for p, row in zip(pats, cnt):
            tf = sa.all_b_set(cases, [p])[1][0]
            assert row.tolist() == [tf.get(i, 0) for i in ids], p


def test_edge_plants(gpu):
    """(e) the driver's only co-occurrence in a document at the other span's rank a - 1, a, end - 1 and end, (f) the last document of
    a shard with every rank below the other span's a: synthetic spans through the device form"""
    cases, groups, want, last_at = sa.edge_set()
    flat, goff = _flat_spans(groups)
    with _build(gpu, cases) as st:
        sp_d, P = _span_dev(flat), len(flat[0])
        for cap, budget in ((8, 0), (0, 0), (2, 3), (1, 0)):
            _check_all(gpu, st, cases, groups, sp_d, P, goff, cap, budget, ("edge", cap, budget))
        gd, go, gh = _all_dev(gpu, st, sp_d, P, goff, 8, 0)
        for i, (doc, hit) in enumerate(want):
            assert (doc in gd[i, :int(gh["written"][i])].tolist()) == hit, (i, groups[i])


# ---- set sizes -----------------------------------------------------------------------------------------------------------------

def test_one_shard_equals_the_single_index(gpu):
    """S = 1: every answer is the shard's own, byte for byte, with the document ids widened"""
    t = tc.texts()["rand_k4"][:3000]
    starts = td.rand_table(t.size, 200, 9)
    case = sd.shard_case(t, starts)
    pats = sa.frequent_patterns([case]) + sd.random_patterns([case])[:30]
    groups = sa.random_groups(len(pats))
    flat_i, goff = sa.flat_groups(groups)
    flat = [pats[i] for i in flat_i]
    ids = np.array([-1, 0, 1, 57, 198, 199, 200, 201, 2 ** 31 - 1], np.int64)
    with gpu.TokenShards.build([t]) as st:
        st.set_documents([starts])
        st.prepare_doc_ranks()
        own = st.shard(0)
        assert own.doc_ranks_info()["present"] == 1
        for mode, max_length in ((0, 0), (1, 0), (1, 2)):
            for cap, budget in ((0, 0), (1, 0), (5, 3), (64, 0), (64, 1000), (16, 1)):
                got = st.all_batch(flat, goff, cap=cap, budget=budget, mode=mode, max_length=max_length, fill=FILL)
                want = own.all_batch(flat, goff, cap=cap, budget=budget, mode=mode, max_length=max_length, fill=FILL)
                where = (mode, max_length, cap, budget)
                assert got["spans"][0].tobytes() == want["spans"].tobytes(), where
                assert got["docs"].dtype == np.uint64 and got["docs"].tobytes() == want["docs"].astype(np.int64).view(np.uint64).tobytes(), where
                assert got["offsets"].tobytes() == want["offsets"].tobytes(), where
                for k in ("written", "driver", "examined", "matched", "candidates", "count"):
                    assert np.array_equal(got["heads"][k], want["heads"][k]), (where, k)
            rows = np.broadcast_to(ids, (len(pats), ids.size))
            wr = (np.arange(len(pats)) % (ids.size + 1)).astype(np.uint32)
            for written in (None, wr):
                got = st.doc_counts_batch(pats, rows.astype(np.int64).view(np.uint64), written=written,
                                          mode=mode, max_length=max_length, fill=FILL)
                want = own.doc_counts_batch(pats, rows.astype(np.int32), written=written, mode=mode, max_length=max_length, fill=FILL)
                assert got["counts"].tobytes() == want["counts"].tobytes() and got["spans"][0].tobytes() == want["spans"].tobytes(), mode
        assert int(st.all_batch(flat, goff, cap=0)["heads"]["matched"].max()) > 10


def _check_host(gpu, st, cases, pats, groups, where, caps=(0, 1, 16), budgets=(0, 1, 7, 300)):
    """the host forms in exact mode against model A, and against model B where the walk saw everything"""
    flat_i, goff = sa.flat_groups(groups)
    flat = [pats[i] for i in flat_i]
    spans = sd.spans_of(cases, flat)
    gsp = [sa.group_spans(spans, range(int(a), int(b))) for a, b in zip(goff[:-1], goff[1:])]
    b_side = [sa.all_b_set(cases, [pats[i] for i in g]) for g in groups]
    for budget in budgets:
        full = sa.all_full(cases, gsp, budget)
        for cap in caps:
            got = st.all_batch(flat, goff, cap=cap, budget=budget, fill=FILL)
            docs, offs, heads = sa.all_rows(full, cap)
            assert [(int(f), int(c)) for f, c in zip(got["spans"]["first"].ravel(), got["spans"]["count"].ravel())] == [x for row in spans for x in row], where
            assert _heads(got["heads"]) == heads, (where, cap, budget)
            assert got["docs"].shape == (len(groups), cap) and np.array_equal(got["docs"], docs) and np.array_equal(got["offsets"], offs), (where, cap, budget)
            for h, (both, tfs) in zip(heads, b_side):
                assert h[2] != h[5] or h[3] == len(both), (where, cap, budget)
    ids = sa.count_ids(cases)
    rows = np.broadcast_to(np.array(ids, np.uint64), (len(pats), len(ids)))
    cnt = st.doc_counts_batch(pats, rows, fill=FILL)["counts"]
    assert np.array_equal(cnt, sa.counts_rows(cases, sd.spans_of(cases, pats), rows)), where
    for p, row in zip(pats[:12], cnt):
        tf = sa.all_b_set(cases, [p])[1][0]
        assert row.tolist() == [tf.get(i, 0) for i in ids], (where, p)


@pytest.fixture(scope="module")
def randoms(gpu):
    built = {name: _build(gpu, sa.ranked(sd.random_set(name))) for name in sd.RANDOM}
    yield built
    for st in built.values():
        st.close()


@pytest.mark.parametrize("name", sorted(sd.RANDOM))
def test_random_sets_against_both_models(gpu, randoms, name):
    """S = 2 and S = 3, empty documents at the end of a shard; exact mode against both models, longest-suffix mode against the models
    on the suffix the set found"""
    cases, st = sa.ranked(sd.random_set(name)), randoms[name]
    pats = sa.frequent_patterns(cases) + sd.random_patterns(cases)[:20]
    groups = sa.random_groups(len(pats))
    _check_host(gpu, st, cases, pats, groups, name)
    ctx = sd.random_contexts(cases)
    cgroups = sa.random_groups(len(ctx), seed=9)
    flat_i, goff = sa.flat_groups(cgroups)
    flat = [ctx[i] for i in flat_i]
    for max_length in (0, 2):
        got = st.all_batch(flat, goff, cap=16, budget=0, mode=1, max_length=max_length, fill=FILL)
        L = got["spans"]["length"].max(axis=0).tolist()
        tails = [c[len(c) - l:] for c, l in zip(flat, L)]
        spans = sd.spans_of(cases, tails)
        gsp = [sa.group_spans(spans, range(int(a), int(b))) for a, b in zip(goff[:-1], goff[1:])]
        docs, offs, heads = sa.all_rows(sa.all_full(cases, gsp, 0), 16)
        assert _heads(got["heads"]) == heads and np.array_equal(got["docs"], docs) and np.array_equal(got["offsets"], offs), (name, max_length)
        for h, a, b in zip(heads, goff[:-1], goff[1:]):
            assert h[3] == len(sa.all_b_set(cases, tails[int(a):int(b)])[0]), (name, max_length)
        ids = sa.count_ids(cases)
        rows = np.broadcast_to(np.array(ids, np.uint64), (len(ctx), len(ids)))
        cnt = st.doc_counts_batch(ctx, rows, mode=1, max_length=max_length)
        Lc = cnt["spans"]["length"].max(axis=0).tolist()
        ctails = [c[len(c) - l:] for c, l in zip(ctx, Lc)]
        assert np.array_equal(cnt["counts"], sa.counts_rows(cases, sd.spans_of(cases, ctails), rows)), (name, max_length)


def test_sixty_four_shards_every_lane_live(gpu):
    """one document of about 40 tokens per shard; a group whose driver occurs in shards 0, 31 and 63 only"""
    rng = np.random.default_rng(64)
    texts = []
    for s in range(64):
        t = rng.integers(1, 4, 36).tolist()
        t[5:7] = sa.Y                                                                                 # every shard holds Y ...
        if s in (0, 31, 63):
            t[20:22] = sa.X                                                                           # ... three hold X
        if s % 2:
            t[28:30] = sa.Z
        texts.append(t + [100 + s])
    cases = sa.ranked([sd.shard_case(t, [0]) for t in texts])
    pats = [sa.X, sa.Y, sa.Z, [1], [163], []]
    groups = [[0, 1], [1, 0], [1, 2], [2, 1, 0], [1], [0, 4], [3, 1, 5], [5, 5]]
    with _build(gpu, cases) as st:
        assert st.doc_bases().tolist() == list(range(65))
        _check_host(gpu, st, cases, pats, groups, "64", caps=(0, 1, 31, 32, 33, 64), budgets=(0, 1, 2, 3, 32, 64, 100))
        got = st.all_batch([sa.X, sa.Y, sa.Y, sa.X, sa.Y, sa.Z], [0, 2, 4, 6], cap=64)
        assert got["docs"][0, :3].tolist() == got["docs"][1, :3].tolist() == [0, 31, 63]
        assert got["heads"]["driver"].tolist() == [0, 1, 1] and got["heads"]["count"].tolist() == [3, 3, 32]
        assert got["docs"][2, :32].tolist() == list(range(1, 64, 2)) and got["heads"]["matched"].tolist() == [3, 3, 32]
        flat_i, goff = sa.flat_groups(groups)
        spans = sd.spans_of(cases, [pats[i] for i in flat_i])
        gsp = [sa.group_spans(spans, range(int(a), int(b))) for a, b in zip(goff[:-1], goff[1:])]
        sp_d = _span_dev(spans)
        for budget in sd.budget_edges(sa.plan_set(cases, gsp[4], 0)[2]):                              # at the front of every one of 64 shards
            _check_all(gpu, st, cases, gsp, sp_d, len(flat_i), goff, 16, budget, ("64", budget))


# ---- counts: short rows ----------------------------------------------------------------------------------------------------------

def test_short_rows_through_the_written_of_heads(gpu, randoms):
    """rows shortened through the `written` of a sa_hip_token_shards_docs[Q] (stride 32), of a sa_hip_token_shards_all[G] (stride 40)
    and of a plain uint32 array (stride 4): a guard pattern in every cell beyond, ids the listing itself wrote"""
    import torch
    name = "r3"
    cases, st = sa.ranked(sd.random_set(name)), randoms[name]
    pats = sa.frequent_patterns(cases)
    q, cap = len(pats), 8
    spans = sd.spans_of(cases, pats)
    sp_d = _span_dev(spans)
    d_d = torch.full((q, cap), FILL, dtype=torch.int64, device="cuda:0")
    o_d = torch.full((q, cap), FILL, dtype=torch.int32, device="cuda:0")
    h_d = torch.zeros((q, 4), dtype=torch.int64, device="cuda:0")
    c_d = torch.full((q, cap), FILL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st.docs_batch_device(sp_d.data_ptr(), q, cap, 0, d_d.data_ptr(), o_d.data_ptr(), h_d.data_ptr())
    st.doc_counts_batch_device(sp_d.data_ptr(), q, cap, d_d.data_ptr(), h_d.data_ptr(), 32, c_d.data_ptr())
    st.sync()
    docs, written = d_d.cpu().numpy().view(np.uint64), h_d.cpu().numpy().view(gpu.SHARDS_DOCS_DTYPE).reshape(q)["written"]
    assert written.min() < cap and written.max() == cap and len(set(written.tolist())) > 3
    want = sa.counts_rows(cases, spans, docs, written)
    assert np.array_equal(c_d.cpu().numpy().view(np.uint32), want) and (want == FILL32).any() and (want[want != FILL32] > 0).all()
    info = st.doc_ranks_info()
    assert info["counts_q"] == q and info["counts_ms"] > 0, info
    # the heads of an all call: group i = {pattern i, pattern i + 1}, counted for pattern i
    goff = np.arange(0, q + 1, 2, dtype=np.uint64)
    g = len(goff) - 1
    flat = [[row[i] for i in range(2 * g)] for row in spans]
    ad, ao, ah = (torch.full((g, cap), FILL, dtype=torch.int64, device="cuda:0"), torch.full((g, cap), FILL, dtype=torch.int32, device="cuda:0"),
                  torch.zeros((g, 5), dtype=torch.int64, device="cuda:0"))
    first = _span_dev([[row[2 * i] for i in range(g)] for row in spans])
    c2 = torch.full((g, cap), FILL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st.all_batch_device(_span_dev(flat).data_ptr(), 2 * g, goff, cap, 0, ad.data_ptr(), ao.data_ptr(), ah.data_ptr())
    st.doc_counts_batch_device(first.data_ptr(), g, cap, ad.data_ptr(), ah.data_ptr(), 40, c2.data_ptr())
    st.sync()
    wr = ah.cpu().numpy().view(gpu.SHARDS_ALL_DTYPE).reshape(g)["written"]
    assert 0 < wr.max() <= cap and wr.min() < cap
    want = sa.counts_rows(cases, [[row[2 * i] for i in range(g)] for row in spans], ad.cpu().numpy().view(np.uint64), wr)
    assert np.array_equal(c2.cpu().numpy().view(np.uint32), want) and (want[want != FILL32] > 0).all()
    # a plain array of lengths
    lens = (np.arange(q) % (cap + 2)).astype(np.uint32)
    ids = np.broadcast_to(np.array(sa.count_ids(cases)[:cap], np.uint64), (q, cap))
    c3 = torch.full((q, cap), FILL, dtype=torch.int32, device="cuda:0")
    l_d, i_d = _dev(lens.view(np.int32)), _dev(ids.view(np.int64))
    torch.cuda.synchronize()
    st.doc_counts_batch_device(sp_d.data_ptr(), q, cap, i_d.data_ptr(), l_d.data_ptr(), 4, c3.data_ptr())
    st.sync()
    assert np.array_equal(c3.cpu().numpy().view(np.uint32), sa.counts_rows(cases, spans, ids, lens))
    assert np.array_equal(st.doc_counts_batch(pats, ids, written=lens, fill=FILL)["counts"], sa.counts_rows(cases, spans, ids, lens))


# ---- the device chain, chunks --------------------------------------------------------------------------------------------------

def _chain(gpu, st, S, flat, goff, mode, cap, budget):
    """spans -> all -> doc_counts on the device, no host trip in between: the counts of every group's first pattern in the
    documents the group's listing wrote"""
    import torch
    P, g = len(flat), len(goff) - 1
    buf, off = tc.pack(flat)
    pd, od = _dev(buf if buf.size else np.zeros(1, np.int32)), _dev(off.view(np.int64))
    sp_d = torch.zeros((S, P, 4), dtype=torch.int32, device="cuda:0")
    ln_d = torch.zeros(P, dtype=torch.int32, device="cuda:0")
    tt_d = torch.zeros(P, dtype=torch.int64, device="cuda:0")
    d_d = torch.full((g, max(cap, 1)), FILL, dtype=torch.int64, device="cuda:0")
    o_d = torch.full((g, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
    h_d = torch.full((g, 5), -1, dtype=torch.int64, device="cuda:0")
    c_d = torch.full((g, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st.spans_batch_device(pd.data_ptr(), od.data_ptr(), P, mode, 0, 0, ln_d.data_ptr(), tt_d.data_ptr(), sp_d.data_ptr())
    st.all_batch_device(sp_d.data_ptr(), P, goff, cap, budget, d_d.data_ptr(), o_d.data_ptr(), h_d.data_ptr())
    st.sync()
    fs_d = sp_d[:, torch.from_numpy(goff[:-1].astype(np.int64)).to("cuda:0"), :].contiguous()        # the spans of every group's first pattern
    if cap:
        torch.cuda.synchronize()
        st.doc_counts_batch_device(fs_d.data_ptr(), g, cap, d_d.data_ptr(), h_d.data_ptr(), 40, c_d.data_ptr())
        st.sync()
    return sp_d.cpu().numpy(), d_d.cpu().numpy(), o_d.cpu().numpy(), h_d.cpu().numpy(), c_d.cpu().numpy()


def _chain_case(cases):
    ctx = sd.random_contexts(cases) + sa.frequent_patterns(cases)[:16]
    groups = sa.random_groups(len(ctx), seed=3)[:40]
    flat_i, goff = sa.flat_groups(groups)
    return [ctx[i] for i in flat_i], goff


def test_device_chain_against_the_host_forms(gpu, randoms):
    name = "r3"
    cases, st = sd.random_set(name), randoms[name]
    flat, goff = _chain_case(cases)
    g = len(goff) - 1
    for mode, cap, budget in ((0, 16, 0), (1, 16, 0), (1, 3, 5), (0, 1, 0)):
        want = st.all_batch(flat, goff, cap=cap, budget=budget, mode=mode, fill=FILL)
        sp, d, o, h, c = _chain(gpu, st, 3, flat, goff, mode, cap, budget)
        assert sp.tobytes() == want["spans"].tobytes(), (mode, cap, budget)
        assert d.tobytes() == want["docs"].tobytes() and o.tobytes() == want["offsets"].tobytes() and h.tobytes() == want["heads"].tobytes(), (mode, cap, budget)
        firsts = [flat[int(a)] for a in goff[:-1]]
        wc = st.doc_counts_batch(firsts, want["docs"], written=want["heads"]["written"], mode=mode, fill=FILL)["counts"]
        assert c.view(np.uint32).tobytes() == wc.tobytes(), (mode, cap, budget)
    assert st.all_batch([], [0], cap=4)["docs"].shape == (0, 4)
    st.all_batch_device(None, 0, [0], 4, 0, None, None, None)                                         # G == 0 and Q == 0: no-ops
    st.doc_counts_batch_device(None, 0, 4, None, None, 4, None)


@pytest.mark.parametrize("chunk", ["1", "3"])
def test_chunks(gpu, randoms, monkeypatch, chunk):
    """G = 7 in chunks of 1 and of 3 groups (the last chunk holds one): the host and the device form against the unchunked set"""
    name = "r3"
    cases = sd.random_set(name)
    pats = sa.frequent_patterns(cases)
    groups = [[0, 1], [2, 3, 4], [5], [6, 7], [8, 9], [10, 11, 12, 13], [14, 15]]
    flat_i, goff = sa.flat_groups(groups)
    flat = [pats[i] for i in flat_i]
    monkeypatch.setenv("SA_HIP_TOKEN_SHARD_CHUNK", chunk)
    with _build(gpu, cases) as st:
        for cap, budget in ((5, 0), (0, 0), (2, 40)):
            want = randoms[name].all_batch(flat, goff, cap=cap, budget=budget, fill=FILL)
            got = st.all_batch(flat, goff, cap=cap, budget=budget, fill=FILL)
            assert all(got[k].tobytes() == want[k].tobytes() for k in want), (chunk, cap, budget)
            info = st.doc_ranks_info()
            assert info["chunk"] == int(chunk) and info["plan_q"] == 7 and info["pairs_q"] == 21, info
            assert info["streamed"] == int(want["heads"]["examined"].sum()), info
            if cap:
                sp, d, o, h, c = _chain(gpu, st, 3, flat, goff, 0, cap, budget)
                assert d.tobytes() == want["docs"].tobytes() and o.tobytes() == want["offsets"].tobytes() and h.tobytes() == want["heads"].tobytes(), (chunk, cap)
        assert randoms[name].doc_ranks_info()["chunk"] == 7
        assert int(want["heads"]["matched"].sum()) > 0


def test_info_follows_the_last_all_call(gpu, randoms, monkeypatch):
    """the per-chunk stopwatch: zeros before the first call, the figures of a call in 7 chunks, then of a call in one chunk on the
    same set; asking twice changes nothing"""
    name = "r3"
    cases = sd.random_set(name)
    pats = sa.frequent_patterns(cases)
    groups = [[0, 1], [2, 3, 4], [5], [6, 7], [8, 9], [10, 11, 12, 13], [14, 15]]
    stages = ("plan_ms", "pairs_ms", "merge_ms")
    monkeypatch.setenv("SA_HIP_TOKEN_SHARD_CHUNK", "1")
    with _build(gpu, cases) as st:
        none = st.doc_ranks_info()
        assert all(none[k] == 0 for k in stages + ("chunk", "plan_q", "pairs_q", "merge_q", "streamed")), none
        for cap in (1, 3):
            for some in (groups, groups[:1]):                                                         # 7 chunks, then 1
                flat_i, goff = sa.flat_groups(some)
                flat = [pats[i] for i in flat_i]
                want = randoms[name].all_batch(flat, goff, cap=cap, fill=FILL)
                got = st.all_batch(flat, goff, cap=cap, fill=FILL)
                assert all(got[k].tobytes() == want[k].tobytes() for k in want), (cap, len(some))
                info = st.doc_ranks_info()
                assert info["chunk"] == 1 and info["plan_q"] == info["merge_q"] == len(some) and info["pairs_q"] == 3 * len(some), info
                assert info["streamed"] == int(want["heads"]["examined"].sum()), info
                assert all(np.isfinite(info[k]) and info[k] > 0 for k in stages), info
                assert st.doc_ranks_info() == info


# ---- the merge step alone ------------------------------------------------------------------------------------------------------

def _merge(gpu, st, S, lists, plan, bases, cap):
    """lists[s][i] = (docs, offsets, written, examined, matched, candidates), plan[i] = (driver, count) -> the merged rows of the
    device, guard pattern kept"""
    import torch
    g = len(lists[0])
    docs = np.full((S, g, max(cap, 1)), 12345, np.int32)
    offs = np.full((S, g, max(cap, 1)), 54321, np.int32)
    heads = np.zeros((S, g), gpu.SHARDS_ALL_PAIR_DTYPE)
    for s in range(S):
        for i, (d, o, w, ex, ma, ca) in enumerate(lists[s]):
            docs[s, i, :min(len(d), cap)], offs[s, i, :min(len(o), cap)] = d[:cap], o[:cap]
            heads[s, i] = (w, ex, ma, ca)
    pl = np.zeros(g, gpu.SHARDS_ALL_PLAN_DTYPE)
    for i, (drv, count) in enumerate(plan):
        pl[i] = (drv, 0, count)
    dd, od, hd = _dev(docs), _dev(offs), _dev(heads.view(np.uint32).view(np.int32).reshape(S, g, 4))
    pd = _dev(pl.view(np.int64).reshape(g, 2))
    bd = None if bases is None else _dev(np.array(bases, np.uint64).view(np.int64))
    o_d = torch.full((g, max(cap, 1)), FILL, dtype=torch.int64, device="cuda:0")
    o_o = torch.full((g, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0")
    o_h = torch.full((g, 5), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st.all_merge_device(dd.data_ptr(), od.data_ptr(), hd.data_ptr(), pd.data_ptr(), g, cap, o_d.data_ptr(), o_o.data_ptr(), o_h.data_ptr(),
                        bases_dev_ptr=None if bd is None else bd.data_ptr())
    st.sync()
    return o_d.cpu().numpy().view(np.uint64), o_o.cpu().numpy(), o_h.cpu().numpy().view(gpu.SHARDS_ALL_DTYPE).reshape(g)


def _merge_model(S, lists, plan, bases, cap):
    out = []
    for i in range(len(lists[0])):
        ent, ex, ma, ca, at = {}, 0, 0, 0, 0
        for s in range(S):
            d, o, w, e, m, c = lists[s][i]
            for j in range(min(w, cap)):
                if at + j < cap:
                    ent[at + j] = (bases[s] + d[j], o[j])
            at, ex, ma, ca = at + m, ex + e, ma + m, ca + c
        out.append((ent, (min(ma, cap), plan[i][0], ex, ma, ca, plan[i][1])))
    return out


@pytest.mark.parametrize("S", [3, 64])
def test_merge_alone_beyond_32_bits(gpu, S):
    M, cap = 0xFFFFFFFF, 6
    bases = [s * (2 ** 32 + 5) for s in range(S + 1)]                                                 # ids beyond 2^32
    cases = [
        [([], [], 0, M, M, M)] * S,                                                                   # counts only sums: S * (2^32 - 1)
        [([7], [s], 1, 1, 1, 1) for s in range(S)],                                                   # one entry per shard: the first cap shards
        [([1, 2, 3, 4, 5, 6], [9] * 6, 9, 9, 9, 9)] + [([8], [8], 1, 1, 1, 1)] * (S - 1),               # written beyond cap: clamped; shard 0 alone fills it
        [([], [], 0, 0, 0, 0)] * (S - 1) + [([2 ** 31 - 1, 0], [5, 6], 2, 2, 2, 2)],                   # only the last shard
        [([4, 5], [1, 2], 2, 5, 2, 7)] + [([], [], 0, 0, 0, 0)] * (S - 2) + [([6, 7, 8, 9, 1], [3, 4, 5, 6, 7], 5, 5, 5, 5)],   # cut inside the last list
        [([3], [3], 1, 2, M, M)] + [([4], [4], 1, 1, 1, 1)] * (S - 1),                                 # matched beyond written: the next shard starts past the cap
        [([1, 2], [1, 2], 1, 4, 1, 4) for s in range(S)],                                             # written below the list: its second entry is not read
    ]
    plan = [(0, S * M), (15, S), (3, 2 ** 36 + 1), (1, 2), (2, 12), (0, M + S), (7, 4 * S)]
    lists = [[cases[i][s] for i in range(len(cases))] for s in range(S)]
    texts = [[1, 2, 3 + s] for s in range(S)]
    with gpu.TokenShards.build(texts) as st:                                                          # (no documents, no rank arrays: the bases are the caller's)
        docs, offs, heads = _merge(gpu, st, S, lists, plan, bases, cap)
        for i, (ent, head) in enumerate(_merge_model(S, lists, plan, bases, cap)):
            assert _heads(heads[i:i + 1]) == [head], (i, heads[i], head)
            for j in range(cap):
                want = ent.get(j, (FILL64, FILL))
                assert (int(docs[i, j]), int(offs[i, j])) == want, (i, j, docs[i], offs[i], ent)
        assert int(heads[0]["matched"]) == int(heads[0]["candidates"]) == int(heads[0]["examined"]) == S * M > 2 ** 32
        assert int(heads[0]["written"]) == cap and (docs[0] == FILL64).all() and int(heads[2]["count"]) == 2 ** 36 + 1
        assert int(docs[3, 0]) == (S - 1) * (2 ** 32 + 5) + 2 ** 31 - 1 and int(docs[1, 2]) == 2 * (2 ** 32 + 5) + 7
        assert docs[5, 1:].tolist() == [FILL64] * (cap - 1)
        with pytest.raises(gpu.SaHipError) as err:                                                    # its own bases: it has none
            _merge(gpu, st, S, lists, plan, None, cap)
        assert err.value.code == -1 and "no documents" in str(err.value)
        st.set_documents([[0, 1]] * S)                                                                # two documents per shard: base[s] = 2 s
        docs, offs, heads = _merge(gpu, st, S, lists, plan, None, cap)
        assert docs[1, :min(S, cap)].tolist() == [2 * s + 7 for s in range(min(S, cap))] and int(heads[1]["matched"]) == S
        d0, _, h0 = _merge(gpu, st, S, lists, plan, bases, 0)                                          # cap == 0: heads alone
        assert (d0 == FILL64).all() and int(h0[0]["matched"]) == S * M and (h0["written"] == 0).all()


# ---- rank arrays that change behind the set ------------------------------------------------------------------------------------

def test_stale_rank_arrays_are_refused_until_prepared_again(gpu):
    import torch
    cases = sa.ranked(sd.random_set("r2"))
    pats = sa.frequent_patterns(cases)[:10]
    goff = np.arange(0, 11, 2, dtype=np.uint64)
    ids = np.zeros((len(pats), 2), np.uint64)
    with gpu.TokenShards.build([c["t"] for c in cases]) as st:
        h_d = torch.zeros((len(pats), 5), dtype=torch.int64, device="cuda:0")
        calls = (lambda: st.all_batch(pats, goff, cap=4), lambda: st.all_batch(pats, goff, cap=0), lambda: st.doc_counts_batch(pats, ids),
                 lambda: st.all_batch_device(h_d.data_ptr(), 10, goff, 0, 0, None, None, h_d.data_ptr()),
                 lambda: st.doc_counts_batch_device(h_d.data_ptr(), 1, 1, h_d.data_ptr(), None, 4, h_d.data_ptr()))

        def refused(what):
            for call in calls:
                with pytest.raises(gpu.SaHipError) as err:
                    call()
                assert err.value.code == -1 and what in str(err.value), str(err.value)

        refused("no documents")
        with pytest.raises(gpu.SaHipError) as err:                                                    # a set without documents
            st.prepare_doc_ranks()
        assert err.value.code == -1 and "no documents" in str(err.value)
        with pytest.raises(gpu.SaHipError):
            st.prepare_doc_ranks(False)
        st.set_documents([c["starts"] for c in cases])
        assert st.doc_ranks_info()["present"] == 0
        refused("sa_hip_token_shards_prepare_doc_ranks")
        st.shard(0).prepare_doc_ranks()                                                               # one shard alone is not the set's table
        refused("sa_hip_token_shards_prepare_doc_ranks")
        st.prepare_doc_ranks()
        info = st.doc_ranks_info()
        assert info["present"] == 1 and info["bytes"] == 4 * sum(len(c["t"]) for c in cases), info
        want = st.all_batch(pats, goff, cap=4, fill=FILL)
        wc = st.doc_counts_batch(pats, ids)["counts"]
        assert int(want["heads"]["matched"].sum()) > 0
        st.prepare_doc_ranks()                                                                        # again: a no-op per shard
        assert all(st.all_batch(pats, goff, cap=4, fill=FILL)[k].tobytes() == want[k].tobytes() for k in want)
        st.shard(1).prepare_doc_ranks(False)                                                          # behind the set's back
        refused("sa_hip_token_shards_prepare_doc_ranks")
        assert st.docs_batch(pats, cap=4)["heads"]["count"].sum() > 0                                 # the documents are as they were
        st.shard(1).prepare_doc_ranks()                                                               # rebuilt elsewhere: still not the set's table
        refused("rank arrays changed")
        st.prepare_doc_ranks()
        assert all(st.all_batch(pats, goff, cap=4, fill=FILL)[k].tobytes() == want[k].tobytes() for k in want)
        assert np.array_equal(st.doc_counts_batch(pats, ids)["counts"], wc)
        st.shard(0).set_documents(cases[0]["starts"])                                                 # drops the shard's array and moves both counts
        refused("adopt_documents")
        st.adopt_documents()
        refused("sa_hip_token_shards_prepare_doc_ranks")
        st.prepare_doc_ranks()
        assert all(st.all_batch(pats, goff, cap=4, fill=FILL)[k].tobytes() == want[k].tobytes() for k in want)
        st.prepare_doc_ranks(False)                                                                   # (set, 0): every call is refused
        assert st.doc_ranks_info()["present"] == 0 and st.doc_ranks_info()["bytes"] == 0
        assert st.shard(0).doc_ranks_info()["present"] == 0 and st.shard(1).doc_ranks_info()["present"] == 0
        refused("sa_hip_token_shards_prepare_doc_ranks")
        st.prepare_doc_ranks(False)
        st.prepare_doc_ranks()
        assert np.array_equal(st.doc_counts_batch(pats, ids)["counts"], wc)
        st.set_documents([c["starts"] for c in cases])                                                # the set's own call drops them too
        assert st.doc_ranks_info()["present"] == 0
        refused("sa_hip_token_shards_prepare_doc_ranks")


# ---- the Python class ----------------------------------------------------------------------------------------------------------

def test_python_class(gpu):
    from suffixarray_amd import ShardedTokenIndex, TokenIndex
    cases = sa.driver_set()
    with ShardedTokenIndex([c["t"] for c in cases], doc_starts=[c["starts"] for c in cases]) as sti:
        r = sti.documents_with_all([list(g) for g in sa.DRIVER_GROUPS], cap=16)
        for x, want, g in zip(r, sa.DRIVER_WANT, sa.DRIVER_GROUPS):
            assert x["documents"].dtype == np.uint64 and x["offsets"].dtype == np.int32 and type(x["matched"]) is int and x["exact"]
            assert (x["driver"], x["matched"]) == (want[0], want[2]) and sorted(x["documents"].tolist()) == sa.all_b_set(cases, g)[0], g
        assert r[0]["documents"].tolist()[2] == 10
        r = sti.documents_with_all([[sa.X, sa.Y]], cap=1, budget=11)
        assert r[0]["documents"].size == 1 and r[0]["matched"] == 3 and not r[0]["exact"]
        m, exact = sti.count_documents_with_all([list(g) for g in sa.DRIVER_GROUPS])
        assert m.dtype == np.uint64 and m.tolist() == [w[2] for w in sa.DRIVER_WANT] and exact.all()
        m, exact = sti.count_documents_with_all([[sa.X, sa.Y]], budget=10)
        assert m.tolist() == [2] and exact.tolist() == [False]
        assert sti.documents_with_all([]) == [] and sti.count_documents_with_all([])[0].size == 0
        tf = sti.term_counts([sa.X, sa.Y], [0, 1, 9, 10, 11, 18, 20, 2 ** 63])
        assert tf.dtype == np.uint32 and tf.tolist() == [[1, 1, 3, 2, 4, 1, 0, 0], [1, 2, 0, 1, 0, 2, 0, 0]]
        assert sti.term_counts([], [0]).shape == (0, 1) and sti.term_counts([sa.X], []).shape == (1, 0)
        for bad in ([-1], [2 ** 64], [0, -5]):
            with pytest.raises(ValueError):
                sti.term_counts([sa.X], bad)
        assert sti.documents_with_all([[[5, 9, 10]]], longest_suffix=True)[0]["matched"] == 9         # backs off to Y
        sti.set_documents([c["starts"] for c in cases])                                               # drops the arrays; the next call prepares
        assert sti._set.doc_ranks_info()["present"] == 0
        assert sti.count_documents_with_all([[sa.X, sa.Y]])[0].tolist() == [5] and sti._set.doc_ranks_info()["present"] == 1
        sti.set_documents(None)
        with pytest.raises(gpu.SaHipError):
            sti.term_counts([sa.X], [0])
    # one shard: the answers of TokenIndex on the same text and table
    c = sd.random_set("r2")[0]
    pats = sa.frequent_patterns([c])
    groups = [[pats[i] for i in g] for g in sa.random_groups(len(pats))]
    with ShardedTokenIndex([c["t"]], doc_starts=[c["starts"]]) as sti, TokenIndex(c["t"], doc_starts=c["starts"]) as ti:
        for kw in ({}, {"cap": 3, "budget": 5}, {"longest_suffix": True, "max_length": 2}):
            for a, b in zip(sti.documents_with_all(groups, **kw), ti.documents_with_all(groups, **kw)):
                assert all(np.array_equal(a[k], b[k]) for k in b), kw
        assert all(np.array_equal(x, y) for x, y in zip(sti.count_documents_with_all(groups, budget=9), ti.count_documents_with_all(groups, budget=9)))
        assert np.array_equal(sti.term_counts(pats, [0, 3, 41, 400]), ti.term_counts(pats, [0, 3, 41, 400]))
