"""Documents over a shard set on the device against the CPU models of token_shard_doc_cases.py: one shard byte for byte against
the shard's own handle; two, three and 64 shards; a shard that misses the n-gram and an empty shard in the middle; budgets at the
sums of the counts in front of every shard, caps at the sums of the distinct documents, locate caps at a shard's last hit, on
all-equal shards whose per-shard counts sit on the edges of the walk; a guard pattern beyond `written`; the device chain against the
host forms; chunks; the merge step alone beyond 2^32; stale, adopted and removed documents; the Python class."""
import numpy as np
import pytest

import token_cases as tc
import token_doc_cases as td
import token_shard_doc_cases as sd

pytestmark = pytest.mark.gpu

FILL, FILL64 = sd.FILL, sd.FILL64


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _build(gpu, cases):
    st = gpu.TokenShards.build([c["t"] for c in cases])
    st.set_documents([c["starts"] for c in cases])
    return st


def _span_dev(spans):
    """[S][Q] (first, count) -> the device array sa_hip_token_span[S * Q]"""
    a = np.zeros((len(spans), len(spans[0]), 4), np.uint32)
    for s, row in enumerate(spans):
        a[s, :, 0], a[s, :, 1] = [f for f, _ in row], [c for _, c in row]
    return _dev(a.view(np.int32))


def _out(q, cap):
    import torch
    return (torch.full((q, max(cap, 1)), FILL, dtype=torch.int64, device="cuda:0"),
            torch.full((q, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0"))


def _docs_dev(gpu, st, sp_d, q, cap, budget):
    """-> (docs uint64, offsets int32, heads) of a device documents call; the lists are given even when cap == 0"""
    import torch
    d_d, o_d = _out(q, cap)
    h_d = torch.full((q, 4), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st.docs_batch_device(sp_d.data_ptr(), q, cap, budget, d_d.data_ptr(), o_d.data_ptr(), h_d.data_ptr())
    st.sync()
    return d_d.cpu().numpy().view(np.uint64), o_d.cpu().numpy(), h_d.cpu().numpy().view(gpu.SHARDS_DOCS_DTYPE).reshape(q)


def _locate_dev(gpu, st, sp_d, q, cap):
    import torch
    d_d, o_d = _out(q, cap)
    h_d = torch.full((q, 2), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st.locate_batch_device(sp_d.data_ptr(), q, cap, d_d.data_ptr(), o_d.data_ptr(), h_d.data_ptr())
    st.sync()
    return d_d.cpu().numpy().view(np.uint64), o_d.cpu().numpy(), h_d.cpu().numpy().view(gpu.SHARDS_LOCATE_DTYPE).reshape(q)


def _docs_heads(h):
    assert (h["reserved"] == 0).all()
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(h["written"], h["examined"], h["distinct"], h["count"])]


def _locate_heads(h):
    assert (h["reserved"] == 0).all()
    return [(int(a), int(b)) for a, b in zip(h["written"], h["count"])]


def _same_rows(got, want, cap, heads, where):
    """the lists cell by cell, the guard pattern beyond `written` included; with cap == 0 nothing was touched"""
    gd, go = got
    wd, wo = want
    if cap == 0:
        assert (gd == FILL64).all() and (go == FILL).all(), where
        return
    bad = np.flatnonzero((gd != wd).any(axis=1) | (go != wo).any(axis=1))
    assert bad.size == 0, (where, [(int(i), heads[i], gd[i, :4].tolist(), wd[i, :4].tolist(), go[i, :4].tolist(), wo[i, :4].tolist()) for i in bad[:4]])


def _check_docs(gpu, st, cases, spans, sp_d, cap, budget, where, full=None):
    q = len(spans[0])
    full = full if full is not None else sd.docs_full(cases, spans, budget)
    docs, offs, heads = sd.docs_rows(full, cap)
    gd, go, gh = _docs_dev(gpu, st, sp_d, q, cap, budget)
    got = _docs_heads(gh)
    bad = [i for i in range(q) if got[i] != heads[i]]
    assert not bad, (where, [(i, sd.context(spans, i), got[i], heads[i]) for i in bad[:4]])
    _same_rows((gd, go), (docs, offs), cap, heads, where)


# ---- the planted sets: budget, cap and locate edges ----------------------------------------------------------------------------

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


@pytest.mark.parametrize("Ld", td.LDS)
def test_budget_edges(gpu, planted, Ld):
    """budgets at the sum of the counts in front of every shard - 1, at it and one above, inside every span, at 0, at C and beyond,
    for per-shard counts at the window and step edges of the walk; counts only and a list"""
    cases, st, spans = sd.equal_set(Ld), planted(Ld), sd.equal_contexts()
    for s, c in enumerate(cases):
        assert np.array_equal(st.shard(s).sa_range(0, len(c["t"])), c["sa"])
    assert st.doc_bases().tolist() == sd.bases(cases) and st.docs_info()["documents"] == sd.bases(cases)[-1]
    sp_d = _span_dev(spans)
    budgets = sd.all_budgets(spans)
    assert len(budgets) > 40
    for budget in budgets:
        full = sd.docs_full(cases, spans, budget)
        for cap in (0, 16):
            _check_docs(gpu, st, cases, spans, sp_d, cap, budget, (Ld, cap, budget), full)
    info = st.docs_info()
    assert info["pairs_q"] == 3 * len(spans[0]) and info["merge_q"] == len(spans[0]) and info["chunk"] == len(spans[0]), info
    assert info["pairs_ms"] > 0 and info["merge_ms"] > 0, info
    assert info["streamed"] == sum(h[1] for h, _, _ in full), info                                   # the last call's examined ranks


@pytest.mark.parametrize("Ld", td.LDS)
def test_cap_edges(gpu, planted, Ld):
    """caps 0, 1, 16, 64 and at the sum of the shards' distinct documents - 1, at it and one above: a shard alone beyond the cap,
    the cap reached exactly at the last shard; without a budget and with one that ends inside a shard"""
    cases, st, spans = sd.equal_set(Ld), planted(Ld), sd.equal_contexts()
    q = len(spans[0])
    sp_d = _span_dev(spans)
    for budget in (0, 300):
        full = sd.docs_full(cases, spans, budget)
        caps = set()
        for i in range(q):
            e = sd.split_budget(sd.counts_of(spans, i), budget)
            caps |= set(sd.cap_edges([sd.docs_set([cases[s]], [(spans[s][i][0], e[s])], sd.MOST, 0)[0][2] for s in range(3)]))
        assert set(td.CAPS) < caps                                                                    # the sums' edges beside them
        for cap in sorted(caps):
            _check_docs(gpu, st, cases, spans, sp_d, cap, budget, (Ld, cap, budget), full)


@pytest.mark.parametrize("Ld", (1, 64, 257))
def test_locate_edges(gpu, planted, Ld):
    """the cap on the last hit of every shard, one before it and one after it"""
    cases, st, spans = sd.equal_set(Ld), planted(Ld), sd.equal_contexts()
    q = len(spans[0])
    sp_d = _span_dev(spans)
    full = sd.locate_full(cases, spans)
    caps = set(td.CAPS) - {0}
    for i in range(q):
        run = 0
        for c in sd.counts_of(spans, i):
            run += c
            caps |= {x for x in (run - 1, run, run + 1) if x > 0}
    for cap in sorted(caps):
        docs, offs, heads = sd.locate_rows(full, cap)
        gd, go, gh = _locate_dev(gpu, st, sp_d, q, cap)
        assert _locate_heads(gh) == heads, (Ld, cap)
        _same_rows((gd, go), (docs, offs), cap, heads, (Ld, cap))
    info = st.docs_info()
    assert info["locate_q"] == q and info["locate_ms"] > 0, info


# ---- set sizes -----------------------------------------------------------------------------------------------------------------

def test_one_shard_equals_the_single_index(gpu):
    """S = 1: every answer is the shard's own, byte for byte, with the document ids widened"""
    t = tc.texts()["rand_k1000"][:3000]
    starts = td.rand_table(t.size, 200, 9)
    case = sd.shard_case(t, starts)
    pats = sd.random_patterns([case])
    with gpu.TokenShards.build([t]) as st:
        st.set_documents([starts])
        own = st.shard(0)
        assert st.doc_bases().tolist() == [0, 200]
        for mode, max_length in ((0, 0), (1, 0), (1, 2)):
            for cap, budget in ((0, 0), (1, 0), (5, 3), (64, 0), (64, 1000), (16, 1)):
                got = st.docs_batch(pats, cap=cap, budget=budget, mode=mode, max_length=max_length, fill=FILL)
                want = own.docs_batch(pats, cap=cap, budget=budget, mode=mode, max_length=max_length, fill=FILL)
                where = (mode, max_length, cap, budget)
                assert got["spans"][0].tobytes() == want["spans"].tobytes(), where
                assert got["docs"].dtype == np.uint64 and got["docs"].tobytes() == want["docs"].astype(np.int64).view(np.uint64).tobytes(), where
                assert got["offsets"].tobytes() == want["offsets"].tobytes(), where
                for k in ("written", "examined", "distinct", "count"):
                    assert np.array_equal(got["heads"][k], want["heads"][k]), (where, k)
                assert (got["heads"]["reserved"] == 0).all()
        for cap in (1, 5, 64):
            got, want = st.locate_batch(pats, cap=cap, fill=FILL), own.locate_batch(pats, cap=cap, fill=FILL)
            assert got["spans"][0].tobytes() == want["spans"].tobytes(), cap
            assert got["docs"].tobytes() == want["docs"].astype(np.int64).view(np.uint64).tobytes() and got["offsets"].tobytes() == want["offsets"].tobytes(), cap
            assert np.array_equal(got["heads"]["written"], want["heads"]["written"]) and np.array_equal(got["heads"]["count"], want["heads"]["count"]), cap
        assert int(got["heads"]["count"].max()) == t.size                                             # the empty pattern


def _check_host(gpu, st, cases, pats, where, caps=(0, 1, 16), budgets=(0, 1, 7, 300)):
    """the host forms in exact mode against model A (and B where the walk saw everything)"""
    spans = sd.spans_of(cases, pats)
    q = len(pats)
    b_side = [sd.model_b(cases, p) for p in pats]
    for budget in budgets:
        full = sd.docs_full(cases, spans, budget)
        for cap in caps:
            got = st.docs_batch(pats, cap=cap, budget=budget, fill=FILL)
            docs, offs, heads = sd.docs_rows(full, cap)
            assert [(int(f), int(c)) for f, c in zip(got["spans"]["first"].ravel(), got["spans"]["count"].ravel())] == [x for row in spans for x in row], where
            assert _docs_heads(got["heads"]) == heads, (where, cap, budget)
            assert got["docs"].shape == (q, cap) and np.array_equal(got["docs"], docs) and np.array_equal(got["offsets"], offs), (where, cap, budget)
            for h, (count, distinct, hits) in zip(heads, b_side):
                assert h[3] == count and (h[1] != count or h[2] == distinct), (where, cap, budget)
    lfull = sd.locate_full(cases, spans)
    for cap in (1, 16, 200):
        got = st.locate_batch(pats, cap=cap, fill=FILL)
        docs, offs, heads = sd.locate_rows(lfull, cap)
        assert _locate_heads(got["heads"]) == heads and np.array_equal(got["docs"], docs) and np.array_equal(got["offsets"], offs), (where, cap)
        for i, (count, _, hits) in enumerate(b_side):
            if count <= cap:
                assert sorted(zip(got["docs"][i, :count].tolist(), got["offsets"][i, :count].tolist())) == hits, (where, cap, i)


@pytest.fixture(scope="module")
def randoms(gpu):
    built = {name: _build(gpu, sd.random_set(name)) for name in sd.RANDOM}
    yield built
    for st in built.values():
        st.close()


@pytest.mark.parametrize("name", sorted(sd.RANDOM))
def test_random_sets_against_both_models(gpu, randoms, name):
    """S = 2 and S = 3, empty documents at the end of a shard, a middle shard that misses most n-grams; exact mode against both
    models, longest-suffix mode against the models on the suffix the set found"""
    cases, st = sd.random_set(name), randoms[name]
    S = len(cases)
    assert st.doc_bases().tolist() == sd.bases(cases)
    pats = sd.random_patterns(cases)
    _check_host(gpu, st, cases, pats, name)
    if S == 3:
        counts = np.array([[c for _, c in row] for row in sd.spans_of(cases, pats)])
        assert ((counts[0] > 0) & (counts[1] == 0) & (counts[2] > 0)).sum() >= 3                      # the middle shard misses
    ctx = sd.random_contexts(cases)
    backed = 0
    for max_length in (0, 2):
        got = st.docs_batch(ctx, cap=16, budget=0, mode=1, max_length=max_length, fill=FILL)
        L = got["spans"]["length"].max(axis=0).tolist()
        tails = [c[len(c) - l:] for c, l in zip(ctx, L)]
        for c, l, tail in zip(ctx, L, tails):                                                         # the longest suffix some shard holds
            limit = min(len(c), max_length or len(c))
            assert l <= limit and sd.model_b(cases, tail)[0] >= 1 and (l == limit or sd.model_b(cases, c[len(c) - l - 1:])[0] == 0), (name, c)
            backed += l < len(c)
        spans = sd.spans_of(cases, tails)
        docs, offs, heads = sd.docs_rows(sd.docs_full(cases, spans, 0), 16)
        assert _docs_heads(got["heads"]) == heads and np.array_equal(got["docs"], docs) and np.array_equal(got["offsets"], offs), (name, max_length)
        for h, tail in zip(heads, tails):
            count, distinct, _ = sd.model_b(cases, tail)
            assert (h[1], h[2], h[3]) == (count, distinct, count), (name, tail)
    assert backed > 10


def test_an_empty_shard_in_the_middle(gpu):
    t = tc.texts()["rand_k4"]
    cases = [sd.shard_case(t[:1500], td.rand_table(1500, 30, 3)), sd.shard_case(np.zeros(0, np.int32), [0, 0]),
             sd.shard_case(t[1500:2600], td.rand_table(1100, 11, 4))]
    assert sd.bases(cases) == [0, 30, 32, 43]                                                         # its two empty documents are counted
    with _build(gpu, cases) as st:
        assert st.doc_bases().tolist() == [0, 30, 32, 43] and st.shard(1).info()["n"] == 0
        pats = sd.random_patterns([cases[0], cases[2]])
        _check_host(gpu, st, cases, pats, "empty shard", caps=(0, 16), budgets=(0, 7))
        got = st.docs_batch(pats, cap=64)
        assert (got["spans"]["count"][1] == 0).all() and not ((got["docs"] >= 30) & (got["docs"] < 32)).any()


def test_sixty_four_shards_every_lane_live(gpu):
    """one document per shard: the bases are 0 .. 64 and an n-gram every shard holds has 64 documents"""
    texts = [[sd.A] * (s % 5 + 1) + [100 + s] + [sd.A] * (s % 3) for s in range(64)]
    cases = [sd.shard_case(t, [0]) for t in texts]
    pats = [[sd.A], [sd.A, sd.A], [sd.A, sd.A, sd.A], [100], [163], [sd.A, 131], [164], []]
    with _build(gpu, cases) as st:
        assert st.doc_bases().tolist() == list(range(65))
        spans = sd.spans_of(cases, pats)
        assert all(c > 0 for _, c in sd.context(spans, 0)) and len(sd.context(spans, 0)) == 64
        _check_host(gpu, st, cases, pats, "64", caps=(0, 1, 63, 64, 65), budgets=(0, 1, 2, 64, 100))
        got = st.docs_batch(pats, cap=64)
        assert got["docs"][0].tolist() == list(range(64)) and got["heads"]["distinct"][0] == 64
        assert got["docs"][4, 0] == 63 and got["heads"]["distinct"][3:7].tolist() == [1, 1, 1, 0]
        sp_d = _span_dev(spans)
        for budget in sd.budget_edges(sd.counts_of(spans, 0)):                                        # at the front of every one of 64 shards
            _check_docs(gpu, st, cases, spans, sp_d, 16, budget, ("64", budget))
        full = sd.docs_full(cases, spans, 0)
        for cap in sd.cap_edges([1] * 64)[::3] + [63, 64, 65]:
            _check_docs(gpu, st, cases, spans, sp_d, cap, 0, ("64", cap), full)


# ---- the device chain, chunks --------------------------------------------------------------------------------------------------

def _chain(gpu, st, S, ctx, mode, cap, budget):
    """spans -> docs and spans -> locate on the device, no host trip in between"""
    import torch
    q = len(ctx)
    buf, off = tc.pack(ctx)
    pd, od = _dev(buf if buf.size else np.zeros(1, np.int32)), _dev(off.view(np.int64))
    sp_d = torch.zeros((S, q, 4), dtype=torch.int32, device="cuda:0")
    ln_d = torch.zeros(q, dtype=torch.int32, device="cuda:0")
    tt_d = torch.zeros(q, dtype=torch.int64, device="cuda:0")
    d_d, o_d = _out(q, cap)
    h_d = torch.full((q, 4), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st.spans_batch_device(pd.data_ptr(), od.data_ptr(), q, mode, 0, 0, ln_d.data_ptr(), tt_d.data_ptr(), sp_d.data_ptr())
    st.docs_batch_device(sp_d.data_ptr(), q, cap, budget, d_d.data_ptr(), o_d.data_ptr(), h_d.data_ptr())
    st.sync()
    return sp_d.cpu().numpy(), d_d.cpu().numpy(), o_d.cpu().numpy(), h_d.cpu().numpy(), sp_d


def test_device_chain_against_the_host_forms(gpu, randoms):
    import torch
    name = "r3"
    cases, st = sd.random_set(name), randoms[name]
    ctx = sd.random_contexts(cases) + sd.random_patterns(cases)[:12]
    q = len(ctx)
    for mode, cap, budget in ((0, 16, 0), (1, 16, 0), (1, 3, 5), (0, 1, 0)):
        want = st.docs_batch(ctx, cap=cap, budget=budget, mode=mode, fill=FILL)
        sp, d, o, h, sp_d = _chain(gpu, st, 3, ctx, mode, cap, budget)
        assert sp.tobytes() == want["spans"].tobytes(), (mode, cap, budget)
        assert d.tobytes() == want["docs"].tobytes() and o.tobytes() == want["offsets"].tobytes() and h.tobytes() == want["heads"].tobytes(), (mode, cap, budget)
        if mode == 0:
            lw = st.locate_batch(ctx, cap=cap, fill=FILL)
            gd, go, gh = _locate_dev(gpu, st, sp_d, q, cap)
            assert gd.tobytes() == lw["docs"].tobytes() and go.tobytes() == lw["offsets"].tobytes() and gh.tobytes() == lw["heads"].tobytes(), cap
    want = st.docs_batch(ctx, cap=0, budget=9)                                                        # counts only: NULL lists are fine
    h_d = torch.full((q, 4), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st.docs_batch_device(sp_d.data_ptr(), q, 0, 9, None, None, h_d.data_ptr())
    st.sync()
    assert h_d.cpu().numpy().tobytes() == st.docs_batch(ctx, cap=0, budget=9, mode=0)["heads"].tobytes() == want["heads"].tobytes()
    assert st.docs_batch([], cap=4)["docs"].shape == (0, 4) and st.locate_batch([], cap=4)["docs"].shape == (0, 4)
    st.docs_batch_device(None, 0, 4, 0, None, None, None)                                             # Q == 0: no-ops
    st.locate_batch_device(None, 0, 4, None, None, None)


@pytest.mark.parametrize("chunk", ["1", "3"])
def test_chunks(gpu, randoms, monkeypatch, chunk):
    """Q = 7 in chunks of 1 and of 3 contexts (the last chunk holds one): the host and the device form against the unchunked set"""
    name = "r3"
    cases = sd.random_set(name)
    ctx = sd.random_patterns(cases)[4:11]
    assert len(ctx) == 7
    monkeypatch.setenv("SA_HIP_TOKEN_SHARD_CHUNK", chunk)
    with _build(gpu, cases) as st:
        for cap, budget in ((5, 0), (0, 0), (2, 40)):
            want = randoms[name].docs_batch(ctx, cap=cap, budget=budget, fill=FILL)
            got = st.docs_batch(ctx, cap=cap, budget=budget, fill=FILL)
            assert all(got[k].tobytes() == want[k].tobytes() for k in want), (chunk, cap, budget)
            info = st.docs_info()
            assert info["chunk"] == int(chunk) and info["pairs_q"] == 21 and info["streamed"] == int(want["heads"]["examined"].sum()), info
            if cap:
                sp, d, o, h, _ = _chain(gpu, st, 3, ctx, 0, cap, budget)
                assert d.tobytes() == want["docs"].tobytes() and o.tobytes() == want["offsets"].tobytes() and h.tobytes() == want["heads"].tobytes(), (chunk, cap)
        assert randoms[name].docs_info()["chunk"] == 7


def test_info_follows_the_last_docs_call(gpu, randoms, monkeypatch):
    """the per-chunk stopwatch: zeros before the first call, the figures of a call in 7 chunks, then of a call in one chunk on the
    same set; asking twice changes nothing"""
    name = "r3"
    cases = sd.random_set(name)
    ctx = sd.random_patterns(cases)[4:11]
    assert len(ctx) == 7
    monkeypatch.setenv("SA_HIP_TOKEN_SHARD_CHUNK", "1")
    with _build(gpu, cases) as st:
        none = st.docs_info()
        assert none["pairs_ms"] == 0 and none["merge_ms"] == 0 and none["chunk"] == 0 and none["pairs_q"] == 0 and none["streamed"] == 0, none
        for cap in (1, 3):
            for part in (ctx, ctx[:1]):                                                               # 7 chunks, then 1
                want = randoms[name].docs_batch(part, cap=cap, fill=FILL)
                got = st.docs_batch(part, cap=cap, fill=FILL)
                assert all(got[k].tobytes() == want[k].tobytes() for k in want), (cap, len(part))
                info = st.docs_info()
                assert info["chunk"] == 1 and info["pairs_q"] == 3 * len(part) and info["merge_q"] == len(part), info
                assert info["streamed"] == int(want["heads"]["examined"].sum()), info
                assert all(np.isfinite(info[k]) and info[k] > 0 for k in ("pairs_ms", "merge_ms")), info
                assert st.docs_info() == info


# ---- the merge step alone ------------------------------------------------------------------------------------------------------

def _merge(gpu, st, S, lists, bases, cap):
    """lists[s][i] = (docs, offsets, written, examined, distinct, count) -> the merged rows of the device, guard pattern kept"""
    import torch
    q = len(lists[0])
    docs = np.full((S, q, max(cap, 1)), 12345, np.int32)
    offs = np.full((S, q, max(cap, 1)), 54321, np.int32)
    heads = np.zeros((S, q), gpu.DOCS_DTYPE)
    for s in range(S):
        for i, (d, o, w, ex, di, ct) in enumerate(lists[s]):
            docs[s, i, :min(len(d), cap)], offs[s, i, :min(len(o), cap)] = d[:cap], o[:cap]
            heads[s, i] = (w, ex, di, ct)
    dd, od, hd = _dev(docs), _dev(offs), _dev(heads.view(np.uint32).view(np.int32).reshape(S, q, 4))
    bd = None if bases is None else _dev(np.array(bases, np.uint64).view(np.int64))
    o_d, o_o = _out(q, cap)
    o_h = torch.full((q, 4), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st.docs_merge_device(dd.data_ptr(), od.data_ptr(), hd.data_ptr(), q, cap, o_d.data_ptr(), o_o.data_ptr(), o_h.data_ptr(),
                         bases_dev_ptr=None if bd is None else bd.data_ptr())
    st.sync()
    return o_d.cpu().numpy().view(np.uint64), o_o.cpu().numpy(), o_h.cpu().numpy().view(gpu.SHARDS_DOCS_DTYPE).reshape(q)


def _merge_model(S, lists, bases, cap):
    out = []
    for i in range(len(lists[0])):
        ent, ex, di, ct, at = {}, 0, 0, 0, 0
        for s in range(S):
            d, o, w, e, dist, count = lists[s][i]
            for j in range(min(w, cap)):
                if at + j < cap:
                    ent[at + j] = (bases[s] + d[j], o[j])
            at, ex, di, ct = at + dist, ex + e, di + dist, ct + count
        out.append((ent, (min(di, cap), ex, di, ct)))
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
        [([3], [3], 1, 2, M, 2)] + [([4], [4], 1, 1, 1, 1)] * (S - 1),                                 # distinct beyond written: the next shard starts past the cap
        [([1, 2], [1, 2], 1, 4, 1, 4) for s in range(S)],                                             # written below the list: its second entry is not read
    ]
    lists = [[cases[i][s] for i in range(len(cases))] for s in range(S)]
    texts = [[1, 2, 3 + s] for s in range(S)]
    with gpu.TokenShards.build(texts) as st:                                                          # (no documents: the bases are the caller's)
        docs, offs, heads = _merge(gpu, st, S, lists, bases, cap)
        for i, (ent, head) in enumerate(_merge_model(S, lists, bases, cap)):
            assert _docs_heads(heads[i:i + 1]) == [head], (i, heads[i], head)
            for j in range(cap):
                want = ent.get(j, (FILL64, FILL))
                assert (int(docs[i, j]), int(offs[i, j])) == want, (i, j, docs[i], offs[i], ent)
        assert int(heads[0]["distinct"]) == S * M > 2 ** 32 and int(heads[0]["written"]) == cap and (docs[0] == FILL64).all()
        assert int(docs[3, 0]) == (S - 1) * (2 ** 32 + 5) + 2 ** 31 - 1 and int(docs[1, 2]) == 2 * (2 ** 32 + 5) + 7
        assert docs[5, 1:].tolist() == [FILL64] * (cap - 1)
        with pytest.raises(gpu.SaHipError) as err:                                                    # its own bases: it has none
            _merge(gpu, st, S, lists, None, cap)
        assert err.value.code == -1 and "no documents" in str(err.value)
        st.set_documents([[0, 1]] * S)                                                                # two documents per shard: base[s] = 2 s
        docs, offs, heads = _merge(gpu, st, S, lists, None, cap)
        assert docs[1, :min(S, cap)].tolist() == [2 * s + 7 for s in range(min(S, cap))] and int(heads[1]["distinct"]) == S
        d0, _, h0 = _merge(gpu, st, S, lists, bases, 0)                                               # cap == 0: heads alone
        assert (d0 == FILL64).all() and int(h0[0]["distinct"]) == S * M and (h0["written"] == 0).all()


# ---- documents that change behind the set --------------------------------------------------------------------------------------

def test_stale_documents_are_refused_until_adopted(gpu):
    cases = sd.random_set("r2")
    pats = sd.random_patterns(cases)[:10]
    built = [gpu.TokenIndex.build(c["t"]) for c in cases]
    built[0].set_documents(cases[0]["starts"])                                                        # before the handle joins a set
    built[1].set_documents([0])
    with gpu.TokenShards.create(built) as st:
        calls = (lambda: st.docs_batch(pats, cap=4), lambda: st.docs_batch(pats, cap=0), lambda: st.locate_batch(pats, cap=4),
                 lambda: st.doc_bases())
        for call in calls:
            with pytest.raises(gpu.SaHipError) as err:
                call()
            assert err.value.code == -1 and "no documents" in str(err.value)
        st.adopt_documents()
        assert st.doc_bases().tolist() == [0, len(cases[0]["starts"]), len(cases[0]["starts"]) + 1]
        one = [cases[0], sd.shard_case(cases[1]["t"], [0])]
        _check_host(gpu, st, one, pats, "adopted", caps=(4,), budgets=(0,))
        st.shard(1).set_documents(cases[1]["starts"])                                                 # behind the set's back
        for call in calls:
            with pytest.raises(gpu.SaHipError) as err:
                call()
            assert err.value.code == -1 and "adopt_documents" in str(err.value), str(err.value)
        import torch
        h_d = torch.zeros((len(pats), 4), dtype=torch.int64, device="cuda:0")
        with pytest.raises(gpu.SaHipError):                                                           # the device forms too, before any launch
            st.docs_batch_device(h_d.data_ptr(), 1, 0, 0, None, None, h_d.data_ptr())
        assert st.shard(1).docs_batch(pats, cap=4)["heads"]["count"].sum() > 0                        # the shard itself answers
        st.adopt_documents()
        assert st.doc_bases().tolist() == sd.bases(cases)
        _check_host(gpu, st, cases, pats, "adopted again", caps=(4,), budgets=(0, 7))
        st.shard(0).set_documents(cases[0]["starts"])                                                 # the same table again still counts
        with pytest.raises(gpu.SaHipError):
            st.docs_batch(pats, cap=4)
        st.shard(0).set_documents(None)
        with pytest.raises(gpu.SaHipError) as err:
            st.adopt_documents()
        assert err.value.code == -1 and "no documents" in str(err.value)
        with pytest.raises(gpu.SaHipError):
            st.docs_batch(pats, cap=4)
        st.set_documents([c["starts"] for c in cases])
        _check_host(gpu, st, cases, pats, "set again", caps=(4,), budgets=(0,))


def test_removing_the_documents_and_refused_tables(gpu):
    cases = sd.random_set("r2")
    pats = sd.random_patterns(cases)[:6]
    with gpu.TokenShards.build([c["t"] for c in cases]) as st:
        assert st.docs_info()["documents"] == 0
        for rep in range(2):
            for call in (lambda: st.docs_batch(pats, cap=4), lambda: st.locate_batch(pats, cap=4), lambda: st.doc_bases()):
                with pytest.raises(gpu.SaHipError) as err:
                    call()
                assert err.value.code == -1 and "no documents" in str(err.value)
            st.set_documents(None)                                                                    # removing nothing: fine
            st.set_documents([c["starts"] for c in cases])
            assert st.docs_info()["documents"] == sd.bases(cases)[-1] and st.shard(1).docs_info()["documents"] == len(cases[1]["starts"])
            assert int(st.docs_batch(pats, cap=4)["heads"]["count"].sum()) > 0
            # a bad table for the LAST shard: refused before the first shard is touched
            n1 = len(cases[1]["t"])
            for bad in ([0, n1 + 1], [1, 2], [0, 5, 4]):
                with pytest.raises(gpu.SaHipError) as err:
                    st.set_documents([[0], bad])
                assert err.value.code == -1
                assert st.shard(0).docs_info()["documents"] == len(cases[0]["starts"]) and st.doc_bases().tolist() == sd.bases(cases)
            lib = gpu.lib()
            import ctypes as C
            tab = np.array([0], np.int32)
            assert lib.sa_hip_token_shards_set_documents(st._h, (C.c_void_p * 2)(tab.ctypes.data, None), (C.c_uint32 * 2)(1, 1)) == -1
            assert lib.sa_hip_token_shards_set_documents(st._h, (C.c_void_p * 2)(tab.ctypes.data, tab.ctypes.data), (C.c_uint32 * 2)(1, 0)) == -1
            assert st.doc_bases().tolist() == sd.bases(cases)
            st.set_documents(None)
            assert st.docs_info()["documents"] == 0 and st.shard(0).docs_info()["documents"] == 0 and st.shard(1).docs_info()["documents"] == 0


# ---- the Python class ----------------------------------------------------------------------------------------------------------

def test_python_class(gpu):
    from suffixarray_amd import ShardedTokenIndex, TokenIndex
    with ShardedTokenIndex([[1, 2, 1, 2, 3], [1, 2, 9, 1, 2]], doc_starts=[[0, 2], [0, 0, 3, 5]]) as sti:   # test_token_shard_docs_cpu.py counts these by hand
        assert sti.document_bases().tolist() == [0, 2, 6] and sti.document_bases().dtype == np.uint64
        d, o = sti.locate([1, 2], 8)
        assert d.dtype == np.uint64 and o.dtype == np.int32 and d.tolist() == [0, 1, 4, 3] and o.tolist() == [0, 0, 0, 0]
        assert [a.tolist() for a in sti.locate([1, 2], 3)] == [[0, 1, 4], [0, 0, 0]] and sti.locate([3, 1], 4)[0].size == 0
        r = sti.documents([[1, 2], [2], [9], [3, 1]], cap=3)
        assert r["docs"].dtype == np.uint64 and r["docs"][:, :3].tolist()[0] == [0, 1, 4] and r["offsets"][1].tolist() == [1, 1, 1]
        assert r["written"].tolist() == [3, 3, 1, 0] and r["distinct"].tolist() == [4, 4, 1, 0] and r["count"].tolist() == [4, 4, 1, 0]
        assert r["docs"][2, 0] == 3 and r["offsets"][2, 0] == 2 and r["exact"].all() and r["distinct"].dtype == np.uint64
        r = sti.documents([[1, 2]], cap=8, budget=3)
        assert r["docs"][0, :3].tolist() == [0, 1, 4] and r["distinct"].tolist() == [3] and r["examined"].tolist() == [3] and not r["exact"][0]
        df, exact = sti.document_counts([[1, 2], [9], [7], []])
        assert df.tolist() == [4, 1, 0, 4] and df.dtype == np.uint64 and exact.all()
        df, exact = sti.document_counts([[1, 2], [9]], budget=2)
        assert df.tolist() == [2, 1] and exact.tolist() == [False, True]
        assert sti.documents([[1, 2]], longest_suffix=True)["distinct"].tolist() == [4]
        assert sti.documents([[5, 9, 1]], longest_suffix=True)["docs"][0, 0] == 3                       # [9 1] only in shard 1's document 1
        sti.set_documents(None)
        with pytest.raises(gpu.SaHipError):
            sti.document_counts([[1]])
        sti.set_documents([[0], [0, 1]])
        assert sti.document_bases().tolist() == [0, 1, 3] and sti.document_counts([[1, 2]])[0].tolist() == [3]
    with pytest.raises(gpu.SaHipError):
        ShardedTokenIndex([[1, 2], [3]], doc_starts=[[0], [0, 2]])                                     # beyond the second shard
    # locate against positions, then searchsorted on the host
    cases = sd.random_set("r3")
    base = sd.bases(cases)
    with ShardedTokenIndex([c["t"] for c in cases], doc_starts=[c["starts"] for c in cases]) as sti:
        for p in sd.random_patterns(cases):
            for limit in (1, 7, 100):
                sh, pos = sti.positions(p, limit=limit)
                d, o = sti.locate(p, limit)
                local = [int(np.searchsorted(cases[s]["starts"], x, "right")) - 1 for s, x in zip(sh.tolist(), pos.tolist())]
                assert d.tolist() == [base[s] + k for s, k in zip(sh.tolist(), local)], (p[:6], limit)
                assert o.tolist() == [x - int(cases[s]["starts"][k]) for s, x, k in zip(sh.tolist(), pos.tolist(), local)], (p[:6], limit)
    # one shard: the answers of TokenIndex on the same text and table
    c = sd.random_set("r2")[0]
    pats = sd.random_patterns([c])
    with ShardedTokenIndex([c["t"]], doc_starts=[c["starts"]]) as sti, TokenIndex(c["t"], doc_starts=c["starts"]) as ti:
        for kw in ({}, {"cap": 3, "budget": 5}, {"longest_suffix": True, "max_length": 2}):
            a, b = sti.documents(pats, **kw), ti.documents(pats, **kw)
            assert all(np.array_equal(a[k], b[k]) for k in b), kw
        assert all(np.array_equal(x, y) for x, y in zip(sti.document_counts(pats, budget=9), ti.document_counts(pats, budget=9)))
        assert all(np.array_equal(x, y) for x, y in zip(sti.locate(pats[4], 9), ti.locate(pats[4], 9)))
