"""Shard sets on the device against the CPU combine model of token_shard_cases.py AND, byte for byte, against the shards' own
handles (sa_hip_token_shards_shard) with a NumPy combine: ranges, spans in both modes, merged next symbols; cap and chunk edges; the
device chain; the merge step alone on synthetic lists with sums beyond 2^32; the plans; the Python class."""
import numpy as np
import pytest

import token_cases as tc
import token_next_cases as nc
import token_shard_cases as sc

pytestmark = pytest.mark.gpu

FILL = -7                                                         # cells a launch must not write keep it
FILL64 = FILL & 0xFFFFFFFFFFFFFFFF


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def sets(gpu):
    """every shard set built once (default plan, SA_HIP_TOKEN_SHARD_CHUNK unset)"""
    built = {name: gpu.TokenShards.build(sc.expected(name)["shards"]) for name in sc.SETS}
    yield built
    for b in built.values():
        b.close()


def _heads(h):
    return [tuple(int(v) for v in r) for r in h.tolist()]


def _check_next(got, e, cfg, cap, where):
    L, totals, spans, entries = e[cfg]
    sym, cnt, heads = sc.capped(sc.span_length(spans), entries, sc.next_total(spans), cap, FILL)
    assert np.array_equal(got["spans"].view(np.uint32).reshape(spans.shape), spans), where
    bad = [i for i in range(len(entries)) if _heads(got["heads"][i:i + 1]) != heads[i:i + 1] or (got["symbols"][i] != sym[i]).any()
           or (got["counts"][i] != cnt[i]).any()]
    assert not bad, (where, [(e["ctx"][i][:6], _heads(got["heads"][i:i + 1]), heads[i], got["symbols"][i, :4].tolist(), got["counts"][i, :4].tolist()) for i in bad[:4]])


def _own_combine(gpu, st, ctx, tails, S, cap):
    """the shards' own handles on the tails, combined in NumPy: (spans[S, Q], symbols, counts, heads)"""
    own = [st.shard(s).next_batch(tails, cap=cap, mode=0, fill=0) for s in range(S)]
    q = len(ctx)
    spans = np.stack([o["spans"] for o in own])
    sym = np.full((q, cap), FILL, np.int32)
    cnt = np.full((q, cap), FILL64, np.uint64)
    heads = np.zeros(q, gpu.SHARDS_NEXT_DTYPE)
    for i in range(q):
        d = {}
        for o in own:
            w = int(o["heads"]["written"][i])
            for y, c in zip(o["symbols"][i, :w].tolist(), o["counts"][i, :w].tolist()):
                d[y] = d.get(y, 0) + c
        keys = sorted(d)[:cap]
        sym[i, :len(keys)] = keys
        cnt[i, :len(keys)] = [d[y] for y in keys]
        heads[i] = (len(keys), max(int(o["spans"]["length"][i]) for o in own), sum(d[y] for y in keys), sum(int(o["heads"]["total"][i]) for o in own))
    return spans, sym, cnt, heads


@pytest.mark.parametrize("name", sc.SETS)
def test_every_set_against_the_model_and_the_shards_own_handles(gpu, sets, name):
    e, st = sc.expected(name), sets[name]
    ctx, S = e["ctx"], len(e["shards"])
    info = st.info()
    assert info["shards"] == S and info["tokens"] == sum(len(t) for t in e["shards"])
    totals, per = st.query_batch(ctx)
    assert np.array_equal(per["first"], e["first"]) and np.array_equal(per["second"], e["count"]), name
    assert totals.dtype == np.uint64 and np.array_equal(totals, e["count"].astype(np.uint64).sum(axis=0)), name
    assert np.array_equal(st.query_batch(ctx, per_shard=False)[0], totals)
    for s in range(S):
        assert st.shard(s).query_batch(ctx).tobytes() == np.ascontiguousarray(per[s]).tobytes(), (name, s)
    with pytest.raises(IndexError):
        st.shard(S)
    cfgs = sc.CONFIGS if S <= 5 else sc.CONFIGS[:3]
    for cfg in cfgs:
        mode, max_length, need_next = cfg
        L, tot, spans, entries = e[cfg]
        r = st.spans_batch(ctx, mode, max_length, need_next)
        assert r["length"].tolist() == L and r["totals"].tolist() == tot, (name, cfg)
        assert np.array_equal(r["spans"].view(np.uint32).reshape(spans.shape), spans), (name, cfg)
        cap = 8
        got = st.next_batch(ctx, cap=cap, mode=mode, max_length=max_length, need_next=need_next, fill=FILL)
        _check_next(got, e, cfg, cap, (name, cfg))
        assert got["spans"].tobytes() == r["spans"].tobytes()
        tails = [c[len(c) - l:] for c, l in zip(ctx, L)]
        o_spans, o_sym, o_cnt, o_heads = _own_combine(gpu, st, ctx, tails, S, cap)
        assert o_spans.tobytes() == got["spans"].tobytes(), (name, cfg)
        assert o_sym.tobytes() == got["symbols"].tobytes() and o_cnt.tobytes() == got["counts"].tobytes(), (name, cfg)
        assert o_heads.tobytes() == got["heads"].tobytes(), (name, cfg)
    info = st.info()
    assert info["q"] == len(ctx) and info["ranges_ms"] > 0 and info["spans_ms"] > 0 and info["next_ms"] > 0 and info["merge_ms"] > 0, info
    assert info["chunk"] == len(ctx), info


def test_sixty_five_shards_are_refused_and_nothing_is_adopted(gpu):
    built = [gpu.TokenIndex.build([1, 2, s]) for s in range(65)]
    with pytest.raises(gpu.SaHipError) as err:
        gpu.TokenShards.create(built)
    assert err.value.code == -1
    assert all(t._h for t in built) and built[64].query_batch([[1, 2]])["second"].tolist() == [1]      # still the caller's
    with pytest.raises(gpu.SaHipError):
        gpu.TokenShards.create([built[0], built[1], built[0]])
    assert built[0]._h and built[1]._h
    with gpu.TokenShards.create(built[:64]) as st:
        assert not any(t._h for t in built[:64]) and st.info()["shards"] == 64
        assert st.query_batch([[1, 2], [2, 63], [64]])[0].tolist() == [64, 1, 0]
    built[64].close()


def test_cap_edges(gpu, sets):
    """the union's distinct successors against cap - 1, cap, cap + 1 while every shard stays below cap: the shards' lists are
    complete, the union is not"""
    e, st = sc.expected("mod_deal"), sets["mod_deal"]
    i, d = e["ctx"].index([sc.A]), sc.MOD_D
    assert max(len(range(s, d, sc.MOD_S)) for s in range(sc.MOD_S)) < d - 1
    for cap in (1, d - 1, d, d + 1, 64, 200):
        got = st.next_batch(e["ctx"], cap=cap, fill=FILL)
        _check_next(got, e, (0, 0, 1), cap, ("mod_deal", cap))
        h = got["heads"][i]
        full = sum(x + 1 for x in range(d))
        assert h["written"] == min(cap, d) and h["total"] == full and h["covered"] == sum(x + 1 for x in range(min(cap, d))), (cap, h)
        assert (h["covered"] == h["total"]) == (cap >= d) and (got["symbols"][i, min(cap, d):] == FILL).all(), (cap, h)
    e, st = sc.expected("one_next64"), sets["one_next64"]                                              # 64 counts into one entry
    i = e["ctx"].index([sc.A])
    for cap in (1, 64, 65, 66):
        got = st.next_batch(e["ctx"], cap=cap, fill=FILL)
        _check_next(got, e, (0, 0, 1), cap, ("one_next64", cap))
        assert got["symbols"][i, 0] == 7 and got["counts"][i, 0] == 64 * 65 // 2 and got["heads"]["written"][i] == min(cap, 65)


@pytest.mark.parametrize("chunk", ["1", "7", "0"])
def test_chunk_edges(gpu, sets, monkeypatch, chunk):
    import torch
    name, cfg, cap = "s3_k2", (1, 0, 1), 5
    e = sc.expected(name)
    monkeypatch.setenv("SA_HIP_TOKEN_SHARD_CHUNK", chunk)
    with gpu.TokenShards.build(e["shards"]) as st:
        for q in (15, 1):
            ctx = e["ctx"][3:3 + q]
            want = sets[name].next_batch(ctx, cap=cap, mode=1, fill=FILL)                              # the unchunked answer
            got = st.next_batch(ctx, cap=cap, mode=1, fill=FILL)
            assert all(got[k].tobytes() == want[k].tobytes() for k in ("spans", "symbols", "counts", "heads")), (chunk, q)
            assert st.info()["chunk"] == (min(int(chunk), q) if chunk != "0" else q)
            # the device form through the same chunks
            buf, off = tc.pack(ctx)
            pd, od = _dev(buf), _dev(off.view(np.int64))
            S = 3
            sp_d = torch.zeros((S, q, 4), dtype=torch.int32, device="cuda:0")
            ln_d = torch.zeros(q, dtype=torch.int32, device="cuda:0")
            tt_d = torch.zeros(q, dtype=torch.int64, device="cuda:0")
            sy_d = torch.full((q, cap), FILL, dtype=torch.int32, device="cuda:0")
            ct_d = torch.full((q, cap), FILL, dtype=torch.int64, device="cuda:0")
            hd_d = torch.zeros((q, 3), dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            st.spans_batch_device(pd.data_ptr(), od.data_ptr(), q, 1, 0, 1, ln_d.data_ptr(), tt_d.data_ptr(), sp_d.data_ptr())
            st.next_batch_device(sp_d.data_ptr(), q, cap, sy_d.data_ptr(), ct_d.data_ptr(), hd_d.data_ptr())   # no host trip in between
            st.sync()
            assert sp_d.cpu().numpy().tobytes() == want["spans"].tobytes(), (chunk, q)
            assert sy_d.cpu().numpy().tobytes() == want["symbols"].tobytes() and ct_d.cpu().numpy().tobytes() == want["counts"].tobytes(), (chunk, q)
            assert hd_d.cpu().numpy().tobytes() == want["heads"].tobytes(), (chunk, q)
            assert ln_d.cpu().numpy().view(np.uint32).tolist() == want["heads"]["length"].tolist()
            assert tt_d.cpu().numpy().tolist() == want["heads"]["total"].tolist()                      # need_next: the same sum
        # Q == 0: no-ops
        assert st.next_batch([], cap=cap)["symbols"].shape == (0, cap) and st.spans_batch([])["spans"].shape == (3, 0)
        assert st.query_batch([])[0].size == 0
        st.next_batch_device(None, 0, cap, None, None, None)
        # device ranges, with and without the per-shard array
        ctx = e["ctx"]
        buf, off = tc.pack(ctx)
        pd, od = _dev(buf), _dev(off.view(np.int64))
        t1 = torch.zeros(len(ctx), dtype=torch.int64, device="cuda:0")
        t2 = torch.zeros(len(ctx), dtype=torch.int64, device="cuda:0")
        pr = torch.zeros((3, len(ctx), 2), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        st.query_batch_device(pd.data_ptr(), od.data_ptr(), len(ctx), t1.data_ptr(), pr.data_ptr())
        st.query_batch_device(pd.data_ptr(), od.data_ptr(), len(ctx), t2.data_ptr(), None)
        st.sync()
        pr = pr.cpu().numpy().view(np.uint32)
        assert np.array_equal(pr[:, :, 0], e["first"]) and np.array_equal(pr[:, :, 1], e["count"])
        assert t1.cpu().numpy().tolist() == t2.cpu().numpy().tolist() == e["count"].astype(np.int64).sum(axis=0).tolist()


def test_info_follows_the_last_next_call(gpu, sets, monkeypatch):
    """the per-chunk stopwatch: zeros before the first call, the figures of a call in 7 chunks, then of a call in one chunk on the
    same set; asking twice changes nothing"""
    name = "s3_k2"
    e = sc.expected(name)
    ctx = e["ctx"][3:10]
    assert len(ctx) == 7
    monkeypatch.setenv("SA_HIP_TOKEN_SHARD_CHUNK", "1")
    with gpu.TokenShards.build(e["shards"]) as st:
        none = st.info()
        assert none["next_ms"] == 0 and none["merge_ms"] == 0 and none["chunk"] == 0 and none["q"] == 0, none
        for cap in (1, 3):
            for part in (ctx, ctx[:1]):                                                               # 7 chunks, then 1
                want = sets[name].next_batch(part, cap=cap, mode=1, fill=FILL)
                got = st.next_batch(part, cap=cap, mode=1, fill=FILL)
                assert all(got[k].tobytes() == want[k].tobytes() for k in want), (cap, len(part))
                info = st.info()
                assert info["chunk"] == 1 and info["q"] == len(part), info
                assert all(np.isfinite(info[k]) and info[k] > 0 for k in ("next_ms", "merge_ms")), info
                assert st.info() == info


def _merge(gpu, st, S, lists, cap):
    """lists[s][i] = (symbols, counts, written, total) -> the merged (symbols, counts, heads) of the device, canaries kept"""
    import torch
    q = len(lists[0])
    sym = np.full((S, q, cap), 12345, np.int32)
    cnt = np.full((S, q, cap), 54321, np.uint32)
    heads = np.zeros((S, q), gpu.NEXT_DTYPE)
    for s in range(S):
        for i, (y, c, w, tot) in enumerate(lists[s]):
            sym[s, i, :len(y)], cnt[s, i, :len(c)] = y, c
            heads[s, i] = (w, 0, tot, 0)                                                           # (covered is not read)
    sy_d, ct_d, hd_d = _dev(sym), _dev(cnt.view(np.int32)), _dev(heads.view(np.uint32).view(np.int32).reshape(S, q, 4))
    o_sy = torch.full((q, cap), FILL, dtype=torch.int32, device="cuda:0")
    o_ct = torch.full((q, cap), FILL, dtype=torch.int64, device="cuda:0")
    o_hd = torch.full((q, 3), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st.merge_device(sy_d.data_ptr(), ct_d.data_ptr(), hd_d.data_ptr(), q, cap, o_sy.data_ptr(), o_ct.data_ptr(), o_hd.data_ptr())
    st.sync()
    return o_sy.cpu().numpy(), o_ct.cpu().numpy().view(np.uint64), o_hd.cpu().numpy().view(gpu.SHARDS_NEXT_DTYPE).reshape(q)


def _merge_model(S, lists, cap):
    out = []
    for i in range(len(lists[0])):
        d, total = {}, 0
        for s in range(S):
            y, c, w, tot = lists[s][i]
            total += tot
            for a, b in list(zip(y, c))[:min(w, cap)]:
                d[a] = d.get(a, 0) + b
        keys = sorted(d)[:cap]
        out.append((keys, [d[k] for k in keys], total))
    return out


@pytest.mark.parametrize("name, S", [("ls", 3), ("tiny64", 64)])
def test_merge_device_on_synthetic_lists(gpu, sets, name, S):
    st, cap, M = sets[name], 4, 0xFFFFFFFF
    # (a list's own total is a u32 of its shard and is summed as it stands: the lists need not add up to it)
    full = ([3, 9, nc.I32_MAX - 1, nc.I32_MAX], [M, M, M, M], cap, M)                                # written == cap everywhere
    cases = [
        [full] * S,                                                                                    # equal symbols in all lists: S * (2^32 - 1)
        [([], [], 0, 0)] * S,                                                                          # empty lists
        [([10 * s, 10 * s + 1], [M, 1], 2, M) for s in range(S)]    ,                                  # strictly disjoint
        [([s % 3, 5 + s % 2, 100 + s], [M, 2, 3], 3, M) for s in range(S)]    ,                        # interleaved and shared
        [([7], [M], 1, M)] + [([], [], 0, 0)] * (S - 1),                                               # only the first lane
        [([], [], 0, 0)] * (S - 1) + [([0, nc.I32_MAX], [1, M], 2, M)]    ,                            # only the last: 2^31 - 1 is a symbol
        [([1, 2, 3, 4], [1, 1, 1, 1], 9, 4)] * S,                                                      # written beyond cap: clamped
        [([4, 6], [2, 2], 1, 9) for s in range(S)],                                                    # written below the list: 6 is not read
    ]
    lists = [[cases[i][s] for i in range(len(cases))] for s in range(S)]
    sym, cnt, heads = _merge(gpu, st, S, lists, cap)
    for i, (keys, counts, total) in enumerate(_merge_model(S, lists, cap)):
        w = len(keys)
        assert heads[i]["written"] == w and heads[i]["length"] == 0 and heads[i]["total"] == total and heads[i]["covered"] == sum(counts), (i, heads[i])
        assert sym[i, :w].tolist() == keys and cnt[i, :w].tolist() == counts, (i, sym[i], cnt[i])
        assert (sym[i, w:] == FILL).all() and (cnt[i, w:] == FILL64).all(), i                          # canaries beyond written
    assert int(cnt[0, 0]) == S * M > 2 ** 32 and int(heads[0]["covered"]) == 4 * S * M
    assert sym[2, :4].tolist() == [0, 1, 10, 11] and int(heads[2]["total"]) == S * M


@pytest.mark.parametrize("plan", sc.PLANS)
def test_plans(gpu, sets, monkeypatch, plan):
    nc.set_plan(monkeypatch, plan)
    for name in sc.PLAN_SETS:
        e = sc.expected(name)
        with gpu.TokenShards.build(e["shards"]) as st:
            assert st.shard(0).info()["key_bytes"] == (8 if plan == "default" else 0)
            assert (st.shard(0).info()["dir_entries"] > 0) == (plan != "text_only")
            for cfg in ((0, 0, 1), (1, 0, 1), (1, 0, 0)):
                got = st.next_batch(e["ctx"], cap=6, mode=cfg[0], max_length=cfg[1], need_next=cfg[2], fill=FILL)
                _check_next(got, e, cfg, 6, (plan, name, cfg))
                want = sets[name].next_batch(e["ctx"], cap=6, mode=cfg[0], max_length=cfg[1], need_next=cfg[2], fill=FILL)
                assert all(got[k].tobytes() == want[k].tobytes() for k in got), (plan, name, cfg)
            totals, per = st.query_batch(e["ctx"])
            assert np.array_equal(per["first"], e["first"]) and np.array_equal(per["second"], e["count"]), (plan, name)


def test_python_class(gpu):
    import suffixarray_amd
    from suffixarray_amd import ShardedTokenIndex, TokenIndex
    with ShardedTokenIndex(sc.LS) as sti:
        assert sti.shards == 3 and sti.n == 17 and sti.shard_sizes().tolist() == [6, 4, 7]
        assert sti.count([[3, 4, 5], [8], [1, 1], []]).tolist() == [3, 2, 0, 17] and sti.count([[3]]).dtype == np.uint64
        first, count = sti.ranges([[3, 4, 5], [7]])
        assert first.tolist() == [[2, 5], [0, 3], [1, 5]] and count.tolist() == [[1, 0], [1, 1], [1, 0]]
        sh, pos = sti.positions([3, 4, 5])
        assert sh.tolist() == [0, 1, 2] and pos.tolist() == [2, 1, 3]
        sh, pos = sti.positions([8])
        assert sh.tolist() == [2, 2] and sorted(pos.tolist()) == [0, 1]
        assert [a.tolist() for a in sti.positions([8], limit=1)] == [[2], [1]]                         # [8, 2, ...] sorts before [8, 8, ...]
        assert sti.positions([3, 4, 5], limit=2)[0].tolist() == [0, 1] and sti.positions([99])[0].size == 0
        length, total, spans = sti.longest_suffix([[7, 3, 4, 5], [0, 8, 2, 3, 4], [1] * 9])
        assert length.tolist() == [3, 4, 1] and total.tolist() == [2, 1, 1] and spans.shape == (3, 3)
        assert spans[:, 0].tolist() == [(2, 1, 3, 0), (0, 1, 3, 1), (1, 1, 3, 0)]
        assert sti.longest_suffix([[7, 3, 4, 5]], need_next=False)[0].tolist() == [4]
        assert sti.longest_suffix([[7, 3, 4, 5]], max_length=2)[0].tolist() == [2]
        assert sti.next_token_counts([3, 4, 5]) == {6: 1, 9: 1} and sti.next_token_counts([7, 3, 4, 5]) == {}
        assert sti.next_token_counts([7, 3, 4, 5], longest_suffix=True) == {6: 1, 9: 1}
        assert sti.next_token_counts([]) == {1: 1, 2: 2, 3: 3, 4: 3, 5: 3, 6: 1, 7: 1, 8: 2, 9: 1}
        assert sti.next_token_counts([], cap=2) == {1: 1, 2: 2}
        r = sti.next_tokens([[3, 4, 5], [], [77]], cap=2)
        assert r["symbols"].shape == (3, 2) and r["counts"].dtype == np.uint64 and r["total"].dtype == np.uint64
        assert r["written"].tolist() == [2, 2, 0] and r["total"].tolist() == [2, 17, 0] and r["length"].tolist() == [3, 0, 1]
        assert r["complete"].tolist() == [True, False, True]
        assert sti.info()["shards"] == 3 and sti.info()["tokens"] == 17
    sti.close()                                                                                        # closing twice is harmless
    # one shard: every answer equals TokenIndex's on the same text
    e = nc.expected("zero_and_max")
    ctx = e["ctx"]
    with ShardedTokenIndex([e["t"]]) as sti, TokenIndex(e["t"]) as ti:
        assert sti.n == ti.n and np.array_equal(sti.count(ctx), ti.count(ctx))
        f1, c1 = sti.ranges(ctx)
        f0, c0 = ti.ranges(ctx)
        assert np.array_equal(f1[0], f0) and np.array_equal(c1[0], c0)
        assert np.array_equal(sti.positions(ctx[20], limit=9)[1], ti.positions(ctx[20], limit=9))
        for kw in ({}, {"max_length": 7, "need_next": False}, {"max_length": 1}):
            length, total, spans = sti.longest_suffix(ctx, **kw)
            l0, first0, count0 = ti.longest_suffix(ctx, **kw)
            assert np.array_equal(length, l0) and np.array_equal(spans["first"][0], first0) and np.array_equal(spans["count"][0], count0), kw
        for kw in ({}, {"longest_suffix": True}, {"longest_suffix": True, "max_length": 2, "cap": 3}, {"cap": 1}):
            a, b = sti.next_tokens(ctx, **kw), ti.next_tokens(ctx, **kw)
            assert all(np.array_equal(a[k], b[k]) for k in b), kw
            assert sti.next_token_counts(ctx[20], **kw) == ti.next_token_counts(ctx[20], **kw)
    assert suffixarray_amd.ShardedTokenIndex is ShardedTokenIndex
