"""Top-k next symbols and draws from a span on the device against the models of token_top_cases.py: every text and context under
four plans (jump step, key array and directory on or off) at k = 8 and 64, byte-identical across plans, and agreeing with the
complete answers of next_batch; k at a span's number of distinct continuations; the budget at every run edge; draws that pin every
run edge of every span; batch shapes and the device chain against the host forms; what the device forms do with a span beyond the
array; the Python class."""
import numpy as np
import pytest

import token_next_cases as nc
import token_top_cases as tt

pytestmark = pytest.mark.gpu

FILL = -7                                                         # cells a launch must not write keep it
UFILL = FILL & 0xFFFFFFFF
WAVE_GRID_MAX = 256 * 16                                          # tq::WAVE_GRID_MAX: workgroups of a wave-per-row launch at most
NEXT_WAVES = 4                                                    # tq::NEXT_WAVES: rows per workgroup


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _compare(got, e, cfg, k, budget, where):
    sym, cnt, heads = tt.top_expected(e, cfg, k, budget, FILL, UFILL)
    sp = got["spans"].view(np.uint32).reshape(-1, 4)
    bad = np.flatnonzero((sp != e["spans"][cfg]).any(axis=1))
    assert bad.size == 0, (where, [(e["ctx"][i][:6], len(e["ctx"][i]), sp[i].tolist(), e["spans"][cfg][i].tolist()) for i in bad[:5]])
    hd = got["heads"].view(np.uint32).reshape(-1, 4)
    bad = np.flatnonzero((hd != heads).any(axis=1) | (got["symbols"] != sym).any(axis=1) | (got["counts"] != cnt).any(axis=1))
    assert bad.size == 0, (where, [(e["ctx"][i][:6], len(e["ctx"][i]), sp[i].tolist(), hd[i].tolist(), heads[i].tolist(),
                                    got["symbols"][i, :6].tolist(), sym[i, :6].tolist(), got["counts"][i, :6].tolist(),
                                    cnt[i, :6].tolist()) for i in bad[:5]])


_SEEN = {}                                                        # (text, configuration, k) -> the bytes of the first plan that ran


@pytest.mark.parametrize("plan", tt.PLANS)
def test_every_text_and_context_under_every_plan(gpu, monkeypatch, plan):
    nc.set_plan(monkeypatch, plan)
    for name in tt.TEXTS:
        e = tt.expected(name)
        with gpu.TokenIndex.build(e["t"]) as ti:
            for cfg in nc.CONFIGS:
                mode, max_length, need_next = cfg
                for k in (8, 64):
                    got = ti.top_batch(e["ctx"], k=k, mode=mode, max_length=max_length, need_next=need_next, fill=FILL)
                    _compare(got, e, cfg, k, 0, (plan, name, cfg, k))
                    blob = b"".join(got[f].tobytes() for f in ("spans", "symbols", "counts", "heads"))
                    assert _SEEN.setdefault((name, cfg, k), blob) == blob, (plan, name, cfg, k, "differs from the first plan")
                # the existing call: where its answer is complete it lists every distinct continuation
                nx = ti.next_batch(e["ctx"], cap=64, mode=mode, max_length=max_length, need_next=need_next)
                full = nx["heads"]["covered"] == nx["heads"]["total"]
                assert np.array_equal(got["heads"]["total"], nx["heads"]["total"]), (plan, name, cfg)
                assert np.array_equal(got["heads"]["distinct"][full], nx["heads"]["written"][full]), (plan, name, cfg)
                assert (got["heads"]["distinct"][~full] > 64).all(), (plan, name, cfg)
                assert np.array_equal(got["spans"], nx["spans"]), (plan, name, cfg)


@pytest.mark.parametrize("plan", ["default", "no_jump", "text_only"])
def test_k_at_the_number_of_distinct_continuations(gpu, monkeypatch, plan):
    nc.set_plan(monkeypatch, plan)
    for name in ("planted",) + tt.NEW_TEXTS:
        e = tt.expected(name)
        i, span = tt.run_span(name)
        sym, cnt = e["entries"][(0, 0, 1)][i]
        d = len(sym)
        with gpu.TokenIndex.build(e["t"]) as ti:
            for k in sorted(k for k in {1, d - 1, d, d + 1, 63, 64} if 1 <= k <= 64):
                got = ti.top_batch(e["ctx"], k=k, mode=0, fill=FILL)
                _compare(got, e, (0, 0, 1), k, 0, (plan, name, k))
                h, w = got["heads"][i], min(k, d)
                assert h["written"] == w and h["distinct"] == d and h["total"] == int(cnt.sum()), (plan, name, k, h)
                assert (h["covered"] == h["total"]) == (k >= d), (plan, name, k, h)
                assert (got["symbols"][i, w:] == FILL).all() and (got["counts"][i, w:] == UFILL).all(), (plan, name, k)
                assert list(zip(got["symbols"][i, :w].tolist(), got["counts"][i, :w].tolist())) == tt.top_of((sym, cnt), k), (plan, name, k)
    e = nc.expected("rand_k1000")                                                                    # ~1000 short runs
    j = e["ctx"].index([])
    ent = e["entries"][(0, 0, 1)][j]
    assert len(ent[0]) > 900
    with gpu.TokenIndex.build(e["t"]) as ti:
        for k in (1, 63, 64):
            got = ti.top_batch([[]], k=k, fill=FILL)
            top = tt.top_of(ent, k)
            assert list(zip(got["symbols"][0].tolist(), got["counts"][0].tolist())) == top, (plan, k)
            assert got["heads"].view(np.uint32).tolist() == [k, len(ent[0]), sum(c for _, c in top), int(ent[1].sum())], (plan, k)


def test_budget_at_every_run_edge(gpu, monkeypatch):
    import suffixarray_amd
    nc.set_plan(monkeypatch, "default")
    k = 8
    for name in ("planted",) + tt.NEW_TEXTS:
        e = tt.expected(name)
        i, span = tt.run_span(name)
        cnt = e["entries"][(0, 0, 1)][i][1]
        total = int(cnt.sum())
        edges = np.cumsum(cnt).tolist()
        budgets = sorted({0, 1, 63, 64, 65, total - 1, total, total + 1} | {b for j in edges for b in (j - 1, j, j + 1)})
        with suffixarray_amd.TokenIndex(e["t"]) as ti:
            for budget in budgets:
                r = ti.top_next_tokens([[tt.A]], k=k, budget=budget)
                ent = tt.walked_entries(e["t"], e["sa"], span, budget)
                top = tt.top_of(ent, k)
                w = int(r["written"][0])
                where = (name, budget)
                assert (w, int(r["distinct"][0]), int(r["covered"][0]), int(r["total"][0])) == \
                    (len(top), len(ent[0]), sum(c for _, c in top), total), where
                assert list(zip(r["symbols"][0, :w].tolist(), r["counts"][0, :w].tolist())) == top, where
                assert bool(r["exact"][0]) == (budget == 0 or total <= budget), where
                assert r["spans"].view(np.uint32).tolist() == span.tolist(), where
                if budget and budget < total:
                    assert int(ent[1].sum()) == budget, where                                          # the cut run counts with what lies inside


def _sample_rows(e, cfg, seen):
    """(row contexts, row draws) pinning every run edge of the spans of cfg that `seen` does not hold yet: one row per draw"""
    ctx, draws, spans = [], [], []
    for i, span in enumerate(e["spans"][cfg].tolist()):
        if tuple(span[:3]) in seen:
            continue
        seen.add(tuple(span[:3]))
        for d in tt.edge_draws(e["entries"][cfg][i][1]):
            ctx.append(e["ctx"][i])
            draws.append(d)
            spans.append(span)
    return ctx, draws, spans


@pytest.mark.parametrize("part", [0, 1])
def test_draws_at_every_run_edge_of_every_span(gpu, monkeypatch, part):
    nc.set_plan(monkeypatch, "default")
    names = tt.TEXTS[part::2]
    empties = 0
    for name in names:
        e = tt.expected(name)
        t, n = e["t"], e["t"].size
        with gpu.TokenIndex.build(t) as ti:
            sa = ti.sa_range(0, n).astype(np.int64)
            seen = set()
            for cfg in nc.CONFIGS:
                mode, max_length, need_next = cfg
                ctx, draws, spans = _sample_rows(e, cfg, seen)
                if not ctx:
                    continue
                want = [tt.sample_of(t, e["sa"], s, d) for s, d in zip(spans, draws)]
                d1 = np.array(draws, np.uint64)
                got = ti.sample_batch(ctx, d1, mode=mode, max_length=max_length, need_next=need_next)                 # m = 1
                assert got["symbols"].shape == (len(ctx), 1) and got["spans"].view(np.uint32).reshape(-1, 4).tolist() == spans, (name, cfg)
                assert list(zip(got["symbols"][:, 0].tolist(), got["ranks"][:, 0].tolist())) == want, (name, cfg)
                for (s, rank), span in zip(want, spans):                                               # the device's own array
                    if s >= 0:
                        assert int(t[sa[rank] + span[2]]) == s, (name, cfg, span, rank)
                    else:
                        assert rank == 0xFFFFFFFF and span[1] == span[3], (name, cfg, span)
                        empties += 1
                # m = 3: the same rows, every row with its own draw, the one before and the one after in the list
                d3 = np.stack([d1, np.roll(d1, 1), np.roll(d1, -1)], axis=1)
                got3 = ti.sample_batch(ctx, d3, mode=mode, max_length=max_length, need_next=need_next)
                want3 = [[tt.sample_of(t, e["sa"], s, int(d)) for d in row] for s, row in zip(spans, d3)]
                assert got3["symbols"].tolist() == [[p[0] for p in row] for row in want3], (name, cfg)
                assert got3["ranks"].tolist() == [[p[1] for p in row] for row in want3], (name, cfg)
        if name in ("n0", "n1"):
            assert empties > 0, name                                                                   # nothing follows anything there
    assert empties > 0                                                                                 # (a miss in mode 0 is in every list)


def test_batch_shapes_and_the_device_chain(gpu, monkeypatch):
    import torch
    nc.set_plan(monkeypatch, "default")
    e = tt.expected("rand_k2")
    cfg, k, m = (1, 0, 1), 5, 3
    sym, cnt, heads = tt.top_expected(e, cfg, k, 0, FILL, UFILL)
    small = [i for i, c in enumerate(e["ctx"]) if len(c) <= 8]
    rng = np.random.default_rng(3)
    with gpu.TokenIndex.build(e["t"]) as ti:
        assert ti.top_batch([], k=k)["symbols"].shape == (0, k) and ti.sample_batch([], np.zeros((0, m), np.uint64))["symbols"].shape == (0, m)
        kept = []
        for q in (1, 4, 5, NEXT_WAVES * WAVE_GRID_MAX + 1):
            rows = [small[(7 * j + q) % len(small)] for j in range(q)]
            sub = [e["ctx"][i] for i in rows]
            draws = rng.integers(0, 2 ** 64, size=(q, m), dtype=np.uint64)
            host = ti.top_batch(sub, k=k, mode=1, fill=FILL)
            assert np.array_equal(host["spans"].view(np.uint32).reshape(-1, 4), e["spans"][cfg][rows]), q
            assert np.array_equal(host["symbols"], sym[rows]) and np.array_equal(host["counts"], cnt[rows]), q
            assert np.array_equal(host["heads"].view(np.uint32).reshape(-1, 4), heads[rows]), q
            hs = ti.sample_batch(sub, draws, mode=1)
            for j in range(0, q, max(q // 64, 1)):
                want = [tt.sample_of(e["t"], e["sa"], e["spans"][cfg][rows[j]], int(d)) for d in draws[j]]
                assert list(zip(hs["symbols"][j].tolist(), hs["ranks"][j].tolist())) == want, (q, j)
            # the device chain: spans -> top and spans -> sample with no host trip, one sync
            buf, off = nc.tc.pack(sub)
            pd, od, dd = _dev(buf if buf.size else np.zeros(1, np.int32)), _dev(off.view(np.int64)), _dev(draws.view(np.int64))
            sp_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
            sy_d = torch.full((q, k), FILL, dtype=torch.int32, device="cuda:0")
            ct_d = torch.full((q, k), FILL, dtype=torch.int32, device="cuda:0")
            hd_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
            ss_d = torch.full((q, m), FILL, dtype=torch.int32, device="cuda:0")
            rk_d = torch.full((q, m), FILL, dtype=torch.int32, device="cuda:0")
            s2_d = torch.full((q, m), FILL, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            ti.spans_batch_device(pd.data_ptr(), od.data_ptr(), q, 1, 0, 1, sp_d.data_ptr())
            ti.top_batch_device(sp_d.data_ptr(), q, k, 0, sy_d.data_ptr(), ct_d.data_ptr(), hd_d.data_ptr())
            ti.sample_batch_device(sp_d.data_ptr(), q, dd.data_ptr(), m, ss_d.data_ptr(), rk_d.data_ptr())
            ti.sample_batch_device(sp_d.data_ptr(), q, dd.data_ptr(), m, s2_d.data_ptr(), None)          # ranks are optional
            ti.sync()
            assert sp_d.cpu().numpy().tobytes() == host["spans"].tobytes(), q
            assert sy_d.cpu().numpy().tobytes() == host["symbols"].tobytes(), q
            assert ct_d.cpu().numpy().tobytes() == host["counts"].tobytes(), q
            assert hd_d.cpu().numpy().tobytes() == host["heads"].tobytes(), q
            assert ss_d.cpu().numpy().tobytes() == hs["symbols"].tobytes() == s2_d.cpu().numpy().tobytes(), q
            assert rk_d.cpu().numpy().tobytes() == hs["ranks"].tobytes(), q
            info = ti.top_info()
            assert info["q"] == q and info["spans_ms"] > 0 and info["top_ms"] > 0 and info["sample_ms"] > 0, info
            kept.append((pd, od, dd))


def _walk_model(t, sa, span, k, draws):
    """the clamped span as the device forms walk it: s(r) = t[sa[r] + length], -1 outside the text; the first rank is stepped
    over when it has no next symbol; runs in rank order -> (top entries, head, [(symbol, rank)] of the draws)"""
    n = t.size
    first, count, length, _ = (int(v) for v in span)
    a = min(first, n)
    end = a + min(count, n - a)
    s = [int(t[int(sa[r]) + length]) if int(sa[r]) + length < n else -1 for r in range(a, end)]
    if s and s[0] < 0:
        a, s = a + 1, s[1:]
    runs = []
    for v in s:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    assert len({v for v, _ in runs}) == len(runs)                                                      # else the entries are unspecified
    top = sorted(((v, c) for v, c in runs), key=lambda p: (-p[1], p[0] & 0xFFFFFFFF))[:k]
    head = [len(top), len(runs), sum(c for _, c in top), len(s)]
    picks = [(s[(d * len(s)) >> 64], a + ((d * len(s)) >> 64)) if s else (-1, 0xFFFFFFFF) for d in draws]
    return top, head, picks


def test_spans_beyond_the_array(gpu, monkeypatch):
    """the device forms clamp first and count to the array and answer the clamped span (the spans are those that
    test_gpu_token_next.py hands to next_batch_device); an in-range array that is not the suffix array: the calls return with
    written <= k and symbols of the text or -1 (nothing else is promised)"""
    import torch
    nc.set_plan(monkeypatch, "default")
    e = nc.expected("rand_k2")
    t, n, k, m = e["t"], e["t"].size, 3, 2
    bad = np.array([(n - 2, 3, 1, 0), (n, 1, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 7, 1), (5, 0xFFFFFFFF, 0xFFFFFFFF, 0), (0, n, 0, 0),
                    (n - 1, 1, 0xFFFFFFFF, 0)], gpu.SPAN_DTYPE)
    draws = [0, 2 ** 64 - 1]
    with gpu.TokenIndex.build(t) as ti:
        sp_d = _dev(bad.view(np.uint32).view(np.int32).reshape(-1, 4))
        sy_d = torch.full((6, k), FILL, dtype=torch.int32, device="cuda:0")
        ct_d = torch.full((6, k), FILL, dtype=torch.int32, device="cuda:0")
        hd_d = torch.full((6, 4), -1, dtype=torch.int32, device="cuda:0")
        dd = _dev(np.array([draws] * 6, np.uint64).view(np.int64))
        ss_d = torch.full((6, m), FILL, dtype=torch.int32, device="cuda:0")
        rk_d = torch.full((6, m), FILL, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ti.top_batch_device(sp_d.data_ptr(), 6, k, 0, sy_d.data_ptr(), ct_d.data_ptr(), hd_d.data_ptr())
        ti.sample_batch_device(sp_d.data_ptr(), 6, dd.data_ptr(), m, ss_d.data_ptr(), rk_d.data_ptr())
        ti.sync()
        hd, sy, ct = hd_d.cpu().numpy().view(np.uint32), sy_d.cpu().numpy(), ct_d.cpu().numpy().view(np.uint32)
        ss, rk = ss_d.cpu().numpy(), rk_d.cpu().numpy().view(np.uint32)
        for i in range(6):
            top, head, picks = _walk_model(t, e["sa"], bad[i].tolist(), k, draws)
            assert hd[i].tolist() == head, (i, hd[i], head)
            assert list(zip(sy[i, :head[0]].tolist(), ct[i, :head[0]].tolist())) == top and (sy[i, head[0]:] == FILL).all(), (i, sy[i], ct[i], top)
            assert list(zip(ss[i].tolist(), rk[i].tolist())) == picks, (i, ss[i], rk[i], picks)
    t_d, rev_d = _dev(t), _dev(np.arange(n, dtype=np.int32)[::-1].copy())                            # (kept alive)
    torch.cuda.synchronize()
    values = set(t.tolist()) | {-1}
    for plan in ("default", "text_only"):
        nc.set_plan(monkeypatch, plan)
        with gpu.TokenIndex.load_device(t_d.data_ptr(), rev_d.data_ptr(), n) as ti:
            for mode in (0, 1):
                got = ti.top_batch(e["ctx"], k=k, mode=mode, fill=FILL)
                assert got["heads"].size == len(e["ctx"]) and (got["heads"]["written"] <= k).all(), (plan, mode)
                dr = np.tile(np.array(draws, np.uint64), (len(e["ctx"]), 1))
                assert set(ti.sample_batch(e["ctx"], dr, mode=mode)["symbols"].reshape(-1).tolist()) <= values, (plan, mode)


def test_python_class(gpu, monkeypatch):
    import suffixarray_amd
    nc.set_plan(monkeypatch, "default")
    with suffixarray_amd.TokenIndex([5, 1, 5, 1, 5], k=6) as ti:
        r = ti.top_next_tokens([[5], [], [7], [5, 1, 5, 1, 5]], k=2)
        assert r["symbols"].shape == (4, 2) and r["counts"].dtype == np.uint32
        assert r["written"].tolist() == [1, 2, 0, 0] and r["distinct"].tolist() == [1, 2, 0, 0]
        assert r["symbols"][0, 0] == 1 and r["counts"][0, 0] == 2                                    # [5] is followed by 1 twice
        assert r["symbols"][1].tolist() == [5, 1] and r["counts"][1].tolist() == [3, 2]              # the first tokens of the five suffixes
        assert r["covered"].tolist() == [2, 5, 0, 0] and r["total"].tolist() == [2, 5, 0, 0] and r["exact"].all()
        assert r["spans"]["length"].tolist() == [1, 0, 1, 5]
        r = ti.top_next_tokens([[5, 1, 5, 1, 5], [2, 2, 1]], k=1, longest_suffix=True)               # backs off to [5, 1, 5] and to [1]
        assert r["symbols"][:, 0].tolist() == [1, 5] and r["counts"][:, 0].tolist() == [1, 2] and r["spans"]["length"].tolist() == [3, 1]
        r = ti.top_next_tokens([[]], k=1, budget=2)                                                  # ranks of 1, 1 behind the empty context
        assert (r["symbols"][0, 0], r["counts"][0, 0], r["total"][0], bool(r["exact"][0])) == (1, 2, 5, False)
        s = ti.sample_next([[5], [1], [7], [5, 1, 5, 1, 5], [2, 2, 1]], samples=4, seed=1)
        assert s.shape == (5, 4) and s.dtype == np.int32
        assert (s[0] == 1).all() and (s[1] == 5).all()
        assert (s[3] == 1).all() and (s[4] == 5).all()                                               # the longest suffix that has a next token
        assert np.array_equal(s, ti.sample_next([[5], [1], [7], [5, 1, 5, 1, 5], [2, 2, 1]], samples=4, seed=1))   # reproducible
        assert set(s[2].tolist()) <= {1, 5}                                                          # [7] backs off to the empty context
        assert (ti.sample_next([[7], [5, 1, 5, 1, 5]], samples=2, seed=0, longest_suffix=False) == -1).all()
        assert ti.sample_next([[5]], draws=[0]).tolist() == [[1]] and ti.sample_next([], samples=3).shape == (0, 3)
    # two continuations of counts 1 and 3 behind [9]: rank = draw * 4 >> 64, the one rank of token 1 stands first
    draws = np.random.default_rng(0).integers(0, 2 ** 64, size=(1, 20000), dtype=np.uint64)
    with suffixarray_amd.TokenIndex([9, 1, 9, 2, 9, 2, 9, 2, 0]) as ti:
        assert ti.next_token_counts([9]) == {1: 1, 2: 3}
        got = ti.sample_next([[9]], draws=draws, longest_suffix=False)
        want = np.where((draws >> np.uint64(62)) == 0, 1, 2).astype(np.int32)
        assert np.array_equal(got, want)
        first, sa = int(ti.ranges([[9]])[0][0]), ti._idx.sa_range(0, 9)
        model = [tt.sample_of([9, 1, 9, 2, 9, 2, 9, 2, 0], sa, (first, 4, 1, 0), int(d))[0] for d in draws[0]]
        assert got[0].tolist() == model
