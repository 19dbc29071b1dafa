"""Top-k next symbols and draws over a shard set on the device against the models of token_shard_top_cases.py: every set and
configuration at k = 8 and 64, byte-identical with the fast path off and under the shards' plans; at S = 1 equal to the shard's own
top_batch; agreeing with the complete answers of the set's next_batch; k at the planted context's number of distinct continuations;
the budget at every merged run edge; refusals that need a set; the device chain across the row stride; fabricated spans beyond a
shard's array and of different lengths; draws that pin every run and shard edge; the Python class."""
import numpy as np
import pytest

import token_next_cases as nc
import token_shard_cases as sc
import token_shard_top_cases as stc
import token_top_cases as tt

pytestmark = pytest.mark.gpu

FILL = -7                                                         # cells a launch must not write keep it
FILL64 = FILL & 0xFFFFFFFFFFFFFFFF
WAVE_GRID_MAX = 256 * 16                                          # tq::WAVE_GRID_MAX: workgroups of a wave-per-row launch at most
NEXT_WAVES = 4                                                    # tq::NEXT_WAVES: rows per workgroup
FAST = "SA_HIP_TOKEN_SHARD_TOP_FAST"


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _plan(monkeypatch, plan="default", fast=None):
    """the shards' plan and the set's switch: both are read when the handles are created"""
    nc.set_plan(monkeypatch, plan)
    monkeypatch.delenv(FAST, raising=False)
    if fast is not None:
        monkeypatch.setenv(FAST, str(fast))


def _heads(h):
    return [tuple(int(v) for v in r) for r in h.tolist()]


def _blob(got):
    return b"".join(np.ascontiguousarray(got[f]).tobytes() for f in ("spans", "symbols", "counts", "heads"))


def _compare(got, e, cfg, k, budget, where):
    sym, cnt, heads = stc.top_expected(e, cfg, k, budget, FILL)
    spans = e[cfg][2]
    assert np.array_equal(got["spans"].view(np.uint32).reshape(spans.shape), spans), where
    bad = [i for i in range(len(heads)) if _heads(got["heads"][i:i + 1]) != heads[i:i + 1] or (got["symbols"][i] != sym[i]).any()
           or (got["counts"][i] != cnt[i]).any()]
    assert not bad, (where, [(e["ctx"][i][:6], _heads(got["heads"][i:i + 1]), heads[i], got["symbols"][i, :6].tolist(), sym[i, :6].tolist(),
                              got["counts"][i, :6].tolist(), cnt[i, :6].tolist()) for i in bad[:4]])


def _run_configs(st, e, where):
    """every configuration at k = 8 and 64 against the model -> {(cfg, k): bytes}; distinct and total against next_batch"""
    out = {}
    for cfg in stc.CONFIGS:
        mode, max_length, need_next = cfg
        for k in (8, 64):
            got = st.top_batch(e["ctx"], k=k, mode=mode, max_length=max_length, need_next=need_next, fill=FILL)
            _compare(got, e, cfg, k, 0, where + (cfg, k))
            out[(cfg, k)] = _blob(got)
        nx = st.next_batch(e["ctx"], cap=64, mode=mode, max_length=max_length, need_next=need_next)
        full = nx["heads"]["covered"] == nx["heads"]["total"]
        assert np.array_equal(got["heads"]["total"], nx["heads"]["total"]) and np.array_equal(got["heads"]["length"], nx["heads"]["length"]), where + (cfg,)
        assert np.array_equal(got["heads"]["distinct"][full], nx["heads"]["written"][full]), where + (cfg,)
        assert (got["heads"]["distinct"][~full] > 64).all(), where + (cfg,)
    return out


@pytest.mark.parametrize("name", stc.SETS)
def test_every_set_against_the_model_with_and_without_the_fast_path(gpu, monkeypatch, name):
    e = stc.expected(name)
    blobs = []
    for fast in (1, 0):
        _plan(monkeypatch, fast=fast)
        with gpu.TokenShards.build(e["shards"]) as st:
            blobs.append(_run_configs(st, e, (name, fast)))
    assert blobs[0] == blobs[1], (name, [key for key in blobs[0] if blobs[0][key] != blobs[1][key]])


@pytest.mark.parametrize("plan", ["no_keys", "text_only", "no_jump"])
def test_the_same_bytes_under_the_shards_plans(gpu, monkeypatch, plan):
    for name in stc.PLAN_SETS + ("queue_edge",):
        e = stc.expected(name)
        blobs = []
        for p in ("default", plan):
            _plan(monkeypatch, p)
            with gpu.TokenShards.build(e["shards"]) as st:
                blobs.append(_run_configs(st, e, (name, p)))
        assert blobs[0] == blobs[1], (name, plan)


@pytest.mark.parametrize("fast", [1, 0])
def test_one_shard_equals_the_single_index(gpu, monkeypatch, fast):
    """S = 1: the set's answer is the shard's own top_batch with the counts widened, and its draws are the shard's own"""
    _plan(monkeypatch, fast=fast)
    cases = [(sc.expected("s1")["shards"][0], sc.expected("s1")["ctx"])] + [(tt.expected(n)["t"], tt.expected(n)["ctx"]) for n in tt.NEW_TEXTS]
    rng = np.random.default_rng(5)
    for t, ctx in cases:
        with gpu.TokenShards.build([t]) as st:
            own = st.shard(0)
            for mode, budget, k in ((0, 0, 8), (1, 0, 64), (1, 65, 8), (0, 1, 3)):
                got = st.top_batch(ctx, k=k, mode=mode, budget=budget, fill=FILL)
                ref = own.top_batch(ctx, k=k, mode=mode, budget=budget, fill=FILL)
                where = (fast, len(t), mode, budget, k)
                assert got["spans"][0].tobytes() == ref["spans"].tobytes(), where
                assert np.array_equal(got["symbols"], ref["symbols"]), where
                keep = np.arange(k)[None, :] < ref["heads"]["written"][:, None]
                assert np.array_equal(got["counts"][keep], ref["counts"].astype(np.uint64)[keep]) and (got["counts"][~keep] == FILL64).all(), where
                for f in ("written", "distinct", "covered", "total"):
                    assert np.array_equal(got["heads"][f].astype(np.uint64), ref["heads"][f].astype(np.uint64)), where + (f,)
                assert np.array_equal(got["heads"]["length"], ref["spans"]["length"]), where
                assert np.array_equal(got["heads"]["shards"], (ref["heads"]["total"] > 0).astype(np.uint32)), where
            draws = rng.integers(0, 2 ** 64, size=(len(ctx), 3), dtype=np.uint64)
            gs, rs = st.sample_batch(ctx, draws, mode=1), own.sample_batch(ctx, draws, mode=1)
            assert np.array_equal(gs["symbols"], rs["symbols"]) and np.array_equal(gs["ranks"], rs["ranks"]), (fast, len(t))
            assert np.array_equal(gs["shards"], np.where(rs["symbols"] >= 0, 0, 0xFFFFFFFF).astype(np.uint32)), (fast, len(t))


@pytest.mark.parametrize("fast", [1, 0])
def test_k_and_budget_edges_of_the_planted_context(gpu, monkeypatch, fast):
    import suffixarray_amd
    _plan(monkeypatch, fast=fast)
    for name in stc.PLANTED + ("mod_deal", "one_next64"):
        e = stc.expected(name)
        cfg = (0, 0, 1)
        i = e["ctx"].index([stc.A])
        ent = e[cfg][3][i]
        d, total = len(ent[0]), sum(ent[1])
        with suffixarray_amd.ShardedTokenIndex(e["shards"]) as sti:
            for k in sorted(k for k in {1, d - 1, d, d + 1, 63, 64} if 1 <= k <= 64):
                got = sti._set.top_batch(e["ctx"], k=k, mode=0, fill=FILL)
                _compare(got, e, cfg, k, 0, (name, fast, k))
                h, w = got["heads"][i], min(k, d)
                assert (h["written"], h["distinct"], h["total"]) == (w, d, total) and (h["covered"] == h["total"]) == (k >= d), (name, fast, k, h)
                assert (got["symbols"][i, w:] == FILL).all() and (got["counts"][i, w:] == FILL64).all(), (name, fast, k)
            edges = np.cumsum(ent[1]).tolist()
            budgets = sorted({1, total - 1, total, total + 1} | {b for j in edges for b in (j - 1, j, j + 1) if b >= 1})
            for budget in budgets:                                 # (one launch of one context each)
                r = sti.top_next_tokens([[stc.A]], k=8, budget=budget)
                walked = stc.cut_entries(ent, budget)
                top = stc.top_of(walked, 8)
                w = int(r["written"][0])
                where = (name, fast, budget)
                assert (w, int(r["distinct"][0]), int(r["covered"][0]), int(r["total"][0])) == (len(top), len(walked[0]), sum(c for _, c in top), total), where
                assert list(zip(r["symbols"][0, :w].tolist(), r["counts"][0, :w].tolist())) == top, where
                assert bool(r["exact"][0]) == (total <= budget), where
                assert sum(walked[1]) == min(budget, total), where                                      # the cut run counts with what lies inside


def test_refusals_that_need_a_set(gpu, monkeypatch):
    _plan(monkeypatch)
    lib = gpu.lib()
    e = stc.expected("ls")
    pat = np.array([3, 4, 5, 77], np.int32)
    off, down = np.array([0, 3, 4], np.uint64), np.array([0, 3, 2], np.uint64)
    spans = np.zeros(2 * 3, gpu.SPAN_DTYPE)
    sym, cnt, heads = np.zeros(130, np.int32), np.zeros(130, np.uint64), np.zeros(2, gpu.SHARDS_TOP_DTYPE)
    draws, sh, rk = np.zeros(2, np.uint64), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    p, o, dn, s, y, c, hd, dr, a, r = (x.ctypes.data for x in (pat, off, down, spans, sym, cnt, heads, draws, sh, rk))
    with gpu.TokenShards.build(e["shards"]) as st:
        h = st._h
        assert lib.sa_hip_token_shards_top_batch(h, p, o, 2, 0, 0, 1, 65, 0, s, y, c, hd) == -1 and b"64" in lib.sa_hip_last_error()
        assert lib.sa_hip_token_shards_top_batch_device(h, 1 << 20, 1 << 25, 64, 0, 1 << 20, 1 << 20, 1 << 20) == -1
        assert b"sa_hip_token_shards_top_batch_device" in lib.sa_hip_last_error() and b"2^31" in lib.sa_hip_last_error()
        assert lib.sa_hip_token_shards_sample_batch_device(h, 1 << 20, 1 << 25, 1 << 20, 64, 1 << 20, None, None) == -1
        assert b"2^31" in lib.sa_hip_last_error()
        assert lib.sa_hip_token_shards_top_batch(h, p, dn, 2, 0, 0, 1, 4, 0, s, y, c, hd) == -1 and b"descend" in lib.sa_hip_last_error()
        assert lib.sa_hip_token_shards_sample_batch(h, p, dn, 2, 0, 0, 1, dr, 1, s, y, a, r) == -1 and b"descend" in lib.sa_hip_last_error()
        assert (sym == 0).all() and (cnt == 0).all()
        # the set still answers
        assert lib.sa_hip_token_shards_top_batch(h, p, o, 2, 0, 0, 1, 4, 0, s, y, c, hd) == 0
        assert heads["total"].tolist() == [2, 0] and heads["shards"].tolist() == [2, 0] and (sym[0], cnt[0]) == (6, 1)


def test_batch_shapes_and_the_device_chain(gpu, monkeypatch):
    import torch
    _plan(monkeypatch)
    e = stc.expected("s3_k2")
    S = len(e["shards"])
    cfg, k, m = (1, 0, 1), 5, 3
    sym, cnt, heads = stc.top_expected(e, cfg, k, 0, FILL)
    spans = e[cfg][2]
    small = [i for i, c in enumerate(e["ctx"]) if len(c) <= 8]
    rng = np.random.default_rng(3)
    with gpu.TokenShards.build(e["shards"]) as st:
        assert st.top_batch([], k=k)["symbols"].shape == (0, k) and st.sample_batch([], np.zeros((0, m), np.uint64))["symbols"].shape == (0, m)
        kept = []
        for q in (1, 4, 5, NEXT_WAVES * WAVE_GRID_MAX + 1):
            rows = [small[(7 * j + q) % len(small)] for j in range(q)]
            sub = [e["ctx"][i] for i in rows]
            draws = rng.integers(0, 2 ** 64, size=(q, m), dtype=np.uint64)
            host = st.top_batch(sub, k=k, mode=1, fill=FILL)
            assert np.array_equal(host["spans"].view(np.uint32).reshape(S, q, 4), spans[:, rows]), q
            assert np.array_equal(host["symbols"], sym[rows]) and np.array_equal(host["counts"], cnt[rows]), q
            assert _heads(host["heads"]) == [heads[i] for i in rows], q
            hs = st.sample_batch(sub, draws, mode=1)
            for j in range(0, q, max(q // 64, 1)):
                want = [stc.sample_of(e, spans, rows[j], int(d)) for d in draws[j]]
                assert list(zip(hs["symbols"][j].tolist(), hs["shards"][j].tolist(), hs["ranks"][j].tolist())) == want, (q, j)
            # the device chain: spans -> top and spans -> sample with no host trip, one sync
            buf, off = nc.tc.pack(sub)
            pd, od, dd = _dev(buf if buf.size else np.zeros(1, np.int32)), _dev(off.view(np.int64)), _dev(draws.view(np.int64))
            i32 = dict(dtype=torch.int32, device="cuda:0")
            sp_d, ln_d = torch.zeros((S, q, 4), **i32), torch.zeros(q, **i32)
            tt_d = torch.zeros(q, dtype=torch.int64, device="cuda:0")
            sy_d = torch.full((q, k), FILL, **i32)
            ct_d = torch.full((q, k), FILL, dtype=torch.int64, device="cuda:0")
            hd_d = torch.zeros((q, 8), **i32)
            ss_d, sh_d, rk_d, s2_d = (torch.full((q, m), FILL, **i32) for _ in range(4))
            torch.cuda.synchronize()
            st.spans_batch_device(pd.data_ptr(), od.data_ptr(), q, 1, 0, 1, ln_d.data_ptr(), tt_d.data_ptr(), sp_d.data_ptr())
            st.top_batch_device(sp_d.data_ptr(), q, k, 0, sy_d.data_ptr(), ct_d.data_ptr(), hd_d.data_ptr())
            st.sample_batch_device(sp_d.data_ptr(), q, dd.data_ptr(), m, ss_d.data_ptr(), sh_d.data_ptr(), rk_d.data_ptr())
            st.sample_batch_device(sp_d.data_ptr(), q, dd.data_ptr(), m, s2_d.data_ptr(), None, None)      # shards and ranks are optional
            st.sync()
            assert sp_d.cpu().numpy().tobytes() == np.ascontiguousarray(host["spans"]).tobytes(), q
            assert sy_d.cpu().numpy().tobytes() == host["symbols"].tobytes(), q
            assert ct_d.cpu().numpy().tobytes() == host["counts"].tobytes(), q
            assert hd_d.cpu().numpy().tobytes() == host["heads"].tobytes(), q
            assert tt_d.cpu().numpy().view(np.uint64).tolist() == host["heads"]["total"].tolist(), q
            assert ss_d.cpu().numpy().tobytes() == hs["symbols"].tobytes() == s2_d.cpu().numpy().tobytes(), q
            assert sh_d.cpu().numpy().tobytes() == hs["shards"].tobytes() and rk_d.cpu().numpy().tobytes() == hs["ranks"].tobytes(), q
            info = st.top_info()
            assert info["q"] == q and info["spans_ms"] > 0 and info["top_ms"] > 0 and info["sample_ms"] > 0, info
            kept.append((pd, od, dd))


def _walk_model(e, row, k, draws):
    """the clamped spans of one context (uint32[S, 4]) as the device forms walk them: s(r) = t[sa[r] + length], the first rank
    stepped over when it has no next symbol -> (top entries, head, [(symbol, shard, rank)] of the draws)"""
    merged, parts, length = {}, [], 0
    for s, sp in enumerate(row.tolist()):
        t, sa = e["shards"][s], e["sas"][s]
        n = len(t)
        first, count, ln, _ = sp
        a = min(first, n)
        end = a + min(count, n - a)
        if a < end and int(sa[a]) + ln >= n:
            a += 1
        seq = [int(t[int(sa[r]) + ln]) if int(sa[r]) + ln < n else -1 for r in range(a, end)]
        runs = [v for j, v in enumerate(seq) if j == 0 or v != seq[j - 1]]
        assert len(set(runs)) == len(runs), (s, sp)                                                    # else the entries are unspecified
        for v in seq:
            merged[v] = merged.get(v, 0) + 1
        parts.append((a, seq))
        length = max(length, ln)
    top = sorted(merged.items(), key=lambda p: (-p[1], p[0] & 0xFFFFFFFF))[:k]
    total = sum(len(seq) for _, seq in parts)
    head = (len(top), len(merged), length, sum(1 for _, seq in parts if seq), sum(c for _, c in top), total)
    picks = []
    for d in draws:
        r = (d * total) >> 64
        pick = (-1, 0xFFFFFFFF, 0xFFFFFFFF)
        for s, (a, seq) in enumerate(parts):
            if total and r < len(seq):
                pick = (seq[r], s, a + r)
                break
            r -= len(seq)
        picks.append(pick)
    return top, head, picks


@pytest.mark.parametrize("fast", [1, 0])
def test_fabricated_spans_beyond_the_arrays_and_of_different_lengths(gpu, monkeypatch, fast):
    """the device forms clamp first and count to every shard's array and read s(r) at every shard's own length; arrays that are
    not suffix arrays: the calls return with written <= k and symbols of the texts or -1 (nothing else is promised)"""
    import torch
    _plan(monkeypatch, fast=fast)
    e = stc.expected("s3_k2")
    S, k, m = len(e["shards"]), 4, 2
    n = [len(t) for t in e["shards"]]
    U = 0xFFFFFFFF
    # per context: one span per shard (first, count, length, ended)
    rows = np.array([
        [(n[0] - 2, 3, 1, 0), (n[1], 1, 0, 0), (U, U, 7, 1)],      # runs over the end; starts at the end; far beyond
        [(5, U, U, 0), (0, n[1], 0, 0), (n[2] - 1, 1, U, 0)],      # a length beyond every text; the whole array; the last rank
        [(0, 40, 0, 0), (10, 30, 1, 0), (20, 90, 2, 0)],           # in range, another length in every shard
        [(U, 0, 0, 0), (0, 0, 3, 0), (7, 130, 1, 1)],              # one live shard: the fast path on a fabricated span
        [(0, n[0] + 5, 0, 0), (n[1] - 1, U, 0, 1), (3, 64, 0, 0)],
    ], np.uint32)                                                   # [Q, S, 4]
    q = rows.shape[0]
    draws = [0, 2 ** 64 - 1]
    with gpu.TokenShards.build(e["shards"]) as st:
        sp_d = _dev(np.ascontiguousarray(rows.transpose(1, 0, 2)).view(np.int32))                      # shard-major
        i32 = dict(dtype=torch.int32, device="cuda:0")
        sy_d = torch.full((q, k), FILL, **i32)
        ct_d = torch.full((q, k), FILL, dtype=torch.int64, device="cuda:0")
        hd_d = torch.full((q, 8), -1, **i32)
        dd = _dev(np.array([draws] * q, np.uint64).view(np.int64))
        ss_d, sh_d, rk_d = (torch.full((q, m), FILL, **i32) for _ in range(3))
        torch.cuda.synchronize()
        st.top_batch_device(sp_d.data_ptr(), q, k, 0, sy_d.data_ptr(), ct_d.data_ptr(), hd_d.data_ptr())
        st.sample_batch_device(sp_d.data_ptr(), q, dd.data_ptr(), m, ss_d.data_ptr(), sh_d.data_ptr(), rk_d.data_ptr())
        st.sync()
        hd = hd_d.cpu().numpy().view(gpu.SHARDS_TOP_DTYPE).reshape(q)
        sy, ct = sy_d.cpu().numpy(), ct_d.cpu().numpy().view(np.uint64)
        ss, sh, rk = ss_d.cpu().numpy(), sh_d.cpu().numpy().view(np.uint32), rk_d.cpu().numpy().view(np.uint32)
        for i in range(q):
            top, head, picks = _walk_model(e, rows[i], k, draws)
            assert _heads(hd[i:i + 1]) == [head], (fast, i, hd[i], head)
            assert list(zip(sy[i, :head[0]].tolist(), ct[i, :head[0]].tolist())) == top and (sy[i, head[0]:] == FILL).all(), (fast, i, sy[i], ct[i], top)
            assert list(zip(ss[i].tolist(), sh[i].tolist(), rk[i].tolist())) == picks, (fast, i, ss[i], sh[i], rk[i], picks)
    # arrays that are not suffix arrays (every shard's ranks reversed)
    t_d = [_dev(t) for t in e["shards"]]
    rev_d = [_dev(np.arange(len(t), dtype=np.int32)[::-1].copy()) for t in e["shards"]]                 # (kept alive)
    torch.cuda.synchronize()
    values = set(v for t in e["shards"] for v in t.tolist()) | {-1}
    with gpu.TokenShards.create([gpu.TokenIndex.load_device(t.data_ptr(), r.data_ptr(), t.numel()) for t, r in zip(t_d, rev_d)]) as st:
        for mode in (0, 1):
            got = st.top_batch(e["ctx"], k=k, mode=mode, fill=FILL)
            assert got["heads"].size == len(e["ctx"]) and (got["heads"]["written"] <= k).all(), (fast, mode)
            dr = np.tile(np.array(draws, np.uint64), (len(e["ctx"]), 1))
            assert set(st.sample_batch(e["ctx"], dr, mode=mode)["symbols"].reshape(-1).tolist()) <= values, (fast, mode)


@pytest.mark.parametrize("part", [0, 1])
def test_draws_at_every_run_and_shard_edge(gpu, monkeypatch, part):
    _plan(monkeypatch)
    empties = 0
    for name in stc.SETS[part::2]:
        e = stc.expected(name)
        with gpu.TokenShards.build(e["shards"]) as st:
            seen = set()
            for cfg in stc.CONFIGS:
                mode, max_length, need_next = cfg
                L, _, spans, _ = e[cfg]
                ctx, draws, at = [], [], []
                for i, c in enumerate(e["ctx"]):
                    key = (need_next, tuple(c[len(c) - L[i]:]))
                    if key in seen:
                        continue
                    seen.add(key)
                    runs = stc.shard_major_runs(e, spans, i)
                    for d in (tt.edge_draws(runs) if runs else [0, 2 ** 64 - 1]):
                        ctx.append(c)
                        draws.append(d)
                        at.append(i)
                if not ctx:
                    continue
                want = [stc.sample_of(e, spans, i, d) for i, d in zip(at, draws)]
                empties += sum(1 for w in want if w[0] < 0)
                d1 = np.array(draws, np.uint64)
                got = st.sample_batch(ctx, d1, mode=mode, max_length=max_length, need_next=need_next)                  # m = 1
                assert got["symbols"].shape == (len(ctx), 1), (name, cfg)
                assert np.array_equal(got["spans"].view(np.uint32).reshape(len(e["shards"]), len(ctx), 4), spans[:, at]), (name, cfg)
                assert list(zip(got["symbols"][:, 0].tolist(), got["shards"][:, 0].tolist(), got["ranks"][:, 0].tolist())) == want, (name, cfg)
                # m = 16: every row with its own draw and its 15 neighbours in the list; shards and ranks not asked for
                d16 = np.stack([np.roll(d1, j) for j in range(16)], axis=1)
                got16 = st.sample_batch(ctx, d16, mode=mode, max_length=max_length, need_next=need_next, shards=False, ranks=False)
                assert got16["shards"] is None and got16["ranks"] is None
                want16 = [[stc.sample_of(e, spans, i, int(d))[0] for d in row] for i, row in zip(at, d16)]
                assert got16["symbols"].tolist() == want16, (name, cfg)
                only_ranks = st.sample_batch(ctx, d1, mode=mode, max_length=max_length, need_next=need_next, shards=False)
                assert only_ranks["shards"] is None and np.array_equal(only_ranks["ranks"], got["ranks"]), (name, cfg)
    assert empties > 0                                                                                 # total == 0 (a miss in mode 0 is in every list)


def test_python_class(gpu, monkeypatch):
    import suffixarray_amd
    _plan(monkeypatch)
    with suffixarray_amd.ShardedTokenIndex([[5, 1, 5, 1, 5], [5, 2, 5, 2, 5, 2, 7], []]) as sti:
        r = sti.top_next_tokens([[5], [], [7], [9]], k=2)
        assert r["symbols"].shape == (4, 2) and r["counts"].dtype == np.uint64 and r["total"].dtype == np.uint64
        assert r["written"].tolist() == [2, 2, 0, 0] and r["distinct"].tolist() == [2, 4, 0, 0]
        assert r["symbols"][0].tolist() == [2, 1] and r["counts"][0].tolist() == [3, 2]               # [5] is followed by 2 x3, 1 x2
        assert r["symbols"][1].tolist() == [5, 2] and r["counts"][1].tolist() == [6, 3]               # first tokens: 5 x6, 2 x3, 1 x2, 7 x1
        assert r["covered"].tolist() == [5, 9, 0, 0] and r["total"].tolist() == [5, 12, 0, 0] and r["exact"].all()
        assert r["shards"].tolist() == [2, 2, 0, 0] and r["length"].tolist() == [1, 0, 1, 1]
        assert r["spans"].shape == (3, 4) and r["spans"]["count"][2].tolist() == [0, 0, 0, 0]
        r = sti.top_next_tokens([[9, 5, 1, 5], [2, 2, 5]], k=1, longest_suffix=True)                  # back off to [5, 1, 5] and to [2, 5]
        assert r["symbols"][:, 0].tolist() == [1, 2] and r["counts"][:, 0].tolist() == [1, 2] and r["length"].tolist() == [3, 2]
        assert r["shards"].tolist() == [1, 1]
        r = sti.top_next_tokens([[]], k=1, budget=3)                                                  # the merged order: 1, 1, then 2 ...
        assert (r["symbols"][0, 0], r["counts"][0, 0], r["total"][0], r["distinct"][0], bool(r["exact"][0])) == (1, 2, 12, 2, False)
        s = sti.sample_next([[5, 1], [1], [7], [9, 2, 5], [8]], samples=4, seed=1)
        assert s.shape == (5, 4) and s.dtype == np.int32
        assert (s[0] == 5).all() and (s[1] == 5).all() and (s[3] == 2).all()
        assert set(s[2].tolist()) <= {1, 2, 5, 7} and set(s[4].tolist()) <= {1, 2, 5, 7}              # back off to the empty context
        assert np.array_equal(s, sti.sample_next([[5, 1], [1], [7], [9, 2, 5], [8]], samples=4, seed=1))   # reproducible
        assert (sti.sample_next([[7], [8]], samples=2, seed=0, longest_suffix=False) == -1).all()
        assert sti.sample_next([[5, 1]], draws=[0]).tolist() == [[5]] and sti.sample_next([], samples=3).shape == (0, 3)
    # [9] is followed by 1 once in shard 0 and by 2 three times in shard 1: r = draw * 4 >> 64, shard 0's one rank stands first
    draws = np.random.default_rng(0).integers(0, 2 ** 64, size=(1, 20000), dtype=np.uint64)
    shards = [[9, 1, 0], [9, 2, 9, 2, 9, 2, 0]]
    with suffixarray_amd.ShardedTokenIndex(shards) as sti:
        assert sti.next_token_counts([9]) == {1: 1, 2: 3}
        got = sti.sample_next([[9]], draws=draws, longest_suffix=False)
        assert np.array_equal(got, np.where((draws >> np.uint64(62)) == 0, 1, 2).astype(np.int32))
        from test_int_cpu import model_sa
        e = {"shards": [np.array(t, np.int32) for t in shards]}
        e["sas"] = [model_sa(t) for t in e["shards"]]
        spans = sti._set.spans_batch([[9]], mode=0)["spans"].view(np.uint32).reshape(2, 1, 4)
        assert got[0].tolist() == [stc.sample_of(e, spans, 0, int(d))[0] for d in draws[0]]
