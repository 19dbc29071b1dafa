"""Spans and next symbols on the device against the two CPU models of token_next_cases.py: every text and context under the six
plans (lane form, jump step, key array and directory on or off), exact and longest-suffix mode with and without the demand for a
next symbol, byte-identical across plans; the cap at a span's number of distinct continuations; which spans take the lane form;
batch shapes; the device chain against the host form; what the two forms do with a span beyond the array; the Python class."""
import numpy as np
import pytest

import token_next_cases as nc

pytestmark = pytest.mark.gpu

FILL = -7                                                         # cells a launch must not write keep it


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def model_b():
    """model B once per text and configuration (shared by the plans)"""
    return {(name, cfg): nc.model_b(nc.expected(name)["t"], nc.expected(name)["ctx"], *cfg) for name in nc.TEXTS for cfg in nc.CONFIGS}


_SEEN = {}                                                        # (text, configuration) -> the bytes of the first plan that ran


def _compare(got, e, cfg, cap, where):
    sym, cnt, heads = nc.capped(e["entries"][cfg], cap, FILL, FILL & 0xFFFFFFFF)
    sp = got["spans"].view(np.uint32).reshape(-1, 4)
    bad = np.flatnonzero((sp != e["spans"][cfg]).any(axis=1))
    assert bad.size == 0, (where, [(e["ctx"][i][:6], len(e["ctx"][i]), sp[i].tolist(), e["spans"][cfg][i].tolist()) for i in bad[:5]])
    hd = got["heads"].view(np.uint32).reshape(-1, 4)
    bad = np.flatnonzero((hd != heads).any(axis=1) | (got["symbols"] != sym).any(axis=1) | (got["counts"] != cnt).any(axis=1))
    assert bad.size == 0, (where, [(e["ctx"][i][:6], len(e["ctx"][i]), sp[i].tolist(), hd[i].tolist(), heads[i].tolist(),
                                    got["symbols"][i, :6].tolist(), got["counts"][i, :6].tolist()) for i in bad[:5]])


@pytest.mark.parametrize("plan", list(nc.PLANS))
def test_every_text_and_context_under_every_plan(gpu, monkeypatch, model_b, plan):
    nc.set_plan(monkeypatch, plan)
    for name in nc.TEXTS:
        e = nc.expected(name)
        with gpu.TokenIndex.build(e["t"]) as ti:
            for cfg in nc.CONFIGS:
                mode, max_length, need_next = cfg
                got = ti.next_batch(e["ctx"], cap=64, mode=mode, max_length=max_length, need_next=need_next, fill=FILL)
                info = ti.next_info()
                _compare(got, e, cfg, 64, (plan, name, cfg))
                for i, (count, length, ended, ctr) in enumerate(model_b[name, cfg]):                 # model B: the counts
                    w = int(got["heads"]["written"][i])
                    assert (got["spans"]["count"][i], got["spans"]["length"][i], got["spans"]["ended"][i]) == (count, length, ended), (plan, name, cfg, i)
                    mine = dict(zip(got["symbols"][i, :w].tolist(), got["counts"][i, :w].tolist()))
                    assert got["heads"]["total"][i] == sum(ctr.values()) and all(ctr[s] == c for s, c in mine.items()), (plan, name, cfg, i)
                    assert w == min(len(ctr), 64), (plan, name, cfg, i)
                lanes = int((e["spans"][cfg][:, 1] <= nc.LANE_MAX).sum())
                assert info["q"] == len(e["ctx"]) and info["lane_spans"] + info["wave_spans"] == len(e["ctx"]), (plan, name, cfg, info)
                assert info["lane_spans"] == (lanes if plan in nc.LANE_PLANS else 0), (plan, name, cfg, info)
                assert np.array_equal(ti.spans_batch(e["ctx"], mode, max_length, need_next), got["spans"]), (plan, name, cfg)
                blob = b"".join(got[k].tobytes() for k in ("spans", "symbols", "counts", "heads"))
                assert _SEEN.setdefault((name, cfg), blob) == blob, (plan, name, cfg, "differs from the first plan")


@pytest.mark.parametrize("plan", ["default", "lanes", "no_jump", "text_only"])
def test_cap_at_the_number_of_distinct_continuations(gpu, monkeypatch, plan):
    nc.set_plan(monkeypatch, plan)
    e = nc.expected("planted")
    d = len(nc.PLANT_S)
    i = e["ctx"].index([nc.PLANT_A])
    assert len(e["entries"][(0, 0, 1)][i][0]) == d
    with gpu.TokenIndex.build(e["t"]) as ti:
        for cap in (1, d - 1, d, d + 1, 64, 65):
            got = ti.next_batch(e["ctx"], cap=cap, mode=0, fill=FILL)
            _compare(got, e, (0, 0, 1), cap, (plan, cap))
            h = got["heads"][i]
            assert h["written"] == min(cap, d) and h["total"] == sum(nc.RUNS) and (h["covered"] == h["total"]) == (cap >= d), (plan, cap, h)
            assert h["covered"] == sum(nc.RUNS[:cap]) and (got["symbols"][i, min(cap, d):] == FILL).all(), (plan, cap, h)
            again = ti.next_of_spans(got["spans"], cap=cap, fill=FILL)                               # host spans in: the same
            assert all(np.array_equal(again[k], got[k]) for k in ("symbols", "counts", "heads")), (plan, cap)
    e = nc.expected("rand_k1000")                                                                    # ~1000 short runs, cap below them
    j = e["ctx"].index([])
    with gpu.TokenIndex.build(e["t"]) as ti:
        for cap in (1, 63, 64, 65, 999, 1000, 1001):
            got = ti.next_batch([[]], cap=cap, fill=FILL)
            sym, cnt, heads = nc.capped([e["entries"][(0, 0, 1)][j]], cap, FILL, FILL & 0xFFFFFFFF)
            assert np.array_equal(got["symbols"], sym) and np.array_equal(got["counts"], cnt), (plan, cap)
            assert got["heads"].view(np.uint32).tolist() == heads[0].tolist(), (plan, cap)


@pytest.mark.parametrize("plan", ["default", "lanes"])
def test_batch_shapes_and_the_device_chain(gpu, monkeypatch, plan):
    import torch
    nc.set_plan(monkeypatch, plan)
    e = nc.expected("rand_k1000")
    cfg, cap = (1, 0, 1), 5
    sym, cnt, heads = nc.capped(e["entries"][cfg], cap, FILL, FILL & 0xFFFFFFFF)
    nctx = len(e["ctx"])
    with gpu.TokenIndex.build(e["t"], 1000) as ti:
        assert ti.next_batch([], cap=cap)["symbols"].shape == (0, cap) and ti.spans_batch([]).size == 0      # Q == 0
        kept = []
        for q in (1, 3, 4, 5, 255, 256, 257):
            pick = [(7 * k + q) % nctx for k in range(q)]
            sub = [e["ctx"][i] if k % 5 else [] for k, i in enumerate(pick)]                                 # empty contexts inside
            rows = [i if k % 5 else e["ctx"].index([]) for k, i in enumerate(pick)]
            host = ti.next_batch(sub, cap=cap, mode=1, fill=FILL)
            assert np.array_equal(host["spans"].view(np.uint32).reshape(-1, 4), e["spans"][cfg][rows]), (plan, q)
            assert np.array_equal(host["symbols"], sym[rows]) and np.array_equal(host["counts"], cnt[rows]), (plan, q)
            assert np.array_equal(host["heads"].view(np.uint32).reshape(-1, 4), heads[rows]), (plan, q)
            # the device chain: spans -> next with no host trip, and a second launch pair before the one sync
            buf, off = nc.tc.pack(sub)
            pd, od = _dev(buf if buf.size else np.zeros(1, np.int32)), _dev(off.view(np.int64))
            outs = []
            for rep in range(2):
                outs.append((torch.zeros((q, 4), dtype=torch.int32, device="cuda:0"),
                             torch.full((q, cap), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((q, cap), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")))
            torch.cuda.synchronize()
            for sp_d, sy_d, ct_d, hd_d in outs:
                ti.spans_batch_device(pd.data_ptr(), od.data_ptr(), q, 1, 0, 1, sp_d.data_ptr())
                ti.next_batch_device(sp_d.data_ptr(), q, cap, sy_d.data_ptr(), ct_d.data_ptr(), hd_d.data_ptr())
            ti.sync()
            for sp_d, sy_d, ct_d, hd_d in outs:
                assert sp_d.cpu().numpy().tobytes() == host["spans"].tobytes(), (plan, q)
                assert sy_d.cpu().numpy().tobytes() == host["symbols"].tobytes(), (plan, q)
                assert ct_d.cpu().numpy().tobytes() == host["counts"].tobytes(), (plan, q)
                assert hd_d.cpu().numpy().tobytes() == host["heads"].tobytes(), (plan, q)
            info = ti.next_info()
            assert info["q"] == q and info["spans_ms"] > 0 and info["next_ms"] > 0 and info["lane_spans"] + info["wave_spans"] == q, info
            kept.append((pd, od, outs))


def test_spans_beyond_the_array(gpu, monkeypatch):
    """the host form refuses first + count > n; the device form clamps: the call returns and written <= cap.  An in-range array
    that is not the suffix array: the calls return with written <= cap (nothing else is promised)"""
    import torch
    nc.set_plan(monkeypatch, "default")
    e = nc.expected("rand_k2")
    t, n, cap = e["t"], e["t"].size, 3
    bad = np.array([(n - 2, 3, 1, 0), (n, 1, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 7, 1), (5, 0xFFFFFFFF, 0xFFFFFFFF, 0), (0, n, 0, 0),
                    (n - 1, 1, 0xFFFFFFFF, 0)], gpu.SPAN_DTYPE)
    lib = gpu.lib()
    with gpu.TokenIndex.build(t) as ti:
        sym, cnt, heads = np.zeros((6, cap), np.int32), np.zeros((6, cap), np.uint32), np.zeros(6, gpu.NEXT_DTYPE)
        for k in range(4):
            one = bad[k:k + 1].copy()
            assert lib.sa_hip_token_index_next_of_spans(ti._h, one.ctypes.data, 1, cap, sym.ctypes.data, cnt.ctypes.data, heads.ctypes.data) == -1, k
            assert b"beyond" in lib.sa_hip_last_error()
        ok = ti.next_of_spans(bad[4:], cap=cap)                                                      # first + count == n: fine
        assert ok["heads"]["written"].tolist() == [2, 0] and ok["heads"]["total"].tolist() == [n, 0]          # symbols 0 and 1; past the text
        sp_d = _dev(bad.view(np.uint32).view(np.int32).reshape(-1, 4))
        sy_d = torch.full((6, cap), FILL, dtype=torch.int32, device="cuda:0")
        ct_d = torch.full((6, cap), FILL, dtype=torch.int32, device="cuda:0")
        hd_d = torch.full((6, 4), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ti.next_batch_device(sp_d.data_ptr(), 6, cap, sy_d.data_ptr(), ct_d.data_ptr(), hd_d.data_ptr())
        ti.sync()
        hd = hd_d.cpu().numpy().view(np.uint32)
        assert (hd[:, 0] <= cap).all() and (hd[:, 3] == 0).all() and (hd[:, 2] <= n).all(), hd
    t_d, rev_d = _dev(t), _dev(np.arange(n, dtype=np.int32)[::-1].copy())                            # (kept alive)
    torch.cuda.synchronize()
    for plan in ("default", "lanes", "text_only"):
        nc.set_plan(monkeypatch, plan)
        with gpu.TokenIndex.load_device(t_d.data_ptr(), rev_d.data_ptr(), n) as ti:
            for mode in (0, 1):
                got = ti.next_batch(e["ctx"], cap=cap, mode=mode)
                assert got["heads"].size == len(e["ctx"]) and (got["heads"]["written"] <= cap).all(), (plan, mode)


def test_python_class(gpu, monkeypatch):
    import suffixarray_amd
    nc.set_plan(monkeypatch, "default")
    with suffixarray_amd.TokenIndex([5, 1, 5, 1, 5], k=6) as ti:
        assert ti.next_token_counts([5]) == {1: 2} and ti.next_token_counts([1]) == {5: 2} and ti.next_token_counts([]) == {1: 2, 5: 3}
        assert ti.next_token_counts([5, 1, 5, 1, 5]) == {} and ti.next_token_counts([2]) == {}
        assert ti.next_token_counts([5, 1, 5, 1, 5], longest_suffix=True) == {1: 1}                  # backs off to [5, 1, 5]
        assert ti.next_token_counts([2, 2, 1], longest_suffix=True) == {5: 2}
        assert ti.next_token_counts([1, 5, 1], longest_suffix=True, max_length=1) == {5: 2}
        assert ti.next_token_counts([], cap=1) == {1: 2}
        length, first, count = ti.longest_suffix([[5, 1, 5, 1, 5], [9, 1, 5], [9], []])
        assert length.tolist() == [3, 2, 0, 0] and count.tolist() == [2, 2, 5, 5] and first.tolist()[2:] == [0, 0]
        assert ti.longest_suffix([[5, 1, 5, 1, 5]], need_next=False)[0].tolist() == [5]
        assert ti.longest_suffix([[5, 1, 5, 1, 5]], max_length=2)[0].tolist() == [2]
        r = ti.next_tokens([[5], [], [7]], cap=1)
        assert r["symbols"].shape == (3, 1) and r["written"].tolist() == [1, 1, 0] and r["total"].tolist() == [2, 5, 0]
        assert r["complete"].tolist() == [True, False, True] and r["length"].tolist() == [1, 0, 1]
    e = nc.expected("zero_and_max")
    with suffixarray_amd.TokenIndex(e["t"]) as ti:
        r = ti.next_tokens(e["ctx"], cap=8, longest_suffix=True)
        sym, cnt, heads = nc.capped(e["entries"][(1, 0, 1)], 8, 0, 0)
        assert np.array_equal(r["symbols"], sym) and np.array_equal(r["counts"], cnt)
        assert np.array_equal(r["written"], heads[:, 0]) and np.array_equal(r["total"], heads[:, 2])
        assert np.array_equal(r["length"], e["spans"][(1, 0, 1)][:, 2]) and np.array_equal(r["complete"], heads[:, 1] == heads[:, 2])
        length, first, count = ti.longest_suffix(e["ctx"], max_length=7, need_next=False)
        want = e["spans"][(1, 7, 0)]
        assert np.array_equal(length, want[:, 2]) and np.array_equal(first, want[:, 0]) and np.array_equal(count, want[:, 1])
        i = int(np.flatnonzero(heads[:, 0] > 1)[0])
        assert ti.next_token_counts(e["ctx"][i], cap=8, longest_suffix=True) == dict(zip(sym[i, :heads[i, 0]].tolist(), cnt[i, :heads[i, 0]].tolist()))
