"""The token index on the device against the two CPU models of token_cases.py, both fields exactly: every text and pattern of
the case list under the four plans (key array and directory on or off), the directory's 2^24 edge, batch shapes (workgroup
edges, empty patterns inside a batch, host and device forms, two launches before one sync), the load path with its refusals,
SA ranges as real occurrences, and the Python class."""
import ctypes as C

import numpy as np
import pytest

import token_cases as tc
from test_int_cpu import rank_remap, ref_int

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _check(ti, name, where):
    t, sa, pats, first, count = tc.expected(name)
    got = ti.query_batch(pats)
    bad = np.flatnonzero((got["first"] != first) | (got["second"] != count))
    assert bad.size == 0, (where, name, [(pats[i][:6], len(pats[i]), tuple(got[i]), (first[i], count[i])) for i in bad[:5]])
    assert np.array_equal(got["second"], tc.model_b(t, pats)), (where, name)


@pytest.fixture(scope="module")
def model_b_counts():
    """model (b) once per text (shared by the plans)"""
    return {name: tc.model_b(tc.expected(name)[0], tc.expected(name)[2]) for name in tc.texts()}


@pytest.mark.parametrize("plan", list(tc.PLANS))
def test_every_text_under_every_plan(gpu, monkeypatch, model_b_counts, plan):
    tc.set_plan(monkeypatch, plan)
    for name in tc.texts():
        t, sa, pats, first, count = tc.expected(name)
        with gpu.TokenIndex.build(t) as ti:
            got = ti.query_batch(pats)
            info = ti.info()                                                   # after the query: q is the last launch
            bad = np.flatnonzero((got["first"] != first) | (got["second"] != count))
            assert bad.size == 0, (plan, name, info, [(pats[i][:6], len(pats[i]), tuple(got[i]), (first[i], count[i])) for i in bad[:5]])
            assert np.array_equal(got["second"], model_b_counts[name]), (plan, name)
            assert info["n"] == t.size and info["q"] == len(pats), (plan, name, info)
            assert info["key_bytes"] == (8 if "KEYS" not in "".join(tc.PLANS[plan]) and t.size else 0), (plan, name, info)
            if t.size:
                assert (info["min_symbol"], info["max_symbol"]) == (int(t.min()), int(t.max())), (plan, name, info)
                assert sa[info["last_rank"]] == t.size - 1, (plan, name, info)
                spread = int(t.max()) - int(t.min()) + 1
                want_dir = spread + 1 if ("DIR" not in "".join(tc.PLANS[plan]) and spread <= 1 << 24) else 0
                assert info["dir_entries"] == want_dir, (plan, name, info)
            if t.size >= 2:
                assert np.array_equal(ti.sa_range(0, t.size), sa), (plan, name)


def test_directory_edge(gpu, monkeypatch):
    tc.set_plan(monkeypatch, "default")
    with gpu.TokenIndex.build(tc.texts()["dir_edge_in"]) as ti:
        assert ti.info()["dir_entries"] == (1 << 24) + 1 and ti.info()["key_bytes"] == 8
        _check(ti, "dir_edge_in", "edge")
    with gpu.TokenIndex.build(tc.texts()["dir_edge_out"]) as ti:
        assert ti.info()["dir_entries"] == 0 and ti.info()["key_bytes"] == 8
        _check(ti, "dir_edge_out", "edge")
    tc.set_plan(monkeypatch, "no_keys")
    with gpu.TokenIndex.build(tc.texts()["dir_edge_out"]) as ti:
        assert ti.info()["dir_entries"] == 0 and ti.info()["key_bytes"] == 0
        _check(ti, "dir_edge_out", "edge, no keys")


@pytest.mark.parametrize("plan", ["default", "text_only"])
def test_batch_shapes_host_and_device_forms(gpu, monkeypatch, plan):
    import torch
    tc.set_plan(monkeypatch, plan)
    t, sa, pats, first, count = tc.expected("rand_k1000")
    with gpu.TokenIndex.build(t, 1000) as ti:
        assert ti.query_batch([]).size == 0                                       # Q == 0: a no-op
        assert gpu.lib().sa_hip_token_index_query_batch(ti._h, None, None, 0, None) == 0
        assert gpu.lib().sa_hip_token_index_query_batch_device(ti._h, None, None, 0, None) == 0
        for q in (1, 255, 256, 257, 1000):
            sel = list(range(q))
            sub = [pats[i] if i % 7 else [] for i in sel]                          # empty patterns in the middle of the batch
            wf = np.array([first[i] if i % 7 else 0 for i in sel], np.uint32)
            wc = np.array([count[i] if i % 7 else t.size for i in sel], np.uint32)
            host = ti.query_batch(sub)
            assert np.array_equal(host["first"], wf) and np.array_equal(host["second"], wc), (plan, q)
            buf, off = tc.pack(sub)
            pd = _dev(buf) if buf.size else _dev(np.zeros(1, np.int32))
            od = _dev(off.view(np.int64))
            out = torch.full((q, 2), -1, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            ti.query_batch_device(pd.data_ptr(), od.data_ptr(), q, out.data_ptr())
            ti.sync()
            assert out.cpu().numpy().tobytes() == host.tobytes(), (plan, q)
            assert ti.info()["q"] == q and ti.info()["kernel_ms"] > 0
        # two launches on one handle, no sync between them, then one sync
        a, b = pats[:300], pats[300:900]
        (ba, oa), (bb, ob) = tc.pack(a), tc.pack(b)
        pa, fa, pb, fb = _dev(ba), _dev(oa.view(np.int64)), _dev(bb), _dev(ob.view(np.int64))
        ra = torch.zeros((len(a), 2), dtype=torch.int32, device="cuda:0")
        rb = torch.zeros((len(b), 2), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ti.query_batch_device(pa.data_ptr(), fa.data_ptr(), len(a), ra.data_ptr())
        ti.query_batch_device(pb.data_ptr(), fb.data_ptr(), len(b), rb.data_ptr())
        ti.sync()
        both = np.concatenate([ra.cpu().numpy(), rb.cpu().numpy()]).view(np.uint32)
        assert np.array_equal(both[:, 0], first[:900]) and np.array_equal(both[:, 1], count[:900]), plan


def test_load_device_answers_like_build(gpu, monkeypatch):
    import torch
    tc.set_plan(monkeypatch, "default")
    for name in ("rand_k4", "repeat_block", "zero_and_max", "n2", "n1"):
        t = tc.texts()[name]
        n = t.size
        t_d = _dev(t)
        sa_d = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        if n >= 2:
            # the int32 k of the device build cannot admit the symbol 2^31 - 1: it gets the order-preserving remap (the same
            # suffix array, test_int_cpu.py: invariance 1), the handle the text itself
            r, sigma = rank_remap(t)
            r_d = _dev(r.astype(np.int32))
            torch.cuda.synchronize()
            gpu.libsais_int_device(r_d.data_ptr(), sa_d.data_ptr(), n, sigma)
        else:
            sa_d.zero_()
            torch.cuda.synchronize()
        with gpu.TokenIndex.load_device(t_d.data_ptr(), sa_d.data_ptr(), n) as ti:
            _check(ti, name, "load_device")
            assert ti.text_dev != t_d.data_ptr() and ti.sa_dev != sa_d.data_ptr()       # copied into the handle
            with gpu.TokenIndex.build(t) as tb:
                pats = tc.expected(name)[2]
                assert ti.query_batch(pats).tobytes() == tb.query_batch(pats).tobytes(), name
    with gpu.TokenIndex.load_device(None, None, 0) as ti:                              # n == 0: a handle that answers
        assert ti.query_batch([[], [1], [-1, 2]]).tolist() == [(0, 0), (0, 0), (0, 0)]


def test_load_refuses_bad_arrays_and_negative_symbols(gpu, monkeypatch):
    tc.set_plan(monkeypatch, "default")
    lib = gpu.lib()
    t, sa, pats, first, count = tc.expected("rand_k4")
    n = t.size
    t_d = _dev(t)
    for bad in (n, -1):
        s = sa.copy()
        s[n // 3] = bad
        h = C.c_void_p(0x1234)
        s_d = _dev(s)
        assert lib.sa_hip_token_index_load_device(C.byref(h), t_d.data_ptr(), s_d.data_ptr(), n, 0) == -1, bad
        assert not h.value and b"outside" in lib.sa_hip_last_error()
    neg = t.copy()
    neg[777] = -1
    h = C.c_void_p(0x1234)
    neg_d, sa_d, rev_d = _dev(neg), _dev(sa), _dev(np.arange(n, dtype=np.int32)[::-1].copy())   # (kept alive: torch reuses freed blocks)
    import torch
    torch.cuda.synchronize()
    assert lib.sa_hip_token_index_load_device(C.byref(h), neg_d.data_ptr(), sa_d.data_ptr(), n, 0) == -1
    assert not h.value and b"negative" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_build(C.byref(h), neg.ctypes.data, n, 4, 0) == -1 and not h.value
    one = np.array([-4], np.int32)
    assert lib.sa_hip_token_index_build(C.byref(h), one.ctypes.data, 1, 1, 0) == -1 and not h.value
    assert lib.sa_hip_token_index_build(C.byref(h), t.ctypes.data, n, 3, 0) == -1 and not h.value      # a symbol >= k
    with gpu.TokenIndex.load_device(t_d.data_ptr(), sa_d.data_ptr(), n) as ti:                         # the next call works
        _check(ti, "rand_k4", "after refusals")
    # an in-range array that is not the suffix array: unspecified answers, but every loop is bounded -- the call returns
    with gpu.TokenIndex.load_device(t_d.data_ptr(), rev_d.data_ptr(), n) as ti:
        got = ti.query_batch(pats)
        assert got.size == len(pats) and (got["first"].astype(np.int64) + got["second"] <= n).all()


def test_sa_range_returns_real_occurrences(gpu, monkeypatch):
    tc.set_plan(monkeypatch, "default")
    for name in ("rand_k2", "repeat_block", "period3"):
        t, sa, pats, first, count = tc.expected(name)
        with gpu.TokenIndex.build(t) as ti:
            got = ti.query_batch(pats)
            seen = 0
            hit = np.flatnonzero(count > 0)
            for i in hit[::max(1, hit.size // 60)]:                             # about 60 of the patterns that occur
                p = pats[i]
                pos = ti.sa_range(int(got["first"][i]), int(got["second"][i]))
                assert pos.dtype == np.int32 and pos.size == count[i]
                where = np.sort(pos)[:50]
                assert all(t[q:q + len(p)].tolist() == p for q in where), (name, p[:6])
                assert np.unique(pos).size == pos.size, (name, p[:6])
                seen += 1
            assert seen >= min(hit.size, 50), name
            assert gpu.lib().sa_hip_token_index_get_sa_range(ti._h, t.size, 1, np.zeros(1, np.int32).ctypes.data) == -1
            assert ti.sa_range(t.size, 0).size == 0


def test_python_class(gpu, monkeypatch):
    import suffixarray_amd
    tc.set_plan(monkeypatch, "default")
    for name in ("rand_k1000", "period2"):
        t, sa, pats, first, count = tc.expected(name)
        with suffixarray_amd.TokenIndex(t) as ti:
            assert ti.n == t.size
            c = ti.count(pats)
            assert c.dtype == np.uint32 and np.array_equal(c, count) and np.array_equal(c, tc.model_b(t, pats)), name
            f, c2 = ti.ranges(tc.pack(pats))                                    # packed form
            assert np.array_equal(f, first) and np.array_equal(c2, count), name
            i = int(np.flatnonzero(count > 3)[0])
            pos = ti.positions(pats[i])
            assert pos.dtype == np.int32 and np.array_equal(pos, sa[first[i]:first[i] + count[i]]), name
            assert np.array_equal(ti.positions(pats[i], limit=2), pos[:2])
            assert ti.positions([-1]).size == 0
    with suffixarray_amd.TokenIndex([5, 1, 5, 1, 5], k=6) as ti:
        assert ti.count([[5, 1], [1, 5, 1], [5], [2]]).tolist() == [2, 1, 3, 0]
        assert ti.positions([5, 1]).tolist() == [2, 0]


def test_reference_suffix_arrays_load(gpu, ref, monkeypatch):
    """the reference's libsais_int array of a text, loaded: the same answers"""
    import torch
    tc.set_plan(monkeypatch, "default")
    for name in ("rand_k1000", "all_equal"):
        t = tc.texts()[name]
        r, sigma = rank_remap(t)
        sa = ref_int(ref, r, sigma)
        t_d, sa_d = _dev(t), _dev(sa)                                            # (kept alive: torch reuses freed blocks)
        torch.cuda.synchronize()
        with gpu.TokenIndex.load_device(t_d.data_ptr(), sa_d.data_ptr(), t.size) as ti:
            _check(ti, name, "reference SA")
