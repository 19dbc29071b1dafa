"""Integer-alphabet suffix arrays and PLCP on the device against the reference's libsais_int / libsais64_long /
libsais_plcp_int (oracle/_ref/libsa_ref.so), bit for bit: the drop-ins under every plan (byte route, integer keys with dense or
raw codes, one symbol per initial key), with the route each plan must take; the contract (T unchanged, SA[n..n+fs) untouched,
symbols outside [0, k)); the device forms on torch buffers and the int64 sufcheck; then 1e8-symbol texts against the
reference on the box's cores, a 1e9-symbol token text and an int64 text beyond 2^32 symbols checked by sufcheck."""
import ctypes as C

import numpy as np
import pytest

import cases
from oracle.oracle import usable_threads
from test_int_cpu import model_sa, rank_remap, ref_int, ref_long, ref_plcp_int

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _give_back_hbm():
    """the large tests leave tens of GB in torch's caching allocator: hand it back so that later tests see the free HBM"""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()


PLANS = {
    "default": {},
    "no_bytes": {"SA_HIP_INT_BYTES": "0"},
    "raw_codes": {"SA_HIP_INT_COMPACT": "0"},
    "one_symbol": {"SA_HIP_INT_KEY_SYMBOLS": "1"},
    "one_symbol_keys": {"SA_HIP_INT_BYTES": "0", "SA_HIP_INT_KEY_SYMBOLS": "1"},   # many doubling rounds on every text
}


def _env(monkeypatch, plan):
    for k in ("SA_HIP_INT_BYTES", "SA_HIP_INT_COMPACT", "SA_HIP_INT_KEY_SYMBOLS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)


def expected_plan(plan, t):
    if plan in ("no_bytes", "raw_codes", "one_symbol_keys"):
        return 1
    return 0 if (int(t.max()) + 1 <= 1 << 24 and np.unique(t).size <= 256) else 1


def zipf_tokens(n, vocab=50257, seed=0):
    """token ids with a Zipf-like (log-uniform) rank distribution over the vocabulary"""
    u = np.random.default_rng(seed).random(n)
    return np.minimum(np.floor(np.power(float(vocab), u)).astype(np.int64) - 1, vocab - 1).astype(np.int32)


def int_texts():
    """(int32 text, k) pairs of the small suite"""
    rng = np.random.default_rng(17)
    c = {"n0": (np.zeros(0, np.int32), 1), "n1": (np.array([4], np.int32), 5), "n2": (np.array([1, 0], np.int32), 2),
         "n2_same": (np.array([3, 3], np.int32), 4),
         "all_equal": (np.full(20000, 7, np.int32), 8),
         "period2": (np.tile(np.array([5, 1], np.int32), 9000), 6),
         "period3": (np.tile(np.array([2, 0, 1], np.int32), 7000), 3),
         "repeat_block": (np.tile(rng.integers(0, 3000, 2000).astype(np.int32), 15), 3000),
         "two_far_values": (rng.choice(np.array([0, 2 ** 30], np.int32), 30000), 2 ** 30 + 1)}
    for k in (2, 4, 255, 256, 257, 1000, 2 ** 16, 2 ** 20, 2 ** 31 - 1):
        c["rand_k%d" % k] = (rng.integers(0, k, 50000).astype(np.int32), k)
    for name, t in cases.small_texts().items():
        if t.size <= 300_000:
            c["bytes_" + name] = (t.astype(np.int32), 256)
    return c


@pytest.fixture(scope="module")
def expected(ref):
    out = {}
    for name, (t, k) in int_texts().items():
        if t.size <= 1:
            out[name] = np.zeros(t.size, np.int32)
        elif name.startswith("bytes_"):
            out[name] = ref.libsais(t.astype(np.uint8)).astype(np.int32)
        else:
            r, sigma = rank_remap(t)     # per-k buckets: the reference gets the order-preserving remap
            out[name] = ref_int(ref, r, sigma) if k > sigma else ref_int(ref, t, k)
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("plan", list(PLANS))
def test_plans_match_reference(gpu, expected, monkeypatch, plan):
    import torch
    _env(monkeypatch, plan)
    for name, (t, k) in int_texts().items():
        keep = t.copy()
        got = gpu.libsais_int(t, k)
        assert np.array_equal(t, keep), (plan, name)                      # T is never written
        assert np.array_equal(got, expected[name]), (plan, name)
        if t.size < 2:
            continue
        t_d = _dev(t)
        sa_d = torch.full((t.size,), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        st = gpu.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), t.size, k)
        assert np.array_equal(sa_d.cpu().numpy(), expected[name]), (plan, name, st)
        assert st["plan"] == expected_plan(plan, t), (plan, name, st)
        assert st["compacted"] == (0 if plan == "raw_codes" or int(t.max()) + 1 > 1 << 24 else 1), (plan, name, st)
        if st["compacted"]:
            assert st["sigma"] == np.unique(t).size, (plan, name, st)
        if st["plan"] == 1 and "one_symbol" in plan:
            assert st["symbols_per_key"] == 1, (plan, name, st)
        assert st["min_symbol"] == int(t.min()) and st["max_symbol"] == int(t.max()), (plan, name, st)


@pytest.mark.parametrize("plan", ["default", "raw_codes", "one_symbol_keys"])
def test_long_matches_reference(gpu, ref, monkeypatch, plan):
    """libsais64_long over values >= 2^32 and k up to 2^62; the reference gets the rank remap"""
    _env(monkeypatch, plan)
    rng = np.random.default_rng(23)
    for k in (3, 300, 2 ** 33, 2 ** 62):
        vals = rng.integers(0, k, 64, dtype=np.int64)
        for n in (2, 1000, 60000):
            t = rng.choice(vals, n)
            r, sigma = rank_remap(t)
            want = ref_long(ref, r, sigma)
            assert np.array_equal(gpu.libsais64_long(t, k), want), (plan, k, n)
    t = np.array([2 ** 62 + 5, 2 ** 40, 0, 2 ** 62 + 5, 2 ** 40], np.int64)
    assert np.array_equal(gpu.libsais64_long(t, 2 ** 63 - 1), model_sa(t))


def test_fs_sentinel_and_bad_symbols(gpu, expected):
    lib = gpu.lib()
    t, k = int_texts()["rand_k1000"]
    for it, f in ((np.int32, lib.sa_hip_libsais_int), (np.int64, lib.sa_hip_libsais64_long)):
        tt = t.astype(it)
        sa = np.full(t.size + 5, -123, it)
        assert f(tt.ctypes.data, sa.ctypes.data, t.size, k, 5) == 0
        assert np.array_equal(sa[:t.size], expected["rand_k1000"]) and (sa[t.size:] == -123).all()
        bd = gpu.last_call_breakdown()
        assert bd["n"] == t.size and bd["workspace_reused"] in (0, 1), bd
        assert bd["total_ms"] >= bd["build_ms"] >= 0, bd
        assert f(tt.ctypes.data, sa.ctypes.data, t.size, 0, 0) == -1          # k < 1: rejected for its arguments
        assert gpu.last_call_breakdown() == bd
        for bad_at, bad in ((777, -1), (4000, k)):
            b = tt.copy()
            b[bad_at] = bad
            bd = gpu.last_call_breakdown()
            assert f(b.ctypes.data, sa.ctypes.data, t.size, k, 0) == -1, (it, bad)
            msg = lib.sa_hip_last_error().decode()
            assert ("T[%d] = %d" % (bad_at, bad)) in msg, msg
            assert gpu.last_call_breakdown() == bd                               # a failed call leaves the breakdown alone
            sa[:] = -123
            assert f(tt.ctypes.data, sa.ctypes.data, t.size, k, 0) == 0          # the next call works
            assert np.array_equal(sa[:t.size], expected["rand_k1000"])
    assert lib.sa_hip_libsais_int_device(_dev(t).data_ptr(), _dev(np.zeros(t.size, np.int32)).data_ptr(), t.size, 999, 0, None) == -1


def test_plcp_int_matches_reference(gpu, ref, expected):
    lib = gpu.lib()
    L = ref.lib
    L.libsais_lcp.restype = C.c_int32
    L.libsais_lcp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    for name, (t, k) in int_texts().items():
        if t.size < 2:
            continue
        sa = expected[name]
        want = ref_plcp_int(ref, t, sa)
        got = gpu.libsais_plcp_int(t, sa)
        assert np.array_equal(got, want), name
        lcp_ref = np.zeros(t.size, np.int32)
        assert L.libsais_lcp(want.ctypes.data, sa.ctypes.data, lcp_ref.ctypes.data, t.size) == 0
        assert np.array_equal(gpu.libsais_lcp(got, sa), lcp_ref), name
    t, _ = int_texts()["rand_k257"]
    sa = expected["rand_k257"].copy()
    sa[100] = t.size
    out = np.zeros(t.size, np.int32)
    assert lib.sa_hip_libsais_plcp_int(t.ctypes.data, sa.ctypes.data, out.ctypes.data, t.size) == -1
    assert np.array_equal(gpu.libsais_plcp_int(t, expected["rand_k257"]), ref_plcp_int(ref, t, expected["rand_k257"]))


def test_device_forms_and_sufcheck(gpu, ref, expected):
    import torch
    for name in ("rand_k4", "rand_k2147483647", "period3", "bytes_fib", "repeat_block", "n2"):
        t, k = int_texts()[name]
        n = t.size
        # int64 device form, sufcheck
        t64 = _dev(t.astype(np.int64))
        sa64 = torch.zeros(n, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        st = gpu.libsais64_long_device(t64.data_ptr(), sa64.data_ptr(), n, k)
        assert np.array_equal(sa64.cpu().numpy(), expected[name].astype(np.int64)), (name, st)
        assert np.array_equal(gpu.libsais64_long(t.astype(np.int64), k), expected[name]), name
        assert gpu.sufcheck_long_device(t64.data_ptr(), sa64.data_ptr(), n) == 0, name
        sw = sa64.clone()
        sw[0], sw[n - 1] = sa64[n - 1], sa64[0]
        torch.cuda.synchronize()
        assert gpu.sufcheck_long_device(t64.data_ptr(), sw.data_ptr(), n) > 0, name
        # PLCP device form, odd and even n, aligned and not
        t32 = _dev(t)
        sa32 = _dev(expected[name])
        out = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        gpu.plcp_int_device(t32.data_ptr(), sa32.data_ptr(), out.data_ptr(), n)
        assert np.array_equal(out.cpu().numpy(), gpu.libsais_plcp_int(t, expected[name])), name
        if n > 3:
            tail = _dev(np.concatenate([[0], t[1:]]).astype(np.int32))[1:]     # 4-byte aligned view: copied into padding
            ref_sa = ref_int(ref, rank_remap(t[1:])[0], rank_remap(t[1:])[1])
            out2 = torch.zeros(n - 1, dtype=torch.int32, device="cuda:0")
            sa_tail = _dev(ref_sa)
            torch.cuda.synchronize()
            gpu.plcp_int_device(tail.data_ptr(), sa_tail.data_ptr(), out2.data_ptr(), n - 1)
            assert np.array_equal(out2.cpu().numpy(), ref_plcp_int(ref, t[1:], ref_sa)), name


@pytest.mark.parametrize("kind", ["rand_k65536", "zipf"])
def test_1e8_against_reference(gpu, ref, kind):
    n = 100_000_000
    if kind == "zipf":
        t, k = zipf_tokens(n, seed=1), 50257
    else:
        t, k = np.random.default_rng(4).integers(0, 1 << 16, n).astype(np.int32), 1 << 16
    th = usable_threads()
    want = ref_int(ref, t, k, threads=th)
    got = gpu.libsais_int(t, k, threads=th)
    assert np.array_equal(got, want), kind
    del got
    assert np.array_equal(gpu.libsais_plcp_int(t, want), ref_plcp_int(ref, t, want, threads=th)), kind


def test_1e9_zipf_tokens_device(gpu):
    import torch
    n = 1_000_000_000
    g = torch.Generator(device="cuda:0").manual_seed(7)
    u = torch.rand(n, device="cuda:0", generator=g, dtype=torch.float32)
    t = torch.clamp(torch.floor(torch.pow(torch.tensor(50257.0, device="cuda:0"), u)).to(torch.int32) - 1, 0, 50256)
    del u
    sa = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = gpu.libsais_int_device(t.data_ptr(), sa.data_ptr(), n, 50257)
    assert st["plan"] == 1 and st["compacted"] == 1, st
    t64 = t.to(torch.int64)
    del t
    sa64 = sa.to(torch.int64)
    del sa
    torch.cuda.synchronize()
    assert gpu.sufcheck_long_device(t64.data_ptr(), sa64.data_ptr(), n) == 0, st


def test_long_beyond_2_32_device(gpu):
    """n = 2^32 + 2^24 int64 symbols, k = 1000 (route B), with a copy of R = 1e7 symbols planted from A = 1e9 + 7 to
    B = 2^32 + 12345: of every tied pair one suffix index lies below 2^32 and one above, their SA slots and ranks are spread
    over all of [0, n), and the rounds need log2(1e7 / 6) = 20.7 doublings.  (B > 2^32 and B + R < n need n > 2^32 + 1e7: the
    text is 2^24 symbols longer than 2^32, not 2^20.)  HBM: text 8 n + SA 8 n + the 64-bit build's 32 n during its initial sort
    = 48 n bytes, about 207 GB of the MI355X's 288 GB; the sufcheck afterwards needs 8 n of scratch."""
    import torch
    n = (1 << 32) + (1 << 24)
    R, A, B = 10_000_000, 1_000_000_007, (1 << 32) + 12345
    gpu.release_workspace()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(0)
    if free < 56 * n:
        pytest.skip("needs %d GB of free HBM" % (56 * n >> 30))
    g = torch.Generator(device="cuda:0").manual_seed(3)
    t = torch.randint(0, 1000, (n,), device="cuda:0", dtype=torch.int64, generator=g)
    a_first = cases.plant_copy_device(t, A, B, R, 1000)
    sa = torch.empty(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = gpu.libsais64_long_device(t.data_ptr(), sa.data_ptr(), n, 1000)
    print("int64 text beyond 2^32 with a planted repeat of 1e7:", st)
    assert st["plan"] == 1 and st["sigma"] == 1000, st
    assert st["tied_after_sort"] >= 2 * (R - st["symbols_per_key"] + 1) and st["rounds"] >= 20, st
    assert gpu.sufcheck_long_device(t.data_ptr(), sa.data_ptr(), n) == 0, st
    s = st["symbols_per_key"]
    slots = cases.check_planted_pairs(sa, A, B, R, s, a_first, cases.pair_samples(R, s, 200, 4))
    assert len(slots) >= 200
