"""PLCP / LCP arrays on the device against the reference's libsais_plcp / libsais_lcp (oracle/_ref/libsa_ref.so) and an
independent Kasai model: the drop-ins (host pointers, 32- and 64-bit), the handle API of a built index, and the int64
device forms -- each with the default plan, without the key shortcut, and with every comparison sent through the wave and
split paths (SA_HIP_LCP_LANE_BYTES=0, a tiny SA_HIP_LCP_WAVE_BYTES).  Then range errors, aliasing, truncated indexes,
1e8-character texts, the work bound on highly repetitive texts and 4.4e9 characters with 64-bit indices."""
import ctypes as C

import numpy as np
import pytest

import cases
from suffixarray_amd import synth
from test_lcp_cpu import kasai_plcp

pytestmark = pytest.mark.gpu

MODES = {
    "default": {},
    "nokeys": {"SA_HIP_LCP_KEYS": "0"},
    "waves_splits": {"SA_HIP_LCP_LANE_BYTES": "0", "SA_HIP_LCP_WAVE_BYTES": "16"},
}


def _bind(ref):
    L = ref.lib
    vp = C.c_void_p
    for name, it in (("libsais_plcp", C.c_int32), ("libsais_lcp", C.c_int32), ("libsais64_plcp", C.c_int64), ("libsais64_lcp", C.c_int64)):
        getattr(L, name).restype = it
        getattr(L, name).argtypes = [vp, vp, vp, it]
        getattr(L, name + "_omp").restype = it
        getattr(L, name + "_omp").argtypes = [vp, vp, vp, it, it]
    return L


def ref_plcp_lcp(ref, t, sa, threads=1):
    from oracle.oracle import usable_threads
    L = _bind(ref)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    s = np.ascontiguousarray(sa, dtype=np.int32)
    p = np.zeros(max(t.size, 1), np.int32)
    q = np.zeros(max(t.size, 1), np.int32)
    if threads == 1:
        assert L.libsais_plcp(t.ctypes.data, s.ctypes.data, p.ctypes.data, t.size) == 0
        assert L.libsais_lcp(p.ctypes.data, s.ctypes.data, q.ctypes.data, t.size) == 0
    else:
        th = usable_threads()
        assert L.libsais_plcp_omp(t.ctypes.data, s.ctypes.data, p.ctypes.data, t.size, th) == 0
        assert L.libsais_lcp_omp(p.ctypes.data, s.ctypes.data, q.ctypes.data, t.size, th) == 0
    return p[:t.size], q[:t.size]


def lcp_texts():
    c = dict(cases.small_texts())
    rng = np.random.default_rng(7)
    c["n0"] = np.zeros(0, np.uint8)
    c["n1"] = np.frombuffer(b"x", np.uint8)
    c["n2_same"] = np.frombuffer(b"xx", np.uint8)
    c["nul_ff"] = rng.choice(np.array([0, 255], np.uint8), 20000)
    c["nul_ff_runs"] = np.repeat(rng.choice(np.array([0, 255, 1, 254], np.uint8), 700), rng.integers(1, 90, 700)).astype(np.uint8)
    c["fib_small"] = synth.fibonacci(10946)
    for p in range(1, 18):
        c["period%d" % p] = synth.periodic(20000 + p, p) if p > 1 else synth.all_same(20001)
    words = synth.d2_words(4097)   # the max-scan over W works in tiles of 4096 positions: exactly one tile, and one position more
    c["tile_4096"], c["tile_4097"] = words[:4096], words
    blk = rng.integers(0, 256, 65536, dtype=np.uint8)
    c["repeat_64k_x12"] = np.tile(blk, 12)
    for sig in cases.ALPHABET_SIGMAS:
        alph = cases.alphabet(sig, "ends" if sig >= 255 else "mid")
        c["alph%d_b%d" % (sig, cases.code_bits(sig))] = cases.alphabet_text(alph, 30000, "binary" if sig % 2 else "uniform", sig)
    return c


TEXTS = lcp_texts()


@pytest.fixture(scope="module")
def expected(ref):
    out = {}
    for name, t in TEXTS.items():
        sa = ref.libsais(t) if t.size else np.zeros(0, np.int32)
        p, q = ref_plcp_lcp(ref, t, sa)
        out[name] = (sa, p, q)
    # the Kasai model on a few of them: the reference itself is judged too
    for name in ("banana", "mississippi", "fib_small", "period5", "nul_ff", "alph3_b2"):
        assert np.array_equal(kasai_plcp(TEXTS[name], out[name][0]), out[name][1]), name
    return out


def _env(monkeypatch, mode):
    for k in ("SA_HIP_LCP_KEYS", "SA_HIP_LCP_LANE_BYTES", "SA_HIP_LCP_WAVE_BYTES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("mode", list(MODES))
def test_dropins_match_reference(gpu, expected, monkeypatch, mode):
    _env(monkeypatch, mode)
    for name, t in TEXTS.items():
        sa, p, q = expected[name]
        got_p = gpu.libsais_plcp(t, sa)
        assert got_p.dtype == np.int32 and np.array_equal(got_p, p), (mode, name)
        assert np.array_equal(gpu.libsais_lcp(p, sa), q), (mode, name)
        got_p64 = gpu.libsais64_plcp(t, sa.astype(np.int64))
        assert got_p64.dtype == np.int64 and np.array_equal(got_p64, p), (mode, name)
        assert np.array_equal(gpu.libsais64_lcp(p.astype(np.int64), sa.astype(np.int64)), q), (mode, name)
    bd = gpu.last_call_breakdown()
    assert bd["n"] == TEXTS[name].size and bd["workspace_reused"] in (0, 1)


@pytest.mark.parametrize("mode", list(MODES))
def test_handle_matches_reference(gpu, expected, monkeypatch, mode):
    import torch
    _env(monkeypatch, mode)
    tied_seen = 0
    for name, t in TEXTS.items():
        sa, p, q = expected[name]
        with gpu.DeviceIndex(max(t.size, 1), 0) as idx:
            idx.build(t)
            assert np.array_equal(idx.sa_u32(), sa.astype(np.uint32)), name
            assert np.array_equal(idx.lcp(plcp=True), p.astype(np.uint32)), (mode, name)
            assert np.array_equal(idx.lcp(), q.astype(np.uint32)), (mode, name)
            if t.size >= 2:
                buf = torch.empty(t.size, dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()
                st = idx.lcp_device(buf.data_ptr(), stats=True)
                assert np.array_equal(buf.cpu().numpy(), q), (mode, name)
                assert st["n"] == t.size, (mode, name, st)
                if mode == "nokeys":
                    assert st["keys"] == 0 and st["tied"] == 0, (name, st)
                if mode == "waves_splits" and st["compared_positions"]:
                    assert st["wave_compares"] > 0, (name, st)
                tied_seen += st["tied"]
    assert (tied_seen > 0) == (mode != "nokeys")


@pytest.mark.parametrize("mode", list(MODES))
def test_int64_device_forms_match_reference(gpu, expected, monkeypatch, mode):
    import torch
    _env(monkeypatch, mode)
    splits = 0
    for name, t in TEXTS.items():
        sa, p, q = expected[name]
        n = t.size
        text_d = torch.from_numpy(np.ascontiguousarray(t).copy()).to("cuda:0") if n else torch.empty(16, dtype=torch.uint8, device="cuda:0")
        sa_d = torch.from_numpy(sa.astype(np.int64)).to("cuda:0") if n else torch.empty(1, dtype=torch.int64, device="cuda:0")
        out_d = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        st = gpu.plcp64_device(text_d.data_ptr(), sa_d.data_ptr(), out_d.data_ptr(), n)
        assert np.array_equal(out_d[:n].cpu().numpy(), p), (mode, name)
        gpu.lcp64_device(text_d.data_ptr(), sa_d.data_ptr(), out_d.data_ptr(), n)
        assert np.array_equal(out_d[:n].cpu().numpy(), q), (mode, name)
        splits += st["split_compares"]
    assert splits > 0, mode   # all_a_70000: PLCP[0] = 69999 is longer than any wave budget


def test_alphabets_code_widths_on_narrow_plans(gpu, ref, monkeypatch):
    """4.5 M characters: the key shortcut over the narrow (u32 keys + bucket bounds), 10-byte and 12-byte record plans, code
    widths 1-9 -- end of text is code 0, so 256 symbols need 9-bit codes"""
    for mode in ("default", "waves_splits"):
        _env(monkeypatch, mode)
        for sig in (1, 2, 4, 8, 16, 32, 64, 128, 255, 256):
            alph = cases.alphabet(sig, "ends" if sig >= 255 else ("lo" if sig % 4 == 0 else "hi"))
            t = cases.alphabet_text(alph, 4_500_001, "binary" if sig in (2, 16, 255) else "uniform", 100 + sig)
            sa = ref.libsais(t, threads=16)
            p, q = ref_plcp_lcp(ref, t, sa, threads=16)
            with gpu.DeviceIndex(t.size, 0) as idx:
                idx.build(t)
                bs = idx.build_stats()
                assert bs["bits_per_symbol"] == cases.code_bits(sig)
                assert np.array_equal(idx.lcp(), q.astype(np.uint32)), (mode, sig, bs["narrow_k"])
                assert np.array_equal(idx.lcp(plcp=True), p.astype(np.uint32)), (mode, sig)


def test_lcp_may_alias_sa(gpu, expected):
    lib = gpu.lib()
    for name in ("mississippi", "d2_300k", "repeat_block"):
        sa, p, q = expected[name]
        buf = sa.astype(np.int32).copy()
        assert lib.sa_hip_libsais_lcp(p.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.size) == 0
        assert np.array_equal(buf, q), name
        b64 = sa.astype(np.int64)
        p64 = p.astype(np.int64)
        assert lib.sa_hip_libsais64_lcp_omp(p64.ctypes.data, b64.ctypes.data, b64.ctypes.data, b64.size, 4) == 0
        assert np.array_equal(b64, q), name


def test_out_of_range_entry_is_refused_then_next_call_works(gpu, expected):
    import torch
    lib = gpu.lib()
    t = TEXTS["d1_300k"]
    sa, p, q = expected["d1_300k"]
    for bad_value in (t.size, t.size + 12345, -1):
        bad = sa.astype(np.int32).copy()
        bad[t.size // 2] = bad_value
        out = np.zeros(t.size, np.int32)
        assert lib.sa_hip_libsais_plcp(t.ctypes.data, bad.ctypes.data, out.ctypes.data, t.size) == -1
        assert lib.sa_hip_libsais_lcp(p.ctypes.data, bad.ctypes.data, out.ctypes.data, t.size) == -1
        b64 = bad.astype(np.int64)
        o64 = np.zeros(t.size, np.int64)
        assert lib.sa_hip_libsais64_plcp(t.ctypes.data, b64.ctypes.data, o64.ctypes.data, t.size) == -1
        text_d = torch.from_numpy(t.copy()).to("cuda:0")
        sa_d = torch.from_numpy(b64).to("cuda:0")
        out_d = torch.empty(t.size, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        assert lib.sa_hip_plcp64_device(text_d.data_ptr(), sa_d.data_ptr(), out_d.data_ptr(), t.size, 0, None) == -1
        assert lib.sa_hip_lcp64_device(text_d.data_ptr(), sa_d.data_ptr(), out_d.data_ptr(), t.size, 0, None) == -1
        assert b"out of range" in lib.sa_hip_last_error()
        # the process goes on: the next calls succeed
        assert np.array_equal(gpu.libsais_plcp(t, sa), p)
        assert np.array_equal(gpu.libsais_lcp(p, sa), q)
    # entries in range but not a suffix array: bounded, unspecified output, return 0
    perm = np.random.default_rng(3).permutation(t.size).astype(np.int32)
    gpu.libsais_plcp(t, perm)
    gpu.libsais_plcp(t[:5000], np.zeros(5000, np.int32))


def test_truncated_and_empty_handles_refused(gpu):
    import torch
    t = synth.d1_uniform27(100_000)
    buf = torch.empty(t.size, dtype=torch.int32, device="cuda:0")
    with gpu.DeviceIndex(t.size, 0) as idx:
        with pytest.raises(gpu.SaHipError) as e:
            idx.lcp_device(buf.data_ptr())
        assert e.value.code == -1
        idx.build(t, max_suffix_length=16)
        for fn in (idx.lcp_device, idx.plcp_device):
            with pytest.raises(gpu.SaHipError) as e:
                fn(buf.data_ptr())
            assert e.value.code == -1 and "truncated" in str(e.value)
        idx.build(t)   # the same handle, full suffix array: fine
        assert idx.lcp().size == t.size


@pytest.mark.parametrize("kind", ["d1", "words"])
def test_1e8_handle_and_dropins_equal_reference_omp(gpu, ref, kind):
    n = 100_000_000
    t = synth.d1_uniform27(n) if kind == "d1" else synth.d2_words(n)
    sa = ref.libsais(t, threads=16)
    p, q = ref_plcp_lcp(ref, t, sa, threads=16)
    with gpu.DeviceIndex(n, 0) as idx:
        idx.build(t)
        assert np.array_equal(idx.lcp(), q.view(np.uint32)), kind
        assert np.array_equal(idx.lcp(plcp=True), p.view(np.uint32)), kind
    assert np.array_equal(gpu.libsais_plcp(t, sa), p), kind
    assert np.array_equal(gpu.libsais_lcp(p, sa), q), kind


def _irreducible_sum(t, sa, plcp):
    n = t.size
    phi = np.full(n, -1, np.int64)
    phi[sa[1:]] = sa[:-1]
    i = np.arange(n)
    irr = (i == 0) | (phi <= 0)
    ok = ~irr
    irr[ok] = t[i[ok] - 1] != t[phi[ok] - 1]
    return int(plcp[irr].astype(np.int64).sum())


@pytest.mark.parametrize("kind", ["repeat_1mib_x95", "all_a_1e7"])
def test_work_bound_on_repetitive_texts(gpu, ref, kind):
    import torch
    if kind == "all_a_1e7":
        t = synth.all_same(10_000_000)
    else:
        t = np.tile(np.random.default_rng(11).integers(97, 123, 1 << 20, dtype=np.uint8), 95)
    n = t.size
    sa = ref.libsais(t, threads=16)
    p, q = ref_plcp_lcp(ref, t, sa, threads=16)
    bound = 2 * _irreducible_sum(t, sa, p) + 64 * n
    buf = torch.empty(n, dtype=torch.int32, device="cuda:0")
    with gpu.DeviceIndex(n, 0) as idx:
        idx.build(t)
        torch.cuda.synchronize()
        for what in ("lcp", "plcp"):
            st = getattr(idx, what + "_device")(buf.data_ptr(), stats=True)
            exp = q if what == "lcp" else p
            assert np.array_equal(buf.cpu().numpy(), exp), (kind, what)
            assert st["compared_bytes"] <= bound, (kind, what, st, bound)
            assert st["total_ms"] < 2000.0, (kind, what, st)
            print(kind, what, st)


def test_4p4e9_int64_device_forms(gpu):
    """n > 2^32: libsais64_device builds the int64 suffix array, plcp64_device / lcp64_device derive PLCP and LCP; checked on
    2^16 random ranks against the text, LCP[r] == PLCP[SA[r]] and PLCP[i] >= PLCP[i-1] - 1"""
    import torch
    n = 4_400_000_000
    free, _ = torch.cuda.mem_get_info(0)
    if free < 46 * n:
        pytest.skip("needs %d GB of free HBM" % (46 * n >> 30))
    t = synth.d1_uniform27(n)
    text_d = torch.from_numpy(t).to("cuda:0")
    sa_d = torch.empty(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    gpu.libsais64_device(text_d.data_ptr(), sa_d.data_ptr(), n)
    torch.cuda.empty_cache()
    out_d = torch.empty(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = gpu.plcp64_device(text_d.data_ptr(), sa_d.data_ptr(), out_d.data_ptr(), n)
    print("plcp64_device 4.4e9:", st)
    rng = np.random.default_rng(5)
    rs = torch.from_numpy(rng.integers(1, n, 1 << 16)).to("cuda:0")
    i_s = sa_d[rs]
    k_s = sa_d[rs - 1]
    plcp_at = out_d[i_s].cpu().numpy()
    i_h = i_s.cpu().numpy()
    k_h = k_s.cpu().numpy()
    prev = out_d[torch.clamp(i_s - 1, min=0)].cpu().numpy()
    for i, k, v, pv in zip(i_h, k_h, plcp_at, prev):
        m = n - max(int(i), int(k))
        a = t[int(i):int(i) + min(m, int(v) + 1)]
        b = t[int(k):int(k) + min(m, int(v) + 1)]
        assert np.array_equal(a[:v], b[:v]), (i, k, v)
        assert v == m or a[v] != b[v], (i, k, v)
        if i > 0:
            assert v >= pv - 1, (i, v, pv)
    del i_s, k_s
    st2 = gpu.lcp64_device(text_d.data_ptr(), sa_d.data_ptr(), out_d.data_ptr(), n)
    print("lcp64_device 4.4e9:", st2)
    assert np.array_equal(out_d[rs].cpu().numpy(), plcp_at)
    assert int((sa_d > 0xFFFFFFFF).sum().item()) == n - (1 << 32)
