"""BWT and inverse BWT on the device against the reference's libsais[64]_bwt[_aux] / _unbwt[_aux]
(oracle/_ref/libsa_ref.so), bit for bit, plus round trips: the drop-ins (host pointers, 32- and 64-bit), the handle API of
a built index, and the int64 device forms.  The inverse runs on its default plan, with tiny walk bounds and ruler spacing
(several ruler rounds and the ranking), and on the aux-only plan.  Then aliasing, input that is not a BWT, an SA entry out
of range, 1e8-character texts and 4.4e9 characters with 64-bit indices."""
import numpy as np
import pytest

import cases
from suffixarray_amd import synth
from test_bwt_cpu import model_bwt, ref_bwt, ref_unbwt

pytestmark = pytest.mark.gpu

PLANS = {
    "default": {},
    "rounds": {"SA_HIP_UNBWT_WALK": "8", "SA_HIP_UNBWT_RULER": "64"},          # many claims, several rounds, ranking
    "aux_only": {"SA_HIP_UNBWT_AUX_MIN": "1", "SA_HIP_UNBWT_WALK": "16"},      # aux rows as rulers, no ranking
}


def _env(monkeypatch, plan):
    for k in ("SA_HIP_UNBWT_WALK", "SA_HIP_UNBWT_RULER", "SA_HIP_UNBWT_AUX_MIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)


def bwt_texts():
    rng = np.random.default_rng(3)
    c = {"n0": np.zeros(0, np.uint8), "n1": np.frombuffer(b"x", np.uint8), "n2": np.frombuffer(b"xy", np.uint8),
         "n2_same": np.frombuffer(b"xx", np.uint8), "n3": np.frombuffer(b"aba", np.uint8)}
    c.update({k: v for k, v in cases.small_texts().items() if v.size <= 400_000})
    c["all_a"] = synth.all_same(30001)
    c["ab_periodic"] = synth.periodic(30000, 2)
    c["binary"] = rng.integers(0, 2, 40000).astype(np.uint8)
    c["bytes256"] = rng.permutation(np.tile(np.arange(256, dtype=np.uint8), 100))
    c["d1"] = synth.d1_uniform27(200_000)
    c["words"] = synth.d2_words(200_000)
    blk = rng.integers(0, 256, 4096, dtype=np.uint8)
    c["repeat_block"] = np.tile(blk, 40)
    return c


TEXTS = bwt_texts()
RS = (2, 4, 64, 1 << 12, 1 << 20)


@pytest.fixture(scope="module")
def expected(ref):
    out = {}
    for name, t in TEXTS.items():
        U, p, f = ref_bwt(ref, t)
        aux = {r: ref_bwt(ref, t, r=r)[1] for r in RS}
        out[name] = (U, p, f, aux)
    for name in ("banana", "n3", "all_a", "bytes256"):   # the model judges the reference too
        sa = ref.libsais(TEXTS[name])
        mU, mp, _ = model_bwt(TEXTS[name], sa)
        assert mp == out[name][1] and np.array_equal(mU, out[name][0]), name
    return out


@pytest.mark.parametrize("bits", [32, 64])
def test_bwt_dropins_match_reference(gpu, expected, bits):
    fwd = gpu.libsais_bwt if bits == 32 else gpu.libsais64_bwt
    for name, t in TEXTS.items():
        U, p, f, aux = expected[name]
        gU, gp, gf = fwd(t, freq=True)
        assert gp == p and np.array_equal(gU, U), (bits, name)
        assert np.array_equal(gf, f), (bits, name)
        for r in RS:
            aU, aI = fwd(t, r=r)
            assert np.array_equal(aU, U) and np.array_equal(aI, aux[r]), (bits, name, r)
    bd = gpu.last_call_breakdown()
    assert bd["n"] == t.size and bd["workspace_reused"] in (0, 1), bd
    assert bd["total_ms"] >= bd["build_ms"] >= 0, bd
    with pytest.raises(gpu.SaHipError):
        fwd(t, r=3)                       # r is not a power of two: rejected for its arguments
    assert gpu.last_call_breakdown() == bd


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("bits", [32, 64])
def test_unbwt_dropins_match_reference(gpu, ref, expected, monkeypatch, plan, bits):
    _env(monkeypatch, plan)
    inv = gpu.libsais_unbwt if bits == 32 else gpu.libsais64_unbwt
    rng = np.random.default_rng(1)
    for name, t in TEXTS.items():
        if t.size < 2:
            continue
        U, p, f, aux = expected[name]
        wrong = rng.integers(0, 1000, 256)
        for freq in (None, f, wrong):   # freq is never read: a wrong table changes nothing
            assert np.array_equal(inv(U, primary=p, freq=freq), t), (plan, bits, name)
        for r in RS:
            rc, back = ref_unbwt(ref, U, I=aux[r], r=r, bits=bits)
            assert rc == 0 and np.array_equal(back, t)
            assert np.array_equal(inv(U, I=aux[r], r=r), t), (plan, bits, name, r)
    bd = gpu.last_call_breakdown()
    assert bd["n"] == t.size and bd["workspace_reused"] in (0, 1), bd
    assert bd["total_ms"] >= bd["build_ms"] >= 0, bd
    for bad in (0, t.size + 1):           # an aux index outside (0, n]: rejected for its arguments
        with pytest.raises(gpu.SaHipError):
            inv(U, primary=bad)
        assert gpu.last_call_breakdown() == bd


def test_aliasing_u_is_t(gpu, expected):
    lib = gpu.lib()
    for name in ("mississippi", "d1", "repeat_block"):
        t = TEXTS[name]
        U, p, _, aux = expected[name]
        buf = t.copy()
        a = np.zeros(1, np.int32)
        assert lib.sa_hip_libsais_bwt(buf.ctypes.data, buf.ctypes.data, a.ctypes.data, buf.size, 0, None) == p
        assert np.array_equal(buf, U), name
        assert lib.sa_hip_libsais_unbwt(buf.ctypes.data, buf.ctypes.data, a.ctypes.data, buf.size, None, p) == 0
        assert np.array_equal(buf, t), name
        buf64 = t.copy()
        I = np.zeros((t.size - 1) // 64 + 1, np.int64)
        a64 = np.zeros(1, np.int64)
        assert lib.sa_hip_libsais64_bwt_aux(buf64.ctypes.data, buf64.ctypes.data, a64.ctypes.data, t.size, 0, None, 64, I.ctypes.data) == 0
        assert np.array_equal(buf64, U) and np.array_equal(I, aux[64])
        assert lib.sa_hip_libsais64_unbwt_aux(buf64.ctypes.data, buf64.ctypes.data, a64.ctypes.data, t.size, None, 64, I.ctypes.data) == 0
        assert np.array_equal(buf64, t), name


def test_handle_equals_dropin(gpu, expected):
    for name in ("banana", "n2", "all_a", "bytes256", "d1", "words", "repeat_block"):
        t = TEXTS[name]
        U, p, _, aux = expected[name]
        with gpu.DeviceIndex(t.size, 0) as idx:
            idx.build(t)
            gU, gp = idx.bwt()
            assert gp == p and np.array_equal(gU, U), name
            aU, aI = idx.bwt(r=4)
            assert np.array_equal(aU, U) and np.array_equal(aI, aux[4]), name


def test_truncated_handle_refused_then_full_build_works(gpu, expected):
    t = TEXTS["mississippi"]
    with gpu.DeviceIndex(t.size, 0) as idx:
        with pytest.raises(gpu.SaHipError):
            idx.bwt()                     # no index yet
        idx.build(t, 4)
        with pytest.raises(gpu.SaHipError) as e:
            idx.bwt()
        assert "truncated" in str(e.value)
        idx.build(t)
        U, p = idx.bwt()
        assert p == expected["mississippi"][1] and np.array_equal(U, expected["mississippi"][0])


def test_alphabet_code_widths_feed_the_bwt(gpu, ref):
    """4.5 M characters: the narrow and narrow48 build plans under the BWT, code widths 1-9"""
    for sig in (1, 2, 4, 16, 64, 128, 255, 256):
        alph = cases.alphabet(sig, "ends" if sig >= 255 else ("lo" if sig % 4 == 0 else "hi"))
        t = cases.alphabet_text(alph, 4_500_001, "binary" if sig in (2, 16, 255) else "uniform", 300 + sig)
        U, p, _ = ref_bwt(ref, t, threads=16)
        gU, gp = gpu.libsais_bwt(t)
        assert gp == p and np.array_equal(gU, U), sig
        assert np.array_equal(gpu.libsais_unbwt(U, primary=p), t), sig


def test_int64_device_forms(gpu, ref, expected, monkeypatch):
    import torch
    for plan in ("default", "rounds"):
        _env(monkeypatch, plan)
        for name in ("banana", "n2", "all_a", "bytes256", "d1", "words"):
            t = TEXTS[name]
            n = t.size
            U, p, _, aux = expected[name]
            text_d = torch.from_numpy(t.copy()).to("cuda:0")
            sa_d = torch.from_numpy(ref.libsais64(t)).to("cuda:0")
            u_d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            rc, st = gpu.bwt64_device(text_d.data_ptr(), sa_d.data_ptr(), u_d.data_ptr(), n)
            assert rc == p and np.array_equal(u_d.cpu().numpy(), U), name
            I_d = torch.zeros((n - 1) // 4 + 1, dtype=torch.int64, device="cuda:0")
            rc, _ = gpu.bwt64_device(text_d.data_ptr(), sa_d.data_ptr(), u_d.data_ptr(), n, r=4, I_ptr=I_d.data_ptr())
            assert rc == 0 and np.array_equal(I_d.cpu().numpy(), aux[4].astype(np.int64)), name
            out_d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
            P_d = torch.tensor([p], dtype=torch.int64, device="cuda:0")
            st = gpu.unbwt64_device(u_d.data_ptr(), out_d.data_ptr(), n, n, P_d.data_ptr())
            assert torch.equal(out_d, text_d), (plan, name, st)
            out_d.zero_()
            gpu.unbwt64_device(u_d.data_ptr(), out_d.data_ptr(), n, 4, I_d.data_ptr())
            assert torch.equal(out_d, text_d), (plan, name)
            # U over the text (forward) and the output over U (inverse)
            rc, _ = gpu.bwt64_device(text_d.data_ptr(), sa_d.data_ptr(), text_d.data_ptr(), n)
            assert rc == p and np.array_equal(text_d.cpu().numpy(), U)
            gpu.unbwt64_device(text_d.data_ptr(), text_d.data_ptr(), n, n, P_d.data_ptr())
            assert np.array_equal(text_d.cpu().numpy(), t), (plan, name)


def test_plans_and_stats(gpu, expected, monkeypatch):
    """the forced plans really ran: several ruler rounds with ranking, and the aux-only plan without"""
    import torch
    t = TEXTS["d1"]
    n = t.size
    U, p, _, aux = expected["d1"]
    u_d = torch.from_numpy(U.copy()).to("cuda:0")
    out_d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    P_d = torch.tensor([p], dtype=torch.int64, device="cuda:0")
    I_d = torch.from_numpy(aux[4].astype(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    _env(monkeypatch, "rounds")
    st = gpu.unbwt64_device(u_d.data_ptr(), out_d.data_ptr(), n, n, P_d.data_ptr())
    assert st["ruler_rounds"] >= 3 and st["rank_rounds"] > 0 and st["longest_walk"] <= 8 and not st["aux_only"], st
    assert np.array_equal(out_d.cpu().numpy(), t)
    _env(monkeypatch, "aux_only")
    out_d.zero_()
    st = gpu.unbwt64_device(u_d.data_ptr(), out_d.data_ptr(), n, 4, I_d.data_ptr())
    assert st["aux_only"] == 1 and st["rank_rounds"] == 0, st
    assert np.array_equal(out_d.cpu().numpy(), t)
    _env(monkeypatch, "default")
    out_d.zero_()
    st = gpu.unbwt64_device(u_d.data_ptr(), out_d.data_ptr(), n, n, P_d.data_ptr())
    assert not st["aux_only"] and st["rulers"] > 1 and st["longest_walk"] <= 2048, st
    assert np.array_equal(out_d.cpu().numpy(), t)


@pytest.mark.parametrize("plan", ["default", "rounds"])
def test_input_that_is_not_a_bwt_stays_in_bounds(gpu, ref, monkeypatch, plan):
    """random bytes and a random primary index: the reference's return code, a bounded time, untouched guard bytes"""
    import time
    import torch
    _env(monkeypatch, plan)
    rng = np.random.default_rng(9)
    for n in (2, 3, 1000, 100_000, 1_000_003):
        U = rng.integers(0, 256, n).astype(np.uint8)
        p = int(rng.integers(1, n + 1))
        rc_ref, _ = ref_unbwt(ref, U, primary=p)
        guard = 4096
        buf = torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
        u_d = torch.from_numpy(U).to("cuda:0")
        P_d = torch.tensor([p], dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        t0 = time.time()
        rc = gpu.lib().sa_hip_unbwt64_device(u_d.data_ptr(), buf.data_ptr() + guard, n, n, P_d.data_ptr(), 0, None)
        assert rc == rc_ref == 0 and time.time() - t0 < 30, (n, rc)
        g = buf.cpu().numpy()
        assert (g[:guard] == 0xA5).all() and (g[guard + n:] == 0xA5).all(), n
        got = gpu.libsais_unbwt(U, primary=p)     # the host drop-in as well
        assert got.size == n
        # aux rows that do not belong together
        r = 4
        I = rng.integers(1, n + 1, (n - 1) // r + 1)
        rc_ref, _ = ref_unbwt(ref, U, I=I, r=r)
        assert gpu.libsais_unbwt(U, I=I, r=r).size == n and rc_ref == 0


def test_sa_entry_out_of_range_then_next_call_works(gpu, ref, expected):
    import torch
    t = TEXTS["mississippi"]
    n = t.size
    text_d = torch.from_numpy(t.copy()).to("cuda:0")
    sa = ref.libsais64(t)
    bad = sa.copy()
    bad[3] = n + 5
    bad_d = torch.from_numpy(bad).to("cuda:0")
    u_d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = gpu.lib().sa_hip_bwt64_device(text_d.data_ptr(), bad_d.data_ptr(), u_d.data_ptr(), n, 0, None, 0, None)
    assert rc == -1 and b"out of range" in gpu.lib().sa_hip_last_error()
    bad[3] = -1
    bad_d = torch.from_numpy(bad).to("cuda:0")
    torch.cuda.synchronize()
    assert gpu.lib().sa_hip_bwt64_device(text_d.data_ptr(), bad_d.data_ptr(), u_d.data_ptr(), n, 0, None, 0, None) == -1
    sa_d = torch.from_numpy(sa).to("cuda:0")
    torch.cuda.synchronize()
    rc, _ = gpu.bwt64_device(text_d.data_ptr(), sa_d.data_ptr(), u_d.data_ptr(), n)
    assert rc == expected["mississippi"][1] and np.array_equal(u_d.cpu().numpy(), expected["mississippi"][0])


@pytest.mark.parametrize("kind", ["d1", "words"])
def test_1e8_equal_reference_omp(gpu, ref, kind):
    n = 100_000_000
    t = synth.d1_uniform27(n) if kind == "d1" else synth.d2_words(n)
    U, p, _ = ref_bwt(ref, t, threads=16)
    gU, gp = gpu.libsais_bwt(t)
    assert gp == p and np.array_equal(gU, U), kind
    rc, back = ref_unbwt(ref, U, primary=p, threads=16)
    assert rc == 0 and np.array_equal(back, t)
    assert np.array_equal(gpu.libsais_unbwt(U, primary=p), t), kind
    with gpu.DeviceIndex(n, 0) as idx:
        idx.build(t)
        hU, hp = idx.bwt()
        assert hp == p and np.array_equal(hU, U), kind


def test_4p4e9_int64_device_forms(gpu):
    """n > 2^32: libsais64_device -> bwt64_device -> unbwt64_device gives the text back on the device; 2^16 sampled ranks
    of U checked against T[SA[r]-1]"""
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
    u_d = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p, st = gpu.bwt64_device(text_d.data_ptr(), sa_d.data_ptr(), u_d.data_ptr(), n)
    print("bwt64_device 4.4e9:", st)
    assert 1 <= p <= n
    rng = np.random.default_rng(5)
    rs = torch.from_numpy(rng.integers(0, n, 1 << 16)).to("cuda:0")
    s = sa_d[rs]
    q = rs + (rs < p - 1).to(torch.int64)
    keep = s != 0
    assert torch.equal(u_d[q[keep]], text_d[s[keep] - 1])
    assert int(u_d[0].item()) == int(t[-1])
    del sa_d, s, q, rs
    torch.cuda.empty_cache()
    out_d = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    P_d = torch.tensor([p], dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = gpu.unbwt64_device(u_d.data_ptr(), out_d.data_ptr(), n, n, P_d.data_ptr())
    print("unbwt64_device 4.4e9:", st)
    assert torch.equal(out_d, text_d)
