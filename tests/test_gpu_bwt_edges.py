"""The BWT kernels (csrc/bwt.hpp) at their edges: the texts of tests/bwt_cases.py -- primary index and n around the 16-byte
output groups and the 4096-byte tiles, alphabets with empty buckets -- through every forward form, plain and with aux rows,
and through the inverse under every plan, whose walk and ranking counts are compared exactly with the ruler model's
(tests/test_bwt_cases_cpu.py checks the model and that the plans reach what they are named for).  Then U and the inverse's
output at byte offsets off the 16- and 8-byte grids, inside guarded buffers."""
import numpy as np
import pytest

import bwt_cases as bc
from test_bwt_cpu import model_bwt

pytestmark = pytest.mark.gpu

TEXTS = bc.all_texts()
GUARD = 0xA5
PAD = 64
STATS = ("rulers", "ruler_rounds", "longest_walk", "rank_rounds", "aux_only")


def _rs(n):
    return (2, 16, bc.next_pow2(n))


@pytest.fixture(scope="module")
def expected(oracle):
    """name -> (sa, U, primary, freq, {r: I})"""
    out = {}
    for name, t in TEXTS.items():
        sa = oracle.sais(t).astype(np.int64)
        U, p, _ = model_bwt(t, sa)
        out[name] = (sa, U, p, np.bincount(t, minlength=256), {r: model_bwt(t, sa, r)[2] for r in set(_rs(t.size)) | {4, 8, 64, 128, 256}})
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def _env(monkeypatch, plan):
    for k in ("SA_HIP_UNBWT_WALK", "SA_HIP_UNBWT_RULER", "SA_HIP_UNBWT_AUX_MIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in bc.PLANS[plan].items():
        monkeypatch.setenv(k, v)


# ---- forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_forward_dropins(gpu, expected, bits):
    fwd = gpu.libsais_bwt if bits == 32 else gpu.libsais64_bwt
    for name, t in TEXTS.items():
        sa, U, p, f, aux = expected[name]
        gU, gp, gf = fwd(t, freq=True)
        assert gp == p and np.array_equal(gU, U) and np.array_equal(gf, f), (bits, name, gp, p)
        for r in _rs(t.size):
            aU, aI = fwd(t, r=r)
            assert np.array_equal(aU, U) and np.array_equal(aI, aux[r]), (bits, name, r)


def test_forward_int64_device_form(gpu, expected):
    import torch
    for name, t in TEXTS.items():
        sa, U, p, f, aux = expected[name]
        n = t.size
        text_d, sa_d = _dev(t), _dev(sa)
        u_d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        rc, _ = gpu.bwt64_device(text_d.data_ptr(), sa_d.data_ptr(), u_d.data_ptr(), n)
        assert rc == p and np.array_equal(u_d.cpu().numpy(), U), (name, rc, p)
        for r in _rs(n):
            I_d = torch.zeros((n - 1) // r + 1, dtype=torch.int64, device="cuda:0")
            u_d.zero_()
            torch.cuda.synchronize()
            rc, _ = gpu.bwt64_device(text_d.data_ptr(), sa_d.data_ptr(), u_d.data_ptr(), n, r=r, I_ptr=I_d.data_ptr())
            assert rc == 0 and np.array_equal(u_d.cpu().numpy(), U) and np.array_equal(I_d.cpu().numpy(), aux[r]), (name, r)


def test_forward_handle(gpu, expected):
    import torch
    for name, t in TEXTS.items():
        sa, U, p, f, aux = expected[name]
        n = t.size
        with gpu.DeviceIndex(n, 0) as idx:
            idx.build(t)
            u_d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            assert idx.bwt_device(u_d.data_ptr()) == p and np.array_equal(u_d.cpu().numpy(), U), name
            for r in _rs(n):
                I_d = torch.zeros((n - 1) // r + 1, dtype=torch.int32, device="cuda:0")
                u_d.zero_()
                torch.cuda.synchronize()
                idx.bwt_device(u_d.data_ptr(), r, I_d.data_ptr())
                assert np.array_equal(u_d.cpu().numpy(), U) and np.array_equal(I_d.cpu().numpy(), aux[r]), (name, r)


@pytest.mark.parametrize("offset", [1, 7, 8, 15])
def test_forward_u_off_the_16_byte_grid(gpu, expected, offset):
    """bwt_gather_kernel stores 16 bytes at a time only into an aligned U"""
    import torch
    for name, t in TEXTS.items():
        sa, U, p, f, aux = expected[name]
        n = t.size
        text_d, sa_d = _dev(t), _dev(sa)
        for form in ("bwt64_device", "handle"):
            if form == "handle" and n > 33 and n % 4096 > 1:   # an index build per text: the sizes on the group and tile edges
                continue
            buf = torch.full((n + 2 * PAD,), GUARD, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            ptr = buf.data_ptr() + PAD + offset
            assert (buf.data_ptr() + PAD) % 16 == 0
            if form == "handle":
                with gpu.DeviceIndex(n, 0) as idx:
                    idx.build(t)
                    got_p = idx.bwt_device(ptr)
            else:
                got_p, _ = gpu.bwt64_device(text_d.data_ptr(), sa_d.data_ptr(), ptr, n)
            got = buf.cpu().numpy()
            lo = PAD + offset
            assert got_p == p and np.array_equal(got[lo:lo + n], U), (name, form, offset)
            assert (got[:lo] == GUARD).all() and (got[lo + n:] == GUARD).all(), (name, form, offset)


# ---- inverse ----------------------------------------------------------------------------------------------------------------
def _aux(expected, name, r):
    sa, U, p, f, aux = expected[name]
    return np.array([p], np.int64) if r is None else aux[r]


@pytest.mark.parametrize("plan", list(bc.PLANS))
def test_inverse_int64_device_form_and_counts(gpu, expected, monkeypatch, plan):
    import torch
    _env(monkeypatch, plan)
    knobs = bc.plan_knobs(plan)
    for name, r in bc.plan_runs(plan):
        t = TEXTS[name]
        n = t.size
        U = expected[name][1]
        I = _aux(expected, name, r)
        sim = bc.simulate(U, I, r or n, **knobs)
        u_d, I_d = _dev(U), _dev(I.astype(np.int64))
        out_d = torch.full((n,), GUARD, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        st = gpu.unbwt64_device(u_d.data_ptr(), out_d.data_ptr(), n, r or n, I_d.data_ptr())
        assert np.array_equal(out_d.cpu().numpy(), t), (plan, name, r, st)
        assert {k: st[k] for k in STATS} == {k: getattr(sim, k) for k in STATS}, (plan, name, r, st, sim)


@pytest.mark.parametrize("plan", list(bc.PLANS))
@pytest.mark.parametrize("bits", [32, 64])
def test_inverse_dropins(gpu, expected, monkeypatch, plan, bits):
    _env(monkeypatch, plan)
    inv = gpu.libsais_unbwt if bits == 32 else gpu.libsais64_unbwt
    for name, r in bc.plan_runs(plan):
        sa, U, p, f, aux = expected[name]
        got = inv(U, primary=p) if r is None else inv(U, I=aux[r], r=r)
        assert np.array_equal(got, TEXTS[name]), (plan, bits, name, r)


@pytest.mark.parametrize("plan", ["default", "aux_only_8", "aux_only_16", "one_ruler"])
@pytest.mark.parametrize("offset", [1, 4, 7, 9])
def test_inverse_out_off_the_8_byte_grid(gpu, expected, monkeypatch, plan, offset):
    """Writer stores 8 bytes at a time only into an aligned output, and only words wholly inside a walk's span"""
    import torch
    _env(monkeypatch, plan)
    names = [x for x in bc.inverse_names() if TEXTS[x].size <= 33 or TEXTS[x].size % 4096 == 1]
    for name, r in bc.plan_runs(plan, names):
        if r not in (None, 2, 16, 64):
            continue
        t = TEXTS[name]
        n = t.size
        u_d, I_d = _dev(expected[name][1]), _dev(_aux(expected, name, r).astype(np.int64))
        buf = torch.full((n + 2 * PAD,), GUARD, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert (buf.data_ptr() + PAD) % 16 == 0
        gpu.unbwt64_device(u_d.data_ptr(), buf.data_ptr() + PAD + offset, n, r or n, I_d.data_ptr())
        got = buf.cpu().numpy()
        lo = PAD + offset
        assert np.array_equal(got[lo:lo + n], t), (plan, name, r, offset)
        assert (got[:lo] == GUARD).all() and (got[lo + n:] == GUARD).all(), (plan, name, r, offset)
