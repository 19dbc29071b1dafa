"""The LCP kernels (csrc/lcp.hpp) at their hand-off depths: the case lists of tests/lcp_cases.py under the knob setting each
was made for, through the drop-ins, the int64 device forms, the handle API and the integer-symbol forms.  Arrays are compared
exactly with the model's (tests/test_lcp_cases_cpu.py checks the model and that the lists reach the edges), and the stage
counters with the phase model's: a phase that hands everything on, or closes what is not its own, changes them.  Then output
pointers off the 16-byte grid, and the tile scan's carry beyond 2^24 positions."""
import ctypes as C

import numpy as np
import pytest

import lcp_cases as lc

pytestmark = pytest.mark.gpu

BYTE = lc.byte_lists()
INT = lc.int_lists()
COUNTERS = ("compared_positions", "wave_compares", "split_compares", "split_rounds")
GUARD = -0x5A5A5A5B


@pytest.fixture(scope="module")
def solved(oracle):
    out = {}
    for c in lc.all_cases():
        sa, plcp = lc.solve(c.text, oracle)
        out[c.name] = (sa, plcp, lc.classify(c.text, sa, plcp, lc.case_edges(c), c.sym_bytes))
    return out


def _env(monkeypatch, knobs, keys=True):
    for k in ("SA_HIP_LCP_KEYS", "SA_HIP_LCP_LANE_BYTES", "SA_HIP_LCP_WAVE_BYTES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in lc.knob_env(knobs).items():
        monkeypatch.setenv(k, v)
    if not keys:
        monkeypatch.setenv("SA_HIP_LCP_KEYS", "0")


def _model_counters(ph):
    return {k: getattr(ph, k) for k in COUNTERS}


def _got_counters(st):
    return {k: st[k] for k in COUNTERS}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


@pytest.mark.parametrize("knobs", list(BYTE))
def test_dropins(gpu, solved, monkeypatch, knobs):
    _env(monkeypatch, knobs)
    for c in BYTE[knobs]:
        sa, plcp, _ = solved[c.name]
        got = gpu.libsais_plcp(c.text, sa)
        assert got.dtype == np.int32 and np.array_equal(got, plcp), c.name
        got = gpu.libsais64_plcp(c.text, sa)
        assert got.dtype == np.int64 and np.array_equal(got, plcp), c.name


@pytest.mark.parametrize("knobs", list(BYTE))
def test_int64_device_forms_and_counters(gpu, solved, monkeypatch, knobs):
    import torch
    _env(monkeypatch, knobs)
    for c in BYTE[knobs]:
        sa, plcp, ph = solved[c.name]
        n = c.text.size
        text_d, sa_d = _dev(c.text), _dev(sa)
        out_d = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        st = gpu.plcp64_device(text_d.data_ptr(), sa_d.data_ptr(), out_d.data_ptr(), n)
        assert np.array_equal(out_d.cpu().numpy(), plcp), c.name
        print(c.name, "plcp64_device", _got_counters(st), "model", _model_counters(ph))
        assert _got_counters(st) == _model_counters(ph) and st["tied"] == 0 and st["keys"] == 0, (c.name, st)
        st = gpu.lcp64_device(text_d.data_ptr(), sa_d.data_ptr(), out_d.data_ptr(), n)
        assert np.array_equal(out_d.cpu().numpy(), plcp[sa]), c.name
        assert _got_counters(st) == _model_counters(ph), (c.name, st)


@pytest.mark.parametrize("knobs", list(BYTE))
def test_handle_keyed_and_unkeyed(gpu, solved, monkeypatch, knobs):
    """the key depth of an index is not exposed: one k in 1..64 must give the model's tied and compared_positions, and with
    that k the wave and split counts as well; without the key shortcut the counters are those of the plain forms"""
    import torch
    for c in BYTE[knobs]:
        sa, plcp, ph = solved[c.name]
        n = c.text.size
        buf = torch.empty(n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        with gpu.DeviceIndex(n, 0) as idx:
            idx.build(c.text)
            assert np.array_equal(idx.sa_u32(), sa.astype(np.uint32)), c.name
            for keys in (True, False):
                _env(monkeypatch, knobs, keys)
                for what, want in (("plcp", plcp), ("lcp", plcp[sa])):
                    st = getattr(idx, what + "_device")(buf.data_ptr(), stats=True)
                    assert np.array_equal(buf.cpu().numpy(), want), (c.name, what, keys)
                    if not st["keys"]:
                        assert _got_counters(st) == _model_counters(ph) and st["tied"] == 0, (c.name, what, st)
                        continue
                    fit = [k for k in range(1, 65) if lc.keyed_counts(plcp, sa, ph.plcp, k) == (st["tied"], st["compared_positions"])]
                    print(c.name, what, "tied", st["tied"], "positions", st["compared_positions"], "key depths that fit", fit)
                    assert fit, (c.name, what, st)
                    models = [_model_counters(lc.classify(c.text, sa, plcp, lc.case_edges(c, k0=k), 1)) for k in fit]
                    assert _got_counters(st) in models, (c.name, what, st, models)


def _int_variants(c, solved, oracle):
    """the case as it is (n is even: read in place), without its first symbol (odd n, handed over 4 bytes into an
    allocation) and without its last (odd n, aligned): the padded copy for either reason"""
    sa, plcp, ph = solved[c.name]
    assert c.text.size % 2 == 0
    yield c.text, sa, plcp, ph, 0
    for t, skip in ((c.text[1:], 1), (c.text[:-1], 0)):
        sa_t, plcp_t = lc.solve(t, oracle)
        assert not skip or np.array_equal(sa_t, sa[sa > 0] - 1)
        yield t, sa_t, plcp_t, lc.classify(t, sa_t, plcp_t, lc.case_edges(c, n=t.size), 4), skip


@pytest.mark.parametrize("knobs", list(INT))
def test_integer_symbols(gpu, solved, oracle, monkeypatch, knobs):
    import torch
    _env(monkeypatch, knobs)
    parities = set()
    for c in INT[knobs]:
        whole = _dev(c.text)
        for t, sa, plcp, ph, skip in _int_variants(c, solved, oracle):
            n = t.size
            assert np.array_equal(gpu.libsais_plcp_int(t, sa), plcp), (c.name, skip)
            sa_d = _dev(sa.astype(np.int32))
            out_d = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            ptr = whole.data_ptr() + 4 * skip
            assert ptr % 8 == 4 * skip
            st = gpu.plcp_int_device(ptr, sa_d.data_ptr(), out_d.data_ptr(), n)
            assert np.array_equal(out_d.cpu().numpy(), plcp), (c.name, skip)
            assert _got_counters(st) == _model_counters(ph), (c.name, skip, st, _model_counters(ph))
            parities.add((n & 1, skip))
    assert parities == {(0, 0), (1, 1), (1, 0)}, parities


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_output_off_the_16_byte_grid(gpu, solved, monkeypatch, offset):
    """lcp_scan_apply_kernel stores 16 bytes at a time only into an aligned output"""
    import torch
    _env(monkeypatch, "default")
    pad = 8
    for c in BYTE["default"][-len(lc.TILE_SIZES):] + BYTE["small"][:1]:
        sa, plcp, _ = solved[c.name]
        n = c.text.size
        text_d, sa_d = _dev(c.text), _dev(sa)
        big = torch.full((n + 2 * pad,), GUARD, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        assert big.data_ptr() % 16 == 0
        gpu.plcp64_device(text_d.data_ptr(), sa_d.data_ptr(), big.data_ptr() + 8 * offset, n)
        got = big.cpu().numpy()
        assert np.array_equal(got[offset:offset + n], plcp), (c.name, offset)
        assert (got[:offset] == GUARD).all() and (got[offset + n:] == GUARD).all(), (c.name, offset)
        big32 = torch.full((n + 2 * pad,), GUARD, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        with gpu.DeviceIndex(n, 0) as idx:
            idx.build(c.text)
            idx.plcp_device(big32.data_ptr() + 4 * offset, stats=True)
        got = big32.cpu().numpy()
        assert np.array_equal(got[offset:offset + n], plcp), (c.name, offset)
        assert (got[:offset] == GUARD).all() and (got[offset + n:] == GUARD).all(), (c.name, offset)


# ---- the tile scan's carry: n > 2^24 --------------------------------------------------------------------------------------
def _ref_sa_plcp(ref, t):
    L = ref.lib
    L.libsais_plcp_omp.restype = C.c_int32
    L.libsais_plcp_omp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    sa = ref.libsais(t, threads=16)
    p = np.zeros(t.size, np.int32)
    from oracle.oracle import usable_threads
    assert L.libsais_plcp_omp(t.ctypes.data, sa.ctypes.data, p.ctypes.data, t.size, usable_threads()) == 0
    return sa, p


@pytest.fixture(scope="module")
def scan_carry(ref):
    out = []
    for start in lc.SCAN_CARRY_STARTS:
        t = lc.scan_carry_text(start)
        sa, p = _ref_sa_plcp(ref, t)
        out.append((start, t, sa, p))
    return out


def test_scan_carry_beyond_2_24_positions(gpu, scan_carry):
    import torch
    for start, t, sa, p in scan_carry:
        n = t.size
        lo, hi = (1 << 24) - 3100, (1 << 24) + 3100
        window = lc.plcp_window(t, sa, lo, hi)
        assert np.array_equal(window, p[lo:hi]) and window[start - lo] >= min(lc.SCAN_CARRY_COPY, n - 1 - start) and window[(1 << 24) - lo] > 1000, start
        got = gpu.libsais_plcp(t, sa)
        assert np.array_equal(got[lo:hi], window), start
        assert np.array_equal(got, p), start
        text_d, sa_d = _dev(t), _dev(sa.astype(np.int64))
        out_d = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        gpu.plcp64_device(text_d.data_ptr(), sa_d.data_ptr(), out_d.data_ptr(), n)
        got = out_d.cpu().numpy()
        assert np.array_equal(got[lo:hi], window), start
        assert np.array_equal(got, p), start
