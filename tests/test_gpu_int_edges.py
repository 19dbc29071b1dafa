"""The integer-alphabet build (csrc/int_build.hpp, int_core in csrc/capi_dropins.hpp) at the edges of its plan: n against the
key and against the keygen's tile and halo, the code width on both sides of every power of two it can cross, the 64-bit-wide
key, the rank table's cap and its scan's tiles, the route switch, and the refusal's "first position".

BigBuilder::build_with repairs by prefix doubling whatever the initial key leaves undecided, so a code one bit too wide, a key
one symbol short or a halo one code short still ends in the right suffix array.  Every build here is therefore compared twice:
the array with test_int_cpu.model_sa (and with the reference where it is built), and the stats with tests/int_cases.py --
plan, compacted, sigma, min_symbol, max_symbol against plan(); on route B bits_per_symbol, symbols_per_key, tied_after_sort,
rounds, tied_total and sort_passes against rounds_model().  All comparisons are equalities."""
import numpy as np
import pytest

import int_cases as ic
from test_int_cases_cpu import sa_of
from test_int_cpu import model_sa, rank_remap, ref_long

pytestmark = pytest.mark.gpu


def _env(monkeypatch, plan):
    for k in ic.KNOB_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in ic.PLANS[plan].items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def ref_or_none():
    from oracle.oracle import Ref
    return Ref() if Ref.available() else None


def device_build(gpu, t, dtype, k):
    """the device form of the width on torch buffers, SA prefilled: -> (array, stats, T read back, sufcheck or None)"""
    import torch
    n = int(t.size)
    t_d = torch.from_numpy(np.ascontiguousarray(t.astype(dtype))).to("cuda:0")
    sa_d = torch.full((n,), -7, dtype=torch.int32 if dtype == np.int32 else torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    if dtype == np.int32:
        st = gpu.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), n, k)
        bad = None
    else:
        st = gpu.libsais64_long_device(t_d.data_ptr(), sa_d.data_ptr(), n, k)
        bad = gpu.sufcheck_long_device(t_d.data_ptr(), sa_d.data_ptr(), n)
    return sa_d.cpu().numpy(), st, t_d.cpu().numpy(), bad


STAT_KEYS = ("tied_after_sort", "rounds", "tied_total", "sort_passes")


@pytest.mark.parametrize("name", [c.name for c in ic.all_cases()])
def test_every_plan_and_width(gpu, ref_or_none, monkeypatch, name):
    c = ic.case(name)
    want = sa_of(name)
    if ref_or_none is not None:
        r, sigma = rank_remap(c.text)
        assert np.array_equal(ref_long(ref_or_none, r, sigma), want), name
    for pn, (b, s, route, compacted) in c.expect.items():
        p = ic.plan(c.text, ic.knobs(pn))
        assert (p["bits"], p["s"], p["route"], p["compacted"]) == (b, s, route, compacted), (name, pn, p)
        model = ic.rounds_model(c.text, want, p) if route == "B" else None
        for dtype in c.dtypes:
            tag = (name, pn, np.dtype(dtype).name)
            _env(monkeypatch, pn)
            sa, st, t_back, bad = device_build(gpu, c.text, dtype, c.k)
            print(name, pn, np.dtype(dtype).name, "route", route, "b x s %d x %d" % (st["bits_per_symbol"], st["symbols_per_key"]),
                  "| measured", [st[x] for x in STAT_KEYS], "model", [model[x] for x in STAT_KEYS] if model else "-")
            assert np.array_equal(sa, want.astype(dtype)), (tag, st, int(np.flatnonzero(sa != want)[0]))
            assert np.array_equal(t_back, c.text.astype(dtype)), tag
            assert bad in (None, 0), (tag, st)
            assert st["n"] == c.text.size and st["plan"] == (0 if route == "A" else 1), (tag, st)
            assert st["compacted"] == p["compacted"] and st["sigma"] == p["sigma"], (tag, st, p)
            assert st["min_symbol"] == p["min"] and st["max_symbol"] == p["max"], (tag, st, p)
            if route == "B":
                assert st["bits_per_symbol"] == b and st["symbols_per_key"] == s, (tag, st, p)
                assert {x: st[x] for x in STAT_KEYS} == {x: model[x] for x in STAT_KEYS}, (tag, st, model)


@pytest.mark.parametrize("name", ic.DROPIN_CASES)
def test_host_dropins(gpu, monkeypatch, name):
    """sa_hip_libsais_int / sa_hip_libsais64_long and one _omp call with fs = 3: the array, SA[n .. n + fs) and T untouched"""
    lib = gpu.lib()
    c = ic.case(name)
    want = sa_of(name)
    n = int(c.text.size)
    _env(monkeypatch, next(iter(c.expect)))
    for dtype in c.dtypes:
        f, fo = ((lib.sa_hip_libsais_int, lib.sa_hip_libsais_int_omp) if dtype == np.int32 else
                 (lib.sa_hip_libsais64_long, lib.sa_hip_libsais64_long_omp))
        t = np.ascontiguousarray(c.text.astype(dtype))
        for fs, call in ((0, lambda sa: f(t.ctypes.data, sa.ctypes.data, n, c.k, 0)),
                         (3, lambda sa: fo(t.ctypes.data, sa.ctypes.data, n, c.k, 3, 2))):
            sa = np.full(n + 3, -7, dtype)
            assert call(sa) == 0, (name, dtype, fs, lib.sa_hip_last_error().decode())
            assert np.array_equal(sa[:n], want.astype(dtype)) and (sa[n:] == -7).all(), (name, dtype, fs)
            assert np.array_equal(t, c.text.astype(dtype)), (name, dtype, fs)


@pytest.mark.parametrize("name", [r.name for r in ic.refusal_cases()])
def test_refusals_name_the_first_bad_position(gpu, name):
    """a symbol outside [0, k): -1 and "T[p] = v" with the smallest such p, from the drop-in and from the device form of
    both widths; the same calls on the text without the bad symbols work right after"""
    import torch
    lib = gpu.lib()
    r = next(x for x in ic.refusal_cases() if x.name == name)
    good = next(x for x in ic.refusal_cases() if x.name == "k_is_max_plus_1")
    good_sa = _good_sa()
    n = int(r.text.size)
    pos = ic.first_bad(r.text, r.k)
    for dtype in r.dtypes:
        f, fd, tdt = ((lib.sa_hip_libsais_int, lib.sa_hip_libsais_int_device, torch.int32) if dtype == np.int32 else
                      (lib.sa_hip_libsais64_long, lib.sa_hip_libsais64_long_device, torch.int64))
        for text, k, p in ((r.text, r.k, pos), (good.text, good.k, None)):
            t = np.ascontiguousarray(text.astype(dtype))
            msg = None if p is None else "T[%d] = %d, k = %d" % (p, int(text[p]), k)
            sa = np.full(n, -7, dtype)
            rc = f(t.ctypes.data, sa.ctypes.data, n, k, 0)
            t_d = torch.from_numpy(t).to("cuda:0")
            sa_d = torch.full((n,), -7, dtype=tdt, device="cuda:0")
            torch.cuda.synchronize()
            if p is None:
                assert rc == 0 and np.array_equal(sa, good_sa.astype(dtype)), (name, dtype)
                assert fd(t_d.data_ptr(), sa_d.data_ptr(), n, k, 0, None) == 0, (name, dtype)
                assert np.array_equal(sa_d.cpu().numpy(), good_sa.astype(dtype)), (name, dtype)
            else:
                assert rc == -1 and msg in lib.sa_hip_last_error().decode(), (name, dtype, msg, lib.sa_hip_last_error().decode())
                assert fd(t_d.data_ptr(), sa_d.data_ptr(), n, k, 0, None) == -1, (name, dtype)
                assert msg in lib.sa_hip_last_error().decode(), (name, dtype, msg, lib.sa_hip_last_error().decode())
            assert np.array_equal(t_d.cpu().numpy(), t), (name, dtype)


_GOOD = []


def _good_sa():
    if not _GOOD:
        _GOOD.append(model_sa(next(x for x in ic.refusal_cases() if x.name == "k_is_max_plus_1").text))
    return _GOOD[0]
