"""LCP arrays without a GPU: every new entry point is declared, exported and bound; argument errors and n <= 1 are answered
on the host before any device call; and the test's own Kasai model (the independent check of tests/test_gpu_lcp.py) agrees
with the reference's libsais_plcp / libsais_lcp."""
import ctypes as C
import os
import re

import numpy as np

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_libsais_plcp", "sa_hip_libsais_plcp_omp", "sa_hip_libsais_lcp", "sa_hip_libsais_lcp_omp",
       "sa_hip_libsais64_plcp", "sa_hip_libsais64_plcp_omp", "sa_hip_libsais64_lcp", "sa_hip_libsais64_lcp_omp",
       "sa_hip_plcp64_device", "sa_hip_lcp64_device", "sa_hip_index_plcp_device", "sa_hip_index_lcp_device"]


def kasai_plcp(t, sa):
    """PLCP[i] = lcp(suffix i, its predecessor in SA order), 0 for SA[0] -- Kasai et al. 2001 in text order"""
    n = len(t)
    phi = np.full(n, -1, dtype=np.int64)
    if n:
        phi[sa[1:]] = sa[:-1]
    b = bytes(t)
    out = np.zeros(n, dtype=np.int64)
    h = 0
    for i in range(n):
        k = int(phi[i])
        if k < 0:
            h = 0
            continue
        m = n - max(i, k)
        while h < m and b[i + h] == b[k + h]:
            h += 1
        out[i] = h
        if h:
            h -= 1
    return out


def ref_plcp(ref, t, sa):
    L = ref.lib
    L.libsais_plcp.restype = C.c_int32
    L.libsais_plcp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    L.libsais_lcp.restype = C.c_int32
    L.libsais_lcp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    t = np.ascontiguousarray(t, dtype=np.uint8)
    s = np.ascontiguousarray(sa, dtype=np.int32)
    p = np.zeros(max(t.size, 1), np.int32)
    q = np.zeros(max(t.size, 1), np.int32)
    assert L.libsais_plcp(t.ctypes.data, s.ctypes.data, p.ctypes.data, t.size) == 0
    assert L.libsais_lcp(p.ctypes.data, s.ctypes.data, q.ctypes.data, t.size) == 0
    return p[:t.size], q[:t.size]


def test_lcp_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        fn = getattr(lib, name)   # exported by libsa_hip.so
        assert fn.argtypes is not None and fn.restype is not None, name
    assert "sa_hip_lcp_stats" in header
    names = [f for f, _ in capi.LcpStats._fields_]
    assert names[:6] == ["n", "tied", "compared_positions", "compared_bytes", "wave_compares", "split_compares"]
    assert C.sizeof(capi.LcpStats) == 6 * 8 + 2 * 4 + 6 * 8


def test_lcp_argument_errors_without_device(capi):
    lib = capi.lib()
    t = np.frombuffer(b"banana", np.uint8).copy()
    s32 = np.array([5, 3, 1, 0, 4, 2], np.int32)
    s64 = s32.astype(np.int64)
    o32 = np.zeros(6, np.int32)
    o64 = np.zeros(6, np.int64)
    p = lambda a: a.ctypes.data   # noqa: E731
    assert lib.sa_hip_libsais_plcp(None, p(s32), p(o32), 6) == -1
    assert lib.sa_hip_libsais_plcp(p(t), None, p(o32), 6) == -1
    assert lib.sa_hip_libsais_plcp(p(t), p(s32), None, 6) == -1
    assert lib.sa_hip_libsais_plcp(p(t), p(s32), p(o32), -1) == -1
    assert lib.sa_hip_libsais_plcp_omp(p(t), p(s32), p(o32), 6, -1) == -1
    assert lib.sa_hip_libsais_lcp(None, p(s32), p(o32), 6) == -1
    assert lib.sa_hip_libsais_lcp(p(o32), p(s32), p(o32), -5) == -1
    assert lib.sa_hip_libsais_lcp_omp(p(o32), p(s32), p(o32), 6, -2) == -1
    assert lib.sa_hip_libsais64_plcp(None, p(s64), p(o64), 6) == -1
    assert lib.sa_hip_libsais64_plcp(p(t), p(s64), p(o64), -1) == -1
    assert lib.sa_hip_libsais64_plcp_omp(p(t), p(s64), p(o64), 6, -1) == -1
    assert lib.sa_hip_libsais64_lcp(p(o64), None, p(o64), 6) == -1
    assert lib.sa_hip_libsais64_lcp_omp(p(o64), p(s64), p(o64), 6, -1) == -1
    assert lib.sa_hip_plcp64_device(None, None, None, -1, 0, None) == -1
    assert lib.sa_hip_lcp64_device(None, None, None, 5, 0, None) == -1
    assert lib.sa_hip_index_plcp_device(None, None, None) == -1
    assert lib.sa_hip_index_lcp_device(None, None, None) == -1
    assert b"NULL" in lib.sa_hip_last_error() or b"invalid" in lib.sa_hip_last_error()


def test_lcp_n_le_1_on_host(capi):
    """n <= 1 as in libsais (libsais.c:7869-7920): no device call, PLCP[0] = 0, LCP[0] = PLCP[SA[0]]"""
    lib = capi.lib()
    t = np.frombuffer(b"q", np.uint8).copy()
    s = np.zeros(1, np.int32)
    o = np.full(1, 7, np.int32)
    assert lib.sa_hip_libsais_plcp(t.ctypes.data, s.ctypes.data, o.ctypes.data, 1) == 0 and o[0] == 0
    pl = np.array([0], np.int32)
    o[0] = 9
    assert lib.sa_hip_libsais_lcp(pl.ctypes.data, s.ctypes.data, o.ctypes.data, 1) == 0 and o[0] == 0
    o[0] = 9
    assert lib.sa_hip_libsais_plcp(t.ctypes.data, s.ctypes.data, o.ctypes.data, 0) == 0 and o[0] == 9
    bad = np.array([3], np.int32)
    assert lib.sa_hip_libsais_lcp(pl.ctypes.data, bad.ctypes.data, o.ctypes.data, 1) == -1
    s64 = np.zeros(1, np.int64)
    o64 = np.full(1, 7, np.int64)
    assert lib.sa_hip_libsais64_plcp(t.ctypes.data, s64.ctypes.data, o64.ctypes.data, 1) == 0 and o64[0] == 0


def test_kasai_model_matches_reference(ref, capi):
    assert callable(capi.libsais_plcp) and callable(capi.libsais_lcp)   # the helpers this model judges on the GPU
    texts = cases.small_texts()
    texts["nul_ff"] = np.frombuffer(b"\x00\xff\x00\xff\xff\x00\x00\xff" * 50, np.uint8)
    for p in range(1, 18):
        texts["period%d" % p] = np.frombuffer((bytes(range(97, 97 + p)) * (2000 // p + 1))[:2000], np.uint8)
    done = 0
    for name, t in texts.items():
        if t.size > 70_000:
            continue
        sa = ref.libsais(t)
        p_ref, l_ref = ref_plcp(ref, t, sa)
        assert np.array_equal(kasai_plcp(t, sa), p_ref), name
        assert np.array_equal(l_ref, p_ref[sa] if t.size else l_ref), name
        done += 1
    assert done > 20
