"""BWT / inverse BWT without a GPU: every new entry point is declared, exported and bound, BwtStats matches the header;
argument errors and n <= 1 are answered on the host before any device call; and the test's own NumPy model (BWT from the
suffix array, inverse by an LF walk -- the independent check of tests/test_gpu_bwt.py) agrees with the reference's
libsais_bwt / _bwt_aux / _unbwt / _unbwt_aux."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_libsais_bwt", "sa_hip_libsais_bwt_omp", "sa_hip_libsais_bwt_aux", "sa_hip_libsais_bwt_aux_omp",
       "sa_hip_libsais_unbwt", "sa_hip_libsais_unbwt_omp", "sa_hip_libsais_unbwt_aux", "sa_hip_libsais_unbwt_aux_omp",
       "sa_hip_libsais64_bwt", "sa_hip_libsais64_bwt_omp", "sa_hip_libsais64_bwt_aux", "sa_hip_libsais64_bwt_aux_omp",
       "sa_hip_libsais64_unbwt", "sa_hip_libsais64_unbwt_omp", "sa_hip_libsais64_unbwt_aux", "sa_hip_libsais64_unbwt_aux_omp",
       "sa_hip_bwt64_device", "sa_hip_unbwt64_device", "sa_hip_index_bwt_device"]


# ---- the model -----------------------------------------------------------------------------------------------------------
def model_bwt(t, sa, r=None):
    """(U, primary, I): U[0] = T[n-1], then T[SA[q]-1] for every rank q with SA[q] != 0; primary = ISA[0] + 1;
    I[t] = ISA[t r] + 1"""
    t = np.asarray(t, np.uint8)
    sa = np.asarray(sa, np.int64)
    n = t.size
    isa = np.empty(n, np.int64)
    isa[sa] = np.arange(n)
    p = int(isa[0])
    U = np.empty(n, np.uint8)
    U[0] = t[n - 1]
    q = np.arange(n)
    keep = sa != 0
    U[(q + (q < p))[keep]] = t[sa[keep] - 1]
    I = isa[np.arange(0, n, r)] + 1 if r else None
    return U, p + 1, I


def model_unbwt(U, primary):
    """LF walk over the n + 1 rows of the matrix: L = U with '$' inserted at row `primary`; '$' sorts first"""
    U = np.asarray(U, np.uint8)
    n = U.size
    L = np.concatenate([U[:primary].astype(np.int64), [-1], U[primary:].astype(np.int64)])
    order = np.argsort(L, kind="stable")          # F column: rank f holds the row order[f]
    lf = np.empty(n + 1, np.int64)
    lf[order] = np.arange(n + 1)
    out = np.empty(n, np.uint8)
    j = 0                                         # row of the suffix "$" (text position n)
    for k in range(n - 1, -1, -1):
        out[k] = L[j]
        j = lf[j]
    return out


# ---- the reference through ctypes ----------------------------------------------------------------------------------------
def bind_ref(ref):
    L = ref.lib
    vp = C.c_void_p
    for pre, it in (("libsais", C.c_int32), ("libsais64", C.c_int64)):
        for sfx, args in (("_bwt", [vp, vp, vp, it, it, vp]), ("_bwt_aux", [vp, vp, vp, it, it, vp, it, vp]),
                          ("_unbwt", [vp, vp, vp, it, vp, it]), ("_unbwt_aux", [vp, vp, vp, it, vp, it, vp])):
            getattr(L, pre + sfx).restype = it
            getattr(L, pre + sfx).argtypes = args
            getattr(L, pre + sfx + "_omp").restype = it
            getattr(L, pre + sfx + "_omp").argtypes = args + [it]
    return L


def ref_bwt(ref, t, r=None, threads=1, bits=32):
    """(U, primary or I, freq) from the reference's libsais[64]_bwt[_aux][_omp]"""
    L = bind_ref(ref)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    n = t.size
    it = np.int32 if bits == 32 else np.int64
    pre = "libsais" if bits == 32 else "libsais64"
    U = np.zeros(max(n, 1), np.uint8)
    A = np.zeros(max(n, 1) + 1, it)
    f = np.zeros(256, it)
    om = "_omp" if threads != 1 else ""
    extra = (threads,) if threads != 1 else ()
    if r:
        I = np.zeros((n - 1) // r + 1 if n else 1, it)
        rc = getattr(L, pre + "_bwt_aux" + om)(t.ctypes.data, U.ctypes.data, A.ctypes.data, n, 0, f.ctypes.data, r, I.ctypes.data, *extra)
        assert rc == 0, rc
        return U[:n], I, f
    rc = getattr(L, pre + "_bwt" + om)(t.ctypes.data, U.ctypes.data, A.ctypes.data, n, 0, f.ctypes.data, *extra)
    assert rc >= 0, rc
    return U[:n], int(rc), f


def ref_unbwt(ref, U, primary=None, I=None, r=None, threads=1, bits=32):
    """(return code, text) from the reference's libsais[64]_unbwt[_aux][_omp] (freq NULL)"""
    L = bind_ref(ref)
    U = np.ascontiguousarray(U, dtype=np.uint8)
    n = U.size
    it = np.int32 if bits == 32 else np.int64
    pre = "libsais" if bits == 32 else "libsais64"
    out = np.zeros(max(n, 1), np.uint8)
    A = np.zeros(max(n, 1) + 1, it)
    om = "_omp" if threads != 1 else ""
    extra = (threads,) if threads != 1 else ()
    if I is None:
        rc = getattr(L, pre + "_unbwt" + om)(U.ctypes.data, out.ctypes.data, A.ctypes.data, n, None, int(primary), *extra)
    else:
        Ia = np.ascontiguousarray(I, dtype=it)
        rc = getattr(L, pre + "_unbwt_aux" + om)(U.ctypes.data, out.ctypes.data, A.ctypes.data, n, None, int(r), Ia.ctypes.data, *extra)
    return int(rc), out[:n]


# ---- tests -----------------------------------------------------------------------------------------------------------------
def test_bwt_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is not None, name
    for name in ("libsais_bwt", "libsais64_bwt", "libsais_unbwt", "libsais64_unbwt", "bwt64_device", "unbwt64_device"):
        assert callable(getattr(capi, name)), name
    assert callable(capi.DeviceIndex.bwt) and callable(capi.DeviceIndex.bwt_device)


def test_bwt_stats_layout_matches_header(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    body = re.search(r"typedef struct sa_hip_bwt_stats \{(.*?)\} sa_hip_bwt_stats;", header, re.S).group(1)
    fields = re.findall(r"^\s*(uint64_t|uint32_t|double)\s+(\w+);", body, re.M)
    size = {"uint64_t": 8, "uint32_t": 4, "double": 8}
    ctypes_of = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}
    assert [f for _, f in fields] == [f for f, _ in capi.BwtStats._fields_]
    off = 0
    for (ty, name), (pname, pty) in zip(fields, capi.BwtStats._fields_):
        off = (off + size[ty] - 1) // size[ty] * size[ty]
        assert getattr(capi.BwtStats, pname).offset == off, name
        assert pty == ctypes_of[ty], name
        off += size[ty]
    assert C.sizeof(capi.BwtStats) == off == 88


def test_bwt_argument_errors_without_device(capi):
    lib = capi.lib()
    t = np.frombuffer(b"banana", np.uint8).copy()
    u = np.zeros(6, np.uint8)
    a32 = np.zeros(6, np.int32)
    a64 = np.zeros(6, np.int64)
    i32 = np.array([4, 3, 2], np.int32)
    i64 = i32.astype(np.int64)
    p = lambda a: a.ctypes.data   # noqa: E731
    for pre, a, I in (("sa_hip_libsais", a32, i32), ("sa_hip_libsais64", a64, i64)):
        bwt = getattr(lib, pre + "_bwt")
        bwt_omp = getattr(lib, pre + "_bwt_omp")
        aux = getattr(lib, pre + "_bwt_aux")
        aux_omp = getattr(lib, pre + "_bwt_aux_omp")
        unbwt = getattr(lib, pre + "_unbwt")
        unbwt_omp = getattr(lib, pre + "_unbwt_omp")
        uaux = getattr(lib, pre + "_unbwt_aux")
        uaux_omp = getattr(lib, pre + "_unbwt_aux_omp")
        assert bwt(None, p(u), p(a), 6, 0, None) == -1
        assert bwt(p(t), None, p(a), 6, 0, None) == -1
        assert bwt(p(t), p(u), None, 6, 0, None) == -1
        assert bwt(p(t), p(u), p(a), -1, 0, None) == -1
        assert bwt(p(t), p(u), p(a), 6, -1, None) == -1
        assert bwt_omp(p(t), p(u), p(a), 6, 0, None, -1) == -1
        for r in (0, 1, 3, 6, -2):
            assert aux(p(t), p(u), p(a), 6, 0, None, r, p(I)) == -1, r
        assert aux(p(t), p(u), p(a), 6, 0, None, 2, None) == -1
        assert aux_omp(p(t), p(u), p(a), 6, 0, None, 2, p(I), -3) == -1
        assert unbwt(None, p(u), p(a), 6, None, 3) == -1
        assert unbwt(p(t), None, p(a), 6, None, 3) == -1
        assert unbwt(p(t), p(u), None, 6, None, 3) == -1
        assert unbwt(p(t), p(u), p(a), -1, None, 3) == -1
        for i in (0, -1, 7):
            assert unbwt(p(t), p(u), p(a), 6, None, i) == -1, i
        assert unbwt_omp(p(t), p(u), p(a), 6, None, 3, -1) == -1
        for r in (1, 3, 5):
            assert uaux(p(t), p(u), p(a), 6, None, r, p(I)) == -1, r
        assert uaux(p(t), p(u), p(a), 6, None, 2, None) == -1
        bad = I.copy()
        bad[2] = 7
        assert uaux(p(t), p(u), p(a), 6, None, 2, p(bad)) == -1
        bad[2] = 0
        assert uaux(p(t), p(u), p(a), 6, None, 2, p(bad)) == -1
        assert uaux_omp(p(t), p(u), p(a), 6, None, 2, p(I), -1) == -1
        assert unbwt(p(t), p(u), p(a), 1, None, 0) == -1       # n <= 1 needs I[0] == n
        assert unbwt(p(t), p(u), p(a), 0, None, 1) == -1
    assert lib.sa_hip_bwt64_device(None, None, None, -1, 0, None, 0, None) == -1
    assert lib.sa_hip_bwt64_device(None, None, None, 5, 0, None, 0, None) == -1
    assert lib.sa_hip_unbwt64_device(None, None, 5, 5, None, 0, None) == -1
    assert lib.sa_hip_index_bwt_device(None, None, 0, None, None, None) == -1
    assert b"invalid" in lib.sa_hip_last_error() or b"NULL" in lib.sa_hip_last_error()


def test_bwt_n_le_1_on_host(capi):
    """n <= 1 as in libsais (libsais.c:6671-6676, 6697-6703, 7606-7610): no device call"""
    lib = capi.lib()
    t = np.frombuffer(b"q", np.uint8).copy()
    for pre, it in (("sa_hip_libsais", np.int32), ("sa_hip_libsais64", np.int64)):
        a = np.zeros(1, it)
        u = np.zeros(1, np.uint8)
        f = np.full(256, 5, it)
        assert getattr(lib, pre + "_bwt")(t.ctypes.data, u.ctypes.data, a.ctypes.data, 1, 0, f.ctypes.data) == 1
        assert u[0] == ord("q") and f[ord("q")] == 1 and f.sum() == 1
        f[:] = 5
        assert getattr(lib, pre + "_bwt")(t.ctypes.data, u.ctypes.data, a.ctypes.data, 0, 0, f.ctypes.data) == 0 and f.sum() == 0
        I = np.full(1, 9, it)
        assert getattr(lib, pre + "_bwt_aux")(t.ctypes.data, u.ctypes.data, a.ctypes.data, 1, 0, None, 4, I.ctypes.data) == 0 and I[0] == 1
        assert getattr(lib, pre + "_bwt_aux")(t.ctypes.data, u.ctypes.data, a.ctypes.data, 0, 0, None, 4, I.ctypes.data) == 0 and I[0] == 0
        u[0] = 0
        assert getattr(lib, pre + "_unbwt")(t.ctypes.data, u.ctypes.data, a.ctypes.data, 1, None, 1) == 0 and u[0] == ord("q")
        assert getattr(lib, pre + "_unbwt")(t.ctypes.data, u.ctypes.data, a.ctypes.data, 0, None, 0) == 0
        I[0] = 1
        assert getattr(lib, pre + "_unbwt_aux")(t.ctypes.data, u.ctypes.data, a.ctypes.data, 1, None, 1, I.ctypes.data) == 0


def model_texts():
    c = {k: v for k, v in cases.small_texts().items() if 2 <= v.size <= 70_000}
    rng = np.random.default_rng(11)
    c["ab"] = np.frombuffer(b"ab", np.uint8)
    c["aa"] = np.frombuffer(b"aa", np.uint8)
    c["aba"] = np.frombuffer(b"aba", np.uint8)
    c["all_a"] = np.full(3000, ord("a"), np.uint8)
    c["ab_periodic"] = np.frombuffer(b"ab" * 1500, np.uint8)
    c["binary"] = rng.integers(0, 2, 5000).astype(np.uint8)
    c["bytes256"] = rng.permutation(np.tile(np.arange(256, dtype=np.uint8), 8))
    for s in range(20):
        n = int(rng.integers(2, 400))
        c["rand%d" % s] = rng.integers(0, int(rng.integers(1, 256)) + 1, n).astype(np.uint8)
    return c


def test_model_matches_reference(ref, capi):
    done = 0
    for name, t in model_texts().items():
        sa = ref.libsais(t)
        U, p, f = ref_bwt(ref, t)
        mU, mp, _ = model_bwt(t, sa)
        assert p == mp and np.array_equal(U, mU), name
        assert np.array_equal(f, np.bincount(t, minlength=256)), name
        assert np.array_equal(model_unbwt(U, p), t), name
        rc, back = ref_unbwt(ref, U, primary=p)
        assert rc == 0 and np.array_equal(back, t), name
        for r in (2, 8, 64):
            U2, I, _ = ref_bwt(ref, t, r=r)
            _, _, mI = model_bwt(t, sa, r=r)
            assert np.array_equal(U2, U) and I[0] == p and np.array_equal(I, mI), (name, r)
            rc, back = ref_unbwt(ref, U, I=I, r=r)
            assert rc == 0 and np.array_equal(back, t), (name, r)
        U64, p64, _ = ref_bwt(ref, t, bits=64)
        assert p64 == p and np.array_equal(U64, U), name
        done += 1
    assert done > 30


@pytest.mark.parametrize("seed", range(3))
def test_reference_on_input_that_is_not_a_bwt_returns_0(ref, seed):
    """the return code the device must match: 0 after the argument checks, whatever the bytes"""
    rng = np.random.default_rng(seed)
    U = rng.integers(0, 256, 5000).astype(np.uint8)
    rc, _ = ref_unbwt(ref, U, primary=int(rng.integers(1, 5001)))
    assert rc == 0
