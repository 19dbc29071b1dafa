"""Integer-alphabet suffix arrays without a GPU: every new entry point is declared, exported and bound, IntStats matches the
C compiler's view of the header; argument errors and n <= 1 are answered on the host before any device call; and the
test's own NumPy model (suffix array by prefix doubling with np.lexsort, PLCP by direct comparison -- the independent check
of tests/test_gpu_int.py) agrees with the reference's libsais_int / libsais64_long / libsais_plcp_int, together with the two
invariances the GPU tests lean on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_libsais_int", "sa_hip_libsais_int_omp", "sa_hip_libsais64_long", "sa_hip_libsais64_long_omp",
       "sa_hip_libsais_plcp_int", "sa_hip_libsais_plcp_int_omp", "sa_hip_libsais_int_device", "sa_hip_libsais64_long_device",
       "sa_hip_plcp_int_device", "sa_hip_sufcheck_long_device"]


# ---- the model -----------------------------------------------------------------------------------------------------------
def model_sa(t):
    """suffix array by prefix doubling: ranks of (rank[i], rank[i + h]) with 0 past the end, sorted by np.lexsort"""
    t = np.asarray(t, np.int64)
    n = t.size
    if n == 0:
        return np.zeros(0, np.int64)
    rank = np.unique(t, return_inverse=True)[1].astype(np.int64).reshape(-1) + 1
    h = 1
    while True:
        r2 = np.zeros(n, np.int64)
        if h < n:
            r2[:n - h] = rank[h:]
        order = np.lexsort((r2, rank))
        a, b = rank[order], r2[order]
        new = np.empty(n, np.int64)
        new[order] = np.cumsum(np.concatenate([[1], (a[1:] != a[:-1]) | (b[1:] != b[:-1])]))
        if new.max() == n:
            return order.astype(np.int64)
        rank = new
        h *= 2


def model_plcp(t, sa):
    """PLCP[SA[r]] = common prefix of the suffixes SA[r] and SA[r-1], compared symbol by symbol; 0 for SA[0]"""
    t = np.asarray(t, np.int64)
    sa = np.asarray(sa, np.int64)
    n = t.size
    plcp = np.zeros(n, np.int64)
    for r in range(1, n):
        i, k = int(sa[r]), int(sa[r - 1])
        m = n - max(i, k)
        ne = np.flatnonzero(t[i:i + m] != t[k:k + m])
        plcp[i] = ne[0] if ne.size else m
    return plcp


def rank_remap(t):
    """the order-preserving remap onto 0 .. sigma-1: the same suffix array, a k the reference can allocate buckets for"""
    u, inv = np.unique(np.asarray(t), return_inverse=True)
    return inv.reshape(-1).astype(np.int64), int(u.size)


# ---- the reference through ctypes ----------------------------------------------------------------------------------------
def bind_ref(ref):
    L = ref.lib
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.libsais_int.restype = i32
    L.libsais_int.argtypes = [vp, vp, i32, i32, i32]
    L.libsais_int_omp.restype = i32
    L.libsais_int_omp.argtypes = [vp, vp, i32, i32, i32, i32]
    L.libsais64_long.restype = i64
    L.libsais64_long.argtypes = [vp, vp, i64, i64, i64]
    L.libsais64_long_omp.restype = i64
    L.libsais64_long_omp.argtypes = [vp, vp, i64, i64, i64, i64]
    L.libsais_plcp_int.restype = i32
    L.libsais_plcp_int.argtypes = [vp, vp, vp, i32]
    L.libsais_plcp_int_omp.restype = i32
    L.libsais_plcp_int_omp.argtypes = [vp, vp, vp, i32, i32]
    return L


def ref_int(ref, t, k, threads=1):
    """the reference's libsais_int[_omp] on a copy of t (it may modify T and restore it)"""
    L = bind_ref(ref)
    t = np.array(t, dtype=np.int32)
    n = t.size
    sa = np.zeros(max(n, 1), np.int32)
    if threads == 1:
        rc = L.libsais_int(t.ctypes.data, sa.ctypes.data, n, int(k), 0)
    else:
        rc = L.libsais_int_omp(t.ctypes.data, sa.ctypes.data, n, int(k), 0, threads)
    assert rc == 0, rc
    return sa[:n]


def ref_long(ref, t, k, threads=1):
    L = bind_ref(ref)
    t = np.array(t, dtype=np.int64)
    n = t.size
    sa = np.zeros(max(n, 1), np.int64)
    if threads == 1:
        rc = L.libsais64_long(t.ctypes.data, sa.ctypes.data, n, int(k), 0)
    else:
        rc = L.libsais64_long_omp(t.ctypes.data, sa.ctypes.data, n, int(k), 0, threads)
    assert rc == 0, rc
    return sa[:n]


def ref_plcp_int(ref, t, sa, threads=1):
    L = bind_ref(ref)
    t = np.ascontiguousarray(t, dtype=np.int32)
    s = np.ascontiguousarray(sa, dtype=np.int32)
    n = t.size
    out = np.zeros(max(n, 1), np.int32)
    if threads == 1:
        rc = L.libsais_plcp_int(t.ctypes.data, s.ctypes.data, out.ctypes.data, n)
    else:
        rc = L.libsais_plcp_int_omp(t.ctypes.data, s.ctypes.data, out.ctypes.data, n, threads)
    assert rc == 0, rc
    return out[:n]


def fibonacci_word(n):
    a, b = [0], [0, 1]
    while len(b) < n:
        a, b = b, b + a
    return np.array(b[:n], np.int64)


def model_texts():
    """(text as int64, k) pairs: k = 1, periodic k = 2, Fibonacci words, random k up to 2^20, sparse large values"""
    rng = np.random.default_rng(5)
    c = {
        "len2": (np.array([1, 0]), 2),
        "k1": (np.zeros(1500, np.int64), 1),
        "k1_short": (np.zeros(7, np.int64), 1),
        "periodic2": (np.tile([0, 1], 900), 2),
        "periodic3": (np.tile([2, 0, 1], 500), 3),
        "fib": (fibonacci_word(4181), 2),
        "fib_shift": (fibonacci_word(987) * 7 + 3, 11),
        "repeat_block": (np.tile(rng.integers(0, 50, 300), 6), 50),
        "sparse_large": (rng.choice(np.array([0, 2 ** 30, 2 ** 31 - 2, 12345]), 3000), 2 ** 31 - 1),
        "two_values": (rng.choice(np.array([0, 2 ** 30]), 2000), 2 ** 30 + 1),
    }
    for k in (2, 3, 4, 255, 256, 257, 1000, 2 ** 16, 2 ** 20):
        for n in (2, 37, 4000):
            c["rand_k%d_n%d" % (k, n)] = (rng.integers(0, k, n), k)
    return c


# ---- tests -----------------------------------------------------------------------------------------------------------------
def test_int_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is not None, name
    for name in ("libsais_int", "libsais64_long", "libsais_plcp_int", "libsais_int_device", "libsais64_long_device",
                 "plcp_int_device", "sufcheck_long_device"):
        assert callable(getattr(capi, name)), name


def test_int_stats_layout_matches_the_compiler(capi, tmp_path):
    S = capi.IntStats
    fields = [f for f, _ in S._fields_]
    src = tmp_path / "int_sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sa_hip.h"\nint main(void) { printf("%zu'
                   + "".join(" %zu" for _ in fields) + '\\n", sizeof(sa_hip_int_stats)'
                   + "".join(", offsetof(sa_hip_int_stats, %s)" % f for f in fields) + "); return 0; }\n")
    exe = tmp_path / "int_sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields], got
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    body = re.search(r"typedef struct sa_hip_int_stats \{(.*?)\} sa_hip_int_stats;", header, re.S).group(1)
    assert [f for f in re.findall(r"^\s*\w+\s+(\w+);", body, re.M)] == fields


def test_int_host_answered_cases(capi):
    """argument errors, n == 0 and n == 1 (T[0] not looked at) before any HIP call: this machine has no GPU"""
    lib = capi.lib()
    p = lambda a: a.ctypes.data   # noqa: E731
    for it, f, fo in ((np.int32, lib.sa_hip_libsais_int, lib.sa_hip_libsais_int_omp),
                      (np.int64, lib.sa_hip_libsais64_long, lib.sa_hip_libsais64_long_omp)):
        t = np.array([3, 1, 2, 1], it)
        sa = np.full(6, 77, it)
        assert f(None, p(sa), 4, 4, 0) == -1
        assert f(p(t), None, 4, 4, 0) == -1
        assert f(p(t), p(sa), -1, 4, 0) == -1
        assert f(p(t), p(sa), 4, 4, -1) == -1
        assert fo(p(t), p(sa), 4, 4, 0, -1) == -1
        assert f(p(t), p(sa), 4, 0, 0) == -1            # k < 1 with n >= 2
        assert f(p(t), p(sa), 0, 4, 0) == 0 and (sa == 77).all()
        bad = np.array([-5], it)                        # n == 1: SA[0] = 0, T[0] not checked
        assert f(p(bad), p(sa), 1, 1, 2) == 0 and sa[0] == 0 and (sa[1:] == 77).all()
        assert fo(p(bad), p(sa), 1, 0, 0, 3) == 0
        assert bad[0] == -5
    t = np.array([1, 0, 1], np.int32)
    sa = np.array([1, 2, 0], np.int32)
    out = np.full(3, 9, np.int32)
    assert lib.sa_hip_libsais_plcp_int(None, p(sa), p(out), 3) == -1
    assert lib.sa_hip_libsais_plcp_int(p(t), None, p(out), 3) == -1
    assert lib.sa_hip_libsais_plcp_int(p(t), p(sa), None, 3) == -1
    assert lib.sa_hip_libsais_plcp_int(p(t), p(sa), p(out), -1) == -1
    assert lib.sa_hip_libsais_plcp_int_omp(p(t), p(sa), p(out), 3, -1) == -1
    assert lib.sa_hip_libsais_plcp_int(p(t), p(sa), p(out), 0) == 0 and (out == 9).all()
    assert lib.sa_hip_libsais_plcp_int(p(t), p(sa), p(out), 1) == 0 and out[0] == 0
    # device forms: argument errors and n == 0 before any HIP call
    assert lib.sa_hip_libsais_int_device(None, None, -1, 4, 0, None) == -1
    assert lib.sa_hip_libsais_int_device(None, None, 5, 4, 0, None) == -1
    assert lib.sa_hip_libsais64_long_device(None, None, 5, 4, 0, None) == -1
    assert lib.sa_hip_libsais_int_device(1 << 20, 1 << 20, 5, 0, 0, None) == -1   # k < 1 (pointers never touched)
    assert lib.sa_hip_plcp_int_device(None, None, None, 5, 0, None) == -1
    assert lib.sa_hip_sufcheck_long_device(None, None, 5, 0, None) == -1
    st = capi.IntStats()
    assert lib.sa_hip_libsais_int_device(None, None, 0, 4, 0, C.byref(st)) == 0 and st.n == 0
    assert lib.sa_hip_libsais64_long_device(None, None, 0, 4, 0, None) == 0


def test_model_matches_reference(ref):
    done = 0
    for name, (t, k) in model_texts().items():
        sa = model_sa(t)
        r, sigma = rank_remap(t)
        got = ref_int(ref, r, sigma) if k > (1 << 21) else ref_int(ref, t, k)
        assert np.array_equal(got, sa), name
        assert np.array_equal(ref_long(ref, r, sigma), sa), name
        plcp = model_plcp(t, sa)
        assert np.array_equal(ref_plcp_int(ref, t, sa), plcp), name
        done += 1
    assert done > 30


def test_long_values_beyond_int32(ref):
    """libsais64_long over values >= 2^32 and k up to 2^62: the model, and the reference on the rank remap"""
    rng = np.random.default_rng(9)
    for k in (2 ** 33, 2 ** 62):
        t = rng.choice(rng.integers(0, k, 40, dtype=np.int64), 3000)
        sa = model_sa(t)
        r, sigma = rank_remap(t)
        assert np.array_equal(ref_long(ref, r, sigma), sa), k
        assert np.array_equal(ref_long(ref, r, sigma, threads=2), sa), k


def test_rank_remap_keeps_the_suffix_array(ref):
    """invariance 1: the order-preserving remap of a text has the text's suffix array (the reference checked where it can
    allocate buckets for the original k)"""
    rng = np.random.default_rng(2)
    for k in (5, 300, 70000, 1 << 20):
        t = rng.integers(0, k, 5000) * 3 + 1
        r, sigma = rank_remap(t)
        assert np.array_equal(ref_int(ref, t, 3 * k + 1), ref_int(ref, r, sigma)), k
        assert np.array_equal(ref_int(ref, r, sigma), model_sa(t)), k


def test_widened_bytes_give_libsais(ref):
    """invariance 2: a byte text widened to int32 with k = 256 has the byte text's suffix array"""
    for name, t in cases.small_texts().items():
        if not 2 <= t.size <= 70_000:
            continue
        assert np.array_equal(ref_int(ref, t.astype(np.int32), 256), ref.libsais(t)), name
