"""The token index without a GPU: every new entry point is declared, exported and bound; sa_hip_token_info matches the C
compiler's view of the header; argument errors are answered before any HIP call and a missing device is -3, never a fallback;
and the two CPU models that test_gpu_token_index.py measures the device against (token_cases.py: bisection over the suffix
array with list comparison, and window counting without any suffix array) agree with each other on the whole case list."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_cases as tc
from test_int_cpu import model_sa, rank_remap, ref_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_index_build", "sa_hip_token_index_load_device", "sa_hip_token_index_destroy", "sa_hip_token_index_query_batch",
       "sa_hip_token_index_query_batch_device", "sa_hip_token_index_sync", "sa_hip_token_index_text_dev", "sa_hip_token_index_sa_dev",
       "sa_hip_token_index_get_sa_range", "sa_hip_token_index_info"]


def test_token_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
    assert lib.sa_hip_token_index_destroy.restype is None
    for name in ("build", "load_device", "query_batch", "query_batch_device", "sync", "sa_range", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(capi.TokenIndex, name)), name
    import suffixarray_amd
    from suffixarray_amd import token_index
    assert suffixarray_amd.TokenIndex is token_index.TokenIndex and "TokenIndex" in suffixarray_amd.__all__
    for name in ("count", "ranges", "positions", "close"):
        assert callable(getattr(token_index.TokenIndex, name)), name


def test_token_info_layout_matches_the_compiler(capi, tmp_path):
    S = capi.TokenInfo
    fields = [f for f, _ in S._fields_]
    assert fields == ["n", "min_symbol", "max_symbol", "dir_entries", "key_bytes", "last_rank", "prepare_ms", "q", "kernel_ms"]
    src = tmp_path / "token_sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sa_hip.h"\nint main(void) { printf("%zu'
                   + "".join(" %zu" for _ in fields) + '\\n", sizeof(sa_hip_token_info)'
                   + "".join(", offsetof(sa_hip_token_info, %s)" % f for f in fields) + "); return 0; }\n")
    exe = tmp_path / "token_sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields], got
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    body = re.search(r"typedef struct sa_hip_token_info \{(.*?)\} sa_hip_token_info;", header, re.S).group(1)
    assert [f for f in re.findall(r"^\s*\w+\s+(\w+);", body, re.M)] == fields


def test_token_argument_errors_before_any_device_call(capi):
    lib = capi.lib()
    t = np.array([3, 1, 2, 1], np.int32)
    p = t.ctypes.data
    h = C.c_void_p(0x1234)
    assert lib.sa_hip_token_index_build(None, p, 4, 4, 0) == -1
    assert lib.sa_hip_token_index_build(C.byref(h), None, 4, 4, 0) == -1 and not h.value       # *out is cleared
    assert b"sa_hip_token_index_build" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_build(C.byref(h), p, -1, 4, 0) == -1
    assert lib.sa_hip_token_index_build(C.byref(h), p, 4, 0, 0) == -1                           # k < 1 with n >= 2
    assert lib.sa_hip_token_index_build(C.byref(h), p, 2, -3, 0) == -1
    assert lib.sa_hip_token_index_load_device(None, 1 << 20, 1 << 20, 4, 0) == -1               # (pointers never touched)
    assert lib.sa_hip_token_index_load_device(C.byref(h), None, 1 << 20, 4, 0) == -1
    assert lib.sa_hip_token_index_load_device(C.byref(h), 1 << 20, None, 4, 0) == -1
    assert lib.sa_hip_token_index_load_device(C.byref(h), 1 << 20, 1 << 20, -2, 0) == -1
    out = np.zeros(2, capi.PAIR_DTYPE)
    off = np.zeros(3, np.uint64)
    assert lib.sa_hip_token_index_query_batch(None, p, off.ctypes.data, 2, out.ctypes.data) == -1
    assert lib.sa_hip_token_index_query_batch_device(None, 1 << 20, 1 << 20, 2, 1 << 20) == -1
    assert lib.sa_hip_token_index_sync(None) == -1
    assert lib.sa_hip_token_index_get_sa_range(None, 0, 1, t.ctypes.data) == -1
    assert lib.sa_hip_token_index_info(None, C.byref(capi.TokenInfo())) == -1
    assert lib.sa_hip_token_index_text_dev(None) is None and lib.sa_hip_token_index_sa_dev(None) is None
    lib.sa_hip_token_index_destroy(None)


def test_token_no_device_is_minus_three(capi):
    """a device that does not exist (any device, on a machine without one): -3 and no handle, for every n"""
    lib = capi.lib()
    t = np.array([3, 1, 2, 1], np.int32)
    devices = [1 << 20] + ([0] if lib.sa_hip_device_count() < 1 else [])
    for dev in devices:
        for n in (0, 1, 4):
            h = C.c_void_p(0x1234)
            assert lib.sa_hip_token_index_build(C.byref(h), t.ctypes.data, n, 4, dev) == -3, (dev, n)
            assert not h.value and lib.sa_hip_last_error()
            assert lib.sa_hip_token_index_load_device(C.byref(h), 1 << 20, 1 << 20, n, dev) == -3, (dev, n)
            assert not h.value
    if lib.sa_hip_device_count() < 1:
        with pytest.raises(capi.SaHipError):
            capi.TokenIndex.build([1, 2, 3])


def test_token_models_agree_on_the_case_list():
    """model (a) (bisection, list comparison) and model (b) (window counting) give the same counts on every text and pattern
    of the GPU test; first is pinned by its definition on a few patterns worked out by hand"""
    total = 0
    for name in tc.texts():
        t, sa, pats, first, count = tc.expected(name)
        assert np.array_equal(tc.model_b(t, pats), count), name
        assert all(-2 ** 31 <= v < 2 ** 31 for p in pats for v in p), name
        e = pats.index([])
        assert (first[e], count[e]) == (0, t.size), name
        total += len(pats)
    assert total > 5000
    assert (count > 0).any() and (count == 0).any()
    # "banana" as tokens: b=1 a=0 n=2; suffixes in order: a, ana, anana, banana, na, nana
    t = np.array([1, 0, 2, 0, 2, 0], np.int32)
    sa = model_sa(t)
    assert sa.tolist() == [5, 3, 1, 0, 4, 2]
    pats = [[0], [0, 2], [0, 2, 0, 2], [2, 0, 2, 0, 2], [0, 1], [0, -5], [3], [-1], [], [0, 2, 0, 2, 0, 7], [1, 0, 2, 0, 2, 0, 0]]
    first, count = tc.model_a(t, sa, pats)
    assert first.tolist() == [0, 1, 2, 6, 1, 1, 6, 0, 0, 3, 4]
    assert count.tolist() == [3, 2, 1, 0, 0, 0, 0, 0, 6, 0, 0]
    assert np.array_equal(tc.model_b(t, pats), count)


def test_token_texts_suffix_arrays_match_reference(ref):
    """the model's suffix arrays of the case list against the reference's libsais_int (on the order-preserving remap)"""
    for name, t in tc.texts().items():
        if t.size < 2:
            continue
        r, sigma = rank_remap(t)
        assert np.array_equal(ref_int(ref, r, sigma), tc.expected(name)[1]), name
