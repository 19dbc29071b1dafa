"""PLCP / LCP on the device: one JSON line with device ms per phase, sa_hip_lcp_stats and a bytes-per-character model for

  * LCP from a built index and PLCP, N = 1e9 D1 (synth_uniform27)
  * Zipf words at 1e8, the repeated 1 MiB block at ~1e8 (95 copies), all-'a' at 1e7
  * the host-to-host drop-ins (sa_hip_libsais_plcp + sa_hip_libsais_lcp) at 1e8 and 1e9, with their call breakdowns
  * the reference's libsais_plcp_omp + libsais_lcp_omp on 16 threads (oracle/_ref, as bench.py uses it) as the CPU comparison,
    and a gate that the device arrays equal the reference's

    SA_HIP_DIAG=1 python tools/gpu_lcp.py [--small]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: one HIP runtime per process)

from suffixarray_amd import _capi, synth  # noqa: E402


def model_bytes(st, what, kb):
    """Algorithmic HBM bytes per character of one pass (no cache-line inflation of the random accesses): memset of W, the
    phi kernel (SA, packed keys of kb bytes, output / W scatter, BWT bytes and text of the compared positions), the scan
    (read W twice, write once) and the gather.  `tied` ranks take the text path and the gather; the others only the keys."""
    n = st["n"]
    tied = st["tied"] / n
    text = 2.0 * st["compared_bytes"] / n + 2.0 * st["compared_positions"] / n
    if st["keys"]:
        phi = 4 + kb + 4 + tied * (4 + 2 + 4)
        gather = 4 + tied * 8 if what == "lcp" else 0
    else:
        phi = 8 + 2 + 4
        gather = 12 if what == "lcp" else 0
    return 4 + phi + text + 12 + gather


def index_case(name, t, reps=2):
    out = {}
    n = t.size
    buf = torch.empty(n, dtype=torch.int32, device="cuda:0")
    with _capi.DeviceIndex(n, 0) as idx:
        idx.build(t)
        bs = idx.build_stats()
        kb = 4 if bs["narrow_k"] else 8
        torch.cuda.synchronize()
        for what in ("lcp", "plcp"):
            for _ in range(reps):
                st = getattr(idx, what + "_device")(buf.data_ptr(), stats=True)
            m = model_bytes(st, what, kb)
            st["model_bytes_per_char"] = round(m, 1)
            st["model_gbps"] = round(m * n / (st["total_ms"] * 1e6), 1)
            st["ms_per_gchar"] = round(st["total_ms"] / (n / 1e9), 2)
            out[what] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}
        out["build_ms"] = round(bs["total_ms"], 2)
        sa = idx.sa_u32().view(np.int32)
        out["_sa"] = sa
        out["_lcp"] = idx.lcp()
        out["_plcp"] = idx.lcp(plcp=True)
    return out


def ref_lib():
    from oracle.oracle import Ref
    if not Ref.available():
        return None
    L = Ref().lib
    vp = C.c_void_p
    L.libsais_plcp_omp.restype = C.c_int32
    L.libsais_plcp_omp.argtypes = [vp, vp, vp, C.c_int32, C.c_int32]
    L.libsais_lcp_omp.restype = C.c_int32
    L.libsais_lcp_omp.argtypes = [vp, vp, vp, C.c_int32, C.c_int32]
    return L


def dropins_and_ref(t, sa, dev_plcp, dev_lcp, L):
    n = t.size
    res = {}
    plcp = np.empty(n, np.int32)
    lcp = np.empty(n, np.int32)
    lib = _capi.lib()
    for _ in range(2):   # the second call reuses the workspace
        t0 = time.perf_counter()
        assert lib.sa_hip_libsais_plcp(t.ctypes.data, sa.ctypes.data, plcp.ctypes.data, n) == 0
        res["plcp_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["plcp_breakdown"] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in _capi.last_call_breakdown().items()}
        t0 = time.perf_counter()
        assert lib.sa_hip_libsais_lcp(plcp.ctypes.data, sa.ctypes.data, lcp.ctypes.data, n) == 0
        res["lcp_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["lcp_breakdown"] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in _capi.last_call_breakdown().items()}
    gate = bool(np.array_equal(plcp.view(np.uint32), dev_plcp) and np.array_equal(lcp.view(np.uint32), dev_lcp))
    if L is not None:
        rp = np.empty(n, np.int32)
        rl = np.empty(n, np.int32)
        t0 = time.perf_counter()
        assert L.libsais_plcp_omp(t.ctypes.data, sa.ctypes.data, rp.ctypes.data, n, 16) == 0
        res["ref_plcp_omp16_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        assert L.libsais_lcp_omp(rp.ctypes.data, sa.ctypes.data, rl.ctypes.data, n, 16) == 0
        res["ref_lcp_omp16_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        gate = gate and bool(np.array_equal(rp, plcp) and np.array_equal(rl, lcp))
        res["gate_vs_reference"] = gate
    else:
        res["gate_vs_reference"] = None
    res["gate_dropins_vs_handle"] = bool(np.array_equal(plcp.view(np.uint32), dev_plcp) and np.array_equal(lcp.view(np.uint32), dev_lcp))
    return res


def main():
    small = "--small" in sys.argv
    scale = 100 if small else 1
    L = ref_lib()
    out = {"device": torch.cuda.get_device_name(0)}
    d1 = _capi.synth_uniform27(1_000_000_000 // scale)
    r = index_case("d1", d1)
    out["d1_1e9"] = {k: v for k, v in r.items() if not k.startswith("_")}
    out["dropins_1e9"] = dropins_and_ref(d1, r["_sa"], r["_plcp"], r["_lcp"], L)
    del d1, r
    d1 = _capi.synth_uniform27(100_000_000 // scale)
    r = index_case("d1_1e8", d1)
    out["d1_1e8"] = {k: v for k, v in r.items() if not k.startswith("_")}
    out["dropins_1e8"] = dropins_and_ref(d1, r["_sa"], r["_plcp"], r["_lcp"], L)
    del d1, r
    w = synth.d2_words(100_000_000 // scale)
    r = index_case("words", w)
    out["words_1e8"] = {k: v for k, v in r.items() if not k.startswith("_")}
    out["words_1e8"]["gate_vs_reference"] = dropins_and_ref(w, r["_sa"], r["_plcp"], r["_lcp"], L)["gate_vs_reference"]
    del w, r
    rep = np.tile(np.random.default_rng(11).integers(97, 123, 1 << 20, dtype=np.uint8), 95 if not small else 2)
    r = index_case("repeat", rep)
    out["repeat_1mib_x95"] = {k: v for k, v in r.items() if not k.startswith("_")}
    out["repeat_1mib_x95"]["gate_vs_reference"] = dropins_and_ref(rep, r["_sa"], r["_plcp"], r["_lcp"], L)["gate_vs_reference"]
    del rep, r
    a = synth.all_same(10_000_000 // scale)
    r = index_case("all_a", a)
    out["all_a_1e7"] = {k: v for k, v in r.items() if not k.startswith("_")}
    out["all_a_1e7"]["gate_vs_reference"] = dropins_and_ref(a, r["_sa"], r["_plcp"], r["_lcp"], L)["gate_vs_reference"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
