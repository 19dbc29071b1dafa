"""BWT / inverse BWT on the device: one JSON line with device ms per phase and sa_hip_bwt_stats for

  * the BWT from a built index: D1 (synth_uniform27) 1e9, Zipf words 1e8, the repeated 1 MiB block (96 copies), all-'a' 1e7
  * the inverse at the same sizes, with r = n (one primary index) and with aux rows r = 4096
  * the host-to-host drop-ins (sa_hip_libsais_bwt + sa_hip_libsais_unbwt) at 1e8 and 1e9, with their call breakdowns
  * the reference's libsais_bwt_omp / libsais_unbwt_omp / libsais_unbwt_aux_omp on 16 threads (oracle/_ref) as the CPU
    comparison, and a gate that every device output equals the reference's

    SA_HIP_DIAG=1 python tools/gpu_bwt.py [--small] [--out FILE]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (first: one HIP runtime per process)

from suffixarray_amd import _capi, synth  # noqa: E402

THREADS = 16


def rnd(d):
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in d.items()}


def ref_lib():
    from oracle.oracle import Ref
    from test_bwt_cpu import bind_ref
    return bind_ref(Ref())


def ref_case(L, t, r):
    """the reference on 16 threads: BWT, inverse with r = n, inverse with aux rows r; (U, primary, I, seconds)"""
    n = t.size
    U = np.empty(n, np.uint8)
    A = np.empty(n + 1, np.int32)
    t0 = time.time()
    p = L.libsais_bwt_omp(t.ctypes.data, U.ctypes.data, A.ctypes.data, n, 0, None, THREADS)
    s_bwt = time.time() - t0
    I = np.empty((n - 1) // r + 1, np.int32)
    U2 = np.empty(n, np.uint8)
    assert L.libsais_bwt_aux_omp(t.ctypes.data, U2.ctypes.data, A.ctypes.data, n, 0, None, r, I.ctypes.data, THREADS) == 0
    back = np.empty(n, np.uint8)
    t0 = time.time()
    rc = L.libsais_unbwt_omp(U.ctypes.data, back.ctypes.data, A.ctypes.data, n, None, p, THREADS)
    s_unbwt = time.time() - t0
    ok = rc == 0 and np.array_equal(back, t)
    t0 = time.time()
    rc = L.libsais_unbwt_aux_omp(U.ctypes.data, back.ctypes.data, A.ctypes.data, n, None, r, I.ctypes.data, THREADS)
    s_aux = time.time() - t0
    ok = ok and rc == 0 and np.array_equal(back, t)
    return U, p, I, {"bwt_omp_ms": round(s_bwt * 1e3, 1), "unbwt_omp_ms": round(s_unbwt * 1e3, 1),
                     "unbwt_aux_omp_ms": round(s_aux * 1e3, 1), "ref_round_trip": bool(ok)}


def device_case(t, U_ref, p_ref, I_ref, r, reps=2):
    n = t.size
    out = {}
    u = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    with _capi.DeviceIndex(n, 0) as idx:
        idx.build(t)
        out["build_ms"] = round(idx.build_stats()["total_ms"], 2)
        torch.cuda.synchronize()
        for _ in range(reps):
            p, st = idx.bwt_device(u.data_ptr(), stats=True)
        out["bwt"] = rnd(st)
        gate = p == p_ref and np.array_equal(u.cpu().numpy(), U_ref)
    text_d = torch.from_numpy(t).to("cuda:0")
    back = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    P = torch.tensor([p_ref], dtype=torch.int64, device="cuda:0")
    I = torch.from_numpy(I_ref.astype(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    for _ in range(reps):
        st = _capi.unbwt64_device(u.data_ptr(), back.data_ptr(), n, n, P.data_ptr())
    out["unbwt_r_n"] = rnd(st)
    gate = gate and bool(torch.equal(back, text_d))
    back.zero_()
    for _ in range(reps):
        st = _capi.unbwt64_device(u.data_ptr(), back.data_ptr(), n, r, I.data_ptr())
    out["unbwt_aux_%d" % r] = rnd(st)
    gate = gate and bool(torch.equal(back, text_d))
    out["gate_vs_reference"] = bool(gate)
    return out


def dropins(t, U_ref, p_ref):
    out = {}
    t0 = time.time()
    U, p = _capi.libsais_bwt(t)
    out["bwt_wall_ms"] = round((time.time() - t0) * 1e3, 1)
    bd = _capi.CallBreakdown()
    _capi.lib().sa_hip_last_call_breakdown(C.byref(bd))
    out["bwt_breakdown"] = rnd(bd.as_dict())
    t0 = time.time()
    back = _capi.libsais_unbwt(U, primary=p)
    out["unbwt_wall_ms"] = round((time.time() - t0) * 1e3, 1)
    _capi.lib().sa_hip_last_call_breakdown(C.byref(bd))
    out["unbwt_breakdown"] = rnd(bd.as_dict())
    out["gate_vs_reference"] = bool(p == p_ref and np.array_equal(U, U_ref) and np.array_equal(back, t))
    return out


def main():
    small = "--small" in sys.argv
    scale = 100 if small else 1
    L = ref_lib()
    r = 4096
    res = {"device": torch.cuda.get_device_name(0)}
    cases = [("d1_1e9", lambda: _capi.synth_uniform27(1_000_000_000 // scale), True),
             ("d1_1e8", lambda: _capi.synth_uniform27(100_000_000 // scale), True),
             ("words_1e8", lambda: synth.d2_words(100_000_000 // scale), False),
             ("repeat_1mib_x95", lambda: np.tile(np.random.default_rng(11).integers(97, 123, 1 << 20, dtype=np.uint8), 96 if not small else 1), False),
             ("all_a_1e7", lambda: synth.all_same(10_000_000 // scale), False)]
    gates = []
    for name, make, with_dropins in cases:
        t = np.ascontiguousarray(make())
        U, p, I, cpu = ref_case(L, t, r)
        d = device_case(t, U, p, I, r)
        d["reference_16_threads"] = cpu
        if with_dropins:
            d["dropins"] = dropins(t, U, p)
            gates.append(d["dropins"]["gate_vs_reference"])
        d["unbwt_speedup_vs_ref_omp"] = round(cpu["unbwt_omp_ms"] / d["unbwt_r_n"]["total_ms"], 1)
        gates += [d["gate_vs_reference"], cpu["ref_round_trip"]]
        res[name] = d
        del t, U, I
    res["gate_all_equal_reference"] = bool(all(gates))
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
