"""Integer-alphabet suffix arrays on the device: one JSON line with, for n = 1e8 and 1e9,

  * the device form (sa_hip_libsais_int_device) -- sa_hip_int_stats: route, sigma, key width, passes, rounds, device ms of the
    alphabet pass and of the whole call (the second of two runs: the first allocates)
  * the host-to-host drop-in (sa_hip_libsais_int_omp) with its call breakdown
  * the reference's libsais_int_omp on 16 threads (oracle/_ref) as the CPU comparison, and a gate that the device result
    equals the reference's (1e8 always; 1e9 with --ref-1e9)

for four texts: sigma = 4 (route A, the byte pipeline), random k = 2^16, Zipf-like tokens over a 50 257-word vocabulary, and a
random block of 10^6 tokens repeated (long repeats: prefix-doubling rounds).

    SA_HIP_DIAG=1 python tools/gpu_int.py [--small] [--no-ref] [--ref-1e9] [--out FILE]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (first: one HIP runtime per process)

from suffixarray_amd import _capi  # noqa: E402

THREADS = 16
VOCAB = 50257


def rnd(d):
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in d.items()}


def make_text(kind, n, seed=1):
    """the text on the device (int32) and its k"""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    if kind == "sigma4":
        return torch.randint(0, 4, (n,), device="cuda:0", dtype=torch.int32, generator=g), 4
    if kind == "rand_k65536":
        return torch.randint(0, 1 << 16, (n,), device="cuda:0", dtype=torch.int32, generator=g), 1 << 16
    if kind == "zipf":
        u = torch.rand(n, device="cuda:0", generator=g)
        t = torch.clamp(torch.floor(torch.pow(torch.tensor(float(VOCAB), device="cuda:0"), u)).to(torch.int32) - 1, 0, VOCAB - 1)
        return t, VOCAB
    if kind == "repeat_block":
        blk = torch.randint(0, VOCAB, (1_000_000,), device="cuda:0", dtype=torch.int32, generator=g)
        return blk.repeat((n + blk.numel() - 1) // blk.numel())[:n].contiguous(), VOCAB
    raise ValueError(kind)


def ref_int_omp(t, k):
    from oracle.oracle import Ref
    from test_int_cpu import bind_ref
    L = bind_ref(Ref())
    tt = np.array(t, dtype=np.int32)
    sa = np.empty(tt.size, np.int32)
    t0 = time.time()
    rc = L.libsais_int_omp(tt.ctypes.data, sa.ctypes.data, tt.size, int(k), 0, THREADS)
    s = time.time() - t0
    assert rc == 0, rc
    return sa, s


def run_case(kind, n, with_ref):
    t_d, k = make_text(kind, n)
    sa_d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    _capi.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), n, k)           # allocations
    t0 = time.time()
    st = _capi.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), n, k)
    dev_wall = (time.time() - t0) * 1e3
    t_h = t_d.cpu().numpy()
    out = {"kind": kind, "n": n, "k": k, "device": rnd(st), "device_call_wall_ms": round(dev_wall, 1)}
    _capi.libsais_int(t_h, k)                                                  # workspace
    t0 = time.time()
    sa_h = _capi.libsais_int(t_h, k)
    out["dropin_ms"] = round((time.time() - t0) * 1e3, 1)
    out["dropin_breakdown"] = rnd(_capi.last_call_breakdown())
    same = bool(np.array_equal(sa_h, sa_d.cpu().numpy()))
    del t_d, sa_d
    torch.cuda.empty_cache()
    if with_ref:
        ref, s = ref_int_omp(t_h, k)
        out["ref_libsais_int_omp_ms"] = round(s * 1e3, 1)
        out["speedup_vs_ref_dropin"] = round(s * 1e3 / out["dropin_ms"], 1)
        same = same and bool(np.array_equal(ref, sa_h))
        out["equal_to_reference"] = same
    else:
        out["dropin_equals_device"] = same
    return out, same


def main():
    small = "--small" in sys.argv
    no_ref = "--no-ref" in sys.argv
    ref_1e9 = "--ref-1e9" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    sizes = [10_000_000] if small else [100_000_000, 1_000_000_000]
    res = {"tool": "gpu_int", "cases": []}
    ok = True
    for n in sizes:
        for kind in ("sigma4", "rand_k65536", "zipf", "repeat_block"):
            with_ref = not no_ref and (n <= 100_000_000 or (ref_1e9 and kind == "zipf"))
            r, same = run_case(kind, n, with_ref)
            ok = ok and same
            res["cases"].append(r)
            print(json.dumps(r), flush=True)
    res["gate_ok"] = ok
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
