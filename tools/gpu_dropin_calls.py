"""The host-to-host drop-in calls, warm, with their call breakdowns: one JSON line for

  * sa_hip_libsais, sa_hip_libsais_plcp + _lcp, sa_hip_libsais_bwt + _unbwt, sa_hip_libsais64_bwt_aux + _unbwt_aux (r = 4096),
    sa_hip_libsais_int on both routes (the byte pipeline; integer keys) and sa_hip_libsais64_long, on D1 text of n characters
  * per call: wall time around the Python binding and sa_hip_last_call_breakdown; of three calls the faster of the two warm ones
  * checksums of the results, so that two libraries can be compared on what they return as well

    SA_HIP_LIB=/path/to/libsa_hip.so python tools/gpu_dropin_calls.py [n]      (n defaults to 1e8; SA_HIP_LIB: an A/B build)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401
from suffixarray_amd import _capi  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
KEYS = ("workspace_ms", "upload_ms", "build_ms", "build_device_ms", "download_ms", "total_ms")


def timed(fn, reps=3):
    best = None
    for i in range(reps):       # the first call allocates; the best of the warm ones is kept
        t0 = time.perf_counter()
        r = fn()
        wall = (time.perf_counter() - t0) * 1e3
        bd = _capi.last_call_breakdown()
        rec = {"wall_ms": round(wall, 2), **{k: round(bd[k], 2) for k in KEYS}, "workspace_reused": bd["workspace_reused"]}
        if i and (best is None or rec["wall_ms"] < best["wall_ms"]):
            best = rec
    return r, best


def main():
    out = {"lib": _capi.LIB_PATH, "n": N}
    t = _capi.synth_uniform27(N)
    sa, out["libsais"] = timed(lambda: _capi.libsais(t))
    sa = np.ascontiguousarray(sa)
    p, out["plcp"] = timed(lambda: _capi.libsais_plcp(t, sa))
    l, out["lcp"] = timed(lambda: _capi.libsais_lcp(p, sa))
    (U, prim), out["bwt"] = timed(lambda: _capi.libsais_bwt(t))
    back, out["unbwt"] = timed(lambda: _capi.libsais_unbwt(U, primary=prim))
    assert np.array_equal(back, t)
    (U2, I), out["bwt_aux"] = timed(lambda: _capi.libsais64_bwt(t, r=4096))
    back, out["unbwt_aux"] = timed(lambda: _capi.libsais64_unbwt(U2, I=I, r=4096))
    assert np.array_equal(back, t) and np.array_equal(U, U2)
    ti = t.astype(np.int32)
    sa_a, out["int_route_a"] = timed(lambda: _capi.libsais_int(ti, 256))
    assert np.array_equal(sa_a, sa)
    tb = np.random.default_rng(5).integers(0, 65536, N, dtype=np.int32)
    sa_b, out["int_route_b"] = timed(lambda: _capi.libsais_int(tb, 65536))
    tl = tb[: N // 4].astype(np.int64) << 20
    sa_l, out["long_route_b"] = timed(lambda: _capi.libsais64_long(tl, 1 << 40))
    out["checksum"] = [int(np.bitwise_xor.reduce(a.astype(np.int64) * np.arange(1, a.size + 1, dtype=np.int64))) for a in (sa, p, l, U, sa_b, sa_l)]
    _capi.release_workspace()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
