"""Shard sets on the device: one JSON line with, for n Zipf tokens over a 50 257-word vocabulary held as ONE token index and as
sets of 1, 4 and 8 shards (the text cut at fixed points), what S shards cost against one --

  * the batches of tools/gpu_token_next.py: "exact" (n-grams of length 1..8, mode 0) and "suffix" (contexts of 32 with one symbol
    replaced, mode 1), Q contexts, cap 64
  * HIP-event times of the ranges launch, the spans launch, the per-shard next-symbol launches and the merge launches
    (sa_hip_token_shards_info; the single index: sa_hip_token_index_info / _next_info) after two warm-ups, median / min / max over
    the repetitions, the configurations taking turns inside every repetition
  * gates: the S = 1 set equals the single index, and 16 sampled answers per batch and set equal a count of the shards' windows on
    the host (windows across a cut do not exist, so sharded and unsharded counts differ by design)
  * --big B: once more with 3 shards of B tokens each (a corpus beyond 2^31 at B = 1e9): build and query times, no host gate beyond
    the sample

    python tools/gpu_token_shards.py [--n N] [--q Q] [--reps R] [--big B] [--out FILE]
"""
import json
import os
import sys
import time

os.environ.setdefault("SA_HIP_DIAG", "1")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (first: one HIP runtime per process)

from suffixarray_amd import _capi  # noqa: E402
from test_gpu_int import zipf_tokens  # noqa: E402
from gpu_token_next import make_batches, window_next, arg, VOCAB, CAP  # noqa: E402

SHARDS = (1, 4, 8)


def load_shard(t):
    """one token index from a host text: device build, then adopted by the handle -> (handle, device build ms)"""
    t_d = torch.from_numpy(np.ascontiguousarray(t)).to("cuda:0")
    sa_d = torch.empty(t.size, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = _capi.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), t.size, VOCAB)
    h = _capi.TokenIndex.load_device(t_d.data_ptr(), sa_d.data_ptr(), t.size)
    return h, st["total_ms"]


def cut(t, S):
    edges = [t.size * s // S for s in range(S + 1)]
    return [t[a:b] for a, b in zip(edges, edges[1:])]


def shards_next(parts, p):
    want = {}
    for part in parts:
        if part.size > len(p):
            for y, c in window_next(part, p).items():
                want[y] = want.get(y, 0) + c
    return want


def stats(v):
    v = np.array(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}


def run_set(st, S, p_d, o_d, q, mode):
    sp = torch.zeros((S, q, 4), dtype=torch.int32, device="cuda:0")
    ln = torch.zeros(q, dtype=torch.int32, device="cuda:0")
    tt = torch.zeros(q, dtype=torch.int64, device="cuda:0")
    sy = torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0")
    ct = torch.zeros((q, CAP), dtype=torch.int64, device="cuda:0")
    hd = torch.zeros((q, 3), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    def once():
        st.query_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, tt.data_ptr(), None)
        st.spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, mode, 0, 1, ln.data_ptr(), tt.data_ptr(), sp.data_ptr())
        st.next_batch_device(sp.data_ptr(), q, CAP, sy.data_ptr(), ct.data_ptr(), hd.data_ptr())
        return st.info()
    return once, (sp, ln, sy, ct, hd)


def main():
    n, q, reps, big = arg("--n", 100_000_000), arg("--q", 1_000_000), arg("--reps", 20), arg("--big", 0)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    t = zipf_tokens(n, VOCAB, seed=1)
    res = {"tool": "gpu_token_shards", "n": n, "vocab": VOCAB, "q": q, "reps": reps, "cap": CAP, "sets": {}}
    single, ms0 = load_shard(t)
    res["single_build_device_ms"] = round(ms0, 3)
    sets, parts = {}, {}
    for S in SHARDS:
        parts[S] = cut(t, S)
        built = [load_shard(p) for p in parts[S]]
        sets[S] = _capi.TokenShards.create([h for h, _ in built])
        res["sets"][str(S)] = {"build_device_ms_sum": round(sum(m for _, m in built), 3)}
    ok = True
    for bname, (buf, off, mode) in make_batches(t, q).items():
        p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
        r0 = torch.zeros((q, 2), dtype=torch.int32, device="cuda:0")
        s0 = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
        y0 = torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0")
        c0 = torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0")
        h0 = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
        runs = {S: run_set(sets[S], S, p_d, o_d, q, mode) for S in SHARDS}
        ms = {S: {k: [] for k in ("ranges", "spans", "next", "merge")} for S in SHARDS}
        ms1 = {k: [] for k in ("ranges", "spans", "next")}
        for rep in range(reps + 2):                               # two warm-up rounds, then the configurations take turns
            single.query_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, r0.data_ptr())
            single.spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, mode, 0, 1, s0.data_ptr())
            single.next_batch_device(s0.data_ptr(), q, CAP, y0.data_ptr(), c0.data_ptr(), h0.data_ptr())
            a, b = single.info(), single.next_info()
            if rep >= 2:
                ms1["ranges"].append(a["kernel_ms"]); ms1["spans"].append(b["spans_ms"]); ms1["next"].append(b["next_ms"])
            for S in SHARDS:
                info = runs[S][0]()
                if rep >= 2:
                    for k in ms[S]:
                        ms[S][k].append(info[k + "_ms"])
                res["sets"][str(S)][bname + "_chunk"] = info["chunk"]
        res.setdefault("single", {})[bname] = {k: stats(v) for k, v in ms1.items()}
        for S in SHARDS:
            res["sets"][str(S)][bname] = {k: stats(v) for k, v in ms[S].items()}
        # gate 1: the S = 1 set equals the single index (cells beyond written are zeros in both)
        sp, ln, sy, ct, hd = (x.cpu().numpy() for x in runs[1][1])
        hd = hd.view(_capi.SHARDS_NEXT_DTYPE).reshape(q)
        h1 = h0.cpu().numpy().view(np.uint32)
        same = (np.array_equal(sp[0], s0.cpu().numpy()) and np.array_equal(sy, y0.cpu().numpy())
                and np.array_equal(ct.view(np.uint64), c0.cpu().numpy().view(np.uint32))
                and np.array_equal(hd["written"], h1[:, 0]) and np.array_equal(hd["covered"], h1[:, 1]) and np.array_equal(hd["total"], h1[:, 2]))
        # gate 2: sampled answers of every set against a window count over its shards
        counted = True
        for S in SHARDS:
            sp, ln, sy, ct, hd = (x.cpu().numpy() for x in runs[S][1])
            hd = hd.view(_capi.SHARDS_NEXT_DTYPE).reshape(q)
            ln = ln.view(np.uint32)
            for i in np.random.default_rng(5).integers(0, q, 16):
                p = buf[int(off[i]):int(off[i + 1])]
                want = shards_next(parts[S], p[len(p) - int(ln[i]):])
                w = int(hd["written"][i])
                keys = sorted(want)[:CAP]
                counted = counted and int(hd["total"][i]) == sum(want.values()) and sy[i, :w].tolist() == keys \
                    and ct.view(np.uint64)[i, :w].tolist() == [want[k] for k in keys]
                if mode == 1 and int(ln[i]) < len(p):             # one symbol more has a next symbol in no shard
                    counted = counted and not shards_next(parts[S], p[len(p) - int(ln[i]) - 1:])
        res[bname + "_s1_equals_single"] = bool(same)
        res[bname + "_samples_equal_window_count"] = bool(counted)
        ok = ok and same and counted
        del runs, p_d, o_d
    for st in sets.values():
        st.close()
    single.close()
    if big:
        del t
        t0 = time.perf_counter()
        texts = [zipf_tokens(big, VOCAB, seed=10 + s) for s in range(3)]
        built = [load_shard(p) for p in texts]
        st = _capi.TokenShards.create([h for h, _ in built])
        wall = time.perf_counter() - t0
        r = {"shards": 3, "tokens": st.info()["tokens"], "build_device_ms": [round(m, 1) for _, m in built], "build_wall_s": round(wall, 1)}
        for bname, (buf, off, mode) in make_batches(texts[2], q).items():
            p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
            once, outs = run_set(st, 3, p_d, o_d, q, mode)
            v = [once() for _ in range(5)][2:]
            r[bname] = {k: round(float(np.median([x[k + "_ms"] for x in v])), 4) for k in ("ranges", "spans", "next", "merge")}
            r[bname + "_max_total"] = int(outs[4].cpu().numpy().view(_capi.SHARDS_NEXT_DTYPE)["total"].max())
        res["big"] = r
        st.close()
    res["gate_ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
