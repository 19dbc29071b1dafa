"""Matching statistics over shard sets on the device: one JSON line with, for n Zipf tokens over a 50 257-word vocabulary held as ONE
token index and as sets of 1, 4 and 8 shards (the text cut at fixed points) and the two query batches of tools/gpu_token_match.py
("copied" and "edited", Q documents of M tokens),

  * HIP-event times of the set's three match launches together (sa_hip_token_shards_match_info) at max_length 0, 64 and 256 and of
    its docs launch at min_length 8, cap 64; the single index's match and docs launches (sa_hip_token_index_match_info) beside them
  * the parent's formulation of the same question: the S shards' own sa_hip_token_index_match_batch_device one after another (the
    sum of their HIP-event times), the maximum taken on the host -- the time of copying the S * total lengths back and of that
    maximum reported separately; the per-shard spans at the maximum and the merged records are then still missing
  * after two warm-ups, median / min / max over the repetitions, the configurations taking turns inside every repetition
  * gates: the S = 1 set equals the single index, the maximum of the shards' own lengths equals the set's, and 16 sampled positions
    per batch and set equal a window scan over the shards on the host (windows across a cut do not exist, so sharded and unsharded
    answers differ by design)

    python tools/gpu_token_shard_match.py [--n N] [--q Q] [--m M] [--reps R] [--out FILE]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (first: one HIP runtime per process)

from suffixarray_amd import _capi  # noqa: E402
from test_gpu_int import zipf_tokens  # noqa: E402
from gpu_token_match import make_docs, windows, stats, arg, VOCAB, CAP, MIN_LENGTH, MAX_LENGTHS  # noqa: E402
from gpu_token_shards import load_shard, cut, SHARDS  # noqa: E402


def zeros(*shape):
    return torch.zeros(shape, dtype=torch.int32, device="cuda:0")


def main():
    n, q, m, reps = arg("--n", 100_000_000), arg("--q", 1000), arg("--m", 1000), arg("--reps", 20)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    t = zipf_tokens(n, VOCAB, seed=1)
    total = q * m
    res = {"tool": "gpu_token_shard_match", "n": n, "vocab": VOCAB, "q": q, "doc_tokens": m, "reps": reps, "cap": CAP, "min_length": MIN_LENGTH,
           "sets": {}, "batches": {}}
    single, ms0 = load_shard(t)
    res["single_build_device_ms"] = round(ms0, 3)
    sets, parts, own = {}, {}, {}
    for S in SHARDS:
        parts[S] = cut(t, S)
        built = [load_shard(p) for p in parts[S]]
        sets[S] = _capi.TokenShards.create([h for h, _ in built])
        own[S] = [sets[S].shard(s) for s in range(S)]
        res["sets"][str(S)] = {"build_device_ms_sum": round(sum(b for _, b in built), 3)}
    print("built: one index and sets of %s shards" % (SHARDS,), file=sys.stderr, flush=True)
    off = np.arange(q + 1, dtype=np.uint64) * m
    o_d = torch.from_numpy(off.view(np.int64)).to("cuda:0")
    ok = True
    for bname, buf in make_docs(t, q, m).items():
        p_d = torch.from_numpy(buf).to("cuda:0")
        sp1, ps1, os1, hd1 = zeros(total, 4), zeros(q, CAP), zeros(q, CAP, 4), zeros(q, 4)
        out = {S: {"merged": zeros(total, 4), "per": zeros(S, total, 4), "pos": zeros(q, CAP), "outs": zeros(q, CAP, 4), "heads": zeros(q, 4),
                   "own": zeros(S, total, 4)} for S in SHARDS}
        torch.cuda.synchronize()
        r = res["batches"].setdefault(bname, {"single": {}, "sets": {str(S): {} for S in SHARDS}})
        own_max = {}
        for M in MAX_LENGTHS[::-1]:                                # max_length 0 last: its answers are the ones gated below
            t1 = {"match": [], "docs": []}
            ts = {S: {"match": [], "docs": [], "parent_match_sum": [], "parent_host_max": []} for S in SHARDS}
            for rep in range(reps + 2):                            # two warm-up rounds, then the configurations take turns
                single.match_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, sp1.data_ptr())
                single.match_docs_batch_device(sp1.data_ptr(), o_d.data_ptr(), q, MIN_LENGTH, CAP, ps1.data_ptr(), os1.data_ptr(), hd1.data_ptr())
                info = single.match_info()                         # waits for both launches
                if rep >= 2:
                    t1["match"].append(info["match_ms"]); t1["docs"].append(info["docs_ms"])
                for S in SHARDS:
                    st, o = sets[S], out[S]
                    st.match_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, o["merged"].data_ptr(), o["per"].data_ptr())
                    st.match_docs_batch_device(o["merged"].data_ptr(), o_d.data_ptr(), q, MIN_LENGTH, CAP, o["pos"].data_ptr(), o["outs"].data_ptr(),
                                               o["heads"].data_ptr())
                    info = st.match_info()
                    # the parent's formulation: every shard's own match launch, one after another, then the maximum on the host
                    launched = 0.0
                    for s, sh in enumerate(own[S]):
                        sh.match_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, o["own"][s].data_ptr())
                        launched += sh.match_info()["match_ms"]
                    t0 = time.perf_counter()
                    own_max[S] = o["own"].cpu().numpy().view(np.uint32)[:, :, 2].max(axis=0)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    if rep >= 2:
                        ts[S]["match"].append(info["match_ms"]); ts[S]["docs"].append(info["docs_ms"])
                        ts[S]["parent_match_sum"].append(launched); ts[S]["parent_host_max"].append(host_ms)
            print("%s max_length %d done" % (bname, M), file=sys.stderr, flush=True)
            r["single"]["match_max_length_%d" % M] = stats(t1["match"])
            r["single"]["docs_max_length_%d" % M] = stats(t1["docs"])
            for S in SHARDS:
                for k, v in ts[S].items():
                    r["sets"][str(S)]["%s_max_length_%d" % (k, M)] = stats(v)
        # the answers at max_length 0
        sp = sp1.cpu().numpy().view(np.uint32)
        got = {S: {k: v.cpu().numpy() for k, v in out[S].items()} for S in SHARDS}
        for S in SHARDS:
            g = got[S]
            g["merged"] = g["merged"].view(_capi.SHARDS_MATCH_DTYPE).reshape(total)
            hd = g["heads"].view(np.uint32)
            r["sets"][str(S)].update({"mean_length": round(float(g["merged"]["length"].mean()), 3), "longest": int(hd[:, 2].max()),
                                      "maximal_spans": int(hd[:, 1].sum()), "covered_tokens": int(hd[:, 3].sum())})
        # gate 1: the S = 1 set equals the single index
        g = got[1]
        w = g["heads"].view(np.uint32)[:, 0]
        outs1 = g["outs"].view(_capi.SHARDS_MATCH_DTYPE).reshape(q, CAP)
        kept = np.arange(CAP)[None, :] < w[:, None]
        same = (np.array_equal(g["per"][0], sp1.cpu().numpy()) and np.array_equal(g["merged"]["length"], sp[:, 2])
                and np.array_equal(g["merged"]["count"], sp[:, 1]) and np.array_equal(g["heads"], hd1.cpu().numpy())
                and np.array_equal(g["pos"][kept], ps1.cpu().numpy()[kept])
                and np.array_equal(outs1["length"][kept], os1.cpu().numpy().view(np.uint32)[:, :, 2][kept]))
        # gate 2: the maximum of the shards' own lengths is the set's; gate 3: sampled positions against a window scan over the shards
        maxed, counted = True, True
        for S in SHARDS:
            mg, per = got[S]["merged"], got[S]["per"].view(np.uint32)
            maxed = maxed and np.array_equal(own_max[S], mg["length"])
            for j in np.random.default_rng(5).integers(0, total, 16):
                j = int(j)
                L, end = int(mg["length"][j]), (j // m + 1) * m
                held = [windows(part, buf[j:j + L]) for part in parts[S]]
                counted = counted and sum(held) == int(mg["count"][j]) and sum(c > 0 for c in held) == int(mg["shards"][j]) \
                    and held == per[:, j, 1].tolist() \
                    and (j + L == end or all(windows(part, buf[j:j + L + 1]) == 0 for part in parts[S]))
        r["s1_equals_single"] = bool(same)
        r["own_maximum_equals_set"] = bool(maxed)
        r["samples_equal_window_scan"] = bool(counted)
        ok = ok and same and maxed and counted
        del p_d, out, sp1, ps1, os1, hd1
    for st in sets.values():
        st.close()
    single.close()
    res["gate_ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
