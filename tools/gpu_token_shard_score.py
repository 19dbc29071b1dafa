"""Infinity-gram scores over shard sets on the device: one JSON line with, for n Zipf tokens over a 50 257-word vocabulary held as ONE
token index and as sets of 1, 4 and 8 shards (the text cut at fixed points) and the two query batches of tools/gpu_token_match.py
("copied" and "edited", Q documents of M tokens), at max_length 64 and 256,

  * plan (a): the set's match launches and the score launches that read the merged records (sa_hip_token_shards_match_batch_device,
    then sa_hip_token_shards_score_batch_device with merged_dev), and the docs launch
  * plan (b): the score launches alone, merged_dev NULL: the search over the context's length
  * plan (c): the formulation through the entry points that were there before: one context per position through
    sa_hip_token_shards_spans_batch_device in mode 1 with need_next = 1; the lengths fetched; one (length + 1)-gram per position
    built on the host; a second spans launch in mode 0.  Host build and upload times are reported separately from the two launches
  * plan (d), at S = 1: the single index's match launch and score launch (tools/gpu_token_score.py's plan (a))
  * HIP-event times of every launch, the plans taking turns inside every repetition, after two warm-ups: median, minimum and
    maximum over the repetitions, and the same of the per-repetition sums of a plan's launches
  * gates: (a), (b) and (c) agree record for record, the S = 1 set equals the single index, the heads equal a NumPy reduction, and
    16 sampled positions per row equal window counts over the shards on the host (windows across a cut do not exist)

    python tools/gpu_token_shard_score.py [--n N] [--q Q] [--m M] [--reps R] [--out FILE]
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
from gpu_token_match import VOCAB, arg, make_docs, stats, windows  # noqa: E402
from gpu_token_score import MAX_LENGTHS, gather, upload  # noqa: E402
from gpu_token_shards import load_shard, cut, SHARDS  # noqa: E402


def zeros(*shape, dtype=torch.int32):
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def main():
    n, q, m, reps = arg("--n", 100_000_000), arg("--q", 1000), arg("--m", 1000), arg("--reps", 20)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    t = zipf_tokens(n, VOCAB, seed=1)
    total = q * m
    res = {"tool": "gpu_token_shard_score", "n": n, "vocab": VOCAB, "q": q, "doc_tokens": m, "reps": reps, "sets": {}, "batches": {}}
    single, ms0 = load_shard(t)
    res["single_build_device_ms"] = round(ms0, 3)
    sets, parts = {}, {}
    for S in SHARDS:
        parts[S] = cut(t, S)
        built = [load_shard(p) for p in parts[S]]
        sets[S] = _capi.TokenShards.create([h for h, _ in built])
        res["sets"][str(S)] = {"build_device_ms_sum": round(sum(b for _, b in built), 3)}
    print("built: one index and sets of %s shards" % (SHARDS,), file=sys.stderr, flush=True)
    off = np.arange(q + 1, dtype=np.uint64) * m
    o_d = torch.from_numpy(off.view(np.int64)).to("cuda:0")
    pos = np.arange(total, dtype=np.int64)
    inside = pos % m                                               # the offset of a position inside its document
    ok = True
    for bname, buf in make_docs(t, q, m).items():
        p_d = torch.from_numpy(buf).to("cuda:0")
        ms1, sc1 = zeros(total, 4), zeros(total, 4)
        out = {S: {"merged": zeros(total, 4), "mper": zeros(S, total, 4), "a": zeros(total, 6), "a_per": zeros(S, total, 4), "b": zeros(total, 6),
                   "b_per": zeros(S, total, 4), "heads": zeros(q, 6), "c_len": zeros(total), "c_tot1": zeros(total, dtype=torch.int64),
                   "c_tot2": zeros(total, dtype=torch.int64), "c_sp1": zeros(S, total, 4), "c_sp2": zeros(S, total, 4)} for S in SHARDS}
        torch.cuda.synchronize()
        rb = res["batches"].setdefault(bname, {})
        for M in MAX_LENGTHS:
            rm = rb.setdefault("max_length_%d" % M, {"single": {}, "sets": {str(S): {} for S in SHARDS}})
            # plan (c), host side: the contexts once, then per set -- from one launch outside the timed loop -- the (length + 1)-grams
            t0 = time.perf_counter()
            lens = np.minimum(inside, M)
            ctx, coff = gather(buf, pos - lens, lens)
            build1_ms = (time.perf_counter() - t0) * 1e3
            c_d, co_d, up1_ms = upload(ctx, coff)
            grams = {}
            for S in SHARDS:
                st, o = sets[S], out[S]
                st.spans_batch_device(c_d.data_ptr(), co_d.data_ptr(), total, 1, M, 1, o["c_len"].data_ptr(), o["c_tot1"].data_ptr(), o["c_sp1"].data_ptr())
                st.sync()
                t0 = time.perf_counter()
                L1 = o["c_len"].cpu().numpy().view(np.uint32).astype(np.int64)
                fetch_ms = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                gram, goff = gather(buf, pos - L1, L1 + 1)
                build2_ms = (time.perf_counter() - t0) * 1e3
                g_d, go_d, up2_ms = upload(gram, goff)
                grams[S] = (g_d, go_d)
                rm["sets"][str(S)]["c_host"] = {"context_tokens": int(coff[-1]), "gram_tokens": int(goff[-1]), "build_contexts_ms": round(build1_ms, 1),
                                                "upload_contexts_ms": round(up1_ms, 1), "fetch_lengths_ms": round(fetch_ms, 1),
                                                "build_grams_ms": round(build2_ms, 1), "upload_grams_ms": round(up2_ms, 1)}
            keys = ("a_match", "a_score", "a_sum", "b_score", "c_spans_mode1", "c_spans_mode0", "c_sum", "docs")
            t1 = {k: [] for k in ("d_match", "d_score", "d_sum")}
            ts = {S: {k: [] for k in keys} for S in SHARDS}
            for rep in range(reps + 2):                            # two warm-up rounds, then the plans take turns
                single.match_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, ms1.data_ptr())
                single.score_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, ms1.data_ptr(), sc1.data_ptr())
                i1 = single.score_info()                           # waits for both launches
                if rep >= 2:
                    t1["d_match"].append(i1["match_ms"]); t1["d_score"].append(i1["score_ms"]); t1["d_sum"].append(i1["match_ms"] + i1["score_ms"])
                for S in SHARDS:
                    st, o = sets[S], out[S]
                    g_d, go_d = grams[S]
                    st.match_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, o["merged"].data_ptr(), o["mper"].data_ptr())
                    st.score_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, o["merged"].data_ptr(), o["a"].data_ptr(), o["a_per"].data_ptr())
                    st.score_docs_batch_device(o["a"].data_ptr(), o_d.data_ptr(), q, o["heads"].data_ptr())
                    ia = st.score_info()                           # waits for the launches
                    st.score_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, None, o["b"].data_ptr(), o["b_per"].data_ptr())
                    ib = st.score_info()
                    st.spans_batch_device(c_d.data_ptr(), co_d.data_ptr(), total, 1, M, 1, o["c_len"].data_ptr(), o["c_tot1"].data_ptr(), o["c_sp1"].data_ptr())
                    ic1 = st.info()
                    st.spans_batch_device(g_d.data_ptr(), go_d.data_ptr(), total, 0, 0, 0, o["c_len"].data_ptr(), o["c_tot2"].data_ptr(), o["c_sp2"].data_ptr())
                    ic2 = st.info()
                    if rep >= 2:
                        x = ts[S]
                        x["a_match"].append(ia["match_ms"]); x["a_score"].append(ia["score_ms"]); x["a_sum"].append(ia["match_ms"] + ia["score_ms"])
                        x["docs"].append(ia["docs_ms"]); x["b_score"].append(ib["score_ms"])
                        x["c_spans_mode1"].append(ic1["spans_ms"]); x["c_spans_mode0"].append(ic2["spans_ms"])
                        x["c_sum"].append(ic1["spans_ms"] + ic2["spans_ms"])
            rm["single"].update({k: stats(v) for k, v in t1.items()})
            one = sc1.cpu().numpy().view(np.uint32)
            for S in SHARDS:
                rs, o = rm["sets"][str(S)], out[S]
                rs.update({k: stats(v) for k, v in ts[S].items()})
                a = o["a"].cpu().numpy().view(_capi.SHARDS_SCORE_DTYPE).reshape(total)
                a_per = o["a_per"].cpu().numpy()
                # gate: the three plans agree record for record
                rs["a_equals_b"] = bool(a.tobytes() == o["b"].cpu().numpy().tobytes() and a_per.tobytes() == o["b_per"].cpu().numpy().tobytes())
                c_len = o["c_sp1"].cpu().numpy().view(np.uint32)[:, :, 2].max(axis=0)
                rs["a_equals_c"] = bool(np.array_equal(a["length"], c_len) and np.array_equal(a["context_count"], o["c_tot1"].cpu().numpy().view(np.uint64))
                                        and np.array_equal(a["token_count"], o["c_tot2"].cpu().numpy().view(np.uint64))
                                        and a_per.tobytes() == o["c_sp2"].cpu().numpy().tobytes())
                hd = o["heads"].cpu().numpy().view(_capi.SCORE_HEAD_DTYPE).reshape(-1)
                rs.update({"mean_length": round(float(a["length"].mean()), 3), "longest": int(hd["longest"].max()), "seen": int(hd["seen"].sum()),
                           "certain": int(hd["certain"].sum()), "heads_equal_numpy": bool(
                               np.array_equal(hd["length_sum"], a["length"].astype(np.uint64).reshape(q, m).sum(axis=1))
                               and np.array_equal(hd["seen"], (a["token_count"] > 0).reshape(q, m).sum(axis=1))
                               and np.array_equal(hd["certain"], (a["token_count"] == a["context_count"]).reshape(q, m).sum(axis=1)))})
                # gate: 16 sampled positions against window counts over the shards (a context counts where a token stands behind it)
                counted = True
                for j in np.random.default_rng(5).integers(0, total, 16):
                    j = int(j)
                    L, k = int(a["length"][j]), j % m
                    cc = sum(windows(part[:-1], buf[j - L:j]) for part in parts[S]) if L else n
                    held = [windows(part, buf[j - L:j + 1]) for part in parts[S]]
                    counted = counted and cc == int(a["context_count"][j]) and sum(held) == int(a["token_count"][j])
                    counted = counted and held == a_per.view(np.uint32)[:, j, 1].tolist() and sum(c > 0 for c in held) == int(a["shards"][j])
                    counted = counted and (L == min(k, M) or all(windows(part[:-1], buf[j - L - 1:j]) == 0 for part in parts[S]))
                rs["sample_equals_window_counts"] = bool(counted)
                good = counted and rs["a_equals_b"] and rs["a_equals_c"] and rs["heads_equal_numpy"]
                if S == 1:                                         # gate: the set of one shard equals the single index
                    rs["equals_single"] = bool(np.array_equal(a["length"], one[:, 0]) and np.array_equal(a["context_count"], one[:, 1])
                                               and np.array_equal(a["token_count"], one[:, 2]) and np.array_equal(a_per.view(np.uint32)[0, :, 0], one[:, 3]))
                    good = good and rs["equals_single"]
                ok = ok and good
            print(bname, "max_length", M, "done", file=sys.stderr, flush=True)
            del c_d, co_d, grams
        del p_d, out, ms1, sc1
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
