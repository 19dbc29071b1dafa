"""Infinity-gram scores of the token index on the device: one JSON line with, for n Zipf tokens over a 50 257-word vocabulary and Q
query documents of M tokens (the corpus and the two batches of tools/gpu_token_match.py),

  * plan (a): the match launch and the score launch that reads its records (sa_hip_token_index_match_batch_device, then
    sa_hip_token_index_score_batch_device with spans_dev)
  * plan (b): the score launch alone, spans_dev NULL: the binary search over the context's length
  * plan (c): the formulation through the entry points that were there before: one context per position, text[max(s, j - L) : j],
    through sa_hip_token_index_spans_batch_device in mode 1 with need_next = 1; the lengths fetched; one (length + 1)-gram per
    position built on the host; a second spans launch in mode 0.  The time of building the contexts and the n-grams on the host and
    of uploading them is reported separately from the two launches
  * HIP-event times of every launch at max_length 64 and 256, the three plans taking turns inside every repetition, after two
    warm-ups: median, minimum and maximum over the repetitions, and the same of the per-repetition sums of a plan's launches
  * gates: (a), (b) and (c) agree record for record, and 16 sampled positions per batch and max_length agree with window counts of
    the corpus on the host
  * "faster": which of (a) and (b) has the lower sum of medians over the batches and caps

    python tools/gpu_token_score.py [--n N] [--q Q] [--m M] [--reps R] [--out FILE]
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

MAX_LENGTHS = (64, 256)


def gather(buf, starts, lens):
    """(packed int32, uint64 offsets): buf[starts[i] : starts[i] + lens[i]] one after another"""
    off = np.zeros(lens.size + 1, np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    out = np.empty(int(off[-1]), np.int32)
    step = 1 << 17                                                 # pieces at a time: the index arrays stay small
    for a in range(0, lens.size, step):
        ln, o = lens[a:a + step], off[a:a + step + 1].astype(np.int64)
        within = np.arange(o[-1] - o[0], dtype=np.int64) - np.repeat(o[:-1] - o[0], ln)
        out[o[0]:o[-1]] = buf[np.repeat(starts[a:a + step], ln) + within]
    return out, off


def upload(a, off):
    t0 = time.perf_counter()
    a_d, o_d = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return a_d, o_d, (time.perf_counter() - t0) * 1e3


def main():
    n, q, m, reps = arg("--n", 100_000_000), arg("--q", 1000), arg("--m", 1000), arg("--reps", 20)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    t = zipf_tokens(n, VOCAB, seed=1)
    t_d = torch.from_numpy(t).to("cuda:0")
    sa_d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = _capi.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), n, VOCAB)
    h = _capi.TokenIndex.load_device(t_d.data_ptr(), sa_d.data_ptr(), n)
    del sa_d
    total = q * m
    res = {"tool": "gpu_token_score", "n": n, "vocab": VOCAB, "q": q, "doc_tokens": m, "reps": reps,
           "build_device_ms": round(st["total_ms"], 3), "batches": {}}
    off = np.arange(q + 1, dtype=np.uint64) * m
    o_d = torch.from_numpy(off.view(np.int64)).to("cuda:0")
    pos = np.arange(total, dtype=np.int64)
    inside = pos % m                                               # the offset of a position inside its document
    ok = True
    sum_a = sum_b = 0.0
    for bname, buf in make_docs(t, q, m).items():
        r = res["batches"].setdefault(bname, {})
        p_d = torch.from_numpy(buf).to("cuda:0")
        ms_d = torch.zeros((total, 4), dtype=torch.int32, device="cuda:0")
        sa_out = torch.zeros((total, 4), dtype=torch.int32, device="cuda:0")
        sb_out = torch.zeros((total, 4), dtype=torch.int32, device="cuda:0")
        c1_out = torch.zeros((total, 4), dtype=torch.int32, device="cuda:0")
        c2_out = torch.zeros((total, 4), dtype=torch.int32, device="cuda:0")
        hd_d = torch.zeros((q, 6), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        for M in MAX_LENGTHS:
            rm = r.setdefault("max_length_%d" % M, {})
            # plan (c), host side: the contexts, then -- from one launch outside the timed loop -- the (length + 1)-grams
            t0 = time.perf_counter()
            lens = np.minimum(inside, M)
            ctx, coff = gather(buf, pos - lens, lens)
            build1_ms = (time.perf_counter() - t0) * 1e3
            c_d, co_d, up1_ms = upload(ctx, coff)
            h.spans_batch_device(c_d.data_ptr(), co_d.data_ptr(), total, 1, M, 1, c1_out.data_ptr())
            h.sync()
            t0 = time.perf_counter()
            c1 = c1_out.cpu().numpy().view(np.uint32)
            fetch_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            L1 = c1[:, 2].astype(np.int64)
            gram, goff = gather(buf, pos - L1, L1 + 1)
            build2_ms = (time.perf_counter() - t0) * 1e3
            g_d, go_d, up2_ms = upload(gram, goff)
            tm = {k: [] for k in ("a_match", "a_score", "a_sum", "b_score", "c_spans_mode1", "c_spans_mode0", "c_sum", "docs")}
            for rep in range(reps + 2):
                h.match_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, ms_d.data_ptr())
                h.score_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, ms_d.data_ptr(), sa_out.data_ptr())
                h.score_docs_batch_device(sa_out.data_ptr(), o_d.data_ptr(), q, hd_d.data_ptr())
                ia = h.score_info()                                # waits for the three launches
                h.score_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, None, sb_out.data_ptr())
                ib = h.score_info()
                h.spans_batch_device(c_d.data_ptr(), co_d.data_ptr(), total, 1, M, 1, c1_out.data_ptr())
                ic1 = h.next_info()
                h.spans_batch_device(g_d.data_ptr(), go_d.data_ptr(), total, 0, 0, 0, c2_out.data_ptr())
                ic2 = h.next_info()
                if rep >= 2:
                    tm["a_match"].append(ia["match_ms"])
                    tm["a_score"].append(ia["score_ms"])
                    tm["a_sum"].append(ia["match_ms"] + ia["score_ms"])
                    tm["docs"].append(ia["docs_ms"])
                    tm["b_score"].append(ib["score_ms"])
                    tm["c_spans_mode1"].append(ic1["spans_ms"])
                    tm["c_spans_mode0"].append(ic2["spans_ms"])
                    tm["c_sum"].append(ic1["spans_ms"] + ic2["spans_ms"])
            rm.update({k: stats(v) for k, v in tm.items()})
            rm["c_host"] = {"context_tokens": int(coff[-1]), "gram_tokens": int(goff[-1]), "build_contexts_ms": round(build1_ms, 1),
                            "upload_contexts_ms": round(up1_ms, 1), "fetch_lengths_ms": round(fetch_ms, 1), "build_grams_ms": round(build2_ms, 1),
                            "upload_grams_ms": round(up2_ms, 1)}
            sum_a += rm["a_sum"]["median_ms"]
            sum_b += rm["b_score"]["median_ms"]
            # gate: the three plans agree record for record
            a = sa_out.cpu().numpy().view(np.uint32)
            b = sb_out.cpu().numpy().view(np.uint32)
            c1 = c1_out.cpu().numpy().view(np.uint32)
            c2 = c2_out.cpu().numpy().view(np.uint32)
            c = np.stack([c1[:, 2], c1[:, 1] - c1[:, 3], c2[:, 1], c2[:, 0]], axis=1)
            rm["a_equals_b"] = bool(np.array_equal(a, b))
            rm["a_equals_c"] = bool(np.array_equal(a, c))
            hd = hd_d.cpu().numpy().view(_capi.SCORE_HEAD_DTYPE).reshape(-1)
            rm.update({"mean_length": round(float(a[:, 0].mean()), 3), "longest": int(hd["longest"].max()), "seen": int(hd["seen"].sum()),
                       "certain": int(hd["certain"].sum()), "heads_equal_numpy": bool(
                           np.array_equal(hd["length_sum"], a[:, 0].astype(np.uint64).reshape(q, m).sum(axis=1))
                           and np.array_equal(hd["seen"], (a[:, 2] > 0).reshape(q, m).sum(axis=1))
                           and np.array_equal(hd["certain"], (a[:, 2] == a[:, 1]).reshape(q, m).sum(axis=1)))})
            # gate: 16 sampled positions against window counts (a context counts where a token stands behind it)
            counted = True
            for j in np.random.default_rng(5).integers(0, total, 16):
                j = int(j)
                L, k = int(a[j, 0]), j % m
                cc = windows(t[:-1], buf[j - L:j]) if L else n
                counted = counted and cc == int(a[j, 1]) and windows(t, buf[j - L:j + 1]) == int(a[j, 2])
                counted = counted and (L == min(k, M) or windows(t[:-1], buf[j - L - 1:j]) == 0)
            rm["sample_equals_window_counts"] = bool(counted)
            ok = ok and counted and rm["a_equals_b"] and rm["a_equals_c"] and rm["heads_equal_numpy"]
            print(bname, "max_length", M, "done", file=sys.stderr, flush=True)
            del c_d, co_d, g_d, go_d
        del p_d, ms_d, sa_out, sb_out, c1_out, c2_out, hd_d
    h.close()
    res["sum_of_medians_ms"] = {"a": round(sum_a, 4), "b": round(sum_b, 4)}
    res["faster"] = "a" if sum_a <= sum_b else "b"
    res["gate_ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
