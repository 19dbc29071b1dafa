"""Per-document counts and AND groups of the token index on the device: one JSON line with, for the corpus of
tools/gpu_token_docs.py (n Zipf tokens over a 50 257-word vocabulary cut into documents of Zipf-ish length by a separator token) --

  * prepare_doc_ranks: HIP-event time of the rank-by-document array (the widening of DA, the sort, the copy)
  * the exact batch of tools/gpu_token_next.py: the listing at cap 16 chained into doc_counts over its rows, HIP-event medians over
    the repetitions after two warm-ups (sa_hip_token_docs_info, sa_hip_token_doc_ranks_info)
  * AND groups of 2 and of 3 n-grams, counts only (cap 0) and at cap 16, for two batches of G groups of 2-grams: `inside` draws
    every group from inside one document, so matches exist; `random` draws the n-grams anywhere, so there are mostly none
  * gates: 16 sampled answers per batch equal the parent's formulation below, and 16 sampled rows of counts equal a host count
  * the parent's formulation of the AND query: the uncapped documents() list per n-gram and np.intersect1d on the host; wall time
    over the first --base-g groups of each batch

    python tools/gpu_token_all.py [--n N] [--q Q] [--g G] [--reps R] [--base-g B] [--out FILE]
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
from gpu_token_next import VOCAB, make_batches  # noqa: E402
from gpu_token_docs import arg, make_documents, med  # noqa: E402

CAP = 16
NGRAM = 2


def make_groups(t, starts, g, m, inside, seed):
    """g groups of m 2-grams -> (packed int32, uint64 offsets[g * m + 1], uint64 group offsets[g + 1])"""
    rng = np.random.default_rng(seed)
    n = t.size
    if inside:                                                     # every n-gram of a group from one document of >= 8 tokens
        ends = np.append(starts[1:], n).astype(np.int64)
        big = np.flatnonzero(ends - starts >= 8)
        d = rng.choice(big, g)
        pos = starts[d][:, None] + (rng.random((g, m)) * (ends[d] - starts[d] - NGRAM - 1)[:, None]).astype(np.int64)
    else:
        pos = rng.integers(0, n - NGRAM, (g, m))
    buf = t[(pos.reshape(-1, 1) + np.arange(NGRAM)).reshape(-1)].astype(np.int32)
    return buf, (np.arange(g * m + 1) * NGRAM).astype(np.uint64), (np.arange(g + 1) * m).astype(np.uint64)


def parent_formulation(h, sp, goff, b):
    """documents holding all n-grams of the first b groups the parent commit's way; -> ([sorted document arrays], wall ms)"""
    t0 = time.perf_counter()
    out = []
    for i in range(b):
        both = None
        for j in range(int(goff[i]), int(goff[i + 1])):
            one = np.zeros(1, _capi.SPAN_DTYPE)
            one["first"], one["count"] = sp[j, 0], sp[j, 1]
            cap = max(int(sp[j, 1]), 1)                            # uncapped: no list is longer than the span
            d_d = torch.zeros(cap, dtype=torch.int32, device="cuda:0")
            f_d = torch.zeros(cap, dtype=torch.int32, device="cuda:0")
            h_d = torch.zeros(4, dtype=torch.int32, device="cuda:0")
            s_d = torch.from_numpy(one.view(np.int32).copy()).to("cuda:0")
            h.docs_batch_device(s_d.data_ptr(), 1, cap, 0, d_d.data_ptr(), f_d.data_ptr(), h_d.data_ptr())
            h.sync()
            docs = d_d[:int(h_d[0].item())].cpu().numpy()
            both = docs if both is None else np.intersect1d(both, docs)
        out.append(np.sort(both))
    return out, (time.perf_counter() - t0) * 1e3


def main():
    n, q, g, reps = arg("--n", 100_000_000), arg("--q", 1_000_000), arg("--g", 200_000), arg("--reps", 20)
    base_g = min(arg("--base-g", 500), g)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    t = zipf_tokens(n, VOCAB, seed=1)
    starts = make_documents(t)
    t_d = torch.from_numpy(t).to("cuda:0")
    sa_d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = _capi.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), n, VOCAB + 1)
    h = _capi.TokenIndex.load_device(t_d.data_ptr(), sa_d.data_ptr(), n)
    del sa_d
    h.set_documents(starts)
    prep = []
    for rep in range(3):                                           # the first builds its buffers
        h.prepare_doc_ranks(False)
        h.prepare_doc_ranks(True)
        if rep:
            prep.append(h.doc_ranks_info()["prepare_ms"])
    info = h.doc_ranks_info()
    res = {"tool": "gpu_token_all", "n": n, "vocab": VOCAB + 1, "documents": int(starts.size), "q": q, "groups": g, "reps": reps, "cap": CAP,
           "build_device_ms": round(st["total_ms"], 3), "rank_bytes": info["bytes"], "sort_passes": info["sort_passes"],
           "prepare_doc_ranks": med(prep), "batches": {}}
    ok = True
    # the listing chained into the counts of its rows
    buf, off, mode = make_batches(t, q)["exact"]
    p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
    sp_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
    d_d, f_d = torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0"), torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0")
    c_d, h_d = torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0"), torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    h.spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, mode, 0, 0, sp_d.data_ptr())
    ms = {"list": [], "doc_counts": []}
    for rep in range(reps + 2):
        h.docs_batch_device(sp_d.data_ptr(), q, CAP, 0, d_d.data_ptr(), f_d.data_ptr(), h_d.data_ptr())
        h.doc_counts_batch_device(sp_d.data_ptr(), q, CAP, d_d.data_ptr(), h_d.data_ptr(), 16, c_d.data_ptr())
        a, b = h.docs_info()["docs_ms"], h.doc_ranks_info()["counts_ms"]   # wait for the launches
        if rep >= 2:
            ms["list"].append(a)
            ms["doc_counts"].append(b)
    sp, hd, docs, cnt = sp_d.cpu().numpy().view(np.uint32), h_d.cpu().numpy().view(np.uint32), d_d.cpu().numpy(), c_d.cpu().numpy()
    sampled = True
    small = np.flatnonzero(sp[:, 1].astype(np.int64) <= 2_000_000)
    for i in np.random.default_rng(5).choice(small, 16, replace=False):
        pos = h.sa_range(int(sp[i, 0]), int(sp[i, 1])).astype(np.int64)
        d = np.searchsorted(starts, pos, "right") - 1
        w = int(hd[i, 0])
        sampled = sampled and cnt[i, :w].tolist() == [int((d == x).sum()) for x in docs[i, :w].tolist()]
    ok = ok and sampled
    res["chain"] = {k: med(v) for k, v in ms.items()}
    res["chain"]["cells_counted"] = int(hd[:, 0].sum())
    res["chain"]["sample_equals_host_count"] = bool(sampled)
    del p_d, o_d, sp_d, d_d, f_d, c_d, h_d
    # AND groups
    for bname, m, inside in (("inside_2", 2, True), ("inside_3", 3, True), ("random_2", 2, False), ("random_3", 3, False)):
        buf, off, goff = make_groups(t, starts, g, m, inside, seed=7 + m)
        S = g * m
        p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
        sp_d = torch.zeros((S, 4), dtype=torch.int32, device="cuda:0")
        d_d, f_d = torch.zeros((g, CAP), dtype=torch.int32, device="cuda:0"), torch.zeros((g, CAP), dtype=torch.int32, device="cuda:0")
        a_d = torch.zeros((g, 8), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        h.spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), S, 0, 0, 0, sp_d.data_ptr())
        ms = {"count": [], "list": []}
        for rep in range(reps + 2):
            for kind, cap in (("count", 0), ("list", CAP)):
                h.all_batch_device(sp_d.data_ptr(), S, goff, cap, 0, d_d.data_ptr() if cap else None, f_d.data_ptr() if cap else None,
                                   a_d.data_ptr())
                v = h.doc_ranks_info()["all_ms"]
                if rep >= 2:
                    ms[kind].append(v)
        sp, ah, docs = sp_d.cpu().numpy().view(np.uint32), a_d.cpu().numpy().view(np.uint32), d_d.cpu().numpy()
        pick = np.sort(np.random.default_rng(5).choice(min(base_g, g), 16, replace=False))
        want, wall = parent_formulation(h, sp, goff, min(base_g, g))
        sampled = all(int(ah[i, 2]) == want[i].size and int(ah[i, 1]) == int(ah[i, 5]) and
                      set(docs[i, :int(ah[i, 0])].tolist()) <= set(want[i].tolist()) for i in pick)
        agree = [int(x.size) for x in want] == ah[:len(want), 2].tolist()
        ok = ok and sampled and agree
        b = {k: med(v) for k, v in ms.items()}
        b.update({"spans_per_group": m, "ranks_walked": int(ah[:, 1].astype(np.int64).sum()), "candidates": int(ah[:, 3].astype(np.int64).sum()),
                  "matched": int(ah[:, 2].astype(np.int64).sum()), "groups_with_a_match": int((ah[:, 2] > 0).sum()),
                  "sample_equals_parent_formulation": bool(sampled),
                  "parent_formulation": {"groups": len(want), "wall_ms": round(wall, 3), "agree": bool(agree),
                                         "note": "an uncapped documents list per n-gram, np.intersect1d on the host"}})
        res["batches"][bname] = b
        del p_d, o_d, sp_d, d_d, f_d, a_d
    h.close()
    res["gate_ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
