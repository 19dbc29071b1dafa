"""Documents of the token index on the device: one JSON line with, for n Zipf tokens over a 50 257-word vocabulary cut into
documents of Zipf-ish length by a separator token, and the two batches of Q contexts of tools/gpu_token_next.py --

  * set_documents: HIP-event times of its document-array pass, its sort of the ranks by document and its previous-rank pass
  * per batch, HIP-event medians over the repetitions after two warm-ups (sa_hip_token_docs_info) of
      counts only (cap 0) with budget 0 and with budget 4096, the listing at cap 16, locate at cap 16
  * the share of the counting launch's time that its 100 longest spans take when launched alone: what a multi-wave split of
    long spans could win at most
  * gates: 16 sampled answers per batch equal the host formulation below, and the sum of `examined` that docs_info reports equals
    the sum computed from the spans
  * the parent's only formulation: ranges, then per n-gram sa_range, searchsorted over the boundary table and unique on the host;
    wall time over the first --base-q contexts of the exact batch (--base-seconds S stops it early and says how far it came)

    python tools/gpu_token_docs.py [--n N] [--q Q] [--reps R] [--base-q B] [--base-seconds S] [--out FILE]
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

CAP = 16
BUDGET = 4096
SEP = VOCAB                                    # the separator: a token of its own behind every document
LONGEST = 100


def arg(name, default):
    return int(float(sys.argv[sys.argv.index(name) + 1])) if name in sys.argv else default


def make_documents(t, seed=3):
    """document starts of Zipf-ish lengths (16 tokens times a Zipf(1.3) draw, at most a million); t gets SEP at every document's end"""
    rng = np.random.default_rng(seed)
    n = t.size
    lens = np.minimum(rng.zipf(1.3, max(n // 16, 1)), 1_000_000 // 16).astype(np.int64) * 16      # (cut first: 16 times a large draw wraps)
    ends = np.cumsum(lens)
    ends = ends[ends < n]
    starts = np.concatenate([[0], ends]).astype(np.int32)
    t[np.concatenate([ends - 1, [n - 1]])] = SEP
    return starts


def host_formulation(h, starts, buf, off, b, seconds):
    """distinct documents of the first b n-grams the parent commit's way; -> (distinct list, wall ms, n-grams done)"""
    t0 = time.perf_counter()
    r = h.query_batch((buf[:int(off[b])], off[:b + 1]))
    out = []
    for i in range(b):
        pos = h.sa_range(int(r["first"][i]), int(r["second"][i]))
        out.append(int(np.unique(np.searchsorted(starts, pos, "right")).size))
        if seconds and time.perf_counter() - t0 > seconds:
            break
    return out, (time.perf_counter() - t0) * 1e3, len(out)


def med(v):
    v = np.array(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}


def main():
    n, q, reps = arg("--n", 100_000_000), arg("--q", 1_000_000), arg("--reps", 20)
    base_q, base_seconds = min(arg("--base-q", 100_000), q), arg("--base-seconds", 0)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    t = zipf_tokens(n, VOCAB, seed=1)
    starts = make_documents(t)
    t_d = torch.from_numpy(t).to("cuda:0")
    sa_d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = _capi.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), n, VOCAB + 1)
    h = _capi.TokenIndex.load_device(t_d.data_ptr(), sa_d.data_ptr(), n)
    del sa_d
    prep = {"da": [], "sort": [], "pv": [], "total": []}
    for rep in range(3):                                           # the first builds its buffers
        h.set_documents(starts)
        info = h.docs_info()
        if rep:
            for k, f in (("da", "da_ms"), ("sort", "sort_ms"), ("pv", "pv_ms"), ("total", "prepare_ms")):
                prep[k].append(info[f])
    res = {"tool": "gpu_token_docs", "n": n, "vocab": VOCAB + 1, "documents": int(starts.size), "q": q, "reps": reps, "cap": CAP,
           "budget": BUDGET, "build_device_ms": round(st["total_ms"], 3), "structure_bytes": info["bytes"], "sort_passes": info["sort_passes"],
           "set_documents": {k: med(v) for k, v in prep.items()}, "batches": {}}
    ok = True
    for bname, (buf, off, mode) in make_batches(t, q).items():
        p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
        sp_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
        d_d, f_d = torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0"), torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0")
        h_d, l_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0"), torch.zeros((q, 2), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        h.spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, mode, 0, 0, sp_d.data_ptr())
        h.sync()
        sp = sp_d.cpu().numpy().view(np.uint32)
        count = sp[:, 1].astype(np.int64)
        kinds = {"count_all": (0, 0), "count_budget": (0, BUDGET), "list": (CAP, 0)}
        ms = {k: [] for k in list(kinds) + ["locate"]}
        sums_ok = True
        for rep in range(reps + 2):
            for kind, (cap, budget) in kinds.items():
                h.docs_batch_device(sp_d.data_ptr(), q, cap, budget, d_d.data_ptr() if cap else None, f_d.data_ptr() if cap else None, h_d.data_ptr())
                info = h.docs_info()                               # waits for the launch
                sums_ok = sums_ok and info["examined"] == int((np.minimum(count, budget) if budget else count).sum())
                if rep >= 2:
                    ms[kind].append(info["docs_ms"])
            h.locate_batch_device(sp_d.data_ptr(), q, CAP, d_d.data_ptr(), f_d.data_ptr(), l_d.data_ptr())
            info = h.docs_info()
            if rep >= 2:
                ms["locate"].append(info["locate_ms"])
        # the 100 longest spans alone
        top = np.argsort(-count, kind="stable")[:LONGEST]
        top_d = torch.from_numpy(sp[top].view(np.int32).copy()).to("cuda:0")
        th_d = torch.zeros((LONGEST, 4), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        tops = []
        for rep in range(reps + 2):
            h.docs_batch_device(top_d.data_ptr(), top.size, 0, 0, None, None, th_d.data_ptr())
            info = h.docs_info()
            if rep >= 2:
                tops.append(info["docs_ms"])
        # gates: a last listing launch, 16 samples against the host formulation
        h.docs_batch_device(sp_d.data_ptr(), q, CAP, 0, d_d.data_ptr(), f_d.data_ptr(), h_d.data_ptr())
        h.sync()
        hd, docs, offs = h_d.cpu().numpy().view(np.uint32), d_d.cpu().numpy(), f_d.cpu().numpy()
        sampled = True
        small = np.flatnonzero(count <= 2_000_000)
        for i in np.random.default_rng(5).choice(small, 16, replace=False):
            pos = h.sa_range(int(sp[i, 0]), int(sp[i, 1])).astype(np.int64)
            d = np.searchsorted(starts, pos, "right") - 1
            first = d[np.sort(np.unique(d, return_index=True)[1])][:CAP]
            w = int(hd[i, 0])
            sampled = sampled and int(hd[i, 2]) == np.unique(d).size and int(hd[i, 1]) == int(hd[i, 3]) == pos.size and w == first.size
            sampled = sampled and docs[i, :w].tolist() == first.tolist()
            sampled = sampled and all(int(starts[docs[i, j]]) + int(offs[i, j]) in pos for j in range(w))
        ok = ok and sums_ok and sampled
        b = {k: med(v) for k, v in ms.items()}
        b["longest_%d_alone" % LONGEST] = med(tops)
        b["longest_%d_share_of_count_all" % LONGEST] = round(float(np.median(tops)) / b["count_all"]["median_ms"], 4)
        b["ranks_streamed_count_all"] = int(count.sum())
        b["ranks_streamed_count_budget"] = int(np.minimum(count, BUDGET).sum())
        b["longest_span"] = int(count.max())
        b["mean_distinct"] = round(float(hd[:, 2].mean()), 3)
        b["examined_sums_agree"] = bool(sums_ok)
        b["sample_equals_host_formulation"] = bool(sampled)
        if mode == 0:
            host_formulation(h, starts, buf, off, min(base_q, 200), 0)      # warm-up
            want, wall, done = host_formulation(h, starts, buf, off, base_q, base_seconds)
            agree = want == hd[:done, 2].tolist()
            ok = ok and agree
            b["parent_formulation"] = {"contexts_asked": base_q, "contexts_done": done, "wall_ms": round(wall, 3), "agree": bool(agree),
                                       "note": "ranges, then per n-gram sa_range + searchsorted + unique on the host"}
        res["batches"][bname] = b
        del p_d, o_d, sp_d, d_d, f_d, h_d, l_d
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
