"""Top-k next symbols and draws from a span on the device: one JSON line with, for n Zipf tokens over a 50 257-word vocabulary and
the two batches of Q contexts of tools/gpu_token_next.py (the same corpus, the same seeds) --

  * HIP-event times after two warm-ups, median, minimum and maximum over the repetitions, every launch taking its turn inside every
    repetition: the top launch at k = 1, 8 and 64 with budget 0 and 65 536, the sample launch at m = 1 and 16, and beside them the
    next launch at cap 64 (sa_hip_token_top_info / sa_hip_token_next_info); the ratio top / next per row, as measured
  * what the batch looks like: spans whose next answer is complete at cap 64, spans the budget cuts, the mean and the largest number
    of distinct continuations
  * gate: 16 sampled contexts per batch -- the top-64 entries, distinct and total, the budgeted top-64 and all 16 draws equal a count
    of the text's windows on the host
  * the parent's only formulation of top-k: next_batch with a cap that makes every span complete, the rows ordered on the host.
    Q * cap < 2^31 and the host's memory hold it to a subset of the "exact" batch (its size is in the record): wall time of both
    ways from host contexts to host top-64 on that subset, and that they agree

    python tools/gpu_token_top.py [--n N] [--q Q] [--reps R] [--base-q B] [--out FILE]
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
from gpu_token_next import VOCAB, CAP, CTX, arg, make_batches, window_next  # noqa: E402

KS = (1, 8, 64)
BUDGETS = (0, 65536)
MS = (1, 16)
BASE_CELLS = 1 << 27                          # Q * cap of the parent's formulation: four host arrays of that many cells


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def top_of(want, k):
    return sorted(want.items(), key=lambda p: (-p[1], p[0]))[:k]


def stats(v):
    v = np.array(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}


def gate(t, buf, off, sp, tops, draws, picks, q):
    """16 sampled contexts against window counts: tops = {budget: (symbols, counts, heads)} at k = 64, picks = symbols of draws"""
    ok = True
    for i in np.random.default_rng(5).integers(0, q, 16):
        p = buf[int(off[i]):int(off[i + 1])]
        p = p[len(p) - int(sp[i, 2]):]
        want = window_next(t, p)
        total = sum(want.values())
        syms = sorted(want)
        flat_edges = np.cumsum([want[s] for s in syms])
        for budget, (sy, ct, hd) in tops.items():
            walked = want
            if budget and total > budget:                         # the first `budget` ranks: ascending symbols, the last one cut
                walked, left = {}, budget
                for s in syms:
                    if left == 0:
                        break
                    walked[s] = min(want[s], left)
                    left -= walked[s]
            w = int(hd[i, 0])
            mine = list(zip(sy[i, :w].tolist(), ct[i, :w].tolist()))
            ok = ok and mine == top_of(walked, 64) and int(hd[i, 1]) == len(walked) and int(hd[i, 3]) == total
            ok = ok and int(hd[i, 2]) == sum(c for _, c in mine)
        for d, s in zip(draws[i].tolist(), picks[i].tolist()):
            r = (int(d) * total) >> 64
            ok = ok and (s == (syms[int(np.searchsorted(flat_edges, r, side="right"))] if total else -1))
    return bool(ok)


def parent_top(h, buf, off, b, cap):
    """the parent's way: every span complete at `cap`, all rows to the host, ordered there -> (symbols, counts)[b, 64], wall ms"""
    t0 = time.perf_counter()
    r = h.next_batch((buf[:int(off[b])], off[:b + 1]), cap=cap, mode=0)
    key = (r["counts"].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - r["symbols"].view(np.uint32).astype(np.uint64))
    key[np.arange(cap)[None, :] >= r["heads"]["written"][:, None]] = 0
    k = min(64, cap)
    part = np.partition(key, cap - k, axis=1)[:, cap - k:] if cap > k else key
    part = np.ascontiguousarray(np.sort(part, axis=1)[:, ::-1])   # descending: count descending, then symbol ascending
    wall = (time.perf_counter() - t0) * 1e3
    return part, bool((r["heads"]["covered"] == r["heads"]["total"]).all()), wall


def main():
    n, q, reps, base_q = arg("--n", 100_000_000), arg("--q", 1_000_000), arg("--reps", 20), arg("--base-q", 20_000)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    t = zipf_tokens(n, VOCAB, seed=1)
    note("text ready")
    t_d = torch.from_numpy(t).to("cuda:0")
    sa_d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = _capi.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), n, VOCAB)
    h = _capi.TokenIndex.load_device(t_d.data_ptr(), sa_d.data_ptr(), n)
    del sa_d
    note("index ready")
    res = {"tool": "gpu_token_top", "n": n, "vocab": VOCAB, "q": q, "reps": reps, "context_length": CTX, "next_cap": CAP,
           "build_device_ms": round(st["total_ms"], 3), "batches": {}}
    ok = True
    for bname, (buf, off, mode) in make_batches(t, q).items():
        p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
        sp_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
        sy_d = {b: torch.zeros((q, 64), dtype=torch.int32, device="cuda:0") for b in BUDGETS}   # (smaller k write the front of the same buffers)
        ct_d = {b: torch.zeros((q, 64), dtype=torch.int32, device="cuda:0") for b in BUDGETS}
        hd_d = {b: torch.zeros((q, 4), dtype=torch.int32, device="cuda:0") for b in BUDGETS}
        nsy_d, nct_d = torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0"), torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0")
        nhd_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
        draws = np.random.default_rng(9).integers(0, 2 ** 64, size=(q, max(MS)), dtype=np.uint64)
        dr_d = torch.from_numpy(draws.view(np.int64)).to("cuda:0")
        pk_d = torch.zeros((q, max(MS)), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        h.spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, mode, 0, 1, sp_d.data_ptr())
        ms = {("top", k, b): [] for k in KS for b in BUDGETS}
        ms.update({("sample", m): [] for m in MS})
        ms["next"] = []
        for rep in range(reps + 2):                               # two warm-up rounds; k = 64 and m = 16 run last and leave the answers
            for b in BUDGETS:
                for k in KS:
                    h.top_batch_device(sp_d.data_ptr(), q, k, b, sy_d[b].data_ptr(), ct_d[b].data_ptr(), hd_d[b].data_ptr())
                    v = h.top_info()["top_ms"]
                    if rep >= 2:
                        ms["top", k, b].append(v)
            for m in MS:
                h.sample_batch_device(sp_d.data_ptr(), q, dr_d.data_ptr(), m, pk_d.data_ptr(), None)
                v = h.top_info()["sample_ms"]
                if rep >= 2:
                    ms["sample", m].append(v)
            h.next_batch_device(sp_d.data_ptr(), q, CAP, nsy_d.data_ptr(), nct_d.data_ptr(), nhd_d.data_ptr())
            v = h.next_info()["next_ms"]
            if rep >= 2:
                ms["next"].append(v)
            note(bname, "rep", rep, round(v, 3))
        sp = sp_d.cpu().numpy().view(np.uint32)
        # k = 64 ran over [q, 64] rows; m = 16 over [q, 16]
        tops = {b: (sy_d[b].cpu().numpy(), ct_d[b].cpu().numpy().view(np.uint32), hd_d[b].cpu().numpy().view(np.uint32)) for b in BUDGETS}
        picks = pk_d.cpu().numpy()
        nhd = nhd_d.cpu().numpy().view(np.uint32)
        counted = gate(t, buf, off, sp, tops, draws, picks, q)
        hd0 = tops[0][2]
        full = nhd[:, 1] == nhd[:, 2]
        agree = bool(np.array_equal(hd0[:, 3], nhd[:, 2]) and np.array_equal(hd0[full, 1], nhd[full, 0]))
        ok = ok and counted and agree
        nx = stats(ms["next"])
        rec = {"mean_length": round(float(sp[:, 2].mean()), 3), "next_complete_at_cap_64": int(full.sum()),
               "spans_cut_by_budget_65536": int((hd0[:, 3] > 65536).sum()), "mean_distinct": round(float(hd0[:, 1].mean()), 2),
               "max_distinct": int(hd0[:, 1].max()), "mean_total": round(float(hd0[:, 3].mean()), 1),
               "next": nx, "top": {}, "sample": {}, "sample_equals_window_count": counted, "heads_agree_with_next": agree}
        for k in KS:
            for b in BUDGETS:
                s = stats(ms["top", k, b])
                s["ratio_to_next"] = round(s["median_ms"] / nx["median_ms"], 3)
                rec["top"]["k%d_budget%d" % (k, b)] = s
        for m in MS:
            rec["sample"]["m%d" % m] = stats(ms["sample", m])
        res["batches"][bname] = rec
        if mode == 0:
            # the parent's formulation on a subset: the cap that completes every span of it is its largest number of distinct continuations
            b = min(base_q, q)
            while True:                                           # (the cap does not grow as the subset shrinks)
                cap = max(int(hd0[:b, 1].max()), 1)
                if b * cap <= BASE_CELLS or b == 1:
                    break
                b = max(min(BASE_CELLS // cap, b - 1), 1)
            note("parent formulation on", b, "contexts, cap", cap)
            sub = (buf[:int(off[b])], off[:b + 1])
            h.top_batch(sub, k=64, mode=0)                        # warm-up: the staging buffers of both ways
            t0 = time.perf_counter()
            mine = h.top_batch(sub, k=64, mode=0)
            new_wall = (time.perf_counter() - t0) * 1e3
            parent_top(h, buf, off, min(b, 64), cap)              # warm-up
            part, complete, wall = parent_top(h, buf, off, b, cap)
            mk = (mine["counts"].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - mine["symbols"].view(np.uint32).astype(np.uint64))
            mk[np.arange(64)[None, :] >= mine["heads"]["written"][:, None]] = 0
            kk = min(64, cap)
            same = bool(complete and np.array_equal(mk[:, :kk], part) and (mk[:, kk:] == 0).all())
            ok = ok and same
            res["parent_formulation"] = {"batch": bname, "contexts": b, "cap": cap, "cells": b * cap, "wall_ms": round(wall, 3),
                                         "top_batch_wall_ms": round(new_wall, 3), "ratio": round(wall / new_wall, 1), "answers_agree": same,
                                         "note": "parent: next_batch at a cap that completes every span, rows to the host, np.partition + "
                                                 "sort of count << 32 | ~symbol there; new: top_batch(k = 64) host form; same contexts"}
        del p_d, o_d, sp_d, sy_d, ct_d, hd_d, nsy_d, nct_d, nhd_d, dr_d, pk_d
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
