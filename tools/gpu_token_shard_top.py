"""Top-k next symbols and draws over a shard set on the device: one JSON line with, for n Zipf tokens over a 50 257-word vocabulary
cut into S equal shards (S = 1, 4, 8) and the two batches of Q contexts of tools/gpu_token_next.py (the same corpus, the same seeds) --

  * HIP-event times after two warm-ups, median, minimum and maximum over the repetitions, every launch taking its turn inside every
    repetition: the set's top launch at k = 1, 8 and 64 with budget 0 and 65 536 in both plans of SA_HIP_TOKEN_SHARD_TOP_FAST (two sets
    over the same device arrays), the set's sample launch at m = 1 and 16, and beside them the shards' own top launches on their
    slices of the spans (their sum: at S = 1 the single index's launch and the ratio to it; at S > 1 the cost of walking the same
    ranks without merging them -- another question, a floor)
  * what the batch looks like: the share of contexts with one live shard (the fast path), the mean and the largest number of distinct
    continuations, contexts the budget cuts
  * gate: 16 sampled contexts per batch -- the top-64 entries, every head field, the budgeted top-64 and all 16 draws equal a count of
    the windows of all shards on the host; the two plans give the same bytes
  * the parent's only exact formulation: the set's next_batch at a cap that completes every span, the rows ordered on the host, on the
    largest prefix of the "exact" batch that Q * cap < 2^31 and the host's memory hold: wall time of both ways from host contexts to
    host top-64, and that they agree

    python tools/gpu_token_shard_top.py [--n N] [--q Q] [--reps R] [--base-q B] [--shards 1,4,8] [--out FILE]
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
from gpu_token_next import VOCAB, CTX, arg, make_batches, window_next  # noqa: E402
from gpu_token_top import KS, BUDGETS, MS, BASE_CELLS, note, top_of, stats  # noqa: E402

FAST = "SA_HIP_TOKEN_SHARD_TOP_FAST"
I32 = dict(dtype=torch.int32, device="cuda:0")
I64 = dict(dtype=torch.int64, device="cuda:0")


def make_set(t_d, sa_d, cuts, fast):
    """a set over the slices [cuts[s], cuts[s + 1]) of the device text and their suffix arrays; the switch is read at creation"""
    os.environ[FAST] = str(fast)
    idx = [_capi.TokenIndex.load_device(t_d[a:b].data_ptr(), sa_d[a:b].data_ptr(), b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    return _capi.TokenShards.create(idx)


def gate(slices, buf, off, sp, tops, draws, picks, q):
    """16 sampled contexts against window counts over all shards: sp uint32[S, q, 4], tops = {budget: (symbols, counts, heads)} at
    k = 64, picks = (symbols, shards) of the draws"""
    ok = True
    for i in np.random.default_rng(5).integers(0, q, 16):
        p = buf[int(off[i]):int(off[i + 1])]
        p = p[len(p) - int(sp[:, i, 2].max()):]
        per = [window_next(t, p) if t.size > len(p) else {} for t in slices]
        want = {}
        for d in per:
            for s, c in d.items():
                want[s] = want.get(s, 0) + c
        total = sum(want.values())
        syms = sorted(want)
        for budget, (sy, ct, hd) in tops.items():
            walked = want
            if budget and total > budget:                         # the first `budget` merged continuations: ascending symbols, the last one cut
                walked, left = {}, budget
                for s in syms:
                    if left == 0:
                        break
                    walked[s] = min(want[s], left)
                    left -= walked[s]
            h = hd[i]
            w = int(h["written"])
            mine = list(zip(sy[i, :w].tolist(), ct[i, :w].tolist()))
            ok = ok and mine == top_of(walked, 64) and int(h["distinct"]) == len(walked) and int(h["total"]) == total
            ok = ok and int(h["covered"]) == sum(c for _, c in mine) and int(h["shards"]) == sum(1 for d in per if d)
            ok = ok and int(h["length"]) == len(p)
        # the shard-major numbering: every shard's continuations in ascending symbol order, the shards one after another
        flat_s, flat_e, flat_sh, before = [], [], [], 0
        for s, d in enumerate(per):
            for y in sorted(d):
                before += d[y]
                flat_s.append(y)
                flat_e.append(before)
                flat_sh.append(s)
        for d, y, s in zip(draws[i].tolist(), picks[0][i].tolist(), picks[1][i].tolist()):
            r = (int(d) * total) >> 64
            j = int(np.searchsorted(flat_e, r, side="right")) if total else -1
            ok = ok and ((y, s) == ((flat_s[j], flat_sh[j]) if total else (-1, 0xFFFFFFFF)))
    return bool(ok)


def key_of(symbols, counts, written, width):
    """count << 32 | ~symbol per cell (counts of this corpus stay below 2^32), 0 beyond written"""
    key = (counts.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - symbols.view(np.uint32).astype(np.uint64))
    key[np.arange(width)[None, :] >= written[:, None]] = 0
    return key


def parent_top(st, buf, off, b, cap):
    """the parent's way: every span complete at `cap`, all rows to the host, ordered there -> keys[b, 64], complete, wall ms"""
    t0 = time.perf_counter()
    r = st.next_batch((buf[:int(off[b])], off[:b + 1]), cap=cap, mode=0)
    key = key_of(r["symbols"], r["counts"], r["heads"]["written"], cap)
    k = min(64, cap)
    part = np.partition(key, cap - k, axis=1)[:, cap - k:] if cap > k else key
    part = np.ascontiguousarray(np.sort(part, axis=1)[:, ::-1])   # descending: count descending, then symbol ascending
    wall = (time.perf_counter() - t0) * 1e3
    return part, bool((r["heads"]["covered"] == r["heads"]["total"]).all()), wall


def run_set(t, t_d, sa_d, S, q, reps, base_q, batches):
    n = t.size
    cuts = [n * s // S for s in range(S + 1)]
    slices = [t[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    build_ms = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        build_ms += _capi.libsais_int_device(t_d[a:b].data_ptr(), sa_d[a:b].data_ptr(), b - a, VOCAB)["total_ms"]
    sets = {fast: make_set(t_d, sa_d, cuts, fast) for fast in (1, 0)}
    os.environ.pop(FAST, None)
    note("S =", S, "sets ready")
    rec = {"shards": S, "build_device_ms": round(build_ms, 3), "batches": {}}
    ok = True
    for bname, (buf, off, mode) in batches.items():
        p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
        sp_d, ln_d, tt_d = torch.zeros((S, q, 4), **I32), torch.zeros(q, **I32), torch.zeros(q, **I64)
        sy_d = {(f, b): torch.zeros((q, 64), **I32) for f in sets for b in BUDGETS}   # (smaller k write the front of the same buffers)
        ct_d = {(f, b): torch.zeros((q, 64), **I64) for f in sets for b in BUDGETS}
        hd_d = {(f, b): torch.zeros((q, 8), **I32) for f in sets for b in BUDGETS}
        osy_d, oct_d, ohd_d = torch.zeros((q, 64), **I32), torch.zeros((q, 64), **I32), torch.zeros((q, 4), **I32)
        draws = np.random.default_rng(9).integers(0, 2 ** 64, size=(q, max(MS)), dtype=np.uint64)
        dr_d = torch.from_numpy(draws.view(np.int64)).to("cuda:0")
        pk_d, ps_d = torch.zeros((q, max(MS)), **I32), torch.zeros((q, max(MS)), **I32)
        torch.cuda.synchronize()
        for st in sets.values():
            st.spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, mode, 0, 1, ln_d.data_ptr(), tt_d.data_ptr(), sp_d.data_ptr())
            st.sync()
        ms = {("top", f, k, b): [] for f in sets for k in KS for b in BUDGETS}
        ms.update({("own", k, b): [] for k in KS for b in BUDGETS})
        ms.update({("sample", m): [] for m in MS})
        for rep in range(reps + 2):                               # two warm-up rounds; k = 64 and m = 16 run last and leave the answers
            for b in BUDGETS:
                for k in KS:
                    for f, st in sets.items():
                        st.top_batch_device(sp_d.data_ptr(), q, k, b, sy_d[f, b].data_ptr(), ct_d[f, b].data_ptr(), hd_d[f, b].data_ptr())
                        v = st.top_info()["top_ms"]
                        if rep >= 2:
                            ms["top", f, k, b].append(v)
                    own = 0.0                                     # the shards' own launches on their slices of the spans
                    for s in range(S):
                        h = sets[1].shard(s)
                        h.top_batch_device(sp_d[s].data_ptr(), q, k, b, osy_d.data_ptr(), oct_d.data_ptr(), ohd_d.data_ptr())
                        own += h.top_info()["top_ms"]
                    if rep >= 2:
                        ms["own", k, b].append(own)
            for m in MS:
                sets[1].sample_batch_device(sp_d.data_ptr(), q, dr_d.data_ptr(), m, pk_d.data_ptr(), ps_d.data_ptr(), None)
                v = sets[1].top_info()["sample_ms"]
                if rep >= 2:
                    ms["sample", m].append(v)
            note("S", S, bname, "rep", rep, round(v, 3))
        sp = sp_d.cpu().numpy().view(np.uint32)
        got = {key: (sy_d[key].cpu().numpy(), ct_d[key].cpu().numpy().view(np.uint64),
                     hd_d[key].cpu().numpy().view(_capi.SHARDS_TOP_DTYPE).reshape(q)) for key in sy_d}
        same = all(all(np.array_equal(x, y) for x, y in zip(got[1, b], got[0, b])) for b in BUDGETS)
        picks = (pk_d.cpu().numpy(), ps_d.cpu().numpy().view(np.uint32))
        counted = gate(slices, buf, off, sp, {b: got[1, b] for b in BUDGETS}, draws, picks, q)
        ok = ok and counted and same
        hd0 = got[1, 0][2]
        r = {"mean_length": round(float(hd0["length"].mean()), 3), "one_live_shard": int((hd0["shards"] == 1).sum()),
             "no_live_shard": int((hd0["shards"] == 0).sum()), "contexts_cut_by_budget_65536": int((hd0["total"] > 65536).sum()),
             "mean_distinct": round(float(hd0["distinct"].mean()), 2), "max_distinct": int(hd0["distinct"].max()),
             "mean_total": round(float(hd0["total"].mean()), 1), "top": {}, "own_launches_sum": {}, "sample": {},
             "answers_equal_window_counts": counted, "plans_give_the_same_bytes": bool(same)}
        for k in KS:
            for b in BUDGETS:
                own = stats(ms["own", k, b])
                r["own_launches_sum"]["k%d_budget%d" % (k, b)] = own
                for f in sets:
                    s = stats(ms["top", f, k, b])
                    s["ratio_to_own_launches"] = round(s["median_ms"] / own["median_ms"], 3)
                    r["top"]["fast%d_k%d_budget%d" % (f, k, b)] = s
        for m in MS:
            r["sample"]["m%d" % m] = stats(ms["sample", m])
        rec["batches"][bname] = r
        if mode == 0:
            # the parent's formulation on a prefix: the cap that completes every span of it is its largest number of distinct continuations
            st = sets[1]
            b = min(base_q, q)
            while True:                                           # (the cap does not grow as the prefix shrinks)
                cap = max(int(hd0["distinct"][:b].max()), 1)
                if b * cap <= BASE_CELLS or b == 1:
                    break
                b = max(min(BASE_CELLS // cap, b - 1), 1)
            note("parent formulation on", b, "contexts, cap", cap)
            sub = (buf[:int(off[b])], off[:b + 1])
            st.top_batch(sub, k=64, mode=0)                       # warm-up: the staging buffers of both ways
            t0 = time.perf_counter()
            mine = st.top_batch(sub, k=64, mode=0)
            new_wall = (time.perf_counter() - t0) * 1e3
            parent_top(st, buf, off, min(b, 64), cap)             # warm-up
            part, complete, wall = parent_top(st, buf, off, b, cap)
            mk = key_of(mine["symbols"], mine["counts"], mine["heads"]["written"], 64)
            kk = min(64, cap)
            agree = bool(complete and np.array_equal(mk[:, :kk], part) and (mk[:, kk:] == 0).all())
            ok = ok and agree
            rec["parent_formulation"] = {"batch": bname, "contexts": b, "cap": cap, "cells": b * cap, "chunk": st.info()["chunk"],
                                         "wall_ms": round(wall, 3), "top_batch_wall_ms": round(new_wall, 3),
                                         "ratio": round(wall / new_wall, 1), "answers_agree": agree,
                                         "note": "parent: the set's next_batch at a cap that completes every span, rows to the host, "
                                                 "np.partition + sort of count << 32 | ~symbol there; new: the set's top_batch(k = 64) "
                                                 "host form; same contexts"}
        del p_d, o_d, sp_d, sy_d, ct_d, hd_d, osy_d, oct_d, ohd_d, dr_d, pk_d, ps_d
    for st in sets.values():
        st.close()
    return rec, ok


def main():
    n, q, reps, base_q = arg("--n", 100_000_000), arg("--q", 1_000_000), arg("--reps", 20), arg("--base-q", 20_000)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    shards = [int(v) for v in (sys.argv[sys.argv.index("--shards") + 1] if "--shards" in sys.argv else "1,4,8").split(",")]
    t = zipf_tokens(n, VOCAB, seed=1)
    note("text ready")
    t_d = torch.from_numpy(t).to("cuda:0")
    sa_d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    batches = make_batches(t, q)
    res = {"tool": "gpu_token_shard_top", "n": n, "vocab": VOCAB, "q": q, "reps": reps, "context_length": CTX, "sets": {}}
    ok = True
    for S in shards:
        rec, good = run_set(t, t_d, sa_d, S, q, reps, base_q, batches)
        res["sets"]["S%d" % S] = rec
        ok = ok and good
        res["gate_ok"] = bool(ok)
        if out_path:                                              # (after every set: a run cut short keeps what it has)
            with open(out_path, "w") as f:
                f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
