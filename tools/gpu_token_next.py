"""Spans and next symbols of the token index on the device: one JSON line with, for n Zipf tokens over a 50 257-word vocabulary
(the recipe of tools/gpu_token_query.py) and Q contexts, the three plans of the next-symbol launch side by side --

  lanes      lane form + jump step        waves      every span by one wave, jump step (the default)        lanes_no_jump    lane form, window steps only

  * batch "exact": n-grams of length 1..8 cut from the text, mode 0, cap 64
  * batch "suffix": contexts of length 32 cut from the text with the symbol 1..8 places before the end replaced, mode 1, cap 64
  * HIP-event times of the span launch and of the next launch (sa_hip_token_next_info) after two warm-ups, median and minimum over
    the repetitions, the plans taking turns inside every repetition
  * gates: the plans answer identically, and a sample of the answers equals a count of the text's windows on the host
  * the parent's only formulation of "suffix": one query_batch over all 32 suffixes of each of the first --base-q contexts, the
    pick of the longest suffix that occurs on the host (the next symbols are not even fetched there); wall time, and its ratio
    to the device chain's time for the same number of contexts

    python tools/gpu_token_next.py [--n N] [--q Q] [--reps R] [--base-q B] [--out FILE]
"""
import json
import os
import sys
import time

os.environ.setdefault("SA_HIP_DIAG", "1")   # the plan switches are read only with this set

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (first: one HIP runtime per process)

from suffixarray_amd import _capi  # noqa: E402
from test_gpu_int import zipf_tokens  # noqa: E402

VOCAB = 50257
CAP = 64
CTX = 32
PLANS = {                                     # both switches set in every plan: the record does not depend on the defaults
    "waves": {"SA_HIP_TOKEN_NEXT_LANES": "0", "SA_HIP_TOKEN_NEXT_JUMP": "1"},
    "lanes": {"SA_HIP_TOKEN_NEXT_LANES": "1", "SA_HIP_TOKEN_NEXT_JUMP": "1"},
    "lanes_no_jump": {"SA_HIP_TOKEN_NEXT_LANES": "1", "SA_HIP_TOKEN_NEXT_JUMP": "0"},
}
FIRST = "waves"


def arg(name, default):
    return int(float(sys.argv[sys.argv.index(name) + 1])) if name in sys.argv else default


def make_batches(t, q, seed=11):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 9, q)
    pos = rng.integers(0, t.size - 8, q)
    off = np.zeros(q + 1, np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    within = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), lens)
    exact = t[np.repeat(pos, lens) + within].astype(np.int32)
    pos = rng.integers(0, t.size - CTX - 1, q)
    ctx = t[pos[:, None] + np.arange(CTX)[None, :]].astype(np.int32)
    back = rng.integers(1, 9, q)                                  # the symbol this many places before the end is replaced
    rows = np.arange(q)
    ctx[rows, CTX - 1 - back] = (ctx[rows, CTX - 1 - back] + rng.integers(1, VOCAB, q)) % VOCAB
    return {"exact": (exact, off, 0), "suffix": (ctx.reshape(-1), np.arange(q + 1, dtype=np.uint64) * CTX, 1)}


def window_next(t, p):
    """{symbol: count} behind the windows of the text equal to p"""
    idx = np.flatnonzero(t[:t.size - len(p)] == p[0]) if len(p) else np.arange(t.size)
    for j in range(1, len(p)):
        idx = idx[t[idx + j] == p[j]]
    s, c = np.unique(t[idx + len(p)], return_counts=True)
    return dict(zip(s.tolist(), c.tolist()))


def parent_formulation(h, ctx, b):
    """the longest suffix that occurs, the parent commit's way: all suffixes through query_batch, the pick on the host"""
    t0 = time.perf_counter()
    lens = np.tile(np.arange(CTX, 0, -1), b)
    off = np.zeros(b * CTX + 1, np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    start = np.repeat(np.arange(b) * CTX, CTX) + np.tile(np.arange(CTX), b)            # suffix j of context i starts at i * CTX + j
    within = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), lens)
    buf = ctx[np.repeat(start, lens) + within]
    r = h.query_batch((buf, off))
    hit = (r["second"].reshape(b, CTX) > 0)
    length = np.where(hit.any(axis=1), CTX - hit.argmax(axis=1), 0)
    return length, (time.perf_counter() - t0) * 1e3


def main():
    n, q, reps, base_q = arg("--n", 100_000_000), arg("--q", 1_000_000), arg("--reps", 20), arg("--base-q", 100_000)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    base_q = min(base_q, q)
    t = zipf_tokens(n, VOCAB, seed=1)
    t_d = torch.from_numpy(t).to("cuda:0")
    sa_d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = _capi.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), n, VOCAB)
    res = {"tool": "gpu_token_next", "n": n, "vocab": VOCAB, "q": q, "reps": reps, "cap": CAP, "context_length": CTX,
           "build_device_ms": round(st["total_ms"], 3), "plans": {p: {} for p in PLANS}}
    handles = {}
    for plan, env in PLANS.items():
        for k in ("SA_HIP_TOKEN_NEXT_LANES", "SA_HIP_TOKEN_NEXT_JUMP"):
            os.environ.pop(k, None)
        os.environ.update(env)
        handles[plan] = _capi.TokenIndex.load_device(t_d.data_ptr(), sa_d.data_ptr(), n)
    del sa_d
    ok = True
    for bname, (buf, off, mode) in make_batches(t, q).items():
        p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
        outs = {plan: (torch.zeros((q, 4), dtype=torch.int32, device="cuda:0"), torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0"),
                       torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0"), torch.zeros((q, 4), dtype=torch.int32, device="cuda:0"))
                for plan in PLANS}
        torch.cuda.synchronize()
        ms = {plan: {"spans": [], "next": []} for plan in PLANS}
        for rep in range(reps + 2):                               # two warm-up rounds, then the plans take turns
            for plan, h in handles.items():
                sp, sy, ct, hd = outs[plan]
                h.spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, mode, 0, 1, sp.data_ptr())
                h.next_batch_device(sp.data_ptr(), q, CAP, sy.data_ptr(), ct.data_ptr(), hd.data_ptr())
                info = h.next_info()                              # waits for both launches
                if rep >= 2:
                    ms[plan]["spans"].append(info["spans_ms"])
                    ms[plan]["next"].append(info["next_ms"])
                res["plans"][plan][bname + "_lane_spans"] = info["lane_spans"]
        got = {plan: [x.cpu().numpy() for x in o] for plan, o in outs.items()}
        hd = got[FIRST][3].view(np.uint32)
        sp = got[FIRST][0].view(np.uint32)
        # cells beyond `written` are not written (zeros here in every plan), so whole buffers compare
        same = all(all(np.array_equal(a, b) for a, b in zip(got[FIRST], g)) for g in got.values())
        counted = True
        for i in np.random.default_rng(5).integers(0, q, 16):
            p = buf[int(off[i]):int(off[i + 1])]
            p = p[len(p) - int(sp[i, 2]):]
            want = window_next(t, p)
            w = int(hd[i, 0])
            mine = dict(zip(got[FIRST][1][i, :w].tolist(), got[FIRST][2].view(np.uint32)[i, :w].tolist()))
            counted = counted and int(hd[i, 2]) == sum(want.values()) and w == min(len(want), CAP) and all(want[s] == c for s, c in mine.items())
            if mode == 1 and int(sp[i, 2]) < CTX:                 # and one symbol more matches nowhere with a next symbol
                longer = buf[int(off[i + 1]) - int(sp[i, 2]) - 1:int(off[i + 1])]
                counted = counted and not window_next(t, longer)
        ok = ok and same and counted
        for plan in PLANS:
            for kind in ("spans", "next"):
                v = np.array(ms[plan][kind])
                res["plans"][plan][bname + "_" + kind] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4),
                                                          "max_ms": round(float(v.max()), 4)}
        res[bname + "_mean_length"] = round(float(sp[:, 2].mean()), 3)
        res[bname + "_complete"] = int((hd[:, 1] == hd[:, 2]).sum())
        res[bname + "_plans_equal"] = bool(same)
        res[bname + "_sample_equals_window_count"] = bool(counted)
        if mode == 1:
            h = handles[FIRST]
            parent_formulation(h, buf, min(base_q, 1000))         # warm-up
            length, wall = parent_formulation(h, buf, base_q)
            # the parent's pick has no need_next: compare with a need_next = 0 launch of the same contexts
            sp0 = torch.zeros((base_q, 4), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), base_q, 1, 0, 0, sp0.data_ptr())
            h.sync()
            chain_wall = (time.perf_counter() - t0) * 1e3
            agree = bool(np.array_equal(sp0.cpu().numpy().view(np.uint32)[:, 2], length))
            ok = ok and agree
            res["parent_formulation"] = {"contexts": base_q, "wall_ms": round(wall, 3), "spans_launch_wall_ms": round(chain_wall, 4),
                                         "ratio": round(wall / chain_wall, 1), "lengths_agree": agree,
                                         "note": "parent: host packing of 32 suffixes per context, query_batch, host pick; no next symbols"}
        del p_d, o_d, outs
    for h in handles.values():
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
