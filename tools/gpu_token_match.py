"""Matching statistics of the token index on the device: one JSON line with, for n Zipf tokens over a 50 257-word vocabulary (the
recipe of tools/gpu_token_next.py) and Q query documents of M tokens,

  * batch "copied": every document a mix of windows copied from the corpus (16 to 256 tokens) and fresh Zipf tokens
  * batch "edited": the same with every 32nd token replaced
  * HIP-event times (sa_hip_token_match_info) of the match launch at max_length 0, 64 and 256 and of the docs launch at min_length 8,
    cap 64, after two warm-ups, median, minimum and maximum over the repetitions
  * the parent's formulation of the same question: one context per end position, text[max(0, e - L) : e], through
    sa_hip_token_index_spans_batch_device in mode 1 with need_next = 0, at L = 64 and 256 -- the launch timed the same way, the time of
    building the m * L contexts on the host and of uploading them reported separately
  * gates: the maximal spans derived from the parent's end-based answer (at a cap no shorter than the longest match) equal the new
    ones, and 16 sampled positions equal a window scan of the corpus on the host

    python tools/gpu_token_match.py [--n N] [--q Q] [--m M] [--reps R] [--out FILE]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (first: one HIP runtime per process)

from suffixarray_amd import _capi  # noqa: E402
from test_gpu_int import zipf_tokens  # noqa: E402

VOCAB = 50257
CAP = 64
MIN_LENGTH = 8
MAX_LENGTHS = (0, 64, 256)
PARENT_LENGTHS = (64, 256)


def arg(name, default):
    return int(float(sys.argv[sys.argv.index(name) + 1])) if name in sys.argv else default


def make_docs(t, q, m, seed=13):
    """q documents of m tokens: copied windows of 16 .. 256 tokens and runs of 1 .. 64 fresh Zipf tokens taking turns"""
    rng = np.random.default_rng(seed)
    fresh = zipf_tokens(q * m, VOCAB, seed=2)
    buf = np.empty(q * m, np.int32)
    for d in range(q):
        at, end, copy = d * m, (d + 1) * m, bool(rng.integers(0, 2))
        while at < end:
            if copy:
                w = min(int(rng.integers(16, 257)), end - at)
                p = int(rng.integers(0, t.size - w))
                buf[at:at + w] = t[p:p + w]
            else:
                w = min(int(rng.integers(1, 65)), end - at)
                buf[at:at + w] = fresh[at:at + w]
            at, copy = at + w, not copy
    edited = buf.copy()
    edited[::32] = (edited[::32] + rng.integers(1, VOCAB, edited[::32].size)) % VOCAB
    return {"copied": buf, "edited": edited}


def windows(t, p):
    """how many windows of the text equal p"""
    if len(p) == 0 or len(p) > t.size:
        return t.size if len(p) == 0 else 0
    idx = np.flatnonzero(t[:t.size - len(p) + 1] == p[0])
    for j in range(1, len(p)):
        idx = idx[t[idx + j] == p[j]]
    return int(idx.size)


def parent_contexts(buf, q, m, L):
    """the contexts of the parent's formulation: for every end position e = 1 .. m of every document its last min(e, L) tokens"""
    t0 = time.perf_counter()
    lens = np.minimum(np.arange(1, m + 1), L).astype(np.int64)
    off = np.zeros(q * m + 1, np.uint64)
    off[1:] = np.cumsum(np.tile(lens, q), dtype=np.uint64)
    within = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    first = np.repeat(np.arange(1, m + 1) - lens, lens) + within                                    # inside a document
    ctx = np.empty(int(off[-1]), np.int32)
    per = int(lens.sum())
    for d in range(q):
        ctx[d * per:(d + 1) * per] = buf[d * m + first]
    return ctx, off, (time.perf_counter() - t0) * 1e3


def maximal_from_ends(ls, q, m, min_length):
    """{(document, start, length)} of the maximal matches of at least min_length from ls[d, e - 1] = the longest match that ends at e"""
    ls = ls.reshape(q, m).astype(np.int64)
    start = np.arange(1, m + 1)[None, :] - ls
    last = np.ones((q, m), bool)
    last[:, :-1] = start[:, 1:] > start[:, :-1]                    # the match that ends at e + 1 does not hold the one that ends at e
    d, e = np.nonzero(last & (ls >= min_length))
    return set(zip(d.tolist(), start[d, e].tolist(), ls[d, e].tolist()))


def stats(v):
    v = np.array(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}


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
    res = {"tool": "gpu_token_match", "n": n, "vocab": VOCAB, "q": q, "doc_tokens": m, "reps": reps, "cap": CAP, "min_length": MIN_LENGTH,
           "build_device_ms": round(st["total_ms"], 3), "batches": {}}
    off = np.arange(q + 1, dtype=np.uint64) * m
    o_d = torch.from_numpy(off.view(np.int64)).to("cuda:0")
    ok = True
    for bname, buf in make_docs(t, q, m).items():
        r = res["batches"].setdefault(bname, {})
        p_d = torch.from_numpy(buf).to("cuda:0")
        sp_d = torch.zeros((total, 4), dtype=torch.int32, device="cuda:0")
        ps_d = torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0")
        os_d = torch.zeros((q, CAP, 4), dtype=torch.int32, device="cuda:0")
        hd_d = torch.zeros((q, 4), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        for M in MAX_LENGTHS[::-1]:                                # max_length 0 last: its answers are the ones gated below
            mt, dc = [], []
            for rep in range(reps + 2):
                h.match_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, total, M, sp_d.data_ptr())
                h.match_docs_batch_device(sp_d.data_ptr(), o_d.data_ptr(), q, MIN_LENGTH, CAP, ps_d.data_ptr(), os_d.data_ptr(), hd_d.data_ptr())
                info = h.match_info()                              # waits for both launches
                if rep >= 2:
                    mt.append(info["match_ms"])
                    dc.append(info["docs_ms"])
            r["match_max_length_%d" % M] = stats(mt)
            r["docs_max_length_%d" % M] = stats(dc)
        sp = sp_d.cpu().numpy().view(np.uint32)
        hd = hd_d.cpu().numpy().view(np.uint32)
        ps = ps_d.cpu().numpy().view(np.uint32)
        ln = os_d.cpu().numpy().view(np.uint32)[:, :, 2]
        longest = int(hd[:, 2].max())
        r.update({"mean_length": round(float(sp[:, 2].mean()), 3), "longest": longest, "maximal_spans": int(hd[:, 1].sum()),
                  "covered_tokens": int(hd[:, 3].sum()), "documents_beyond_cap": int((hd[:, 1] > CAP).sum())})
        # gate: 16 sampled positions against a window scan
        counted = True
        for j in np.random.default_rng(5).integers(0, total, 16):
            j = int(j)
            L, end = int(sp[j, 2]), (j // m + 1) * m
            counted = counted and windows(t, buf[j:j + L]) == int(sp[j, 1]) and (j + L == end or windows(t, buf[j:j + L + 1]) == 0)
        r["sample_equals_window_scan"] = bool(counted)
        # the parent's formulation, and the gate on its maximal spans at a cap no shorter than the longest match
        for L in PARENT_LENGTHS + (max(longest, 1),):
            gate = L not in PARENT_LENGTHS
            ctx, coff, build_ms = parent_contexts(buf, q, m, L)
            t0 = time.perf_counter()
            c_d, co_d = torch.from_numpy(ctx).to("cuda:0"), torch.from_numpy(coff.view(np.int64)).to("cuda:0")
            torch.cuda.synchronize()
            upload_ms = (time.perf_counter() - t0) * 1e3
            out_d = torch.zeros((total, 4), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            ms = []
            for rep in range(2 + (1 if gate else reps)):
                h.spans_batch_device(c_d.data_ptr(), co_d.data_ptr(), total, 1, L, 0, out_d.data_ptr())
                info = h.next_info()
                if rep >= 2:
                    ms.append(info["spans_ms"])
            if gate:
                mine = {(d, int(ps[d, k]), int(ln[d, k])) for d in range(q) for k in range(int(hd[d, 0]))}
                theirs = maximal_from_ends(out_d.cpu().numpy().view(np.uint32)[:, 2], q, m, MIN_LENGTH)
                full = hd[:, 1] <= CAP                             # documents whose list is complete compare as sets, the others by count
                same = ({x for x in mine if full[x[0]]} == {x for x in theirs if full[x[0]]}
                        and np.array_equal(np.bincount([x[0] for x in theirs], minlength=q), hd[:, 1]))
                r["maximal_spans_equal_parent"] = bool(same)
                ok = ok and same
            else:
                r["parent_max_length_%d" % L] = {"context_tokens": int(coff[-1]), "host_build_ms": round(build_ms, 1), "upload_ms": round(upload_ms, 1),
                                                 "spans_launch": stats(ms)}
            del c_d, co_d, out_d
        ok = ok and counted
        del p_d, sp_d, ps_d, os_d, hd_d
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
