"""CNF document queries of the token index on the device: one JSON line with, for the corpus of tools/gpu_token_docs.py (n Zipf
tokens over a 50 257-word vocabulary cut into documents of Zipf-ish length by a separator token) --

  * batches of G queries of 2 and of 3 clauses of 1, 2 and 4 2-grams each, without and with one exclusion (a negated clause of one
    2-gram drawn anywhere): `inside` draws every literal of a query from inside one document, so matches exist; `random` draws the
    2-grams anywhere, so there are mostly none.  Counts only (cap 0) and at cap 16, HIP-event medians over the repetitions after two
    warm-ups (sa_hip_token_index_cnf_info)
  * baseline (a), the parent's only formulation: one uncapped documents list per literal, np.union1d per clause, np.intersect1d over
    the positive clauses, np.setdiff1d for the exclusion, over the first --base-g queries of every batch; the device time of its
    launches (sa_hip_token_docs_info) and the host time of its set algebra are reported apart, beside the wall time
  * baseline (b), for the batches of one literal per clause without an exclusion: the AND launch of token_all.hpp on the same spans
    in the same process, launches alternating with the cnf launches
  * gates: in every batch the first --base-g answers equal baseline (a) in their number, 16 sampled lists are subsets of it, and for
    one literal per clause heads and lists equal those of the AND launch

    python tools/gpu_token_cnf.py [--n N] [--g G] [--reps R] [--base-g B] [--out FILE]
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
from gpu_token_next import VOCAB  # noqa: E402
from gpu_token_docs import arg, make_documents, med  # noqa: E402

CAP = 16
NGRAM = 2


def make_queries(t, starts, g, m, k, inside, excl, seed):
    """g queries of m clauses of k 2-grams, plus one negated clause of one 2-gram when excl -> (packed int32, uint64 offsets[S + 1],
    clause offsets uint64[C + 1], negated uint8[C], group offsets uint64[g + 1])"""
    rng = np.random.default_rng(seed)
    n = t.size
    if inside:                                                     # every literal of a query from one document of >= 8 tokens
        ends = np.append(starts[1:], n).astype(np.int64)
        big = np.flatnonzero(ends - starts >= 8)
        d = rng.choice(big, g)
        pos = starts[d][:, None] + (rng.random((g, m * k)) * (ends[d] - starts[d] - NGRAM - 1)[:, None]).astype(np.int64)
    else:
        pos = rng.integers(0, n - NGRAM, (g, m * k))
    if excl:
        pos = np.concatenate([pos, rng.integers(0, n - NGRAM, (g, 1))], axis=1)
    S = pos.size
    buf = t[(pos.reshape(-1, 1) + np.arange(NGRAM)).reshape(-1)].astype(np.int32)
    sizes = np.tile(np.array([k] * m + [1] * excl, np.uint64), g)
    coff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    neg = np.tile(np.array([0] * m + [1] * excl, np.uint8), g)
    return buf, (np.arange(S + 1) * NGRAM).astype(np.uint64), coff, neg, (np.arange(g + 1) * (m + excl)).astype(np.uint64)


def parent_formulation(h, sp, coff, neg, goff, b):
    """the documents that satisfy the first b queries the parent commit's way
    -> ([sorted document arrays], device ms of the launches, host ms of the set algebra, wall ms)"""
    t0 = time.perf_counter()
    out, dev_ms, host_ms = [], 0.0, 0.0
    for i in range(b):
        keep, drop = None, None
        for c in range(int(goff[i]), int(goff[i + 1])):
            union = None
            for j in range(int(coff[c]), int(coff[c + 1])):
                one = np.zeros(1, _capi.SPAN_DTYPE)
                one["first"], one["count"] = sp[j, 0], sp[j, 1]
                cap = max(int(sp[j, 1]), 1)                        # uncapped: no list is longer than the span
                d_d = torch.zeros(cap, dtype=torch.int32, device="cuda:0")
                f_d = torch.zeros(cap, dtype=torch.int32, device="cuda:0")
                h_d = torch.zeros(4, dtype=torch.int32, device="cuda:0")
                s_d = torch.from_numpy(one.view(np.int32).copy()).to("cuda:0")
                h.docs_batch_device(s_d.data_ptr(), 1, cap, 0, d_d.data_ptr(), f_d.data_ptr(), h_d.data_ptr())
                dev_ms += h.docs_info()["docs_ms"]                 # waits for the launch
                docs = d_d[:int(h_d[0].item())].cpu().numpy()
                t1 = time.perf_counter()
                union = docs if union is None else np.union1d(union, docs)
                host_ms += (time.perf_counter() - t1) * 1e3
            t1 = time.perf_counter()
            if neg[c]:
                drop = union if drop is None else np.union1d(drop, union)
            else:
                keep = np.unique(union) if keep is None else np.intersect1d(keep, union)
            host_ms += (time.perf_counter() - t1) * 1e3
        t1 = time.perf_counter()
        out.append(np.sort(keep if drop is None else np.setdiff1d(keep, drop)))
        host_ms += (time.perf_counter() - t1) * 1e3
    return out, dev_ms, host_ms, (time.perf_counter() - t0) * 1e3


def main():
    n, g, reps = arg("--n", 100_000_000), arg("--g", 200_000), arg("--reps", 20)
    base_g = min(arg("--base-g", 64), g)
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
    h.prepare_doc_ranks(True)
    res = {"tool": "gpu_token_cnf", "n": n, "vocab": VOCAB + 1, "documents": int(starts.size), "groups": g, "reps": reps, "cap": CAP,
           "base_groups": base_g, "build_device_ms": round(st["total_ms"], 3), "batches": {}}
    ok = True
    for inside in (True, False):
        for m in (2, 3):
            for k in (1, 2, 4):
                for excl in (0, 1):
                    bname = "%s_%dx%d%s" % ("inside" if inside else "random", m, k, "_not" if excl else "")
                    buf, off, coff, neg, goff = make_queries(t, starts, g, m, k, inside, excl, seed=7 + 10 * m + k)
                    S = int(off.size - 1)
                    p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
                    sp_d = torch.zeros((S, 4), dtype=torch.int32, device="cuda:0")
                    d_d, f_d = (torch.zeros((g, CAP), dtype=torch.int32, device="cuda:0") for _ in range(2))
                    c_d = torch.zeros((g, 12), dtype=torch.int32, device="cuda:0")
                    single = k == 1 and not excl                   # baseline (b): the AND launch answers the same question
                    if single:
                        ad_d, af_d = (torch.zeros((g, CAP), dtype=torch.int32, device="cuda:0") for _ in range(2))
                        a_d = torch.zeros((g, 8), dtype=torch.int32, device="cuda:0")
                    torch.cuda.synchronize()
                    h.spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), S, 0, 0, 0, sp_d.data_ptr())
                    ms = {"count": [], "list": [], "all_count": [], "all_list": []}
                    for rep in range(reps + 2):                    # the two kernels alternate
                        for kind, cap in (("count", 0), ("list", CAP)):
                            h.cnf_batch_device(sp_d.data_ptr(), S, coff, neg, goff, cap, 0, d_d.data_ptr() if cap else None,
                                               f_d.data_ptr() if cap else None, c_d.data_ptr())
                            v = h.cnf_info()["ms"]                 # waits for the launch
                            if rep >= 2:
                                ms[kind].append(v)
                            if single:
                                h.all_batch_device(sp_d.data_ptr(), S, goff, cap, 0, ad_d.data_ptr() if cap else None,
                                                   af_d.data_ptr() if cap else None, a_d.data_ptr())
                                v = h.doc_ranks_info()["all_ms"]
                                if rep >= 2:
                                    ms["all_" + kind].append(v)
                    sp, ch, docs = sp_d.cpu().numpy().view(np.uint32), c_d.cpu().numpy().view(np.uint32), d_d.cpu().numpy()
                    examined = ch[:, 6].astype(np.int64) | (ch[:, 7].astype(np.int64) << 32)
                    count = ch[:, 8].astype(np.int64) | (ch[:, 9].astype(np.int64) << 32)
                    want, dev_ms, host_ms, wall = parent_formulation(h, sp, coff, neg, goff, base_g)
                    pick = np.sort(np.random.default_rng(5).choice(base_g, min(16, base_g), replace=False))
                    sampled = all(int(ch[i, 1]) == want[i].size and examined[i] == count[i] and
                                  set(docs[i, :int(ch[i, 0])].tolist()) <= set(want[i].tolist()) for i in pick)
                    agree = [int(x.size) for x in want] == ch[:len(want), 1].tolist()
                    ok = ok and sampled and agree
                    b = {k_: med(v) for k_, v in ms.items() if v}
                    b.update({"clauses": m, "literals_per_clause": k, "exclusion": bool(excl), "ranks_walked": int(examined.sum()),
                              "candidates": int(ch[:, 2].astype(np.int64).sum()), "duplicates": int(ch[:, 3].astype(np.int64).sum()),
                              "matched": int(ch[:, 1].astype(np.int64).sum()), "groups_with_a_match": int((ch[:, 1] > 0).sum()),
                              "sample_equals_parent_formulation": bool(sampled),
                              "parent_formulation": {"groups": len(want), "device_ms": round(dev_ms, 3), "host_ms": round(host_ms, 3),
                                                     "wall_ms": round(wall, 3), "agree": bool(agree),
                                                     "note": "an uncapped documents list per literal, np.union1d / intersect1d / setdiff1d on the host"}})
                    if single:
                        ah = a_d.cpu().numpy().view(np.uint32)
                        same = (np.array_equal(ch[:, (0, 1, 2, 4)], ah[:, (0, 2, 3, 4)]) and np.array_equal(examined, ah[:, 1]) and
                                np.array_equal(count, ah[:, 5]) and d_d.cpu().numpy().tobytes() == ad_d.cpu().numpy().tobytes() and
                                f_d.cpu().numpy().tobytes() == af_d.cpu().numpy().tobytes())
                        b["equals_all_launch"] = bool(same)
                        ok = ok and same
                        del ad_d, af_d, a_d
                    res["batches"][bname] = b
                    print(bname, json.dumps(b), file=sys.stderr, flush=True)   # progress: the JSON line comes at the end
                    del p_d, o_d, sp_d, d_d, f_d, c_d
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
