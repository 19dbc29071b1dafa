"""Per-document counts and AND groups over shard sets on the device: one JSON line with, for the corpus of
tools/gpu_token_shard_docs.py (n Zipf tokens over a 50 257-word vocabulary cut into documents of Zipf-ish length by a separator
token) held as sets of 1, 4 and 8 shards cut at document boundaries, and the batches of tools/gpu_token_all.py --

  * per set: prepare_doc_ranks of the set (the shards' HIP-event times, summed) and the bytes of the shards' RK
  * the exact batch of tools/gpu_token_next.py: the listing at cap 16 chained into doc_counts over its rows, HIP-event medians over
    the repetitions after two warm-ups (sa_hip_token_shards_docs_info, sa_hip_token_shards_doc_ranks_info)
  * AND groups of 2 and of 3 2-grams, counts only (cap 0) and at cap 16, `inside` one document and `random`: the plan, pair and
    merge launches apart
  * against the parent's formulation, never against itself: the shards' own sa_hip_token_index_docs_batch_device /
    _doc_counts_batch_device / _all_batch_device through the borrowed handles one after another (the sum of their HIP-event times,
    "own"), then the copy of the S answers and their concatenation in NumPy on the host (wall time, "host").  That formulation picks
    a driver per shard; with a budget it would answer a different question, so no budget is measured
  * gates: 16 sampled groups per batch and set -- the unbudgeted `matched` equals the sum of the shards' own, and where it fits the
    cap the set of documents equals theirs (both are driver-independent); 16 sampled rows of counts equal a host count; the streamed
    ranks that doc_ranks_info reports equal the sum of the heads' examined

    python tools/gpu_token_shard_all.py [--n N] [--q Q] [--g G] [--reps R] [--out FILE]
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
from gpu_token_next import make_batches, arg, VOCAB  # noqa: E402
from gpu_token_docs import make_documents, med  # noqa: E402
from gpu_token_all import make_groups, CAP  # noqa: E402
from gpu_token_shard_docs import load_shard, cut_at_documents, SHARDS  # noqa: E402

T0 = time.perf_counter()


def say(*what):
    print("[gpu_token_shard_all %.0fs]" % (time.perf_counter() - T0), *what, file=sys.stderr, flush=True)


def zeros(shape, dtype):
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def chain(st, S, sp_d, q, reps, bases, tables):
    """the listing at cap 16 chained into the counts of its rows: the set, and the shards' own calls one after another"""
    d_d, f_d, h_d, c_d = zeros((q, CAP), torch.int64), zeros((q, CAP), torch.int32), zeros((q, 4), torch.int64), zeros((q, CAP), torch.int32)
    od, of, oh, oc = zeros((S, q, CAP), torch.int32), zeros((S, q, CAP), torch.int32), zeros((S, q, 4), torch.int32), zeros((S, q, CAP), torch.int32)
    torch.cuda.synchronize()
    shard = [st.shard(s) for s in range(S)]
    ms = {"list": [], "doc_counts": [], "own_list": [], "own_doc_counts": []}
    for rep in range(reps + 2):
        st.docs_batch_device(sp_d.data_ptr(), q, CAP, 0, d_d.data_ptr(), f_d.data_ptr(), h_d.data_ptr())
        st.doc_counts_batch_device(sp_d.data_ptr(), q, CAP, d_d.data_ptr(), h_d.data_ptr(), 32, c_d.data_ptr())
        di, ri = st.docs_info(), st.doc_ranks_info()               # wait for the launches
        a = b = 0.0
        for s in range(S):
            shard[s].docs_batch_device(sp_d[s].data_ptr(), q, CAP, 0, od[s].data_ptr(), of[s].data_ptr(), oh[s].data_ptr())
            shard[s].doc_counts_batch_device(sp_d[s].data_ptr(), q, CAP, od[s].data_ptr(), oh[s].data_ptr(), 16, oc[s].data_ptr())
            a += shard[s].docs_info()["docs_ms"]
            b += shard[s].doc_ranks_info()["counts_ms"]
        if rep >= 2:
            ms["list"].append(di["pairs_ms"] + di["merge_ms"]); ms["doc_counts"].append(ri["counts_ms"])
            ms["own_list"].append(a); ms["own_doc_counts"].append(b)
    out = {k: med(v) for k, v in ms.items()}
    walls = []
    for rep in range(3):                                           # the host step of the parent's formulation: copy and concatenate
        t0 = time.perf_counter()
        heads, docs, cnts = oh.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy()
        w = np.minimum(heads[:, :, 0], CAP)
        mask = np.arange(CAP)[None, None, :] < w[:, :, None]
        gids = (docs.astype(np.int64) + np.asarray(bases[:S], np.int64)[:, None, None])[mask]
        flat = cnts[mask]
        walls.append((time.perf_counter() - t0) * 1e3)
    out["host_concat_wall"] = med(walls)
    out["cells_counted"] = int(h_d.cpu().numpy().view(_capi.SHARDS_DOCS_DTYPE).reshape(q)["written"].astype(np.int64).sum())
    out["own_cells_counted"] = int(flat.size) if gids.size == flat.size else -1
    # 16 sampled rows against a host count
    sp = sp_d.cpu().numpy().view(np.uint32)
    gh, gd, gc = h_d.cpu().numpy().view(_capi.SHARDS_DOCS_DTYPE).reshape(q), d_d.cpu().numpy().view(np.uint64), c_d.cpu().numpy().view(np.uint32)
    total = sp[:, :, 1].astype(np.int64).sum(axis=0)
    small = np.flatnonzero(total <= 2_000_000)
    ok = True
    for i in np.random.default_rng(5).choice(small, 16, replace=False):
        want = {}
        for s in range(S):
            pos = shard[s].sa_range(int(sp[s, i, 0]), int(sp[s, i, 1])).astype(np.int64)
            d = np.searchsorted(tables[s], pos, "right") - 1
            u, k = np.unique(d, return_counts=True)
            want.update({int(bases[s]) + int(x): int(y) for x, y in zip(u, k)})
        w = int(gh["written"][i])
        ok = ok and gc[i, :w].tolist() == [want.get(int(x), 0) for x in gd[i, :w]]
    out["sample_equals_host_count"] = bool(ok)
    return out, ok


def groups(st, S, sp_d, P, goff, reps, bases):
    """AND groups, counts only and at cap 16: the set's three launches, and the shards' own launches one after another"""
    g = len(goff) - 1
    d_d, f_d, a_d = zeros((g, CAP), torch.int64), zeros((g, CAP), torch.int32), zeros((g, 5), torch.int64)
    od, of, oa = zeros((S, g, CAP), torch.int32), zeros((S, g, CAP), torch.int32), zeros((S, g, 8), torch.int32)
    torch.cuda.synchronize()
    shard = [st.shard(s) for s in range(S)]
    ms = {k: {"plan": [], "pairs": [], "merge": [], "set": [], "own": []} for k in ("count", "list")}
    sums_ok = True
    for rep in range(reps + 2):
        for kind, cap in (("count", 0), ("list", CAP)):
            st.all_batch_device(sp_d.data_ptr(), P, goff, cap, 0, d_d.data_ptr() if cap else None, f_d.data_ptr() if cap else None, a_d.data_ptr())
            info = st.doc_ranks_info()                             # waits for the launches
            own = 0.0
            for s in range(S):
                shard[s].all_batch_device(sp_d[s].data_ptr(), P, goff, cap, 0, od[s].data_ptr() if cap else None, of[s].data_ptr() if cap else None,
                                          oa[s].data_ptr())
                own += shard[s].doc_ranks_info()["all_ms"]
            if rep >= 2:
                m = ms[kind]
                m["plan"].append(info["plan_ms"]); m["pairs"].append(info["pairs_ms"]); m["merge"].append(info["merge_ms"])
                m["set"].append(info["plan_ms"] + info["pairs_ms"] + info["merge_ms"]); m["own"].append(own)
    out = {k: {m: med(v) for m, v in d.items()} for k, d in ms.items()}
    ah = a_d.cpu().numpy().view(_capi.SHARDS_ALL_DTYPE).reshape(g)
    sums_ok = info["streamed"] == int(ah["examined"].sum())
    walls = []
    for rep in range(3):                                           # the host step of the parent's formulation: copy and concatenate
        t0 = time.perf_counter()
        heads, docs = oa.cpu().numpy().view(np.uint32), od.cpu().numpy()
        matched = heads[:, :, 2].astype(np.uint64).sum(axis=0)
        w = np.minimum(heads[:, :, 0], CAP)
        mask = np.arange(CAP)[None, None, :] < w[:, :, None]
        gids = np.where(mask, docs.astype(np.int64) + np.asarray(bases[:S], np.int64)[:, None, None], -1)
        walls.append((time.perf_counter() - t0) * 1e3)
    out["host_concat_wall"] = med(walls)
    gd = d_d.cpu().numpy().view(np.uint64)
    ok = True
    for i in np.random.default_rng(5).choice(g, 16, replace=False):
        ok = ok and int(ah["matched"][i]) == int(matched[i]) and int(ah["examined"][i]) == int(ah["count"][i])
        if int(matched[i]) <= CAP:
            own_docs = sorted(int(x) for x in gids[:, i, :].ravel() if x >= 0)
            ok = ok and sorted(int(x) for x in gd[i, :int(ah["written"][i])]) == own_docs
    out.update({"ranks_walked": int(ah["examined"].sum()), "own_ranks_walked": int(heads[:, :, 1].astype(np.int64).sum()),
                "candidates": int(ah["candidates"].sum()), "matched": int(ah["matched"].sum()),
                "groups_with_a_match": int((ah["matched"] > 0).sum()), "groups_per_chunk": info["chunk"],
                "sample_equals_parent_formulation": bool(ok), "streamed_sums_agree": bool(sums_ok)})
    return out, ok and sums_ok


def main():
    n, q, g, reps = arg("--n", 100_000_000), arg("--q", 1_000_000), arg("--g", 200_000), arg("--reps", 20)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    t = zipf_tokens(n, VOCAB, seed=1)
    starts = make_documents(t)
    say("corpus made")
    res = {"tool": "gpu_token_shard_all", "n": n, "vocab": VOCAB + 1, "documents": int(starts.size), "q": q, "groups": g, "reps": reps,
           "cap": CAP, "sets": {}}
    sets, bases, tabs = {}, {}, {}
    for S in SHARDS:
        texts, tables = cut_at_documents(t, starts, S)
        st = _capi.TokenShards.create([load_shard(x) for x in texts])
        st.set_documents(tables)
        prep = []
        for rep in range(3):                                       # the first builds its buffers
            st.prepare_doc_ranks(False)
            st.prepare_doc_ranks(True)
            if rep:
                prep.append(st.doc_ranks_info()["prepare_ms"])
        sets[S], bases[S], tabs[S] = st, st.doc_bases(), tables
        res["sets"][str(S)] = {"shard_tokens": [int(x.size) for x in texts], "prepare_doc_ranks": med(prep),
                               "rank_bytes": st.doc_ranks_info()["bytes"]}
        say("set of", S, "built")
    ok = True
    buf, off, mode = make_batches(t, q)["exact"]
    p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
    for S in SHARDS:
        sp_d, ln_d, tt_d = zeros((S, q, 4), torch.int32), zeros(q, torch.int32), zeros(q, torch.int64)
        torch.cuda.synchronize()
        sets[S].spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, mode, 0, 0, ln_d.data_ptr(), tt_d.data_ptr(), sp_d.data_ptr())
        sets[S].sync()
        r, good = chain(sets[S], S, sp_d, q, reps, bases[S], tabs[S])
        res["sets"][str(S)]["chain"] = r
        say("chain", S, good)
        ok = ok and good
        del sp_d, ln_d, tt_d
    del p_d, o_d
    for bname, m, inside in (("inside_2", 2, True), ("inside_3", 3, True), ("random_2", 2, False), ("random_3", 3, False)):
        buf, off, goff = make_groups(t, starts, g, m, inside, seed=7 + m)
        P = g * m
        p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
        for S in SHARDS:
            sp_d, ln_d, tt_d = zeros((S, P, 4), torch.int32), zeros(P, torch.int32), zeros(P, torch.int64)
            torch.cuda.synchronize()
            sets[S].spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), P, 0, 0, 0, ln_d.data_ptr(), tt_d.data_ptr(), sp_d.data_ptr())
            sets[S].sync()
            r, good = groups(sets[S], S, sp_d, P, goff, reps, bases[S])
            r["spans_per_group"] = m
            res["sets"][str(S)][bname] = r
            say(bname, S, good)
            ok = ok and good
            del sp_d, ln_d, tt_d
        del p_d, o_d
    for st in sets.values():
        st.close()
    res["gate_ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
