"""Documents over shard sets on the device: one JSON line with, for n Zipf tokens over a 50 257-word vocabulary cut into documents
of Zipf-ish length by a separator token (the corpus of tools/gpu_token_docs.py) and held as sets of 1, 4 and 8 shards cut at
document boundaries, and the two batches of Q contexts of tools/gpu_token_next.py --

  * per batch and set, HIP-event medians over the repetitions after two warm-ups (sa_hip_token_shards_docs_info) of
      counts only (cap 0) with budget 0 and with budget 4096, the listing at cap 16 -- the pair launches and the merge launches
      apart -- and locate at cap 16
  * against the parent's formulation, never against itself: the shards' own sa_hip_token_index_docs_batch_device /
    _locate_batch_device through the borrowed handles one after another (the sum of their HIP-event times, "own"), then the merge
    on the host (copying the S head and list arrays back, summing and concatenating in NumPy: wall time, "host").  With a budget
    that formulation examines min(c_s, budget) ranks in EVERY shard and cannot cut the budget across shards; its time is reported,
    its answer is not the set's
  * the 100 longest spans alone at every S: what the split of a long span over the shards' waves buys
  * gates: 16 sampled answers per batch and set equal that host formulation (budget 0), and the streamed ranks that docs_info
    reports equal the sum computed from the spans

    python tools/gpu_token_shard_docs.py [--n N] [--q Q] [--reps R] [--out FILE]
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
from gpu_token_docs import make_documents, med, CAP, BUDGET, LONGEST  # noqa: E402

SHARDS = (1, 4, 8)
KINDS = {"count_all": (0, 0), "count_budget": (0, BUDGET), "list": (CAP, 0)}


def load_shard(t):
    t_d = torch.from_numpy(np.ascontiguousarray(t)).to("cuda:0")
    sa_d = torch.empty(t.size, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    _capi.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), t.size, VOCAB + 1)
    return _capi.TokenIndex.load_device(t_d.data_ptr(), sa_d.data_ptr(), t.size)


def cut_at_documents(t, starts, S):
    """-> (texts, tables): S shards whose cuts are the document starts nearest to n * s / S, every shard at least one document"""
    if starts.size < S:
        raise SystemExit("fewer documents than shards")
    idx = [0]
    for s in range(1, S):
        near = int(np.argmin(np.abs(starts.astype(np.int64) - t.size * s // S)))
        idx.append(min(max(near, idx[-1] + 1), starts.size - (S - s)))
    at = [int(starts[i]) for i in idx] + [t.size]
    texts, tables = [], []
    for a, b in zip(at, at[1:]):
        texts.append(t[a:b])
        tables.append((starts[(starts >= a) & (starts < b)] - a).astype(np.int32))
    return texts, tables


def host_merge(own_heads, own_docs, own_offs, bases, cap, what):
    """the parent's last step: S per-shard answers [S, q, ...] on the host into one.  what = 2: the `distinct` column decides a
    shard's first slot (docs); what = 1: `count` does (locate, whose heads are {written, count})"""
    S, q = own_heads.shape[0], own_heads.shape[1]
    col = own_heads[:, :, what].astype(np.uint64)
    total = col.sum(axis=0)
    if cap == 0:
        return total, None, None
    docs, offs = np.zeros((q, cap), np.uint64), np.zeros((q, cap), np.int32)
    at = np.zeros(q, np.int64)
    rows = np.arange(q)
    for s in range(S):
        w = np.minimum(own_heads[s, :, 0], cap).astype(np.int64)
        for j in range(cap):
            m = (j < w) & (at + j < cap)
            if m.any():
                docs[rows[m], at[m] + j] = bases[s] + own_docs[s][m, j].astype(np.uint64)
                offs[rows[m], at[m] + j] = own_offs[s][m, j]
        at += col[s].astype(np.int64)
    return total, docs, offs


def measure(st, S, sp_d, q, reps, bases, count):
    """one set on one batch of device spans [S, q, 4]: the set's launches and the parent's formulation, taking turns"""
    d_d = torch.zeros((q, CAP), dtype=torch.int64, device="cuda:0")
    f_d = torch.zeros((q, CAP), dtype=torch.int32, device="cuda:0")
    h_d = torch.zeros((q, 4), dtype=torch.int64, device="cuda:0")
    l_d = torch.zeros((q, 2), dtype=torch.int64, device="cuda:0")
    od = torch.zeros((S, q, CAP), dtype=torch.int32, device="cuda:0")
    of = torch.zeros((S, q, CAP), dtype=torch.int32, device="cuda:0")
    oh = torch.zeros((S, q, 4), dtype=torch.int32, device="cuda:0")
    ol = torch.zeros((S, q, 2), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    shard = [st.shard(s) for s in range(S)]
    ms = {k: {"pairs": [], "merge": [], "set": [], "own": []} for k in KINDS}
    ms["locate"] = {"set": [], "own": []}
    sums_ok = True
    chunks = {}
    for rep in range(reps + 2):
        for kind, (cap, budget) in KINDS.items():
            st.docs_batch_device(sp_d.data_ptr(), q, cap, budget, d_d.data_ptr() if cap else None, f_d.data_ptr() if cap else None, h_d.data_ptr())
            info = st.docs_info()                                  # waits for the launches
            chunks[kind] = info["chunk"]
            sums_ok = sums_ok and info["streamed"] == int((np.minimum(count, budget) if budget else count).sum())
            own = 0.0
            for s in range(S):
                shard[s].docs_batch_device(sp_d[s].data_ptr(), q, cap, budget, od[s].data_ptr() if cap else None, of[s].data_ptr() if cap else None,
                                           oh[s].data_ptr())
                own += shard[s].docs_info()["docs_ms"]
            if rep >= 2:
                ms[kind]["pairs"].append(info["pairs_ms"]); ms[kind]["merge"].append(info["merge_ms"])
                ms[kind]["set"].append(info["pairs_ms"] + info["merge_ms"]); ms[kind]["own"].append(own)
        st.locate_batch_device(sp_d.data_ptr(), q, CAP, d_d.data_ptr(), f_d.data_ptr(), l_d.data_ptr())
        info = st.docs_info()
        own = 0.0
        for s in range(S):
            shard[s].locate_batch_device(sp_d[s].data_ptr(), q, CAP, od[s].data_ptr(), of[s].data_ptr(), ol[s].data_ptr())
            own += shard[s].docs_info()["locate_ms"]
        if rep >= 2:
            ms["locate"]["set"].append(info["locate_ms"]); ms["locate"]["own"].append(own)
    out = {k: {m: med(v) for m, v in d.items()} for k, d in ms.items()}
    # the host step of the parent's formulation, and the gates against it: locate (the last launches above), then the listing
    host = {}
    ok = True
    sample = np.random.default_rng(5).choice(q, 16, replace=False)
    for kind in ("locate", "list", "count_all"):
        cap = 0 if kind == "count_all" else CAP
        if kind != "locate":
            st.docs_batch_device(sp_d.data_ptr(), q, cap, 0, d_d.data_ptr() if cap else None, f_d.data_ptr() if cap else None, h_d.data_ptr())
            for s in range(S):
                shard[s].docs_batch_device(sp_d[s].data_ptr(), q, cap, 0, od[s].data_ptr() if cap else None, of[s].data_ptr() if cap else None, oh[s].data_ptr())
                shard[s].sync()
        st.sync()
        walls = []
        for rep in range(3):
            t0 = time.perf_counter()
            heads = (ol if kind == "locate" else oh).cpu().numpy().view(np.uint32)
            lists = (od.cpu().numpy(), of.cpu().numpy()) if cap else (None, None)
            total, docs, offs = host_merge(heads, lists[0], lists[1], bases, cap, 1 if kind == "locate" else 2)
            walls.append((time.perf_counter() - t0) * 1e3)
        host[kind] = med(walls)
        if kind == "locate":
            got = l_d.cpu().numpy().view(_capi.SHARDS_LOCATE_DTYPE).reshape(q)
            got_total = got["count"]
        else:
            got = h_d.cpu().numpy().view(_capi.SHARDS_DOCS_DTYPE).reshape(q)
            got_total = got["distinct"]
            ok = ok and bool((got["examined"][sample] == got["count"][sample]).all()) and np.array_equal(got["count"][sample], count[sample].astype(np.uint64))
        ok = ok and np.array_equal(got_total[sample], total[sample])
        if cap:
            gd, gf = d_d.cpu().numpy().view(np.uint64), f_d.cpu().numpy()
            for i in sample:
                w = int(got["written"][i])
                ok = ok and w == min(int(total[i]), cap) and gd[i, :w].tolist() == docs[i, :w].tolist() and gf[i, :w].tolist() == offs[i, :w].tolist()
    out["host_merge_wall"] = host
    out["streamed_sums_agree"] = bool(sums_ok)
    out["samples_equal_host_formulation"] = bool(ok)
    # the 100 longest spans alone
    top = np.argsort(-count, kind="stable")[:LONGEST]
    top_d = sp_d[:, torch.from_numpy(top).to("cuda:0"), :].contiguous()
    th_d = torch.zeros((LONGEST, 4), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    tops, owns = [], []
    for rep in range(reps + 2):
        st.docs_batch_device(top_d.data_ptr(), top.size, 0, 0, None, None, th_d.data_ptr())
        info = st.docs_info()
        own = 0.0
        for s in range(S):
            shard[s].docs_batch_device(top_d[s].data_ptr(), top.size, 0, 0, None, None, oh[s].data_ptr())
            own += shard[s].docs_info()["docs_ms"]
        if rep >= 2:
            tops.append(info["pairs_ms"] + info["merge_ms"]); owns.append(own)
    out["longest_%d_alone" % LONGEST] = {"set": med(tops), "own": med(owns), "ranks": int(count[top].sum()), "longest_span": int(count.max())}
    out["contexts_per_chunk"] = chunks
    return out, ok and sums_ok


def main():
    n, q, reps = arg("--n", 100_000_000), arg("--q", 1_000_000), arg("--reps", 20)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    t = zipf_tokens(n, VOCAB, seed=1)
    starts = make_documents(t)
    res = {"tool": "gpu_token_shard_docs", "n": n, "vocab": VOCAB + 1, "documents": int(starts.size), "q": q, "reps": reps, "cap": CAP,
           "budget": BUDGET, "sets": {}}
    sets, bases = {}, {}
    for S in SHARDS:
        texts, tables = cut_at_documents(t, starts, S)
        st = _capi.TokenShards.create([load_shard(x) for x in texts])
        st.set_documents(tables)
        sets[S], bases[S] = st, st.doc_bases()
        res["sets"][str(S)] = {"shard_tokens": [int(x.size) for x in texts], "shard_documents": [int(x.size) for x in tables]}
        assert int(bases[S][-1]) == starts.size
    ok = True
    for bname, (buf, off, mode) in make_batches(t, q).items():
        p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
        for S in SHARDS:
            st = sets[S]
            sp_d = torch.zeros((S, q, 4), dtype=torch.int32, device="cuda:0")
            ln_d = torch.zeros(q, dtype=torch.int32, device="cuda:0")
            tt_d = torch.zeros(q, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            st.spans_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, mode, 0, 0, ln_d.data_ptr(), tt_d.data_ptr(), sp_d.data_ptr())
            st.sync()
            count = sp_d.cpu().numpy().view(np.uint32)[:, :, 1].astype(np.int64).sum(axis=0)
            r, good = measure(st, S, sp_d, q, reps, bases[S], count)
            r["ranks_streamed_count_all"] = int(count.sum())
            res["sets"][str(S)][bname] = r
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
