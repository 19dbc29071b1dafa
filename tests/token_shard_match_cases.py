"""Shard sets, query batches and the two CPU models of the tests of matching statistics over shard sets
(test_token_shard_match_cpu.py, test_gpu_token_shard_match.py).

A set is a list of shards (int32 texts); a batch is a list of query documents; a position is a flat index into the packed batch.
The answer of a position is the merged record (length, shards, count) and, per shard, the span (first, count, length, ended), as
include/sa_hip.h section 6c (matching statistics) defines them.
  model A  as the device does it: per shard the matched length by token_match_cases.spans_a (one bisection, the two neighbour
           LCPs), the maximum over the shards, every shard's exact span of that prefix (token_next_cases._spans_of), then the sums;
           the heads by token_match_cases.heads_a (predecessor rule, the sum of end(j) - max(j, E(j)));
  model B  brute force without a suffix array, without a per-shard maximum and without the three facts: for every L the set of
           the windows of L symbols of every shard (windows named jointly with the query's by their symbols); a position's answer
           is the largest L at which its window is in that set, with the number of shard windows equal to it and of shards that
           have one; the heads by token_match_cases.heads_b (containment for maximality, a set union for coverage).
"""
import numpy as np

import token_cases as tc
import token_match_cases as mc
import token_next_cases as nc
import token_shard_cases as sc
from test_int_cpu import model_sa

NONE = mc.NONE
MAX_LENGTHS = mc.MAX_LENGTHS
MIN_LENGTHS = mc.MIN_LENGTHS
PLANS = tc.PLANS
set_plan = tc.set_plan

# the texts of token_match_cases cut into S shards: name -> the S it is cut into ("rand_k2/3" is rand_k2 in 3 shards)
CUTS = {"n0": (1, 3), "n1": (1, 2), "n2": (1, 2), "all_equal": (1, 2), "period2": (1, 3), "rand_k2": (1, 2, 3), "rand_k1000": (1, 3),
        "zero_and_max": (1, 2), "planted": (1, 3)}
CUT_SETS = tuple("%s/%d" % (k, s) for k, ss in CUTS.items() for s in ss)
HAND_SETS = ("tiny64", "small_beside_long", "disjoint", "mod_deal", "planted3", "cut_window")
SETS = CUT_SETS + HAND_SETS

W = 20                                          # planted windows of the set planted3: symbols no shard holds otherwise
W_FIRST = [5000 + i for i in range(W)]          # only in the first shard
W_LAST = [6000 + i for i in range(W)]           # only in the last shard
W_BOTH = [7000 + i for i in range(W)]           # once in shard 0 and twice in shard 1, nowhere longer
W_END = [8000 + i for i in range(W)]            # the last W symbols of shard 1 and nowhere else: the match only ends that text
CUT_LEN, CUT_AT = mc.PLANT_LEN, 50              # a window of 130 tokens whose occurrence is cut after 50 of them


def _cut(t, S):
    n = len(t)
    return [np.array(t[n * s // S:n * (s + 1) // S], np.int32) for s in range(S)]


def _pairs_batches(tl, rng):
    """the pair layout's edges with S = 3: 255 and 258 (position, shard) pairs -- a position's three lanes straddle a wave's end
    (63 | 64, 127 | 128, 191 | 192) and the block's"""
    return {"pairs85": [mc._piece(tl, rng, 40), mc._piece(tl, rng, 45)], "pairs86": [mc._piece(tl, rng, 40), [], mc._piece(tl, rng, 46)]}


def _windows_doc(tl, rng, widths):
    doc = []
    for m in widths:
        p = int(rng.integers(0, max(len(tl) - m, 1)))
        doc += tl[p:p + m] + [NONE]
    return doc


def _hand(name):
    """-> (shards, {batch: docs}) of a hand-made set"""
    rng = np.random.default_rng(73)
    k1000 = [int(v) for v in tc.texts()["rand_k1000"][:1500]]
    if name == "tiny64":
        shards = sc._sets()["tiny64"]
        docs = [[int(v) for v in shards[s]] + [NONE] + [int(v) for v in shards[63 - s][:9]] for s in (0, 31, 63)]
        mix = [int(v) for v in rng.integers(0, 5, 70)]
        return shards, {"shard_texts": docs, "mixed": [mix, [], mix[:33] + [9] + mix[:5]], "pairs_wave": [mix[:2], mix[:1]]}
    if name == "small_beside_long":                                # a prefix longer than n_s must clamp, an empty shard answers zeros
        shards = [np.zeros(0, np.int32), np.array(k1000[7:8], np.int32), np.array(k1000[20:22], np.int32), np.array(k1000, np.int32)]
        docs = [k1000[5:12] + [NONE] + k1000[18:25], k1000[20:22], k1000[7:8] + k1000[7:8], k1000[-3:] + [k1000[0]]]
        return shards, {"clamp": docs, "pieces": [mc._piece(k1000, rng, s) for s in (1, 64, 65)]}
    if name == "disjoint":
        shards = sc._sets()["disjoint"]
        tls = [[int(v) for v in t] for t in shards]
        docs = [tls[s][10:40] + tls[(s + 1) % 4][5:25] + [NONE] for s in range(4)]
        return shards, {"across": docs, "pairs_block": [_windows_doc(tls[2], rng, (30, 33))]}                # 4 * 65 = 260 pairs
    if name == "mod_deal":                                         # shard s holds the symbols with symbol mod S == s, in text order
        S = 5
        base = [int(v) for v in rng.integers(0, 40, 900)]
        shards = [np.array([v for v in base if v % S == s], np.int32) for s in range(S)]
        sub = [[int(v) for v in t] for t in shards]
        docs = [base[:60], sub[3][10:50] + sub[0][:12], [v for v in base[100:300] if v % S in (1, 2)]]
        return shards, {"dealt": docs}
    if name == "planted3":
        a, b, c = k1000[:400], k1000[400:800], k1000[800:1200]
        shards = [np.array(a[:100] + W_FIRST + a[100:250] + W_BOTH + a[250:], np.int32),
                  np.array(b[:50] + W_BOTH + b[50:300] + W_BOTH + b[300:] + W_END, np.int32),
                  np.array(c[:200] + W_LAST + c[200:], np.int32)]
        docs = [[NONE] + W_FIRST + [NONE] + W_LAST + [NONE], W_BOTH + [NONE], W_END + [NONE], W_END, W_LAST[5:] + W_FIRST[:5]]
        return shards, {"planted": docs}
    if name == "cut_window":
        p = 700
        shards = [np.array(k1000[:p + CUT_AT], np.int32), np.array(k1000[p + CUT_AT:], np.int32)]
        return shards, {"window": [[NONE] * 3 + k1000[p:p + CUT_LEN] + [NONE] * 2]}
    raise KeyError(name)


def make(name):
    """-> (shards, {batch: docs})"""
    if name in HAND_SETS:
        return _hand(name)
    text, S = name.split("/")
    e = mc.expected(text)
    bs = dict(e["batches"])
    bs["whole"] = [d[-mc.BODY_CAP:] for d in bs["whole"]]          # every shard searches the batch: the last BODY_CAP tokens stand in
    if int(S) == 3:
        bs.update(_pairs_batches([int(v) for v in e["t"]], np.random.default_rng(19)))
    return _cut(e["t"], int(S)), bs


def unsharded(name):
    """the shards of a set joined into one text"""
    return np.concatenate(make(name)[0]).astype(np.int32)


# ---- model A -----------------------------------------------------------------------------------------------------------------

def model_a(shards, sas, docs, max_length):
    """-> (merged uint64[total, 3]: length, shards, count; per uint32[S, total, 4]: first, count, length, ended)"""
    S = len(shards)
    total = sum(len(d) for d in docs)
    per = np.zeros((S, total, 4), np.uint32)
    merged = np.zeros((total, 3), np.uint64)
    lists = [([int(v) for v in t], [int(v) for v in sa]) for t, sa in zip(shards, sas)]
    if total == 0:
        return merged, per
    own = np.array([mc.spans_a(tl, sl, docs, max_length)[:, 2] for tl, sl in lists], np.int64)      # what every shard matches alone
    L = own.max(axis=0)
    flat = [(doc, j) for doc in docs for j in range(len(doc))]
    pref = [doc[j:j + int(l)] for (doc, j), l in zip(flat, L)]
    for s, (tl, sl) in enumerate(lists):
        if tl:
            per[s] = np.array(nc._spans_of(tl, sl, pref), np.uint32).reshape(-1, 4)
    if any(len(t) for t in shards):
        merged[:, 0] = L
    merged[:, 1] = (per[:, :, 1] > 0).sum(axis=0)
    merged[:, 2] = per[:, :, 1].astype(np.uint64).sum(axis=0)
    return merged, per


# ---- model B -----------------------------------------------------------------------------------------------------------------

def model_b(shards, batches, max_lengths=MAX_LENGTHS):
    """{(batch, max_length): (length int64[total], shards int64[total], count int64[total], per-shard counts int64[S, total])}"""
    S = len(shards)
    names = list(batches)
    seqs = [np.asarray(t, np.int64) for t in shards] + [np.asarray(d, np.int64) for b in names for d in batches[b]]
    x = np.concatenate(seqs) if seqs else np.zeros(0, np.int64)
    N = x.size
    left = np.concatenate([np.arange(len(q), 0, -1, dtype=np.int64) for q in seqs]) if N else np.zeros(0, np.int64)   # symbols up to the end of the sequence
    owner = np.concatenate([np.full(len(q), k, np.int64) for k, q in enumerate(seqs)]) if N else np.zeros(0, np.int64)
    in_shard = owner < S
    xr = np.unique(x, return_inverse=True)[1].astype(np.int64) if N else x
    K = int(xr.max()) + 1 if N else 1
    sizes = np.array([len(t) for t in shards], np.int64)
    qpos = np.flatnonzero(~in_shard)
    res = {M: [np.zeros(qpos.size, np.int64), np.full(qpos.size, int((sizes > 0).sum()), np.int64), np.full(qpos.size, int(sizes.sum()), np.int64),
               np.tile(sizes[:, None], (1, qpos.size))] for M in max_lengths}
    ids = np.zeros(N, np.int64)                                     # the name of the window of L symbols at p; L = 0: all alike
    for L in range(1, int(left[qpos].max()) + 1 if qpos.size else 1):
        p = np.flatnonzero(left >= L)
        if p.size == 0:
            break
        ids[p] = np.unique(ids[p] * K + xr[p + L - 1], return_inverse=True)[1]
        sp = p[in_shard[p]]                                         # the windows of L symbols of every shard
        names_n = int(ids[p].max()) + 1
        held = np.zeros((S, names_n), np.int64)
        np.add.at(held, (owner[sp], ids[sp]), 1)
        qv = left[qpos] >= L
        mine = held[:, np.where(qv, ids[qpos], 0)]                 # [S, positions]: the shard windows equal to the position's
        mine[:, ~qv] = 0                                            # (a position with fewer than L symbols left has no window)
        cnt = mine.sum(axis=0)
        hit = cnt > 0
        if not hit.any():
            break                                                   # no window of the query is held at L: none of L + 1 symbols is
        for M in max_lengths:
            if M == 0 or L <= M:
                r = res[M]
                r[0][hit] = L
                r[1][hit] = (mine > 0).sum(axis=0)[hit]
                r[2][hit] = cnt[hit]
                r[3][:, hit] = mine[:, hit]
    out, at = {}, 0
    for b in names:
        total = sum(len(d) for d in batches[b])
        for M in max_lengths:
            out[b, M] = tuple(a[..., at:at + total] for a in res[M])
        at += total
    return out


# ---- shared, computed once per process ---------------------------------------------------------------------------------------

_CACHE = {}
_CACHE_B = {}


def expected(name):
    """{"shards", "sas", "batches", "merged": {(batch, M): uint64[total, 3]}, "per": {(batch, M): uint32[S, total, 4]}}: model A"""
    if name not in _CACHE:
        shards, bs = make(name)
        sas = [model_sa(t).astype(np.int32) for t in shards]
        e = {"shards": shards, "sas": sas, "batches": bs, "merged": {}, "per": {}}
        for b, docs in bs.items():
            for M in MAX_LENGTHS:
                e["merged"][b, M], e["per"][b, M] = model_a(shards, sas, docs, M)
        _CACHE[name] = e
    return _CACHE[name]


def expected_b(name):
    if name not in _CACHE_B:
        shards, bs = make(name)
        _CACHE_B[name] = model_b(shards, bs)
    return _CACHE_B[name]


def merged_bytes(merged):
    """model A's merged rows as the device writes them: sa_hip_token_shards_match[total]"""
    out = np.zeros(len(merged), np.dtype([("length", "<u4"), ("shards", "<u4"), ("count", "<u8")]))
    out["length"], out["shards"], out["count"] = merged[:, 0], merged[:, 1], merged[:, 2]
    return out


def rows(found, heads, merged, cap, fill):
    """what a docs launch with `cap` writes: positions uint32[Q, cap], out_matches as uint32[Q, cap, 4] (cells beyond written keep
    the fill), heads uint32[Q, 4]"""
    q = len(heads)
    rec = merged_bytes(merged).view(np.uint32).reshape(-1, 4)
    pos = np.full((q, cap), fill & 0xFFFFFFFF, np.uint32)
    outs = np.full((q, cap, 4), fill & 0xFFFFFFFF, np.uint32)
    hd = np.zeros((q, 4), np.uint32)
    for d, (f, (maximal, longest, covered)) in enumerate(zip(found, heads)):
        w = min(len(f), cap)
        for k in range(w):
            pos[d, k] = f[k][0]
            outs[d, k] = rec[f[k][1]]
        hd[d] = (w, maximal, longest, covered)
    return pos, outs, hd
