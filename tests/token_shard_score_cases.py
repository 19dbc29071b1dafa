"""Shard sets, query batches and the two CPU models of the tests of infinity-gram scores over shard sets
(test_token_shard_score_cpu.py, test_gpu_token_shard_score.py).

A set is a list of shards (int32 texts); a batch is a list of query documents; a position is a flat index into the packed batch.
The answer of a position is the record (length, shards, context_count, token_count) and, per shard, the span (first, count, length,
ended) of the context with the token appended, as include/sa_hip.h section 6j defines them.  The sets and batches are those of
token_shard_match_cases.py, by import, and hand-made sets about the second fact (HAND): tails that several shards share.
  model A  as the device does it: the merged matching statistics of token_shard_match_cases.model_a, the smallest start whose match
           reaches the position by bisection over end(i) = i + ms(i), one span of that context per shard, the sum of the effective
           counts; where it is 0 the bisection over the shorter contexts with "some shard has an effective count >= 1" (the
           fallback), then per shard the numerator by two bisections over the next symbols of the context's range.  It keeps a trace
           of every fallback: (position, shards that held the candidate context -- each of them as its tail --, by how much the
           start moved).
  model B  no suffix array and neither fact: the (shard, position) pairs that stand behind an occurrence of the last L symbols,
           all positions of all shards and queries at once, named jointly and grown one symbol to the left per round; the answer
           of a position is the last round in which such a pair had its name.
"""
import numpy as np

import token_match_cases as mc
import token_score_cases as sc
import token_shard_match_cases as smc
from test_int_cpu import model_sa

NONE = mc.NONE
MAX_LENGTHS = mc.MAX_LENGTHS                    # (0, 1, 2, 3, 7)
PLANS = mc.PLANS
set_plan = mc.set_plan
pack = mc.pack

HAND = ("tail_of_two", "tail_and_interior", "tail_behind_window", "equal_shards", "followed", "cut_context", "tiny_beside_long")
SETS = smc.SETS + HAND
A, B, C, D = 100, 101, 102, 103                 # tokens that occur in no body


def _bodies():
    rng = np.random.default_rng(29)
    return [[int(v) for v in rng.integers(0, 5, 300)] for _ in range(3)]


def _hand(name):
    """-> (shards as lists, documents)"""
    b0, b1, b2 = _bodies()
    tail = [A, B, C]
    if name == "tail_of_two":
        # the same tail of three unique tokens ends two shards and stands nowhere else: wherever a query's context reaches into it
        # the total count is 2, both ended, the effective count 0, and the start moves to behind the tail
        return [b0 + tail, b1 + tail, b2], [[0] + tail + [1], tail + [A], b0[-10:] + tail + [2, 3], [B, C, 0], [C, C], [1, 2] + tail,
                                            b1[-4:] + tail + tail]
    if name == "tail_and_interior":
        # the tail ends shard 0 and stands in the interior of shard 1: an effective count of 1, no fallback
        return [b0 + tail, b1[:200] + tail + b1[200:]], [[0] + tail + [1], tail + [b1[200], 0], b1[190:200] + tail + [b1[200], b1[201]],
                                                         b0[-5:] + tail + [b1[200]]]
    if name == "tail_behind_window":
        # the tail of the last shard alone, behind a longer copied window: the fallback moves the start by the whole window
        return [b0, b1, b2 + tail], [b2[-20:] + tail + [2], b2[-3:] + tail + [b2[0]], [4] + tail[1:] + [0]]
    if name == "equal_shards":
        # all-equal shards scored with more of the same token: from the longer shard's length on the start moves by one
        return [[7] * 20, [7] * 12, [7] * 20], [[7] * 30, [7] * 12, [7] * 21 + [8, 7]]
    if name == "followed":
        # (1, 2) stands in every shard; 5 follows it in shard 1 only, 9 nowhere
        return [[1, 2, 3, 8, 1, 2, 4], [1, 2, 5, 8, 1, 2, 5, 7], [6, 1, 2, 3]], [[1, 2, 5], [1, 2, 9], [8, 1, 2, 3, 1], [7, 1, 2, 4, 4], [3, 1, 2, -1, 2]]
    if name == "cut_context":
        # (A, B | C, D): its only occurrence in the concatenation lies across the cut
        return [b0 + [A, B], [C, D] + b1], [[A, B, C, D, b1[0]], [B, C, D, b1[0], b1[1]], b0[-3:] + [A, B, C]]
    if name == "tiny_beside_long":
        return [[], [3], [3, A], b0 + [3]], [[3, A, 3], [A, 3, 3, A, 1], b0[5:12] + [3, A], b0[-2:] + [3, 3]]
    raise KeyError(name)


def make(name):
    """-> (shards, {batch: docs})"""
    if name in HAND:
        shards, docs = _hand(name)
        return [np.array(t, np.int32) for t in shards], {"hand": docs}
    return smc.make(name)


def unsharded(name):
    return np.concatenate(make(name)[0]).astype(np.int32)


# ---- model A -----------------------------------------------------------------------------------------------------------------

def score_a(shards, sas, docs, max_length, ms=None):
    """-> (scores uint64[total, 4] = (length, shards, context_count, token_count), per uint32[S, total, 4] = (first, count, length,
    ended), trace = [(position, shards that held the candidate, shift)]).  ms: the merged matching statistics of the batch under
    the same cap (None: way 2, the search over L from the capped context)"""
    S = len(shards)
    lists = [([int(v) for v in t], [int(v) for v in sa]) for t, sa in zip(shards, sas)]
    sizes = [len(tl) for tl, _ in lists]
    max_n = max(sizes)
    total = sum(len(d) for d in docs)
    scores, per, trace = np.zeros((total, 4), np.uint64), np.zeros((S, total, 4), np.uint32), []

    def spans(ctx):
        return [sc._span(tl, sl, ctx) if tl else (0, 0, 0) for tl, sl in lists]

    base = 0
    for doc in docs:
        for k in range(len(doc)):
            j = base + k
            if max_n == 0:
                continue
            hi = min(k, max_length or k, max_n)
            if ms is not None and hi:
                a, b = j - hi, j                                    # the smallest start whose match reaches j
                while a < b:
                    i = (a + b) // 2
                    if i + int(ms[i]) >= j:
                        b = i
                    else:
                        a = i + 1
                hi = j - b
            L, sp = hi, spans(doc[k - hi:k])
            if sum(c - e for _, c, e in sp) == 0 and hi > 0:        # every shard that holds it holds it as its tail alone
                lo, top = 0, hi - 1
                while lo < top:
                    mid = lo + (top - lo + 1) // 2
                    if any(c - e > 0 for _, c, e in spans(doc[k - mid:k])):
                        lo = mid
                    else:
                        top = mid - 1
                trace.append((j, sum(c > 0 for _, c, _ in sp), hi - lo))
                L, sp = lo, spans(doc[k - lo:k])
            cc = tc = held = 0
            for s, ((tl, sl), (f, c, e)) in enumerate(zip(lists, sp)):
                if not tl:
                    continue
                nf, ncnt = sc._narrow(tl, sl, f, c, e, L, doc[k])
                per[s, j] = (nf, ncnt, L + 1, int(ncnt > 0 and sl[nf] + L + 1 == len(tl)))
                cc, tc, held = cc + c - e, tc + ncnt, held + (ncnt > 0)
            scores[j] = (L, held, cc, tc)
        base += len(doc)
    return scores, per, trace


# ---- model B -----------------------------------------------------------------------------------------------------------------

def model_b(shards, batches, max_lengths=MAX_LENGTHS):
    """{(batch, max_length): (length, shards, context_count, token_count: int64[total]; per-shard token counts int64[S, total])}"""
    S = len(shards)
    names = list(batches)
    seqs = [np.asarray(t, np.int64) for t in shards] + [np.asarray(d, np.int64) for b in names for d in batches[b]]
    x = np.concatenate(seqs) if seqs else np.zeros(0, np.int64)
    N = x.size
    local = np.concatenate([np.arange(len(q), dtype=np.int64) for q in seqs]) if N else np.zeros(0, np.int64)   # symbols in front of it in its sequence
    owner = np.concatenate([np.full(len(q), k, np.int64) for k, q in enumerate(seqs)]) if N else np.zeros(0, np.int64)
    in_shard = owner < S
    xr = np.unique(x, return_inverse=True)[1].astype(np.int64).reshape(-1) if N else x
    K = int(xr.max()) + 1 if N else 1
    qpos = np.flatnonzero(~in_shard)
    res = {M: [np.zeros(qpos.size, np.int64) for _ in range(4)] + [np.zeros((S, qpos.size), np.int64)] for M in max_lengths}
    ctx = np.zeros(N, np.int64)                                     # the name of the L symbols in front of p; L = 0: all alike
    for L in range(0, int(local[qpos].max()) + 1 if qpos.size else 0):
        p = np.flatnonzero(local >= L)
        if L:
            ctx[p] = np.unique(ctx[p] * K + xr[p - L], return_inverse=True)[1].reshape(-1)
        gram = np.zeros(N, np.int64)                                # the name of those L symbols with the one at p behind them
        gram[p] = np.unique(ctx[p] * K + xr[p], return_inverse=True)[1].reshape(-1)
        sp = p[in_shard[p]]                                         # the pairs (shard, position) behind L symbols of their shard
        if sp.size == 0:
            break                                                   # no shard is as long as L + 1
        held = np.zeros((S, int(ctx[p].max()) + 1), np.int64)
        np.add.at(held, (owner[sp], ctx[sp]), 1)
        with_token = np.zeros((S, int(gram[p].max()) + 1), np.int64)
        np.add.at(with_token, (owner[sp], gram[sp]), 1)
        qv = local[qpos] >= L
        cc = held[:, np.where(qv, ctx[qpos], 0)].sum(axis=0)
        tc = with_token[:, np.where(qv, gram[qpos], 0)]
        hit = qv & (cc > 0)
        for M in max_lengths:
            if M == 0 or L <= M:
                r = res[M]
                r[0][hit] = L
                r[1][hit] = (tc > 0).sum(axis=0)[hit]
                r[2][hit] = cc[hit]
                r[3][hit] = tc.sum(axis=0)[hit]
                r[4][:, hit] = tc[:, hit]
    out, at = {}, 0
    for b in names:
        total = sum(len(d) for d in batches[b])
        for M in max_lengths:
            out[b, M] = tuple(a[..., at:at + total] for a in res[M])
        at += total
    return out


def heads_of(scores, docs):
    """uint64[Q, 5]: (scored, seen, certain, longest, length_sum) of every document, a NumPy reduction of uint64[total, 4] records"""
    out, base = np.zeros((len(docs), 5), np.uint64), 0
    for d, doc in enumerate(docs):
        r = scores[base:base + len(doc)]
        if len(doc):
            out[d] = (len(doc), (r[:, 3] > 0).sum(), (r[:, 3] == r[:, 2]).sum(), r[:, 0].max(), r[:, 0].sum())
        base += len(doc)
    return out


def score_bytes(scores):
    """model A's rows as the device writes them: sa_hip_token_shards_score[total]"""
    out = np.zeros(len(scores), np.dtype([("length", "<u4"), ("shards", "<u4"), ("context_count", "<u8"), ("token_count", "<u8")]))
    out["length"], out["shards"], out["context_count"], out["token_count"] = scores[:, 0], scores[:, 1], scores[:, 2], scores[:, 3]
    return out


# ---- shared, computed once per process ---------------------------------------------------------------------------------------

_MADE = {}
_CACHE = {}
_CACHE_B = {}


def base(name):
    """{"shards", "sas", "batches", "ms": {(batch, M): the merged lengths int64[total]}}"""
    if name not in _MADE:
        if name in HAND:
            shards, bs = make(name)
            sas = [model_sa(t).astype(np.int32) for t in shards]
            ms = {(b, M): smc.model_a(shards, sas, docs, M)[0][:, 0].astype(np.int64) for b, docs in bs.items() for M in MAX_LENGTHS}
        else:
            e = smc.expected(name)
            shards, sas, bs = e["shards"], e["sas"], e["batches"]
            ms = {key: m[:, 0].astype(np.int64) for key, m in e["merged"].items()}
        _MADE[name] = {"shards": shards, "sas": sas, "batches": bs, "ms": ms}
    return _MADE[name]


def expected(name):
    """base(name) and "scores": {(batch, M): uint64[total, 4]}, "per": {(batch, M): uint32[S, total, 4]}, "trace": {(batch, M): list}:
    model A with the matching statistics"""
    if name not in _CACHE:
        e = dict(base(name))
        e["scores"], e["per"], e["trace"] = {}, {}, {}
        for b, docs in e["batches"].items():
            for M in MAX_LENGTHS:
                e["scores"][b, M], e["per"][b, M], e["trace"][b, M] = score_a(e["shards"], e["sas"], docs, M, e["ms"][b, M])
        _CACHE[name] = e
    return _CACHE[name]


def expected_b(name):
    if name not in _CACHE_B:
        shards, bs = make(name)
        _CACHE_B[name] = model_b(shards, bs)
    return _CACHE_B[name]
