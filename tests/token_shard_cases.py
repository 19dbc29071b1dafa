"""Shard sets, contexts and the CPU combine model of the shard-set tests (test_token_shards_cpu.py, test_gpu_token_shards.py).

Per shard everything comes from the models the token tests already have: ranges by token_cases.model_a over
test_int_cpu.model_sa, spans and entries by token_next_cases (_spans_of / entries_a), the longest suffix by
token_next_cases.model_b.  What is new is the combination, in Python ints and sorted dicts:
  totals   the sum of the shards' (effective) counts;
  length   model B's qualifying sets are nested in L by construction, so shard s qualifies at L iff L <= L_s (its own longest
           suffix) and the sum over the shards is >= 1 iff some term is: L = max over s of L_s;
  spans    every shard's exact span of the last L symbols (an empty shard answers zeros, as its own handle does);
  entries  the shards' next-symbol counts added per symbol, ascending.
"""
import numpy as np

import token_cases as tc
import token_next_cases as nc
from test_int_cpu import model_sa

I32_MAX = nc.I32_MAX
A = 70001                                                          # the context symbol of the planted sets
MOD_S, MOD_D = 5, 40                                               # symbols 0..39 dealt to 5 shards by symbol mod 5

# (mode, max_length, need_next)
CONFIGS = ((0, 0, 1), (1, 0, 1), (1, 0, 0), (1, 1, 1), (1, 3, 1), (1, 4, 0))
SETS = ("s1", "s2", "s3", "s3_k2", "tiny64", "disjoint", "mod_deal", "one_next64", "ls")
PLAN_SETS = ("s3_k2", "ls", "mod_deal")                            # rebuilt under the plans of token_next_cases.PLANS
PLANS = ("default", "no_keys", "text_only")

# the longest-suffix set, by hand: [3, 4, 5] is in every shard -- followed by 9, ending the text, followed by 6
LS = ([1, 2, 3, 4, 5, 9], [7, 3, 4, 5], [8, 8, 2, 3, 4, 5, 6])
LS_CTX = [
    [0, 2, 3, 4, 5, 6],            # 5 symbols in the last shard only, where they end the text: L = 5 without need_next, 0 with
    [0, 8, 2, 3, 4],               # 4 symbols in the last shard only, with a successor
    [1, 2, 3, 4, 5, 9],            # the whole of the first shard: ends it, occurs nowhere else -> backs off under need_next
    [0, 1, 2, 3, 4, 5],            # 5 symbols in the first shard only (with a successor)
    [3, 4, 5],                     # ends shard 1, has a successor in shards 0 and 2: totals 2 with need_next, 3 without
    [7, 3, 4, 5],                  # only in shard 1, where it ends the text: L = 4 without need_next, 3 with
    [9, 7, 3, 4, 5],
    [8, 8, 2, 3, 4, 5, 6],         # the whole of the last shard
    [5, 6], [6], [9], [5, 9], [4, 5],
    [1] * 9,                       # longer than every shard
    [1, 2, 3, 4, 5, 9, 1, 2, 3, 4, 5, 9],
    [], [-4], [I32_MAX],
]


def _sets():
    nt = nc.texts()
    rng = np.random.default_rng(41)
    k2 = nt["rand_k2"]
    c = {
        "s1": [nt["zero_and_max"]],                                # holds 2^31 - 1: the merge's idle key must not collide
        "s2": [nt["planted"], nt["n1"]],
        "s3": [nt["n0"], nt["zero_and_max"][:2500], nt["n2"]],
        "s3_k2": [k2[:1500], k2[700:2500], k2[-1200:]],            # shared n-grams in all three
        "tiny64": [rng.integers(0, 5, 20 + s % 17).astype(np.int32) for s in range(64)],
        "disjoint": [(100 * s + rng.integers(0, 5, 300)).astype(np.int32) for s in range(4)],
        "ls": [np.array(t, np.int32) for t in LS],
    }
    # [A, x] for every x = s mod MOD_S, x + 1 times: every merge step takes its symbol from another shard
    c["mod_deal"] = [np.array([v for x in range(s, MOD_D, MOD_S) for v in [A, x] * (x + 1)] + [A], np.int32) for s in range(MOD_S)]
    # [A, 7] s + 1 times in shard s, then something of the shard's own: 64 counts are summed into the entry of 7
    c["one_next64"] = [np.array([A, 7] * (s + 1) + [A, 100 + s, 3], np.int32) for s in range(64)]
    return c


def contexts(name, shards, seed=17):
    rng = np.random.default_rng(seed)
    ctx = [[], [-1], [I32_MAX] * 3, [tc.I32_MIN], [A], [A, 7], [0, A], [A, A]]
    if name == "ls":
        ctx += LS_CTX
    pick = list(range(len(shards))) if len(shards) <= 5 else [0, 1, 31, 62, 63]
    for s in pick:
        tl = [int(v) for v in shards[s]]
        n = len(tl)
        if n == 0:
            continue
        for m in (1, 2, 3, 8):
            for p in [0, max(n - m, 0)] + [int(v) for v in rng.integers(0, n, 2)]:
                w = tl[p:p + m]
                ctx += [w, [-9] + w[1:], [min(tl)] + w]
        tail = tl[-3:]
        ctx += [tail, [-9] + tail, tail + [min(tl)], tl[-1:]]
    ctx += [[1] * (max(len(t) for t in shards) + 3)] if max(len(t) for t in shards) < 100 else []
    small = [[int(v) for v in t] for t in shards if 0 < len(t) < 100]
    ctx += small[:2] + [t + [t[0]] for t in small[:1]]
    seen, out = set(), []
    for c in ctx:
        if tuple(c) not in seen:
            seen.add(tuple(c))
            out.append(c)
    return out


def combine(shards, sas, ctx, mode, max_length, need_next):
    """-> length [Q], totals [Q] (Python ints), spans uint32[S, Q, 4], entries [(symbols, counts)] (Python int lists)"""
    S, Q = len(shards), len(ctx)
    if mode == 0:
        L = [len(c) for c in ctx]
    else:
        per = [nc.model_b(t, ctx, 1, max_length, need_next) for t in shards]
        L = [max(per[s][i][1] for s in range(S)) for i in range(Q)]
    tails = [c[len(c) - l:] for c, l in zip(ctx, L)]
    spans = np.zeros((S, Q, 4), np.uint32)
    merged = [dict() for _ in range(Q)]
    for s, (t, sa) in enumerate(zip(shards, sas)):
        if len(t) == 0:
            continue
        tl, sl = [int(v) for v in t], [int(v) for v in sa]
        spans[s] = np.array(nc._spans_of(tl, sl, tails), np.uint32).reshape(-1, 4)
        memo = {}
        for i in range(Q):
            key = tuple(spans[s, i, :3].tolist())
            if key not in memo:
                memo[key] = nc.entries_a(t, sa, spans[s, i])
            for y, c in zip(*(a.tolist() for a in memo[key])):
                merged[i][y] = merged[i].get(y, 0) + c
    totals = [sum(int(spans[s, i, 1]) - (int(spans[s, i, 3]) if need_next else 0) for s in range(S)) for i in range(Q)]
    entries = [(sorted(d), [d[y] for y in sorted(d)]) for d in merged]
    return L, totals, spans, entries


_CACHE = {}


def expected(name):
    """{"shards", "sas", "ctx", "first" / "count": uint32[S, Q], cfg: (length, totals, spans, entries)} of one set"""
    if name not in _CACHE:
        shards = _sets()[name]
        sas = [model_sa(t).astype(np.int32) for t in shards]
        ctx = contexts(name, shards)
        e = {"shards": shards, "sas": sas, "ctx": ctx}
        fc = [tc.model_a(t, sa, ctx) for t, sa in zip(shards, sas)]
        e["first"], e["count"] = np.array([f for f, _ in fc], np.uint32), np.array([c for _, c in fc], np.uint32)
        for cfg in CONFIGS:
            e[cfg] = combine(shards, sas, ctx, *cfg)
        _CACHE[name] = e
    return _CACHE[name]


def capped(length_of, entries, total_next, cap, fill):
    """what a launch with `cap` leaves: symbols int32[Q, cap], counts uint64[Q, cap] (cells beyond written keep the fill) and
    heads as rows (written, length, covered, total).  total_next[i]: the suffixes of context i's spans that have a next symbol"""
    q = len(entries)
    sym = np.full((q, cap), fill, np.int32)
    cnt = np.full((q, cap), fill & 0xFFFFFFFFFFFFFFFF, np.uint64)
    heads = []
    for i, (s, c) in enumerate(entries):
        w = min(len(s), cap)
        sym[i, :w], cnt[i, :w] = s[:w], c[:w]
        assert sum(c) == total_next[i]
        heads.append((w, length_of[i], sum(c[:w]), sum(c)))
    return sym, cnt, heads


def span_length(spans):
    """the `length` of a merged head: the largest among the context's S spans (an empty shard's span says 0)"""
    return spans[:, :, 2].max(axis=0).tolist()


def next_total(spans):
    return (spans[:, :, 1].astype(np.int64) - spans[:, :, 3]).sum(axis=0).tolist()


def brute(shards, pat):
    """(windows equal to pat over all shards, those with a symbol behind them, Counter-like dict of that symbol)"""
    m, hits, with_next, nxt = len(pat), 0, 0, {}
    for t in shards:
        tl = [int(v) for v in t]
        for p in range(len(tl) - m + 1 if m else len(tl)):
            if tl[p:p + m] == pat:
                hits += 1
                if p + m < len(tl):
                    with_next += 1
                    nxt[tl[p + m]] = nxt.get(tl[p + m], 0) + 1
    return hits, with_next, nxt
