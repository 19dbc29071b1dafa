"""Texts, contexts and the two CPU models of the span / next-symbol tests (test_token_next_cpu.py, test_gpu_token_next.py).

A span is (first, count, length, ended) and its next symbols are (symbol, count) pairs in ascending symbol order, as
include/sa_hip.h section 6b defines them.
  model A  from the model suffix array: ranges by token_cases.model_a (bisection with list comparison), the longest suffix by
           the binary search over L that the header's monotonicity argument allows, entries by counting t[p + length] over
           sa[first : first + count];
  model B  no suffix array and no monotonicity argument: E(L) = the text positions e such that the last L symbols of the
           context stand in front of e.  E(L) is E(L - 1) filtered by one more symbol, so the sets are nested by construction and
           the largest L whose set still qualifies is what trying every L from min(m, max_length) downwards finds.  Entries: a
           counter of t[e] over E(L).
"""
from collections import Counter

import numpy as np

import token_cases as tc
from test_int_cpu import model_sa

I32_MAX = 2 ** 31 - 1
LANE_MAX = 4                                   # tq::NEXT_LANE_MAX: spans of at most this many suffixes are answered by one lane
LANE_PLANS = ("lanes",)                        # the plans with the lane form (SA_HIP_TOKEN_NEXT_LANES defaults to 0)

RUNS = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)      # window edges, and the first jump stride (64^2) +- 1
PLANT_A = 1000003
PLANT_S = (0, 3, 5, 9, 17, 100, 1000, 65536, 2 ** 24 + 5, I32_MAX - 1, I32_MAX)

TEXTS = ("n0", "n1", "n2", "all_equal", "period2", "rand_k2", "rand_k1000", "zero_and_max", "dir_edge_out", "planted")

# (mode, max_length, need_next) of one launch; a context of the kind "8 symbols, the first replaced" has L = 7
CONFIGS = ((0, 0, 1), (1, 0, 1), (1, 0, 0), (1, 1, 1), (1, 7, 1), (1, 6, 1), (1, 7, 0))

PLANS = {
    "default": {},
    "lanes": {"SA_HIP_TOKEN_NEXT_LANES": "1"},
    "no_lanes": {"SA_HIP_TOKEN_NEXT_LANES": "0"},
    "no_jump": {"SA_HIP_TOKEN_NEXT_JUMP": "0"},
    "no_keys": {"SA_HIP_TOKEN_KEYS": "0"},
    "text_only": {"SA_HIP_TOKEN_KEYS": "0", "SA_HIP_TOKEN_DIR": "0"},
}


def set_plan(monkeypatch, plan):
    for k in ("SA_HIP_TOKEN_KEYS", "SA_HIP_TOKEN_DIR", "SA_HIP_TOKEN_NEXT_LANES", "SA_HIP_TOKEN_NEXT_JUMP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)


def planted_text():
    """[A, s_j] repeated r_j times for ascending s_j, then one more A: the span of [A] holds the ended suffix and 11 runs of
    the lengths RUNS"""
    parts = [np.tile(np.array([PLANT_A, s], np.int32), r) for s, r in zip(PLANT_S, RUNS)]
    return np.concatenate(parts + [np.array([PLANT_A], np.int32)])


def texts():
    c = tc.texts()
    c["planted"] = planted_text()
    return {k: c[k] for k in TEXTS}


def contexts(t, seed=11):
    """the context list of one text (lists of Python ints within int32)"""
    rng = np.random.default_rng(seed)
    tl = [int(v) for v in t]
    n = len(tl)
    ctx = [[], [-1], [-5, -6], [I32_MAX, I32_MAX, I32_MAX], [tc.I32_MIN]]
    if n == 0:
        return ctx + [[0], [1, 2, 3]]
    mn, mx = min(tl), max(tl)
    ctx += [[mx + 1]] if mx < I32_MAX else []                      # matches nowhere: L = 0
    starts = [0, max(n - 70, 0)] + [int(p) for p in rng.integers(0, n, 4)]
    for m in (1, 2, 3, 8, 64):
        for p in starts:
            w = tl[p:p + m]
            ctx += [w, [-9] + w[1:]]                               # the window, and with its first symbol replaced: L = m - 1
        tail = tl[max(n - m, 0):]                                  # ends at n: the ended suffix
        ctx += [tail, [-9] + tail, tail + [mn]]
    # the whole text, and one symbol more.  Model B costs the sum of its set sizes, n^2 / 2 on a text of period 1 or 2: of
    # such a text the last 3000 symbols stand in for the whole
    body = tl if n <= 6000 or len(set(tl[:64])) > 2 else tl[-3000:]
    ctx += [body + [mn], body + [mx], body]
    ctx += [[tl[-1]], [tl[0]], [mn], [mx]]
    if mn == mx:
        ctx += [[mn] * m for m in (2, 5, 100, 2999)]               # one run of n - m, the ended suffix first
    seen, out = set(), []
    for c in ctx:
        if tuple(c) not in seen and all(tc.I32_MIN <= v <= I32_MAX for v in c):
            seen.add(tuple(c))
            out.append(c)
    return out


# ---- model A -----------------------------------------------------------------------------------------------------------------

def _spans_of(t, sa, pats):
    """(first, count, length, ended) of whole patterns, by token_cases.model_a"""
    first, count = tc.model_a(t, sa, pats)
    return [(int(f), int(c), len(p), int(c > 0 and int(sa[int(f)]) + len(p) == len(t))) for f, c, p in zip(first, count, pats)]


def spans_a(t, sa, ctx, mode, max_length, need_next):
    n = len(t)
    if n == 0:
        return np.zeros((len(ctx), 4), np.uint32)
    if mode == 0:
        return np.array(_spans_of(t, sa, ctx), np.uint32).reshape(-1, 4)
    lo = [0] * len(ctx)
    hi = [min(len(c), max_length or len(c), n) for c in ctx]
    best = [(0, n, 0, 0)] * len(ctx)
    while True:                                                    # the binary searches of all contexts, one probe each per round
        live = [i for i in range(len(ctx)) if lo[i] < hi[i]]
        if not live:
            return np.array(best, np.uint32).reshape(-1, 4)
        probe = [(lo[i] + hi[i] + 1) // 2 for i in live]
        for i, L, s in zip(live, probe, _spans_of(t, sa, [ctx[i][len(ctx[i]) - L:] for i, L in zip(live, probe)])):
            if s[1] - (s[3] if need_next else 0) >= 1:
                lo[i], best[i] = L, s
            else:
                hi[i] = L - 1


def entries_a(t, sa, span):
    """(symbols, counts) of one span, uncapped"""
    first, count, length, _ = (int(v) for v in span)
    pos = np.asarray(sa[first:first + count], np.int64) + length
    nxt = np.asarray(t, np.int64)[pos[pos < len(t)]]
    sym, cnt = np.unique(nxt, return_counts=True)
    return sym.astype(np.int64), cnt.astype(np.int64)


# ---- model B -----------------------------------------------------------------------------------------------------------------

def model_b(t, ctx, mode, max_length, need_next):
    """per context: (count, length, ended, Counter of next symbols)"""
    tt = np.asarray(t, np.int64)
    n = tt.size
    out = []
    for c in ctx:
        m = len(c)
        if n == 0:
            out.append((0, 0, 0, Counter()))
            continue
        E = np.arange(n + 1, dtype=np.int64)                       # E(0): every position, the end (n) included ...
        limit = m if mode == 0 else min(m, max_length or m)
        L, best = 0, (0, E)                                        # the largest L seen so far whose set qualifies
        while L < limit and E.size:
            L += 1
            E = E[E - L >= 0]
            E = E[tt[E - L] == c[m - L]]
            if (int((E < n).sum()) if need_next else E.size) >= 1:
                best = (L, E)
        L, E = (m, E if L == m else E[:0]) if mode == 0 else best
        if L == 0:
            E = E[:n]                                              # ... but {0, n} is the n suffixes: the empty one is none
        out.append((int(E.size), L, int((E == n).any()), Counter(tt[E[E < n]].tolist())))
    return out


# ---- shared, computed once per process ---------------------------------------------------------------------------------------

_CACHE = {}


def expected(name):
    """{"t", "sa", "ctx", "spans": {config: uint32[Q, 4]}, "entries": {config: [(symbols, counts)]}} of one text"""
    if name not in _CACHE:
        t = texts()[name]
        sa = model_sa(t).astype(np.int32)
        ctx = contexts(t)
        tl, sl = [int(v) for v in t], [int(v) for v in sa]
        spans, entries, memo = {}, {}, {}
        for cfg in CONFIGS:
            spans[cfg] = spans_a(tl, sl, ctx, *cfg)
            entries[cfg] = []
            for s in spans[cfg].tolist():
                if tuple(s[:3]) not in memo:                       # (shared among the configurations: most spans recur)
                    memo[tuple(s[:3])] = entries_a(t, sa, s)
                entries[cfg].append(memo[tuple(s[:3])])
        _CACHE[name] = {"t": t, "sa": sa, "ctx": ctx, "spans": spans, "entries": entries}
    return _CACHE[name]


def capped(entries, cap, fill_sym, fill_cnt):
    """what a launch with `cap` writes: symbols[Q, cap], counts[Q, cap] (cells beyond written keep the fills), heads[Q, 4]"""
    q = len(entries)
    sym = np.full((q, cap), fill_sym, np.int32)
    cnt = np.full((q, cap), fill_cnt, np.uint32)
    heads = np.zeros((q, 4), np.uint32)
    for i, (s, c) in enumerate(entries):
        w = min(len(s), cap)
        sym[i, :w], cnt[i, :w] = s[:w], c[:w]
        heads[i] = (w, int(c[:w].sum()), int(c.sum()), 0)
    return sym, cnt, heads
