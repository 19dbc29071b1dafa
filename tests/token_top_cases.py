"""Texts and the CPU models of the top-k / sampling tests (test_token_top_cases_cpu.py, test_gpu_token_top.py), on top of
token_next_cases.py: its texts, contexts, configurations and span / entry models are used as they are.

  top-k model   the uncapped entries of a span (token_next_cases.entries_a), cut to a budget by running entries_a again on the span
                cut to `budget` ranks behind the ended suffix, then sorted by (-count, symbol); the head is (written = min(k,
                distinct), distinct, covered = the sum of the written counts, total = count - ended of the WHOLE span);
  sample model  exact Python integers: start = first + ended, total = count - ended, rank = start + (draw * total >> 64),
                symbol = t[sa[rank] + length]; total == 0 gives (-1, 0xFFFFFFFF).

Added texts: one context symbol A followed by prescribed runs, built the way token_next_cases.planted_text() builds RUNS -- the
span of [A] holds the ended suffix and then run j of RUN_TEXTS[name][j] ranks, symbols ascending.
"""
import numpy as np

import token_next_cases as nc
from test_int_cpu import model_sa

A = nc.PLANT_A
WINDOW = 64                                    # ranks of one window step
PLANS = ("default", "no_jump", "no_keys", "text_only")


def _shuffled(n, seed):
    return tuple(int(v) for v in np.random.default_rng(seed).permutation(np.arange(1, n + 1)))


RUN_TEXTS = {
    "top_desc": (40, 30, 20, 12, 9, 7, 5, 4, 3, 2, 1),        # descending counts: nothing behind the first k evicts
    "top_ties": (1,) * 130,                                   # equal counts across two window edges: the k-th place is a tie by symbol
    "top_edge64": (5, 59, 7, 58, 3),                          # the largest run is carried and ends exactly at rank 64
    "top_edge128": (5, 123, 7, 100, 3),                       # ... at rank 128, behind a window that is all that run
    "top_last": (3, 2, 70, 1, 200),                           # the largest run is the last: inserted behind the loop
    "top_jump": (5, 3, 4097, 2, 9),                           # a run long enough for the jump step, in the middle
    "top_many": _shuffled(70, 4),                             # >= 65 distinct continuations, every count different
}
NEW_TEXTS = tuple(RUN_TEXTS)
TEXTS = nc.TEXTS + NEW_TEXTS


def run_symbols(name):
    return [7 * j for j in range(len(RUN_TEXTS[name]))]


def run_text(name):
    parts = [np.tile(np.array([A, s], np.int32), r) for s, r in zip(run_symbols(name), RUN_TEXTS[name])]
    return np.concatenate(parts + [np.array([A], np.int32)])


_CACHE = {}


def expected(name):
    """token_next_cases.expected() for its own texts and, built the same way, for the added ones"""
    if name in nc.TEXTS:
        return nc.expected(name)
    if name not in _CACHE:
        t = run_text(name)
        sa = model_sa(t).astype(np.int32)
        ctx = nc.contexts(t)
        tl, sl = [int(v) for v in t], [int(v) for v in sa]
        spans, entries, memo = {}, {}, {}
        for cfg in nc.CONFIGS:
            spans[cfg] = nc.spans_a(tl, sl, ctx, *cfg)
            entries[cfg] = []
            for s in spans[cfg].tolist():
                if tuple(s[:3]) not in memo:
                    memo[tuple(s[:3])] = nc.entries_a(t, sa, s)
                entries[cfg].append(memo[tuple(s[:3])])
        _CACHE[name] = {"t": t, "sa": sa, "ctx": ctx, "spans": spans, "entries": entries}
    return _CACHE[name]


def run_span(name):
    """(index of the context [A], its exact span) of an added text or of "planted" """
    e = expected(name)
    i = e["ctx"].index([A])
    return i, e["spans"][(0, 0, 1)][i]


# ---- the top-k model ---------------------------------------------------------------------------------------------------------

def walked_entries(t, sa, span, budget):
    """(symbols, counts) of the first `budget` ranks behind the ended suffix (0: all of them)"""
    first, count, length, ended = (int(v) for v in span)
    total = count - ended
    walked = min(total, budget) if budget else total
    return nc.entries_a(t, sa, (first + ended, walked, length, 0))


def top_of(entries, k):
    """[(symbol, count)] by count descending, ties by symbol ascending, the first k"""
    sym, cnt = entries
    return sorted(zip(sym.tolist(), cnt.tolist()), key=lambda p: (-p[1], p[0]))[:k]


def top_expected(e, cfg, k, budget, fill_sym, fill_cnt):
    """what a launch writes for the contexts of e under cfg: symbols[Q, k], counts[Q, k] (cells beyond written keep the fills),
    heads[Q, 4] = (written, distinct, covered, total)"""
    q = len(e["ctx"])
    sym = np.full((q, k), fill_sym, np.int32)
    cnt = np.full((q, k), fill_cnt, np.uint32)
    heads = np.zeros((q, 4), np.uint32)
    memo = {}
    for i, span in enumerate(e["spans"][cfg].tolist()):
        key = tuple(span[:3])
        if key not in memo:
            ent = walked_entries(e["t"], e["sa"], span, budget) if budget else e["entries"][cfg][i]
            memo[key] = (top_of(ent, k), len(ent[0]))
        top, distinct = memo[key]
        for j, (s, c) in enumerate(top):
            sym[i, j], cnt[i, j] = s, c
        heads[i] = (len(top), distinct, sum(c for _, c in top), span[1] - span[3])
    return sym, cnt, heads


# ---- the sample model --------------------------------------------------------------------------------------------------------

def sample_of(t, sa, span, draw):
    """(symbol, rank) of one draw, in exact integers"""
    first, count, length, ended = (int(v) for v in span)
    start, total = first + ended, count - ended
    if total == 0:
        return -1, 0xFFFFFFFF
    rank = start + ((int(draw) * total) >> 64)
    return int(t[int(sa[rank]) + length]), rank


def edge_draws(counts):
    """the draws that pin every run edge of a span with these run lengths: 0, 2^64 - 1 and, for every edge j (a proper prefix sum
    of the counts), the smallest draw that lands on rank j and the one before it"""
    total = int(sum(int(c) for c in counts))
    out = [0, 2 ** 64 - 1]
    j = 0
    for c in list(counts)[:-1]:
        j += int(c)
        d = -((-j << 64) // total)                     # ceil(j * 2^64 / total)
        out += [d, d - 1]
    return out


def window_counter(t, pattern):
    """{symbol: count} behind the windows of the text equal to `pattern`, by brute force (no suffix array)"""
    t = np.asarray(t, np.int64)
    m = len(pattern)
    idx = np.arange(max(t.size - m, 0), dtype=np.int64)            # windows that have a symbol behind them
    for j, v in enumerate(pattern):
        idx = idx[t[idx + j] == v]
    s, c = np.unique(t[idx + m], return_counts=True)
    return dict(zip(s.tolist(), c.tolist()))
