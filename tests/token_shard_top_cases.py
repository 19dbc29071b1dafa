"""Shard sets and the CPU models of the top-k / sampling tests over a set (test_token_shard_top_cpu.py, test_gpu_token_shard_top.py),
on top of token_shard_cases.py (its sets, contexts, configurations and the combine model) and token_top_cases.py (top_of).

  top-k model   the uncapped merged entries of a context (token_shard_cases.combine: the shards' counts added per symbol, ascending),
                cut in ascending symbol order at the budget -- the entry that the budget cuts keeps what lies inside -- then
                token_top_cases.top_of; the head is (written = min(k, distinct), distinct, length = the largest among the S spans,
                shards = those with count - ended > 0, covered = the sum of the written counts, total = the sum of count - ended);
  sample model  exact Python integers over the shard-major numbering: r = draw * total >> 64, s the shard with before_s <= r <
                before_s + total_s, rank = first_s + ended_s + (r - before_s), symbol = t_s[sa_s[rank] + length_s]; total == 0 gives
                (-1, 0xFFFFFFFF, 0xFFFFFFFF).

Planted sets: every shard is [A, symbol] x count ... [A] as token_top_cases.run_text builds a text, so every shard's span of [A]
starts with an ended suffix and holds its runs in the order of their symbols.
"""
import numpy as np

import token_next_cases as nc
import token_shard_cases as sc
import token_top_cases as tt
from test_int_cpu import model_sa

A = sc.A
CONFIGS = sc.CONFIGS
REUSED = ("s1", "s3", "s3_k2", "disjoint", "ls", "mod_deal", "one_next64", "tiny64")
PLANTED = ("sum_beats", "ties3", "queue_edge", "all_shared", "last_wins")
SETS = REUSED + PLANTED
PLAN_SETS = sc.PLAN_SETS
QUEUE = 1024                                                       # tq::SHARD_TOP_QUEUE: queue entries of one wave
JUMP_MIN = 256                                                     # tq::NEXT_JUMP_MIN


def depth(S):
    """tq::shard_top_depth: entries of one shard's queue"""
    return 64 if S <= 16 else 32 if S <= 32 else 16


def _queue_edge():
    runs = [[(1000 + 3 * j, 1) for j in range(70)],                # more than D completed runs in one window: cut at D, again at 64
            [(10, 5), (20, 70), (30, 3)],                          # a run longer than a window, short of the jump
            [(11, 5), (20, 4097), (31, 2)],                        # ... long enough for the jump; 20 is summed with the shard above
            [(12, 64), (40, 3)],                                   # a run that ends exactly at rank 64 of its window
            []]                                                    # an empty shard
    runs += [[(13 + s, s % 3 + 1), (1001 + 3 * (s - 5), 2)] for s in range(5, 17)]   # short runs between the other shards' symbols
    return runs


# per set and shard: [(symbol, count)] in ascending symbol order
RUNS = {
    "sum_beats": [[(50, 9), (100 + 2 * s, 10), (101 + 2 * s, 10)] for s in range(4)],
    "ties3": [[(7 * j, 1) for j in range(s, 130, 3)] for s in range(3)],
    "queue_edge": _queue_edge(),
    "all_shared": [[(3 * j, (7 * j + 3 * s) % 11 + 1) for j in range(40)] for s in range(5)],
    "last_wins": [[(1, 2), (4, 1), (900, 30)], [(2, 3), (900, 30)], [(1, 1), (3, 2), (5, 4)]],
}


def run_shard(runs):
    """[A, symbol] x count for every run, then one more A; no runs: an empty shard"""
    if not runs:
        return np.zeros(0, np.int32)
    return np.concatenate([np.tile(np.array([A, s], np.int32), c) for s, c in runs] + [np.array([A], np.int32)])


def merged_runs(name):
    """[(symbol, summed count)] of the planted context [A], ascending by symbol"""
    d = {}
    for runs in RUNS[name]:
        for s, c in runs:
            d[s] = d.get(s, 0) + c
    return sorted(d.items())


def planted_contexts(name):
    s0 = RUNS[name][0][0][0]
    return [[A], [], [A, s0], [s0, A], [s0], [A, A], [-9, A], [-9, s0], [A, s0, A], [s0, A, s0], [-1], [sc.I32_MAX] * 3, [5, A, 5]]


_CACHE = {}


def expected(name):
    """token_shard_cases.expected() for its own sets and, built the same way, for the planted ones"""
    if name in sc.SETS:
        return sc.expected(name)
    if name not in _CACHE:
        shards = [run_shard(r) for r in RUNS[name]]
        sas = [model_sa(t).astype(np.int32) for t in shards]
        ctx = planted_contexts(name)
        e = {"shards": shards, "sas": sas, "ctx": ctx}
        for cfg in CONFIGS:
            e[cfg] = sc.combine(shards, sas, ctx, *cfg)
        _CACHE[name] = e
    return _CACHE[name]


# ---- the top-k model ---------------------------------------------------------------------------------------------------------

def cut_entries(entries, budget):
    """(symbols, counts) ascending by symbol -> the first `budget` continuations of them (0: all); the cut entry keeps what lies inside"""
    sym, cnt = entries
    if not budget:
        return list(sym), list(cnt)
    out_s, out_c, left = [], [], int(budget)
    for s, c in zip(sym, cnt):
        if left == 0:
            break
        out_s.append(s)
        out_c.append(min(c, left))
        left -= out_c[-1]
    return out_s, out_c


def top_of(entries, k):
    sym, cnt = entries
    return tt.top_of((np.array(sym, np.int64), np.array(cnt, np.int64)), k)


def live_shards(spans):
    return ((spans[:, :, 1].astype(np.int64) - spans[:, :, 3]) > 0).sum(axis=0).tolist()


def top_expected(e, cfg, k, budget, fill):
    """what a launch writes for the contexts of e under cfg: symbols int32[Q, k], counts uint64[Q, k] (cells beyond written keep the
    fill), heads as rows (written, distinct, length, shards, covered, total)"""
    _, _, spans, entries = e[cfg]
    q = len(entries)
    sym = np.full((q, k), fill, np.int32)
    cnt = np.full((q, k), fill & 0xFFFFFFFFFFFFFFFF, np.uint64)
    length, live, total = sc.span_length(spans), live_shards(spans), sc.next_total(spans)
    heads = []
    for i, ent in enumerate(entries):
        assert sum(ent[1]) == total[i]
        walked = cut_entries(ent, budget)
        top = top_of(walked, k)
        for j, (s, c) in enumerate(top):
            sym[i, j], cnt[i, j] = s, c
        heads.append((len(top), len(walked[0]), length[i], live[i], sum(c for _, c in top), total[i]))
    return sym, cnt, heads


# ---- the sample model --------------------------------------------------------------------------------------------------------

def sample_of(e, spans, i, draw):
    """(symbol, shard, rank) of one draw on context i, spans uint32[S, Q, 4]: exact integers, the continuations numbered shard-major"""
    parts = [(int(sp[0]) + int(sp[3]), int(sp[1]) - int(sp[3]), int(sp[2])) for sp in spans[:, i]]
    total = sum(p[1] for p in parts)
    if total == 0:
        return -1, 0xFFFFFFFF, 0xFFFFFFFF
    r = (int(draw) * total) >> 64
    for s, (start, tot, length) in enumerate(parts):
        if r < tot:
            rank = start + r
            return int(e["shards"][s][int(e["sas"][s][rank]) + length]), s, rank
        r -= tot
    raise AssertionError("r < total")


def shard_major_runs(e, spans, i):
    """the run lengths of context i's continuations in the shard-major numbering: every shard's runs in its suffix order, the shards
    one after another (a run edge between two shards is a shard edge)"""
    out = []
    for s, sp in enumerate(spans[:, i]):
        if len(e["shards"][s]):
            out += nc.entries_a(e["shards"][s], e["sas"][s], sp)[1].tolist()
    return out


def shard_major_flat(e, spans, i):
    """the next symbol of every continuation of context i, in the shard-major numbering"""
    out = []
    for s, sp in enumerate(spans[:, i]):
        if len(e["shards"][s]):
            sym, cnt = nc.entries_a(e["shards"][s], e["sas"][s], sp)
            out += np.repeat(sym, cnt).tolist()
    return out
