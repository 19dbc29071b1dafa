"""Shard sets with rank-by-document arrays, and the two CPU models of the set's per-document counts and AND groups
(test_token_shard_all_cpu.py, test_gpu_token_shard_all.py).  include/sa_hip.h section 6h.

A set is a list of shards as token_shard_doc_cases builds them, each with RK and the closed table of token_all_cases added
(ranked).  gspans[s][j] is the (first, count) of a group's pattern j in shard s; c[s][j] its count after the clamp and
C[j] = the sum over s.
  model A  per shard from a model suffix array: the count of a span in a document by two searches in its segment of RK
           (token_all_cases.count_a), the shard of a global id by bisection of the bases; the driver of a group by the rule on the
           C[j] in Python ints (smallest sum, lowest index on a tie), ONE per group; the budget cut e_s by
           token_shard_doc_cases.split_budget over the driver's counts; per shard a walk of the driver's first e_s ranks with a seen
           set for the candidates and set membership for the matches; the lists one after another with the bases added;
  model B  no suffix array: a window scan of every shard's text per document (token_all_cases.tf_b) gives the counts and, as an
           intersection, the set of documents that hold all n-grams.  Without a budget it does not depend on the driver.
Planted sets: the all-equal shards of token_shard_doc_cases with groups made of its contexts (every count on an edge of the walk);
driver_set(), three shards over a small alphabet with the planted 2-grams X, Y, Z, W (what the plants are for: DRIVER_NOTES);
edge_set(), whose middle shard carries the plants of token_all_cases.planted_case on a text of 4 000 tokens, asked with synthetic
spans through the device form.
"""
import bisect

import numpy as np

import token_all_cases as ta
import token_cases as tc
import token_doc_cases as td
import token_shard_doc_cases as sd

FILL, FILL64 = sd.FILL, sd.FILL64
FILL32 = FILL & 0xFFFFFFFF
MOST = sd.MOST


def ranked(cases):
    for c in cases:
        if "rk" not in c:
            c["rk"], c["cl"] = ta.model_rk(c["da"]), ta.closed(c["starts"], len(c["t"]))
    return cases


def clamped(cases, gspans):
    return [[ta.clamp(len(c["t"]), f, k) for f, k in row] for c, row in zip(cases, gspans)]


# ---- model A: counts -----------------------------------------------------------------------------------------------------------

def count_set(cases, spans_i, gid):
    """occurrences of one context (its S (first, count)) in the document with the global id gid"""
    base = sd.bases(cases)
    if not 0 <= gid < base[-1]:
        return 0
    s = bisect.bisect_right(base, gid) - 1
    c = cases[s]
    a, end = ta.clamp(len(c["t"]), *spans_i[s])
    return ta.count_a(c["rk"], c["cl"], a, end, gid - base[s])


def counts_rows(cases, spans, docs, written=None):
    """what a doc_counts call writes: counts uint32[Q, cap] (FILL beyond a row's length); spans [S][Q], docs [Q, cap] global ids"""
    q, cap = len(docs), len(docs[0])
    out = np.full((q, cap), FILL32, np.uint32)
    for i in range(q):
        sp = sd.context(spans, i)
        for j in range(cap if written is None else min(int(written[i]), cap)):
            out[i, j] = count_set(cases, sp, int(docs[i][j]))
    return out


# ---- model A: AND groups -------------------------------------------------------------------------------------------------------

def plan_set(cases, gspans, budget):
    """-> (driver, [C_j], [c_{s,driver}], [e_s])"""
    cl = clamped(cases, gspans)
    m = len(gspans[0])
    C = [sum(row[j][1] - row[j][0] for row in cl) for j in range(m)]
    drv = ta.driver_of(C)
    cd = [row[drv][1] - row[drv][0] for row in cl]
    return drv, C, cd, sd.split_budget(cd, budget)


def _walk(case, n, spans_s, drv):
    """the driver's candidates of one shard in rank order: (ranks, match flags, (doc, offset))"""
    memo = case.setdefault("_all_walk", {})
    key = (tuple(spans_s), drv)
    if key not in memo:
        cs = [ta.clamp(n, f, k) for f, k in spans_s]
        a, end = cs[drv]
        has = [set(case["da"][x:y].tolist()) for x, y in cs]
        seen, ranks, flags, ent = set(), [], [], []
        for r in range(a, end):
            d = int(case["da"][r])
            if d in seen:
                continue
            seen.add(d)
            ranks.append(r)
            flags.append(all(d in has[j] for j in range(len(cs)) if j != drv))
            ent.append((d, int(case["sa"][r]) - int(case["starts"][d])))
        memo[key] = (a, ranks, flags, ent)
    return memo[key]


def all_set(cases, gspans, cap, budget):
    """-> (head (written, driver, examined, matched, candidates, count), [(global doc, offset)] cut at cap, per-shard
    (examined, matched, candidates))"""
    base = sd.bases(cases)
    drv, C, cd, es = plan_set(cases, gspans, budget)
    entries, parts = [], []
    for s, c in enumerate(cases):
        a, ranks, flags, ent = _walk(c, len(c["t"]), gspans[s], drv)
        k = bisect.bisect_left(ranks, a + es[s])
        hits = [(base[s] + d, o) for (d, o), f in zip(ent[:k], flags[:k]) if f]
        entries += hits
        parts.append((es[s], len(hits), k))
    matched = sum(p[1] for p in parts)
    return (min(matched, cap), drv, sum(es), matched, sum(p[2] for p in parts), C[drv]), entries[:cap], parts


def all_full(cases, groups, budget):
    """all_set of every group without a cap, the entries as (uint64 documents, int32 offsets): what all_rows cuts to any cap"""
    out = []
    for gs in groups:
        head, ent, _ = all_set(cases, gs, MOST, budget)
        out.append((head, np.array([d for d, _ in ent], np.uint64), np.array([o for _, o in ent], np.int32)))
    return out


def all_rows(full, cap):
    """what an all call with `cap` writes: docs uint64[G, cap] (FILL64 beyond written), offsets int32[G, cap] (FILL), and the heads
    as (written, driver, examined, matched, candidates, count) tuples"""
    g = len(full)
    docs, offs, heads = np.full((g, cap), FILL64, np.uint64), np.full((g, cap), FILL, np.int32), []
    for i, (head, ed, eo) in enumerate(full):
        w = min(head[3], cap)
        heads.append((w,) + tuple(head[1:]))
        docs[i, :w], offs[i, :w] = ed[:w], eo[:w]
    return docs, offs, heads


def group_spans(spans, members):
    """spans [S][P] and the pattern indices of a group -> gspans[s][j]"""
    return [[row[p] for p in members] for row in spans]


def flat_groups(groups):
    """index groups -> (flat pattern indices, uint64 group offsets)"""
    flat, goff = [], [0]
    for g in groups:
        flat += list(g)
        goff.append(len(flat))
    return flat, np.array(goff, np.uint64)


# ---- model B -------------------------------------------------------------------------------------------------------------------

def all_b_set(cases, pats):
    """-> (sorted global ids of the documents that hold every pattern, [{global id: occurrences} of every pattern])"""
    base = sd.bases(cases)
    tfs = [{} for _ in pats]
    for s, c in enumerate(cases):
        for j, p in enumerate(pats):
            tfs[j].update({base[s] + d: k for d, k in ta.tf_b(c["t"], c["starts"], p).items()})
    both = set(tfs[0])
    for f in tfs[1:]:
        both &= set(f)
    return sorted(both), tfs


# ---- the all-equal shards: groups of token_shard_doc_cases.equal_contexts ------------------------------------------------------

def equal_groups():
    """index groups over the contexts of the all-equal shards: pairs whose per-shard counts sit on different edges of the walk, the
    empty and the one-shard contexts beside a long one, a single, a triple, ALL_MAX members and a repeated member"""
    q = len(sd.equal_contexts()[0])
    out = [[i, (i + 3) % q] for i in range(q)] + [[(i + 7) % q, i] for i in range(0, q, 2)]
    out += [[5], [11, 8, 9], list(range(ta.ALL_MAX)), [10, 10], [q - 6, 11], [q - 5, 11], [q - 4, 11], [q - 3, 11]]
    return out


# ---- the driver plants ---------------------------------------------------------------------------------------------------------
# Filler symbols 1 .. 3, the separator 0 closes every document, X .. W are 2-grams of symbols the filler never holds: an n-gram
# occurs exactly where it is planted.
X, Y, Z, W = [7, 8], [9, 10], [11, 12], [13, 14]
DRIVER_DOCS = (
    ([X, Y], [X, Y, Y], [Y], [Y, Y], [Y], [Y, Y, Y], [Z, W], [Z], []),                  # shard 0: X rare (2), Y frequent (10)
    ([X, X, X], [X, X, Y], [X, X, X, X], [X, X, X], [W, W], [W], [W]),                  # shard 1: X frequent (12), Y rare (1), no Z
    ([X, Y, Z], [X, Z], [Y, Y, X, Z], []),                                              # shard 2: no W
)
DRIVER_TOTALS = {"X": (2, 12, 3), "Y": (10, 1, 3), "Z": (2, 0, 3), "W": (1, 4, 0)}
DRIVER_NOTES = """
(a) {X, Y}: C_X = 17 > C_Y = 14, so the driver is Y although shard 0's rarest span is X (2 against 10); shard 1 is the reverse;
(b) {Z, W} and {W, Z}: C_Z = C_W = 5, the lowest index wins, Z in the first and W in the second;
(c) {Z, W}: shard 1 misses the driver Z entirely;
(d) {Z, W}: shard 2 holds the driver (3 candidates) but no W: candidates and no match.
"""
DRIVER_GROUPS = ([X, Y], [Z, W], [W, Z], [X, Y, Z], [Y], [X, [5, 5]], [W, X])
DRIVER_WANT = (          # (driver, count, matched, candidates) without a budget, counted by hand from DRIVER_DOCS
    (1, 14, 5, 9), (0, 5, 1, 5), (0, 5, 1, 4), (2, 5, 2, 5), (0, 14, 9, 9), (1, 0, 0, 0), (0, 5, 0, 4))


def driver_set():
    if "driver" not in _CACHE:
        rng = np.random.default_rng(77)
        cases = []
        for docs in DRIVER_DOCS:
            t, starts = [], []
            for plants in docs:
                starts.append(len(t))
                for p in plants:
                    t += rng.integers(1, 4, int(rng.integers(3, 20))).tolist() + p
                t += rng.integers(1, 4, int(rng.integers(3, 20))).tolist() + [0]
            cases.append(sd.shard_case(t, starts))
        _CACHE["driver"] = ranked(cases)
    return _CACHE["driver"]


# ---- the edge plants -----------------------------------------------------------------------------------------------------------
# token_all_cases.planted_case on a shorter text: A = two ranks that begin at the first rank of document d, B = three ranks placed
# so that one other rank q of d sits at a_B - 1, a_B, end_B - 1 or end_B; d has no further rank near q.  The last document: every
# rank below a_B.  The outer shards answer A and B with one rank each, so the driver stays A (C_A = 4 < C_B = 5).

def edge_set():
    """-> (cases, groups as gspans, want = (global id of the planted document, whether it matches), index of the first group of the
    last document)"""
    if "edge" in _CACHE:
        return _CACHE["edge"]
    t = tc.texts()["rand_k4"]
    n = 4000
    mid = sd.shard_case(t[:n], td.rand_table(n, 60, 21, last_owns=False))
    cases = ranked([sd.shard_case(t[5000:5600], td.rand_table(600, 9, 3)), mid, sd.shard_case(t[7000:7900], td.rand_table(900, 14, 4))])
    rk, cl, D = mid["rk"], mid["cl"], len(mid["starts"])
    inner, want = [], []
    for d in range(D - 1):
        seg = rk[cl[d]:cl[d + 1]].astype(np.int64)
        if seg.size < 4:
            continue
        i = seg.size // 2
        q, p = int(seg[i]), int(seg[0])
        if q - seg[i - 1] < 8 or seg[i + 1] - q < 8 or q < 8 or q + 8 > n or p + 2 > n or abs(p - q) < 8:
            continue
        for first, hit in ((q + 1, False), (q, True), (q - 2, True), (q - 3, False)):
            inner.append([(p, 2), (first, 3)])
            want.append((len(cases[0]["starts"]) + d, hit))
    seg = rk[cl[D - 1]:n].astype(np.int64)
    top = int(seg[-1])
    last_at = len(inner)
    inner += [[(int(seg[0]), 2), (top + 1, 3)], [(int(seg[0]), 2), (top, 3)], [(int(seg[-1]), 1), (top + 1, n)]]
    want += [(len(cases[0]["starts"]) + D - 1, hit) for hit in (False, True, False)]
    groups = [[[(0, 1), (0, 1)], g, [(3, 1), (40, 1)]] for g in inner]
    _CACHE["edge"] = (cases, groups, want, last_at)
    return _CACHE["edge"]


# ---- the random sets -----------------------------------------------------------------------------------------------------------

def random_groups(npat, seed=5):
    """index groups over the patterns of a random set: sizes 1, 2, 3 and ALL_MAX, some with a repeated member"""
    rng = np.random.default_rng(seed)
    out = [[int(i)] for i in rng.integers(0, npat, 4)]
    out += [rng.integers(0, npat, 2).tolist() for _ in range(40)] + [rng.integers(0, npat, 3).tolist() for _ in range(20)]
    out += [rng.integers(0, npat, ta.ALL_MAX).tolist(), [3, 3], [5, 9, 5]]
    return out


def frequent_patterns(cases):
    """short windows of every shard and single symbols: n-grams that many documents hold, so that groups of them match"""
    rng = np.random.default_rng(41)
    pats = [[]]
    for c in cases:
        tl = c["t"].tolist()
        for m in (1, 1, 1, 2, 2, 3):
            for p in rng.integers(0, len(tl) - m, 3):
                pats.append(tl[int(p):int(p) + m])
    return pats


def count_ids(cases):
    """global ids at base[s] - 1, base[s] and base[s + 1] - 1 of every shard, at base[S], beyond it and at 2^63"""
    base = sd.bases(cases)
    ids = set()
    for b in base:
        ids |= {b - 1, b, b + 1}
    ids |= {base[-1] + 5, 2 ** 32, 2 ** 63, 2 ** 64 - 1}
    return sorted(i for i in ids if i >= 0)


_CACHE = {}
