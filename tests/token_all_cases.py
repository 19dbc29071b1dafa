"""Texts, tables and the two CPU models of the per-document count and AND-group tests (test_token_all_cpu.py, test_gpu_token_all.py).

The rank-by-document array RK (include/sa_hip.h section 6e): for every document d, RK[starts[d] : starts[d + 1]] (starts closed by
n) holds the ranks r with DA[r] == d, ascending.
  model A  from a model suffix array: RK by np.lexsort over (rank, DA[rank]); the count of a span in a document by two
           np.searchsorted inside its segment; the driver of a group by the rule (smallest count, lowest index on a tie); its
           candidates by a Python set over the driver's ranks; a match by set membership in every other span's documents.
  model B  no suffix array: the occurrences of every pattern by a window scan of the text (token_doc_cases.occurrences), counted
           per document; the documents that hold all patterns of a group as a set intersection.
"""
import bisect

import numpy as np

import token_cases as tc
import token_doc_cases as dc

FILL = dc.FILL
ALL_MAX = 16                                    # SA_HIP_TOKEN_ALL_MAX
I32_MAX = 2 ** 31 - 1


# ---- model A -------------------------------------------------------------------------------------------------------------------

def closed(starts, n):
    return np.append(np.asarray(starts, np.int64), n)


def model_rk(da):
    da = np.asarray(da)
    return np.lexsort((np.arange(da.size), da)).astype(np.int32)


def clamp(n, first, count):
    """(a, end) of a span as the device walks it"""
    a = min(int(first), n)
    return a, a + min(int(count), n - a)


def count_a(rk, cl, a, end, d):
    """ranks of [a, end) that belong to document d; an id outside the table counts 0"""
    if not 0 <= d < cl.size - 1:
        return 0
    seg = rk[cl[d]:cl[d + 1]]
    return int(np.searchsorted(seg, end, "left") - np.searchsorted(seg, a, "left"))


def counts_rows(rk, cl, n, spans, docs, written=None):
    """what a doc_counts launch writes: counts[Q, cap] (FILL beyond a row's length)"""
    docs = np.asarray(docs)
    q, cap = docs.shape
    out = np.full((q, cap), FILL & 0xFFFFFFFF, np.uint32)
    for i, (f, c) in enumerate(spans):
        a, end = clamp(n, f, c)
        for j in range(cap if written is None else min(int(written[i]), cap)):
            out[i, j] = count_a(rk, cl, a, end, int(docs[i, j]))
    return out


def driver_of(counts):
    return min(range(len(counts)), key=lambda j: (counts[j], j))


def all_walk(sa, da, cl, n, spans):
    """-> (driver, count, [(rank, doc, offset, match)] of the driver's candidates in rank order, their ranks, the ranks of those
    that match) of one group of (first, count)"""
    cs = [clamp(n, f, c) for f, c in spans]
    counts = [e - a for a, e in cs]
    drv = driver_of(counts)
    a, end = cs[drv]
    has = [set(da[x:y].tolist()) for x, y in cs]
    seen, out = set(), []
    for r in range(a, end):
        d = int(da[r])
        if d in seen:
            continue
        seen.add(d)
        out.append((r, d, int(sa[r]) - int(cl[d]), all(d in has[j] for j in range(len(cs)) if j != drv)))
    return drv, counts[drv], out, [c[0] for c in out], [c[0] for c in out if c[3]]


def all_a(walk, first, budget, most=64):
    """-> (head (written, examined, matched, candidates, driver, count), [(doc, offset)] of the first `most` matches)"""
    drv, count, cand, ranks, hits = walk
    examined = min(count, budget) if budget else count
    ncand, matched = bisect.bisect_left(ranks, first + examined), bisect.bisect_left(hits, first + examined)
    ent = []
    for _, d, o, m in cand[:ncand]:
        if len(ent) == min(matched, most):
            break
        if m:
            ent.append((d, o))
    return (min(matched, most), examined, matched, ncand, drv, count), ent


def group_first(n, spans):
    cs = [clamp(n, f, c) for f, c in spans]
    return cs[driver_of([e - a for a, e in cs])][0]


def all_rows(full, cap):
    """what an all launch with `cap` writes: docs[G, cap], offsets[G, cap] (FILL beyond written), heads[G, 8]"""
    g = len(full)
    docs, offs, heads = np.full((g, cap), FILL, np.int32), np.full((g, cap), FILL, np.int32), np.zeros((g, 8), np.uint32)
    for i, (head, ent) in enumerate(full):
        heads[i, :6] = (min(head[2], cap),) + tuple(head[1:])
        for j, (d, o) in enumerate(ent[:cap]):
            docs[i, j], offs[i, j] = d, o
    return docs, offs, heads


# ---- model B -------------------------------------------------------------------------------------------------------------------

def tf_b(t, starts, p):
    """{document: occurrences of p in it}"""
    d = dc.doc_of(starts, dc.occurrences(t, p))
    u, c = np.unique(d, return_counts=True)
    return dict(zip(u.tolist(), c.tolist()))


def all_b(t, starts, pats):
    """-> (sorted documents that hold every pattern, [tf_b of every pattern])"""
    tfs = [tf_b(t, starts, p) for p in pats]
    both = set(tfs[0])
    for f in tfs[1:]:
        both &= set(f)
    return sorted(both), tfs


# ---- the all-equal text --------------------------------------------------------------------------------------------------------
# SA[r] = N_EQ - 1 - r, document d = positions [d * Ld, (d + 1) * Ld), so its segment of RK is the ranks
# [N_EQ - min((d + 1) * Ld, N_EQ), N_EQ - d * Ld), consecutive; the count of [a, end) in d is the overlap of the two intervals.

N_EQ = dc.N_EQ
TF_LDS = (1, 2, 63, 64, 65)


def equal_segment(Ld, d):
    return N_EQ - min((d + 1) * Ld, N_EQ), N_EQ - d * Ld


def equal_count(Ld, a, end, d):
    D = len(dc.equal_starts(Ld))
    if not 0 <= d < D:
        return 0
    s, e = equal_segment(Ld, d)
    return max(0, min(e, end) - max(s, a))


def tf_docs(Ld):
    D = len(dc.equal_starts(Ld))
    return sorted({0, 1, D // 2, D - 2, D - 1})


def tf_cells(Ld):
    """(spans [(first, count)], docs int32[Q, 8]) of the count test: for the first, a middle and the last documents, spans that begin
    or end on the segment's first and last rank and one rank either side; empty spans; spans beyond the array; in every row the
    document, its neighbours and the ids -1, D and 2^31 - 1"""
    D = len(dc.equal_starts(Ld))
    spans, docs = [], []
    for d in tf_docs(Ld):
        s, e = equal_segment(Ld, d)
        bounds = sorted({max(s - 1, 0), s, min(s + 1, N_EQ), max(e - 1, 0), e, min(e + 1, N_EQ)})
        for a in bounds:
            for b in bounds:
                if b >= a:
                    spans.append((a, b - a))
                    docs.append([d, d - 1, d + 1, -1, D, I32_MAX, 0, D - 1])
        spans += [(s, 0), (N_EQ + 5, 3), (N_EQ, 0), (s, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF)]
        docs += [[d, d - 1, d + 1, -1, D, I32_MAX, 0, D - 1]] * 5
    return spans, np.array(docs, np.int64).astype(np.int32)


# AND groups on the all-equal text cut every token (Ld = 1): every rank is a candidate and document N_EQ - 1 - r is matched by a
# span iff the span holds rank r, so the matches of {[0, c), [lo, hi)} are the ranks [lo, min(c, hi)).
AND_COUNTS = (0, 1, 63, 64, 65, 66, 78, 79, 80, 81, 255, 256, 257, 258, 1025)
AND_OTHERS = ((63, 1400), (64, 1401), (65, 1402), (255, 1500), (256, 1500), (257, 1500), (0, 1500))
AND_CAPS = (0, 1, 16)
AND_BUDGETS = tuple(sorted({0} | {b for c in AND_COUNTS for b in (c - 1, c, c + 1) if b > 0}))


def and_groups():
    """groups of two spans (first, count): the driver [0, c) and a longer one"""
    return [[(0, c), (lo, hi - lo)] for c in AND_COUNTS for lo, hi in AND_OTHERS]


# ---- planted spans on a random text --------------------------------------------------------------------------------------------
# Synthetic spans (the device form takes any): A = two ranks that begin at a rank of document d, B = three ranks placed so that one
# other rank q of d sits at a_B - 1, a_B, end_B - 1 or end_B; d has no further rank near q, so B holds d in the middle two only.

_CACHE = {}


def planted_case():
    """{"t", "sa", "starts", "da", "pv", "rk", "cl", "groups": [[A, B]], "want": [bool], "last": [[A, B]]}"""
    if "planted" in _CACHE:
        return _CACHE["planted"]
    t = tc.texts()["rand_k4"]
    n = t.size
    sa = dc.model_sa(t).astype(np.int32)
    starts = dc.rand_table(n, 700, 21, last_owns=False)
    da, pv = dc.model_da_pv(sa, starts)
    rk, cl = model_rk(da), closed(starts, n)
    D = starts.size
    groups, want = [], []
    for d in range(0, D - 1, 37):
        seg = rk[cl[d]:cl[d + 1]].astype(np.int64)
        if seg.size < 4:
            continue
        i = seg.size // 2
        q, p = int(seg[i]), int(seg[0])
        if q - seg[i - 1] < 8 or seg[i + 1] - q < 8 or q < 8 or q + 8 > n or p + 2 > n or abs(p - q) < 8:
            continue
        A = (p, 2)
        for first, hit in ((q + 1, False), (q, True), (q - 2, True), (q - 3, False)):
            groups.append([A, (first, 3)])
            want.append(hit)
    # the last document: all of its ranks below a_B, so every lower bound of a_B lands at its segment's end, RK[n]
    seg = rk[cl[D - 1]:n].astype(np.int64)
    top = int(seg[-1])
    last = [[(int(seg[0]), 2), (top + 1, 3)], [(int(seg[0]), 2), (top, 3)], [(int(seg[-1]), 1), (top + 1, n)]]
    _CACHE["planted"] = {"t": t, "sa": sa, "starts": starts, "da": da, "pv": pv, "rk": rk, "cl": cl, "groups": groups, "want": want,
                         "last": last, "top": top, "last_size": int(seg.size)}
    return _CACHE["planted"]


def random_case(name):
    """token_doc_cases.random_case plus RK and the closed table"""
    key = ("rk", name)
    if key not in _CACHE:
        c = dict(dc.random_case(name))
        c["rk"], c["cl"] = model_rk(c["da"]), closed(c["starts"], c["t"].size)
        _CACHE[key] = c
    return _CACHE[key]


def random_groups(nctx, seed=5):
    """index groups over the contexts of a text: sizes 1, 2, 3 and 16, some with a repeated member"""
    rng = np.random.default_rng(seed)
    out = [[int(i)] for i in rng.integers(0, nctx, 6)]
    out += [rng.integers(0, nctx, 2).tolist() for _ in range(30)] + [rng.integers(0, nctx, 3).tolist() for _ in range(20)]
    out += [rng.integers(0, nctx, ALL_MAX).tolist(), [3, 3], [5, 9, 5]]
    return out
