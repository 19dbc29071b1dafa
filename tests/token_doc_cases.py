"""Texts, boundary tables and the two CPU models of the document tests (test_token_docs_cpu.py, test_gpu_token_docs.py).

Documents are a table `starts` (starts[0] == 0, non-decreasing, <= n): document d is t[starts[d] : starts[d + 1]], the last one runs
to n; equal neighbours are empty documents; doc(p) is the LARGEST d with starts[d] <= p.  An occurrence belongs to the document of
its first token (include/sa_hip.h section 6d).
  model A  from a model suffix array: DA[r] = doc(SA[r]) by np.searchsorted(starts, p, "right") - 1, PV by a dict sweep, the
           heads and entries of a span from a Python set over its first `examined` ranks;
  model B  no suffix array: the occurrences of a pattern by a window scan of the text, distinct = the size of the set of their
           documents (comparable when examined == count), the locate entries as a multiset.
"""
import numpy as np

import token_cases as tc
from test_int_cpu import model_sa

FILL = -7                                       # cells a launch must not write keep it

# ---- the all-equal text: closed forms beside the model -------------------------------------------------------------------------
# t = [A] * N_EQ cut every Ld tokens.  SA[r] = N_EQ - 1 - r (a shorter suffix sorts first), so DA is runs of Ld equal documents in
# descending order, PV[r] = r - 1 inside a run and -1 at its first rank, and the ranks [f, f + e) hold
# (N_EQ - 1 - f) // Ld - (N_EQ - f - e) // Ld + 1 distinct documents.
A = 7
N_EQ = 1500
LDS = (1, 2, 63, 64, 65, 256, 257)
UNROLL = 4                                      # tq::DOC_UNROLL: windows per step of the walk; the step is UNROLL * 64 ranks
COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025)      # window edges, the step +- 1, several steps and a rest
CAPS = (0, 1, 16, 64)
BUDGETS = tuple(sorted({0, 1, 64, 65} | {b for c in COUNTS for b in (c - 1, c, c + 1) if b > 0}))


def equal_text():
    return np.full(N_EQ, A, np.int32)


def equal_sa():
    return (N_EQ - 1 - np.arange(N_EQ)).astype(np.int32)


def equal_starts(Ld):
    return np.arange(0, N_EQ, Ld, dtype=np.int32)


def equal_mid(Ld):
    """a rank whose two neighbours hold the same document (Ld >= 3): PV[first] == first - 1, outside the range and a head;
    PV[first + 1] == first, inside it and none"""
    p = (N_EQ - 152) // Ld * Ld + 1             # the second position of a document
    return N_EQ - 1 - p


def equal_spans(Ld):
    """(first, count): every count from rank 0, ending at rank n, and from equal_mid"""
    out = []
    for c in COUNTS:
        out += [(0, c), (N_EQ - c, c), (equal_mid(Ld), c)]
    return out


def equal_distinct(Ld, first, examined):
    return 0 if examined == 0 else (N_EQ - 1 - first) // Ld - (N_EQ - first - examined) // Ld + 1


# ---- boundary tables -----------------------------------------------------------------------------------------------------------

def rand_table(n, D, seed, last_owns=True):
    """D sorted starts drawn with replacement from [0, n): empty documents wherever two are equal (always when D > n); with
    last_owns the last document starts at n - 1 and owns that token, so the largest document number occurs in DA"""
    rng = np.random.default_rng(seed)
    s = np.sort(rng.integers(0, max(n, 1), D)).astype(np.int32)
    s[0] = 0
    if last_owns and D > 1 and n > 0:
        s[-1] = n - 1
    return s


def with_empties(n):
    """empty documents at the front (0 and 1: document 2 owns position 0), in the middle and at the end (start == n)"""
    a, b = n // 3, 2 * n // 3
    return np.array([0, 0, 0, a, a, a, b, n, n], np.int32)


def one_token_each(n):
    return np.arange(n, dtype=np.int32)


# ---- model A -------------------------------------------------------------------------------------------------------------------

def doc_of(starts, p):
    return (np.searchsorted(np.asarray(starts, np.int64), np.asarray(p, np.int64), "right") - 1).astype(np.int32)


def model_da_pv(sa, starts):
    da = doc_of(starts, sa)
    pv = np.empty(len(sa), np.int32)
    last = {}
    for r, d in enumerate(da.tolist()):
        pv[r] = last.get(d, -1)
        last[d] = r
    return da, pv


def docs_a(sa, da, starts, first, count, cap, budget):
    """-> (head (written, examined, distinct, count), [(doc, offset)] of the written entries) of one span"""
    examined = min(count, budget) if budget else count
    seen, entries = set(), []
    for r in range(first, first + examined):
        d = int(da[r])
        if d not in seen:
            seen.add(d)
            entries.append((d, int(sa[r]) - int(starts[d])))
    return (min(len(entries), cap), examined, len(entries), count), entries[:cap]


def locate_a(sa, da, starts, first, count, cap):
    w = min(count, cap)
    return (w, count), [(int(da[r]), int(sa[r]) - int(starts[int(da[r])])) for r in range(first, first + w)]


def docs_full(sa, da, starts, spans, budget, most=64):
    """docs_a of every span (first, count) with cap = most: what docs_rows cuts to any cap <= most"""
    return [docs_a(sa, da, starts, int(f), int(c), most, budget) for f, c in spans]


def docs_rows(full, cap):
    """what a documents launch with `cap` writes: docs[Q, cap], offsets[Q, cap] (FILL beyond written), heads[Q, 4]"""
    q = len(full)
    docs, offs, heads = np.full((q, cap), FILL, np.int32), np.full((q, cap), FILL, np.int32), np.zeros((q, 4), np.uint32)
    for i, (head, ent) in enumerate(full):
        heads[i] = (min(head[2], cap), head[1], head[2], head[3])
        for j, (d, o) in enumerate(ent[:cap]):
            docs[i, j], offs[i, j] = d, o
    return docs, offs, heads


def locate_rows(sa, da, starts, spans, cap):
    q = len(spans)
    docs, offs, heads = np.full((q, cap), FILL, np.int32), np.full((q, cap), FILL, np.int32), np.zeros((q, 2), np.uint32)
    for i, (f, c) in enumerate(spans):
        heads[i], ent = locate_a(sa, da, starts, int(f), int(c), cap)
        for j, (d, o) in enumerate(ent):
            docs[i, j], offs[i, j] = d, o
    return docs, offs, heads


# ---- model B -------------------------------------------------------------------------------------------------------------------

def occurrences(t, p):
    """text positions at which the window equals p (the empty pattern: every position)"""
    t = np.asarray(t, np.int64)
    n, m = t.size, len(p)
    if m == 0:
        return np.arange(n)
    if m > n:
        return np.zeros(0, np.int64)
    idx = np.flatnonzero(t[:n - m + 1] == p[0])
    for j in range(1, m):
        if idx.size == 0:
            break
        idx = idx[t[idx + j] == p[j]]
    return idx


def model_b(t, starts, p):
    """-> (count, distinct documents, sorted [(doc, offset)] of all occurrences) of one pattern"""
    pos = occurrences(t, p)
    d = doc_of(starts, pos)
    s = np.asarray(starts, np.int64)
    return int(pos.size), len(set(d.tolist())), sorted(zip(d.tolist(), (pos - s[d]).tolist()))


# ---- the random texts, with model A's arrays, computed once per process --------------------------------------------------------

RANDOM = {"rand_k2": (300, 5), "rand_k1000": (4000, 6)}      # text of token_cases -> (D, seed) of its random table

_CACHE = {}


def random_case(name):
    """{"t", "sa", "starts", "da", "pv"} of one random text"""
    if name not in _CACHE:
        t = tc.texts()[name]
        sa = model_sa(t).astype(np.int32)
        D, seed = RANDOM[name]
        starts = rand_table(t.size, D, seed)
        da, pv = model_da_pv(sa, starts)
        _CACHE[name] = {"t": t, "sa": sa, "starts": starts, "da": da, "pv": pv}
    return _CACHE[name]


def equal_case(Ld):
    key = ("eq", Ld)
    if key not in _CACHE:
        sa, starts = equal_sa(), equal_starts(Ld)
        da, pv = model_da_pv(sa, starts)
        _CACHE[key] = {"t": equal_text(), "sa": sa, "starts": starts, "da": da, "pv": pv}
    return _CACHE[key]
