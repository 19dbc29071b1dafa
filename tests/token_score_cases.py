"""Corpora, query batches and the two CPU models of the infinity-gram score tests (test_token_score_cpu.py, test_gpu_token_score.py).

A batch is a list of query documents; a position is a flat index into the packed batch.  The score of a position j of a document
that starts at s is (length, context_count, token_count, first) as include/sa_hip.h section 6i defines it: the longest context
doc[j - L : j] (L <= min(j - s, max_length, n); max_length 0: no cap) that the corpus holds with a token behind it, how often it
does, how often that token is doc[j], and the number of suffixes that sort before the context followed by doc[j].
  model A  as the device does it, from the model suffix array and the matching statistics of token_match_cases.spans_a: the
           smallest start whose match reaches j by bisection over end(i) = i + ms(i); one range of that context; where it is the
           corpus's tail and nothing else, the bisection over the shorter contexts (the fallback); the numerator by two bisections
           over the next symbols of the context's range.  It also keeps a trace of what each position met.
  model B  brute force, no suffix array, no matching statistics and no monotonicity: the set of text positions that stand behind
           an occurrence of the context, grown one symbol to the left at a time until it is empty; the counts are set sizes.
           It gives (length, context_count, token_count).
A case is one corpus (at most 2000 tokens) with one batch; every case is scored for every max_length of MAX_LENGTHS.
"""
import numpy as np

import token_match_cases as mc
from test_int_cpu import model_sa

NONE = mc.NONE
MAX_LENGTHS = mc.MAX_LENGTHS                    # (0, 1, 2, 3, 7)
PLANS = mc.PLANS
set_plan = mc.set_plan
pack = mc.pack

# the batches of token_match_cases.batches that every text is scored with: windows and tails of the text, tokens outside the
# alphabet, empty documents, the docs kernel's window edges (documents of 1, 63, 64, 65, 127, 128, 129 tokens) and workgroup edge
# (3, 4, 5 documents), the score kernel's block edge (255, 256, 257 positions), long copied windows
BATCHES = ("windows", "tails", "whole", "odd_tokens", "empty_docs", "all_empty", "doc_sizes", "q3", "q4", "q5", "total255", "total256",
           "total257", "carried")


def _special():
    """name -> (corpus, documents): the cases the fallback and the numerator are about"""
    rng = np.random.default_rng(17)
    body = [int(v) for v in rng.integers(0, 5, 400)]
    a, b, c = 100, 101, 102                                          # occur nowhere in body
    out = {}
    # an all-equal corpus of 20 tokens scored with 30 of them: from position 19 on the context is 7^19 (in the corpus twice, once
    # ended) followed by 7 once; from position 20 on fact 1 gives 7^20, the corpus itself, and the fallback moves the start by one
    out["equal20"] = ([7] * 20, [[7] * 30, [7] * 19, [7] * 21 + [8, 7]])
    # a corpus that ends in three tokens that occur nowhere else, pasted into queries: behind the paste every context that reaches
    # into it is the corpus's tail, and the fallback moves the start by 3, 2 and 1 down to L = 0
    out["unique_tail"] = (body + [a, b, c], [[0, a, b, c, 1], [a, b, c, a], body[390:] + [a, b, c, 2, 3], [b, c, 0], [c, c], [1, 2, a, b, c]])
    # the same tail standing twice: count 2, one of them ended, an effective count of 1 and no fallback
    out["tail_twice"] = (body[:200] + [a, b, c] + body[200:] + [a, b, c], [[0, a, b, c, 1], [a, b, c, body[200], 0], body[190:200] + [a, b, c, body[200], body[201]]])
    # a context that occurs but is never followed by the query's token: token_count 0 with L > 0
    out["never_followed"] = ([1, 2, 3, 1, 2, 4, 5, 1, 2, 3], [[1, 2, 9], [5, 1, 2, 5], [1, 2, 3, 1, 2, 3], [4, 5, 1, 2, 4, 4], [3, 1, 2, -1, 2]])
    return out


def cases():
    """name -> (int32 corpus, list of documents)"""
    out = {}
    for name, t in mc.texts().items():
        bs = mc.batches(t)
        for b in BATCHES:
            if b in bs:
                out["%s/%s" % (name, b)] = (t, bs[b])
    for name, (t, docs) in _special().items():
        out[name] = (np.array(t, np.int32), docs)
    return out


# ---- model A -----------------------------------------------------------------------------------------------------------------

def _span(tl, sl, p):
    """(first, count, ended) of the pattern p (a list) by bisection over the suffix array with list comparison"""
    n, m = len(tl), len(p)
    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) // 2
        if tl[sl[mid]:sl[mid] + m] < p:
            lo = mid + 1
        else:
            hi = mid
    first, hi = lo, n
    while lo < hi:
        mid = (lo + hi) // 2
        if tl[sl[mid]:sl[mid] + m] <= p:
            lo = mid + 1
        else:
            hi = mid
    count = lo - first
    return first, count, int(count > 0 and sl[first] + m == n)


def _narrow(tl, sl, first, count, ended, L, v):
    """(first, count) of the ranks of a context's range whose next symbol is v: the ended suffix stands first and has none"""
    lo, hi = first + ended, first + count
    a, b = lo, hi
    while a < b:
        mid = (a + b) // 2
        if tl[sl[mid] + L] < v:
            a = mid + 1
        else:
            b = mid
    f, b = a, hi
    while a < b:
        mid = (a + b) // 2
        if tl[sl[mid] + L] <= v:
            a = mid + 1
        else:
            b = mid
    return f, a - f


def score_a(tl, sl, docs, max_length, ms=None):
    """(uint32[total, 4] = (length, context_count, token_count, first), trace int64[total, 3] = (L found by fact 1, Lmax, offset
    inside the document)).  ms: the matching statistics of the batch under the same cap (None: way 2, the bisection over L alone)"""
    n = len(tl)
    rows, trace, base = [], [], 0
    for doc in docs:
        for k in range(len(doc)):
            j = base + k
            if n == 0:
                rows.append((0, 0, 0, 0))
                trace.append((0, 0, k))
                continue
            lmax = min(k, max_length or k, n)
            found = hi = lmax
            best = (0, n, 0)                                        # the span of the empty context
            lo = 0
            if ms is not None and lmax:
                a, b = j - lmax, j                                  # the smallest start whose match reaches j
                while a < b:
                    i = (a + b) // 2
                    if i + int(ms[i]) >= j:
                        b = i
                    else:
                        a = i + 1
                found = hi = j - b
                if hi:
                    s = _span(tl, sl, doc[k - hi:k])
                    if s[1] - s[2] > 0:
                        lo, best = hi, s
                    else:
                        hi -= 1                                     # the corpus's tail and nothing else
            while lo < hi:
                L = lo + (hi - lo + 1) // 2
                s = _span(tl, sl, doc[k - L:k])
                if s[1] - s[2] > 0:
                    lo, best = L, s
                else:
                    hi = L - 1
            f, c = _narrow(tl, sl, best[0], best[1], best[2], lo, doc[k])
            rows.append((lo, best[1] - best[2], c, f))
            trace.append((found, lmax, k))
        base += len(doc)
    return np.array(rows, np.uint32).reshape(-1, 4), np.array(trace, np.int64).reshape(-1, 3)


# ---- model B -----------------------------------------------------------------------------------------------------------------

def _score_b(tt, ctx, v):
    n = tt.size
    if n == 0:
        return 0, 0, 0
    S, L = np.arange(n, dtype=np.int64), 0                          # the text positions behind an occurrence of the last L symbols
    m = len(ctx)
    while L < m:
        nx = S[S - L - 1 >= 0]
        nx = nx[tt[nx - L - 1] == ctx[m - 1 - L]]
        if nx.size == 0:
            break
        S, L = nx, L + 1
        if S.size == 1:                                             # one occurrence left: compare on to the left
            e = int(S[0])
            k = min(m - L, e - L)
            seg = tt[e - L - k:e - L][::-1]
            want = np.asarray(ctx[m - L - k:m - L], np.int64)[::-1]
            diff = np.flatnonzero(seg != want)
            L += int(diff[0]) if diff.size else k
            break
    return L, int(S.size), int((tt[S] == v).sum())


def score_b(t, docs, max_length):
    """int64[total, 3]: (length, context_count, token_count) of every position"""
    tt = np.asarray(t, np.int64)
    rows, memo = [], {}
    for doc in docs:
        for k in range(len(doc)):
            key = tuple(doc[k - min(k, max_length or k):k + 1])
            if key not in memo:
                memo[key] = _score_b(tt, key[:-1], key[-1])
            rows.append(memo[key])
    return np.array(rows, np.int64).reshape(-1, 3)


def heads_of(scores, docs):
    """uint64[Q, 5]: (scored, seen, certain, longest, length_sum) of every document, a NumPy reduction of uint32[total, 4] records"""
    out, base = np.zeros((len(docs), 5), np.uint64), 0
    for d, doc in enumerate(docs):
        r = scores[base:base + len(doc)].astype(np.uint64)
        if len(doc):
            out[d] = (len(doc), (r[:, 2] > 0).sum(), (r[:, 2] == r[:, 1]).sum(), r[:, 0].max(), r[:, 0].sum())
        base += len(doc)
    return out


# ---- shared, computed once per process ---------------------------------------------------------------------------------------

_CASES = None
_SA = {}
_CACHE = {}
_CACHE_B = {}


def case(name):
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES[name]


def names():
    case("equal20")
    return list(_CASES)


def expected(name):
    """{"t", "sa", "docs", "ms": {M: uint32[total, 4] matches}, "scores": {M: uint32[total, 4]}, "trace": {M: int64[total, 3]}}: model A"""
    if name not in _CACHE:
        t, docs = case(name)
        key = t.tobytes()
        if key not in _SA:
            _SA[key] = model_sa(t).astype(np.int32)
        sa = _SA[key]
        tl, sl = [int(v) for v in t], [int(v) for v in sa]
        e = {"t": t, "sa": sa, "docs": docs, "ms": {}, "scores": {}, "trace": {}}
        for M in MAX_LENGTHS:
            e["ms"][M] = mc.spans_a(tl, sl, docs, M)
            e["scores"][M], e["trace"][M] = score_a(tl, sl, docs, M, e["ms"][M][:, 2])
        _CACHE[name] = e
    return _CACHE[name]


def expected_b(name):
    """{M: int64[total, 3]}: model B"""
    if name not in _CACHE_B:
        t, docs = case(name)
        _CACHE_B[name] = {M: score_b(t, docs, M) for M in MAX_LENGTHS}
    return _CACHE_B[name]
