"""Texts, query batches and the two CPU models of the matching-statistics tests (test_token_match_cpu.py, test_gpu_token_match.py).

A batch is a list of query documents; a position is a flat index into the packed batch.  The match of a position is (first, count,
length, ended) of the longest prefix of what follows in its document (at most max_length symbols, 0: no cap) that the text holds,
as include/sa_hip.h section 6f defines it; the head of a document is (written, maximal, longest, covered).
  model A  from the model suffix array, as the device does it: one bisection for the capped prefix (token_cases.model_a), the two
           neighbour LCPs for a miss, a second bisection for the matched prefix; maximal matches by the predecessor rule
           end(j) > end(j - 1), coverage by the sum of end(j) - max(j, E(j));
  model B  no suffix array and no neighbour argument: the set of text positions at which the prefix occurs, filtered symbol by
           symbol until it is empty (a set of one position is followed by direct comparison); maximal matches from the definition
           ("contained in no other position's match"), coverage from the union of the matches.
The texts are the kinds of token_next_cases.texts(), cut to TEXT_CAP tokens: model B costs the sum of its set sizes.
"""
import numpy as np

import token_cases as tc
import token_next_cases as nc
from test_int_cpu import model_sa

I32_MAX = 2 ** 31 - 1
TEXT_CAP = 2000
BODY_CAP = 300                                 # of a text of few distinct bigrams the last BODY_CAP tokens stand in for the whole
FEW_BIGRAMS = 20                               # ... all-equal, period 2, random over 2 symbols, planted: long repeats
NONE = -1                                      # a token that occurs in no text (text symbols are >= 0)

TEXTS = ("n0", "n1", "n2", "all_equal", "period2", "rand_k2", "rand_k1000", "zero_and_max", "planted")
MAX_LENGTHS = (0, 1, 2, 3, 7)                  # straddle the two symbols a key holds
MIN_LENGTHS = (1, 2, 8)
DOC_SIZES = (1, 63, 64, 65, 127, 128, 129)     # the docs kernel's window edges
PLANT_AT, PLANT_LEN = 60, 130                  # a copied window that starts in window 0 of its document and covers windows 1 and 2

PLANS = tc.PLANS                               # default, no_keys, no_dir (SA_HIP_TOKEN_DIR=0), text_only
set_plan = tc.set_plan


def texts():
    c = nc.texts()
    return {k: c[k][:TEXT_CAP].copy() for k in TEXTS}


def _piece(tl, rng, size):
    """a document of exactly `size` tokens: windows of the text of 1 .. 40 tokens, each joined to the next by NONE"""
    n, out = len(tl), []
    while len(out) < size:
        if n == 0:
            out.append(int(rng.integers(-1, 3)))
            continue
        p, m = int(rng.integers(0, n)), int(rng.integers(1, 41))
        out += tl[p:p + m] + [NONE]
    return out[:size]


def batches(t, seed=5):
    """the query batches of one text: {name: list of documents (lists of Python ints within int32)}"""
    rng = np.random.default_rng(seed)
    tl = [int(v) for v in t]
    n = len(tl)
    mn, mx = (min(tl), max(tl)) if n else (0, 0)
    out = {}
    starts = ([0, max(n - 70, 0)] + [int(p) for p in rng.integers(0, n, 4)]) if n else []
    # windows of 1, 2, 3, 8 and 64 tokens, each joined to the next by a token that does not occur: one document per width
    wins = []
    for m in (1, 2, 3, 8, 64):
        doc = []
        for p in starts:
            doc += tl[p:p + m] + [NONE]
        wins.append(doc or [NONE])
    out["windows"] = wins
    # the text's tail with one token more: the comparison runs off the text's end
    out["tails"] = [tl[max(n - m, 0):] + [mn] for m in (1, 2, 3, 8, 64)] + [tl[max(n - 8, 0):] + [NONE, mx]]
    # the whole text, and with one token more (a text that repeats itself: its last BODY_CAP tokens)
    body = tl if len(set(zip(tl, tl[1:]))) > FEW_BIGRAMS else tl[-BODY_CAP:]
    out["whole"] = [body, body + [mn], body + [mx]]
    # tokens below min, above max, negative and INT32_MAX, alone and between tokens of the text
    odd = [v for v in (mn - 1, mx + 1, -5, tc.I32_MIN, I32_MAX) if tc.I32_MIN <= v <= I32_MAX]
    mixed = []
    for k, v in enumerate(odd):
        mixed += tl[k:k + 3] + [v] + tl[:2]
    out["odd_tokens"] = [[v] for v in odd] + [mixed, odd + odd]
    # an empty document at the front, in the middle and at the end
    out["empty_docs"] = [[], _piece(tl, rng, 5), [], [], _piece(tl, rng, 70), []]
    out["all_empty"] = [[], [], []]
    # the window edges of the docs kernel
    out["doc_sizes"] = [_piece(tl, rng, s) for s in DOC_SIZES]
    # its workgroup edge: 3, 4 and 5 documents
    for q in (3, 4, 5):
        out["q%d" % q] = [_piece(tl, rng, int(s)) for s in rng.integers(1, 40, q)]
    # the match kernel's block edge: flat totals of 255, 256 and 257 positions
    for total in (255, 256, 257):
        out["total%d" % total] = [_piece(tl, rng, 100), _piece(tl, rng, 100), _piece(tl, rng, total - 200)]
    # a copied window whose match starts in one window of its document and covers the next two: the carried values decide
    if n >= PLANT_LEN:
        p = int(rng.integers(0, n - PLANT_LEN + 1))
        out["carried"] = [[NONE] * 3, [NONE] * PLANT_AT + tl[p:p + PLANT_LEN] + [NONE] * 30, tl[p:p + PLANT_LEN] + [NONE] + tl[p:p + 70]]
    return out


def pack(docs, front=0):
    """(packed int32 with `front` tokens before the first document, uint64 offsets)"""
    buf, off = tc.pack(docs)
    if front:
        buf = np.concatenate([np.full(front, 7, np.int32), buf])
        off = off + np.uint64(front)
    return buf, off


# ---- model A -----------------------------------------------------------------------------------------------------------------

def _lcp(a, b):
    k = 0
    while k < len(a) and k < len(b) and a[k] == b[k]:
        k += 1
    return k


def spans_a(tl, sl, docs, max_length):
    """uint32[total, 4]: (first, count, length, ended) of every position"""
    n = len(tl)
    pref = []
    for doc in docs:
        for j in range(len(doc)):
            pref.append(doc[j:j + min(len(doc) - j, max_length or len(doc), n)])
    if n == 0 or not pref:
        return np.zeros((len(pref), 4), np.uint32)
    first, count = tc.model_a(tl, sl, pref)
    length = []
    for P, r, c in zip(pref, first.tolist(), count.tolist()):
        if c:
            length.append(len(P))
        else:
            below = _lcp(tl[sl[r - 1]:sl[r - 1] + len(P)], P) if r > 0 else 0
            above = _lcp(tl[sl[r]:sl[r] + len(P)], P) if r < n else 0
            length.append(max(below, above))
    first, count = tc.model_a(tl, sl, [P[:L] for P, L in zip(pref, length)])
    return np.array([(f, c, L, int(c > 0 and sl[f] + L == n)) for f, c, L in zip(first.tolist(), count.tolist(), length)],
                    np.uint32).reshape(-1, 4)


def heads_a(lengths, docs, min_length):
    """per document: ([(offset inside the document, flat position)] of the maximal matches of >= min_length, (maximal, longest,
    covered)), by the predecessor rule and the sum of end(j) - max(j, E(j))"""
    out, base = [], 0
    for doc in docs:
        prev_end, E, covered, longest, found = base, 0, 0, 0, []
        for j in range(base, base + len(doc)):
            L = int(lengths[j])
            end = j + L
            if L >= max(min_length, 1) and end > prev_end:
                found.append((j - base, j))
            if L >= min_length:
                covered += max(end - max(j, E), 0)
                E = max(E, end)
            longest = max(longest, L)
            prev_end = end
        out.append((found, (len(found), longest, covered)))
        base += len(doc)
    return out


# ---- model B -----------------------------------------------------------------------------------------------------------------

def match_b(tt, P):
    """(count, length, ended) of the longest prefix of P that occurs in tt"""
    n = tt.size
    if n == 0:
        return 0, 0, 0
    S, L = np.arange(n, dtype=np.int64), 0                         # the text positions at which P[:L] occurs
    while L < len(P):
        nx = S[S + L < n]
        nx = nx[tt[nx + L] == P[L]]
        if nx.size == 0:
            break
        S, L = nx, L + 1
        if S.size == 1:                                            # one occurrence left: compare on
            e = int(S[0])
            rest = np.asarray(P[L:n - e], np.int64)
            diff = np.flatnonzero(tt[e + L:e + L + rest.size] != rest)
            L += int(diff[0]) if diff.size else rest.size
            break
    return (int(S.size), L, int((S + L == n).any())) if L else (n, 0, 0)


def spans_b(t, docs, max_length):
    """int64[total, 3]: (count, length, ended) of every position"""
    tt = np.asarray(t, np.int64)
    rows, memo = [], {}
    for doc in docs:
        for j in range(len(doc)):
            P = tuple(doc[j:j + (max_length or len(doc))])
            if P not in memo:
                memo[P] = match_b(tt, P)
            rows.append(memo[P])
    return np.array(rows, np.int64).reshape(-1, 3)


def heads_b(lengths, docs, min_length):
    """as heads_a, from the definitions: a match is maximal when no other position's match of the document contains it; covered
    is the size of the union of the matches of >= min_length"""
    out, base = [], 0
    for doc in docs:
        m = len(doc)
        L = np.asarray(lengths[base:base + m], np.int64)
        beg = np.arange(m, dtype=np.int64)
        end = beg + L
        inside = (beg[None, :] <= beg[:, None]) & (end[None, :] >= end[:, None]) & (beg[None, :] != beg[:, None])   # [j, i]: i's holds j's
        found = [(int(j), base + int(j)) for j in np.flatnonzero((L >= max(min_length, 1)) & ~inside.any(axis=1))]
        mark = np.zeros(m + 1, np.int64)
        for j in np.flatnonzero(L >= min_length):
            mark[j] += 1
            mark[end[j]] -= 1
        covered = int((np.cumsum(mark)[:m] > 0).sum())
        out.append((found, (len(found), int(L.max()) if m else 0, covered)))
        base += m
    return out


# ---- shared, computed once per process ---------------------------------------------------------------------------------------

_CACHE = {}


def expected(name):
    """{"t", "sa", "batches": {batch: docs}, "spans": {(batch, max_length): uint32[total, 4]}} of one text: model A"""
    if name not in _CACHE:
        t = texts()[name]
        sa = model_sa(t).astype(np.int32)
        tl, sl = [int(v) for v in t], [int(v) for v in sa]
        bs = batches(t)
        spans = {(b, M): spans_a(tl, sl, docs, M) for b, docs in bs.items() for M in MAX_LENGTHS}
        _CACHE[name] = {"t": t, "sa": sa, "batches": bs, "spans": spans}
    return _CACHE[name]


_CACHE_B = {}


def expected_b(name):
    """{(batch, max_length): int64[total, 3]} of one text: model B"""
    if name not in _CACHE_B:
        e = expected(name)
        _CACHE_B[name] = {(b, M): spans_b(e["t"], docs, M) for b, docs in e["batches"].items() for M in MAX_LENGTHS}
    return _CACHE_B[name]


def rows(found, heads, spans, cap, fill):
    """what a docs launch with `cap` writes: positions uint32[Q, cap], out_spans uint32[Q, cap, 4] (cells beyond written keep the
    fill), heads uint32[Q, 4]"""
    q = len(heads)
    pos = np.full((q, cap), fill & 0xFFFFFFFF, np.uint32)
    outs = np.full((q, cap, 4), fill & 0xFFFFFFFF, np.uint32)
    hd = np.zeros((q, 4), np.uint32)
    for d, (f, (maximal, longest, covered)) in enumerate(zip(found, heads)):
        w = min(len(f), cap)
        for k in range(w):
            pos[d, k] = f[k][0]
            outs[d, k] = spans[f[k][1]]
        hd[d] = (w, maximal, longest, covered)
    return pos, outs, hd
