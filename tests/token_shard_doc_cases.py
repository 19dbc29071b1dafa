"""Shard sets with documents, and the two CPU models of the set's document calls (test_token_shard_docs_cpu.py,
test_gpu_token_shard_docs.py).  include/sa_hip.h section 6g.

A set is a list of shards, each a case of token_doc_cases: {"t", "sa", "starts", "da", "pv"}.  A document lives in one shard; with
D_s = len(starts_s), empty documents included, base[0] = 0 and base[s + 1] = base[s] + D_s, and document d of shard s has the global
id base[s] + d.  The hits of a context are the concatenation of the shards' rank ranges in shard order.
  model A  per shard token_doc_cases.model_da_pv, docs_a and locate_a on a model suffix array, combined in Python ints: shard s
           examines e_s = clamp(budget - sum of the counts in front, 0, c_s) ranks, the lists follow one another with the bases
           added, the concatenation is cut at cap;
  model B  no suffix array: a window scan of every shard's text (token_doc_cases.occurrences, doc_of) gives the hits and the set of
           (shard, document) pairs, comparable when examined == count.
The planted sets are all-equal texts of different lengths cut every Ld tokens, whose spans are given by hand so that every shard's
count sits on an edge of the walk (token_doc_cases.COUNTS).
"""
import numpy as np

import token_cases as tc
import token_doc_cases as td
from test_int_cpu import model_sa

FILL = td.FILL                                   # cells a launch must not write keep it
FILL64 = FILL & 0xFFFFFFFFFFFFFFFF               # ... in the uint64 document lists
A = td.A
MOST = 1 << 30                                   # "no cap" of the models


def shard_case(t, starts):
    t = np.asarray(t, np.int32)
    sa = model_sa(t).astype(np.int32)
    starts = np.asarray(starts, np.int32)
    da, pv = td.model_da_pv(sa, starts)
    return {"t": t, "sa": sa, "starts": starts, "da": da, "pv": pv}


def bases(cases):
    out = [0]
    for c in cases:
        out.append(out[-1] + len(c["starts"]))
    return out


def spans_of(cases, pats):
    """[S][Q] (first, count) of whole patterns by token_cases.model_a"""
    out = []
    for c in cases:
        first, count = tc.model_a(c["t"], c["sa"], pats)
        out.append([(int(f), int(k)) for f, k in zip(first, count)])
    return out


# ---- model A -------------------------------------------------------------------------------------------------------------------

def split_budget(counts, budget):
    """e_s of every shard: the ranks it examines when `budget` ranks are taken from the front of the concatenation (0: all)"""
    out, run = [], 0
    for c in counts:
        out.append(c if not budget else max(0, min(c, budget - run)))
        run += c
    return out


def docs_set(cases, spans_i, cap, budget):
    """spans_i: the S (first, count) of one context.  -> (head (written, examined, distinct, count), [(global doc, offset)])"""
    base = bases(cases)
    counts = [c for _, c in spans_i]
    entries, examined, distinct = [], 0, 0
    for s, (c, (f, _), e) in enumerate(zip(cases, spans_i, split_budget(counts, budget))):
        memo = c.setdefault("_docs_a", {})                                     # (most budgets leave a shard all of its span, or nothing)
        if (f, e) not in memo:
            memo[(f, e)] = td.docs_a(c["sa"], c["da"], c["starts"], f, e, MOST, 0)  # the first e ranks of the shard's span, all of them
        head, ent = memo[(f, e)]
        examined += head[1]
        distinct += head[2]
        entries += [(base[s] + d, o) for d, o in ent]
    return (min(distinct, cap), examined, distinct, sum(counts)), entries[:cap]


def locate_set(cases, spans_i, cap):
    base = bases(cases)
    total = sum(c for _, c in spans_i)
    entries = []
    for s, (c, (f, k)) in enumerate(zip(cases, spans_i)):
        if len(entries) >= cap:
            break
        _, ent = td.locate_a(c["sa"], c["da"], c["starts"], f, k, cap - len(entries))
        entries += [(base[s] + d, o) for d, o in ent]
    return (min(total, cap), total), entries


def context(spans, i):
    return [spans[s][i] for s in range(len(spans))]


def _arrays(ent):
    return np.array([d for d, _ in ent], np.uint64), np.array([o for _, o in ent], np.int32)


def docs_full(cases, spans, budget):
    """docs_set of every context without a cap, the entries as (uint64 documents, int32 offsets): what docs_rows cuts to any cap"""
    out = []
    for i in range(len(spans[0])):
        head, ent = docs_set(cases, context(spans, i), MOST, budget)
        out.append((head,) + _arrays(ent))
    return out


def locate_full(cases, spans):
    out = []
    for i in range(len(spans[0])):
        head, ent = locate_set(cases, context(spans, i), MOST)
        out.append(((0, head[1], head[1], head[1]),) + _arrays(ent))     # shaped as docs_full: "distinct" = the hits
    return out


def docs_rows(full, cap):
    """what a documents call with `cap` writes: docs uint64[Q, cap] (FILL64 beyond written), offsets int32[Q, cap] (FILL), and the
    heads as (written, examined, distinct, count) tuples"""
    q = len(full)
    docs, offs, heads = np.full((q, cap), FILL64, np.uint64), np.full((q, cap), FILL, np.int32), []
    for i, (head, ed, eo) in enumerate(full):
        w = min(head[2], cap)
        heads.append((w, head[1], head[2], head[3]))
        docs[i, :w], offs[i, :w] = ed[:w], eo[:w]
    return docs, offs, heads


def locate_rows(full, cap):
    """what a locate call with `cap` writes, from locate_full: docs, offsets, and the heads as (written, count) tuples"""
    docs, offs, heads = docs_rows(full, cap)
    return docs, offs, [(h[0], h[3]) for h in heads]


# ---- model B -------------------------------------------------------------------------------------------------------------------

def model_b(cases, p):
    """-> (count, distinct documents, sorted [(global doc, offset)] of all hits) of one pattern over the set"""
    base = bases(cases)
    count, pairs, hits = 0, set(), []
    for s, c in enumerate(cases):
        pos = td.occurrences(c["t"], p)
        d = td.doc_of(c["starts"], pos)
        st = np.asarray(c["starts"], np.int64)
        count += int(pos.size)
        pairs |= {(s, int(x)) for x in d.tolist()}
        hits += [(base[s] + int(x), int(o)) for x, o in zip(d.tolist(), (pos - st[d]).tolist())]
    return count, len(pairs), sorted(hits)


# ---- the planted sets: all-equal shards of different lengths, spans by hand ----------------------------------------------------

EQ_N = (td.N_EQ, 1100, 1300)                     # every shard holds the largest of COUNTS


def equal_set(Ld):
    """three all-equal shards cut every Ld tokens; SA[r] = n - 1 - r in each (token_doc_cases)"""
    key = ("eq", Ld)
    if key not in _CACHE:
        cases = []
        for n in EQ_N:
            sa, starts = (n - 1 - np.arange(n)).astype(np.int32), np.arange(0, n, Ld, dtype=np.int32)
            da, pv = td.model_da_pv(sa, starts)
            cases.append({"t": np.full(n, A, np.int32), "sa": sa, "starts": starts, "da": da, "pv": pv})
        _CACHE[key] = cases
    return _CACHE[key]


def _first(n, c, kind):
    """where a span of c ranks starts: at rank 0, ending at rank n, or inside a document's run of ranks"""
    return (0, n - c, (n - c) // 2 + 1 if n - c > 2 else 0)[kind % 3]


def equal_contexts():
    """[S][Q] (first, count): every count of COUNTS in every shard, beside different counts in the others; a middle shard that
    misses; a context nobody holds; a context only the last shard holds; one shard alone beyond every cap; equal counts"""
    K = td.COUNTS
    triples = [(c, K[(k + 5) % len(K)], K[(k + 9) % len(K)]) for k, c in enumerate(K)]
    triples += [(257, 0, 129), (0, 0, 0), (0, 0, 65), (1025, 0, 0), (64, 64, 64), (1, 1, 1), (256, 256, 256)]
    spans = [[], [], []]
    for i, tr in enumerate(triples):
        for s, c in enumerate(tr):
            spans[s].append((_first(EQ_N[s], c, i + s), c))
    return spans


def counts_of(spans, i):
    return [spans[s][i][1] for s in range(len(spans))]


def budget_edges(counts):
    """0, the sums of the counts in front of every shard - 1, at them and one above, inside every span, at C and beyond"""
    out, run = {0}, 0
    for c in counts:
        out |= {run - 1, run, run + 1, run + c // 2}
        run += c
    out |= {run - 1, run, run + 1, run + 1000}
    return sorted(b for b in out if b >= 0)


def cap_edges(distincts):
    """token_doc_cases.CAPS, and the sums of the shards' distinct documents - 1, at them and one above (the last sum: the cap that
    is reached exactly at the last shard)"""
    out, run = set(td.CAPS), 0
    for d in distincts:
        run += d
        out |= {run - 1, run, run + 1}
    return sorted(c for c in out if c >= 0)


def all_budgets(spans):
    out = set()
    for i in range(len(spans[0])):
        out |= set(budget_edges(counts_of(spans, i)))
    return sorted(out)


# ---- the random sets: texts of token_cases cut into shards, random tables ------------------------------------------------------

RANDOM = {                                       # name -> (text of token_cases, shard lengths, documents per shard, empty ones appended)
    "r2": ("rand_k2", (3000, 1900), (40, 7), (2, 0)),
    "r3": ("rand_k1000", (2500, 700, 2000), (300, 1, 64), (0, 3, 1)),
}


def random_set(name):
    if name not in _CACHE:
        text, lens, Ds, empties = RANDOM[name]
        t = tc.texts()[text]
        cases, at = [], 0
        for s, (n, D, e) in enumerate(zip(lens, Ds, empties)):
            starts = np.concatenate([td.rand_table(n, D, 50 + s), np.full(e, n, np.int32)])        # empty documents at the end: start == n
            cases.append(shard_case(t[at:at + n], starts))
            at += n
        _CACHE[name] = cases
    return _CACHE[name]


def random_patterns(cases, seed=23):
    """windows of every shard (so some shards miss them), their neighbours, the empty pattern, symbols nobody holds"""
    rng = np.random.default_rng(seed)
    pats = [[], [-1], [2 ** 31 - 1], [5, 6, 5, 6, 5, 6, 5]]
    for c in cases:
        tl = c["t"].tolist()
        n = len(tl)
        for m in (1, 2, 3, 8, 16):
            for p in [0, n - m] + [int(x) for x in rng.integers(0, n - m, 4)]:
                w = tl[p:p + m]
                pats += [w, w[:-1] + [w[-1] + 1]]
        pats.append(tl[-3:] + [tl[0]])           # runs over the cut into nothing: an n-gram never spans two shards
    return pats


def random_contexts(cases, seed=31):
    """contexts for the longest-suffix mode: a window with a foreign symbol in front, so the longest suffix is the window"""
    rng = np.random.default_rng(seed)
    ctx = []
    for c in cases:
        tl = c["t"].tolist()
        n = len(tl)
        for m in (1, 2, 5):
            for p in [int(x) for x in rng.integers(0, n - m, 3)]:
                ctx += [[-9] + tl[p:p + m], tl[p:p + m] + [-9], tl[p:p + m]]
    return ctx


_CACHE = {}
