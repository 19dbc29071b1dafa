"""Tables, case lists and the two CPU models of the CNF document query tests (test_token_cnf_cpu.py, test_gpu_token_cnf.py).

A group (one query) is (clauses, neg): clauses a list of clauses, a clause a list of literals (first, count) -- rank ranges, as the
device form takes them -- and neg one 0 / 1 per clause (include/sa_hip.h section 6m).
  model A  from a model suffix array: the driver by the rule (smallest 64-bit sum over the positive clauses, lowest index on a tie);
           the walk literal by literal, first occurrences by PV[r] < a_l, duplicates and probes by lower bounds in the segments of
           RK; the budget cuts the walk by its position in walk order; the head tuple.
  model B  no suffix array: per literal the set of documents from a window scan of the text (token_doc_cases.occurrences), a clause
           the union of its literals' sets, a query the intersection of its positive clauses minus the union of its negated ones.
"""
import numpy as np

import token_all_cases as ac
import token_cases as tc
import token_doc_cases as dc

FILL = dc.FILL
MAX_CLAUSES = 16                                # SA_HIP_TOKEN_CNF_MAX_CLAUSES
MAX_LITERALS = 64                               # SA_HIP_TOKEN_CNF_MAX_LITERALS
N_EQ = dc.N_EQ
HEAD = ("written", "matched", "candidates", "duplicates", "driver", "literals", "examined", "count")


# ---- tables --------------------------------------------------------------------------------------------------------------------

def tables(groups):
    """-> (flat literals, clause_offsets uint64[C + 1], negated uint8[C], group_offsets uint64[G + 1])"""
    flat, coff, neg, goff = [], [0], [], [0]
    for clauses, ng in groups:
        assert len(clauses) == len(ng)
        for c in clauses:
            flat += list(c)
            coff.append(len(flat))
        neg += [int(x) for x in ng]
        goff.append(len(neg))
    return flat, np.array(coff, np.uint64), np.array(neg, np.uint8), np.array(goff, np.uint64)


def positive(clauses):
    """the group of these clauses with none negated"""
    return [list(c) for c in clauses], [0] * len(clauses)


# ---- model A -------------------------------------------------------------------------------------------------------------------

def holds(rk, cl, d, a, end):
    """document d has a rank in [a, end): the lower bound of a in its segment lands inside it on a value < end"""
    seg = rk[cl[d]:cl[d + 1]]
    i = int(np.searchsorted(seg, a, "left"))
    return i < seg.size and int(seg[i]) < end


def driver_of(sums, neg):
    """the positive clause with the smallest sum (Python integers: no width), the lowest index on a tie"""
    return min((j for j in range(len(sums)) if not neg[j]), key=lambda j: (sums[j], j))


def cnf_walk(sa, da, pv, rk, cl, n, group):
    """-> (driver, its literals, its sum, [(position in walk order, rank, doc, offset, kind)] of every first occurrence of the whole
    walk; kind 0: a duplicate, 1: a candidate that does not match, 2: a match)"""
    clauses, neg = group
    cs = [[ac.clamp(n, f, c) for f, c in cla] for cla in clauses]
    sums = [sum(e - a for a, e in c) for c in cs]
    drv = driver_of(sums, neg)
    events, base = [], 0
    for li, (a, e) in enumerate(cs[drv]):
        for r in (np.flatnonzero(pv[a:e] < a) + a).tolist():
            d = int(da[r])
            if any(holds(rk, cl, d, *cs[drv][k]) for k in range(li)):
                kind = 0
            else:
                ok = all(any(holds(rk, cl, d, x, y) for x, y in cs[j]) != bool(neg[j]) for j in range(len(cs)) if j != drv)
                kind = 2 if ok else 1
            events.append((base + r - a, r, d, int(sa[r]) - int(cl[d]), kind))
        base += e - a
    return drv, len(cs[drv]), sums[drv], events


def cnf_a(walk, budget, most=64):
    """-> (head as HEAD, [(doc, offset)] of the first `most` matches)"""
    drv, lits, count, events = walk
    examined = min(count, budget) if budget else count
    seen = [x for x in events if x[0] < examined]
    matched = sum(1 for x in seen if x[4] == 2)
    ent = [(x[2], x[3]) for x in seen if x[4] == 2][:most]
    return (min(matched, most), matched, sum(1 for x in seen if x[4]), sum(1 for x in seen if x[4] == 0), drv, lits, examined, count), ent


def cnf_rows(full, cap):
    """what a cnf launch with `cap` writes: docs[G, cap], offsets[G, cap] (FILL beyond written), heads uint32[G, 12] (the 48 bytes of
    sa_hip_token_cnf as words: six uint32, then examined, count and reserved as low and high words)"""
    g = len(full)
    docs, offs, heads = np.full((g, cap), FILL, np.int32), np.full((g, cap), FILL, np.int32), np.zeros((g, 12), np.uint32)
    for i, (head, ent) in enumerate(full):
        heads[i, :6] = (min(head[1], cap),) + tuple(head[1:6])
        for k, v in ((6, head[6]), (8, head[7])):
            heads[i, k], heads[i, k + 1] = v & 0xFFFFFFFF, v >> 32
        for j, (d, o) in enumerate(ent[:cap]):
            docs[i, j], offs[i, j] = d, o
    return docs, offs, heads


# ---- model B -------------------------------------------------------------------------------------------------------------------

def cnf_b(t, starts, clauses, neg):
    """clauses of PATTERNS -> (sorted matching documents, occurrences per clause)"""
    sets, sums = [], []
    for cla in clauses:
        pos = [dc.occurrences(t, p) for p in cla]
        sets.append(set().union(*[set(dc.doc_of(starts, p).tolist()) for p in pos]))
        sums.append(sum(int(p.size) for p in pos))
    keep = None
    for s, ng in zip(sets, neg):
        if not ng:
            keep = set(s) if keep is None else keep & s
    for s, ng in zip(sets, neg):
        if ng:
            keep -= s
    return sorted(keep), sums


# ---- the all-equal text: de-duplication, budgets, caps, limits -----------------------------------------------------------------
# SA[r] = N_EQ - 1 - r.  Cut every token, document N_EQ - 1 - r owns rank r alone, so a literal holds a document iff it holds its
# rank; cut every 2 tokens, the ranks 2i + 1 and 2i + 2 from the end share a document.

WHOLE = (0, N_EQ)
DEDUP_K1, DEDUP_K2 = 401, 333
DEDUP_OVERLAPS = (0, 1, 63, 64, 65, 255, 256, 257, DEDUP_K2)      # the last one: nested


def dedup_groups():
    """two driver literals [0, k1) and [k1 - o, k1 - o + k2): the second literal's first candidate is its rank number o, so it sits
    at lane o % 64 of window o // 64 of a literal that starts at k1 - o, on no window boundary of the first; alone, beside a larger
    clause that holds everything, and beside one that holds only part; the same literal twice"""
    out = []
    for o in DEDUP_OVERLAPS:
        two = [(0, DEDUP_K1), (DEDUP_K1 - o, DEDUP_K2)]
        out += [positive([two]), positive([two, [WHOLE]]), positive([two, [(350, 900)]]), ([two, [(390, 30)]], [0, 1])]
    out += [positive([[(0, DEDUP_K1), (0, DEDUP_K1)]]), positive([[(5, 70), (5, 70), (5, 70)], [WHOLE]])]
    return out


def budgets_of(group, n=N_EQ):
    """0, and one either side of the first driver literal's count and of the driver's sum"""
    clauses, neg = group
    cs = [[ac.clamp(n, f, c) for f, c in cla] for cla in clauses]
    sums = [sum(e - a for a, e in c) for c in cs]
    drv = driver_of(sums, neg)
    c0 = cs[drv][0][1] - cs[drv][0][0]
    return sorted({0} | {b for b in (c0 - 1, c0, c0 + 1, sums[drv] - 1, sums[drv], sums[drv] + 1) if b > 0})


CAPS = (0, 1, 16)
CAP_MATCHES = ((0, 0), (1, 0), (15, 0), (15, 1), (15, 2))          # matches from the first and from the second driver literal


def cap_groups():
    """driver [0, 15) or [100, 120); the other clause holds m0 ranks of the first and k of the second literal and is larger: 0, 1, 15,
    16 and 17 matches, the 16th and 17th from the second literal"""
    return [positive([[(0, 15), (100, 20)], [(0, m0), (100, k), (600, 800)]]) for m0, k in CAP_MATCHES]


def limit_groups():
    """64 literals in one driver clause (a chain, each overlapping the next by 5 ranks), beside a clause and alone; 64 literals over
    16 clauses; 16 single-literal clauses, the last one the driver, the one before it negated"""
    chain = [(20 * i, 25) for i in range(MAX_LITERALS)]
    wide = [[(10 * j + i, 700) for i in range(4)] for j in range(MAX_CLAUSES - 1)] + [[(300, 9), (305, 9), (400, 9), (300, 9)]]
    single = [[(i, 900)] for i in range(MAX_CLAUSES - 2)] + [[(1000, 100)], [(200, 40)]]
    return [positive([chain]), ([chain[:63], [(700, 100)]], [0, 1]), positive(wide), (single, [0] * (MAX_CLAUSES - 2) + [1, 0])]


# ---- planted literals on a random text: the driver rule and the probes ----------------------------------------------------------

def driver_groups(n):
    big = (0, n)
    return [
        positive([[(100, 5), (200, 5)], [(300, 8)]]),                  # sums 10 against 8: not the clause with the smallest literal
        positive([[(300, 8)], [(100, 5), (200, 5)], [(400, 8)]]),      # ... and a tie of 8 and 8 behind it: the lower index
        positive([[(100, 5)], [(200, 3), (300, 2)]]),                  # a tie of sums
        positive([[(200, 3), (300, 2)], [(100, 5)]]),
        ([[(100, 5)], [(7, 0)]], [0, 1]),                              # a negated clause with sum 0 never drives and excludes nothing
        ([[(7, 0)], [(100, 5)]], [1, 0]),
        ([[(100, 5)], [(200, 2)]], [0, 1]),                            # ... nor one with the smallest nonzero sum
        ([[(200, 2)], [(100, 5)], [(300, 1)]], [1, 0, 1]),
        positive([[(7, 0)]]),                                          # a positive all-empty clause: everything is 0
        positive([[big], [(7, 0), (n + 9, 9)]]),
        ([[big], [(7, 0), (n, 3)], [(100, 5)]], [0, 0, 1]),
        positive([[(7, 0), (100, 5)], [big]]),                         # an empty literal inside a non-empty clause
        positive([[(100, 5), (n + 1, 4), (200, 2)], [big]]),
    ]


def probe_groups(c):
    """From token_all_cases.planted_case: A lists document d; of the four literals B one other rank q of d sits at a - 1, a, end - 1 and
    end, so the middle two hold d.  -> [(group, whether A's document matches)]: a probed clause of 1, 2 and 16 literals that holds d
    only in its first literal, only in its last or in none, positive and negated; a negated clause of several literals; two negated
    clauses; the last document, whose lower bound lands on RK[n]"""
    out = []
    quads = [c["groups"][i:i + 4] for i in range(0, len(c["groups"]), 4)]
    for quad in quads[:6]:
        A = quad[0][0]
        below, at_a, at_last, at_end = (g[1] for g in quad)
        for m in (1, 2, 16):
            fill = [below, at_end] * 8
            for B, hit in ((below, False), (at_a, True), (at_last, True), (at_end, False)):
                for clause in ([B] + fill[:m - 1], fill[:m - 1] + [B]):
                    out.append((positive([[A], clause]), hit))
                    out.append((([[A], clause], [0, 1]), not hit))
            out.append((positive([[A], fill[:m]]), False))
        out.append((([[A], [below, at_a], [at_end]], [0, 1, 1]), False))
        out.append((([[A], [below, at_end], [at_end]], [0, 1, 1]), True))
        out.append((([[A], [at_end], [at_last]], [0, 1, 1]), False))
        out.append((([[A], [at_a, below], [at_end, at_last]], [0, 0, 0]), True))
    (A, B), (A2, B2), (A3, B3) = c["last"]
    out += [(positive([[A], [B]]), False), (([[A], [B]], [0, 1]), True), (positive([[A], [B, (7, 0)]]), False),
            (positive([[A2], [(7, 0), B2]]), True), (([[A2], [B2]], [0, 1]), False), (positive([[A3], [B3]]), False)]
    return out


# ---- random CNF queries over the contexts of a text -----------------------------------------------------------------------------

def random_queries(nctx, seed=11):
    """[(clauses of context indices, neg)]: 1 .. 3 positive clauses of 1, 2 and 4 literals, every second one with an exclusion of 1 or
    2 literals; one of 16 clauses; one of 64 literals"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(48):
        clauses = [rng.integers(0, nctx, int(rng.choice((1, 2, 4)))).tolist() for _ in range(1 + k % 3)]
        neg = [0] * len(clauses)
        if k % 2:
            clauses.append(rng.integers(0, nctx, 1 + k % 4 // 2).tolist())
            neg.append(1)
        out.append((clauses, neg))
    out.append(([[int(i)] for i in rng.integers(0, nctx, MAX_CLAUSES)], [0] * (MAX_CLAUSES - 1) + [1]))
    out.append(([rng.integers(0, nctx, 60).tolist(), rng.integers(0, nctx, 4).tolist()], [0, 0]))
    out.append(([[3, 3], [3]], [0, 0]))
    return out


def planted_case():
    """token_all_cases.planted_case (its PV is there already)"""
    return ac.planted_case()


def equal_case(Ld):
    """token_doc_cases.equal_case plus RK and the closed table"""
    c = dict(dc.equal_case(Ld))
    c["rk"], c["cl"] = ac.model_rk(c["da"]), ac.closed(c["starts"], N_EQ)
    return c


def walk_of(c, group):
    return cnf_walk(c["sa"], c["da"], c["pv"], c["rk"], c["cl"], c["sa"].size, group)
