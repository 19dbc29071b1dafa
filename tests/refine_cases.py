"""Generator and model of the refinement tests of the 32-bit build (tests/test_gpu_refine.py); plain NumPy, no GPU.

What the initial sort leaves tied goes through the tiny-group finisher (csrc/sa_build.hpp: tiny_groups_kernel), the group
finisher in LDS (csrc/group_finish.hpp), the rounds sorted tile-wise in LDS (csrc/round_sort.hpp) and the periodic-run shortcut
(csrc/period_finish.hpp).  Every stage has a fallback, so the final array cannot show a stage that quietly does less; the
counts of BuildStats can.  This module builds texts whose tied groups have exact sizes and exact depths (planted_groups),
reads the groups off a checked suffix array (groups_after_keys), restates the tile plan (plan_tiles) and the host loop of
Builder::build (simulate) and so gives the expected counts.  tests/test_refine_cases_cpu.py checks that the case lists hold
what they claim and that the constants below are the headers'.

Representation: the active list after the initial sort is the tied records in suffix-array order.  glue[i] is the number of
symbols beyond the key that records i and i + 1 of that list share (-1: different groups).  At depth key + d the pairs with
glue >= d are still tied; a group is a maximal run of tied pairs.  A stage that resolves a group kills its pairs."""
from collections import namedtuple

import numpy as np

import cases

D1_SYMBOLS = np.concatenate([[10], np.arange(97, 123)]).astype(np.uint8)   # 27 bytes: b = 5, 12 symbols per key
K = 12

# restated from the headers; (file under suffixarray_amd/csrc, regular expression whose group 1 is the value's definition, value)
TINY_MAX, TINY_DEPTH, BLD_TILE = 8, 64, 4096
FIN_CAP, FIN_TILE, FIN_COUNT_MAX, FIN_MAX_ROUNDS, FIN_POS_BITS = 4096, 3584, 96, 24, 12
LOC_CAP, LOC_TILE, LOC_GID_BITS = 4096, 3584, 12
PER_TILE = 4096
CHUNK_ROUNDS_BEFORE_DOUBLING = 2
RADIX_BITS = 8
HEADER_CONSTANTS = [
    ("sa_build.hpp", r"constexpr int TINY_MAX = (\d+);", "8"),
    ("sa_build.hpp", r"constexpr u32 TINY_DEPTH = (\d+);", "64"),
    ("sa_build.hpp", r"constexpr int BLD_BLOCK = (\d+);", "256"),
    ("sa_build.hpp", r"constexpr int BLD_ITEMS = (\d+);", "16"),
    ("sa_build.hpp", r"constexpr int BLD_TILE = (BLD_BLOCK \* BLD_ITEMS);", "BLD_BLOCK * BLD_ITEMS"),
    ("sa_build.hpp", r"int chunk_rounds_before_doubling = (\d+);", "2"),
    ("sa_build.hpp", r"\(u64\)M \* (16) <= n", "16"),
    ("sa_build.hpp", r"period_finish && L == 0 && M >= (64) ", "64"),
    ("group_finish.hpp", r"#define SA_FIN_CAP (\d+)", "4096"),
    ("group_finish.hpp", r"constexpr u32 FIN_TILE = (FIN_CAP - FIN_CAP / 8);", "FIN_CAP - FIN_CAP / 8"),
    ("group_finish.hpp", r"constexpr u32 FIN_COUNT_MAX = (\d+);", "96"),
    ("group_finish.hpp", r"constexpr u32 FIN_MAX_ROUNDS = (\d+);", "24"),
    ("group_finish.hpp", r"if \(kc > (8)\) kc = 8;", "8"),
    ("group_finish.hpp", r"rounds == a.max_rounds \|\| stall >= (2)\)", "2"),
    ("round_sort.hpp", r"#define SA_LOC_BLOCK (\d+)", "256"),
    ("round_sort.hpp", r"constexpr int LOC_ITEMS = (\d+);", "16"),
    ("round_sort.hpp", r"#define SA_LOC_SLACK_DIV (\d+)", "8"),
    ("round_sort.hpp", r"if \(lt.end - a (>) CAP\)", ">"),
    ("period_finish.hpp", r"constexpr int PER_TILE = (\d+);", "4096"),
]
assert BLD_TILE == 256 * 16 and FIN_TILE == FIN_CAP - FIN_CAP // 8 and LOC_CAP == 256 * 16 and LOC_TILE == LOC_CAP - LOC_CAP // 8


def bits_for(count):
    """smallest b with 2^b >= count (csrc/common.hpp: bits_for; group_finish.hpp: fin_bits_for)"""
    return 0 if count <= 1 else int(count - 1).bit_length()


# ---- texts ------------------------------------------------------------------------------------------------------------------

def planted_groups(n, plants, seed, symbols=D1_SYMBOLS, at_end=None):
    """Random text of n symbols with, for every (s, d) or (s, d, cls) of plants, s copies of a fresh random word of d symbols.
    With s <= symbols.size the symbols left and right of the copies of one word are pairwise distinct, so with keys of k
    symbols the plant yields exactly d - k + 1 groups of exactly s records, the group at offset i of the word sharing exactly
    d - k - i symbols beyond the key.  Larger s: random symbols on both sides (they collide: shifted groups of about s / 27,
    s / 729 .. records come with the planted one; the model counts what that gives).
    cls places a word in suffix-array order by its first symbol (symbols ascending): "lo" the lowest third, "hi" the highest
    third, "mid" the middle symbol, which no other word starts with -- and the rest of a "mid" word and the k - 1 symbols to
    the left of its copies are "hi", so that every group derived from a "mid" plant sorts after all "lo" and "mid" groups.
    The copies lie in a random order with random gaps.  at_end: index of a plant whose last copy ends on the text's last
    symbol (nothing follows it: the end is its right guard).  -> (text, [positions of the copies of every plant])"""
    rng = np.random.default_rng(seed)
    symbols = np.asarray(symbols)
    S = symbols.size
    mid = S // 2
    lo_set, hi_set = np.arange(0, max(S // 3, 1)), np.arange(S - max(S // 3, 1), S)
    not_mid = np.concatenate([np.arange(0, mid), np.arange(mid + 1, S)])
    t = symbols[rng.integers(0, S, n)]
    plants = [tuple(p) + (None,) * (3 - len(p)) for p in plants]
    Wl = [K - 1 if p[2] == "mid" else 1 for p in plants]   # guard symbols to the left; one to the right
    assert all(p[0] > S for p in plants if p[2] == "mid")
    copies = [(pi, ci) for pi, (s, d, _) in enumerate(plants) for ci in range(s)]
    last = None
    if at_end is not None:
        last = (at_end, plants[at_end][0] - 1)
        copies.remove(last)
    order = [copies[i] for i in rng.permutation(len(copies))]
    need = sum(plants[pi][1] + Wl[pi] + 1 for pi, _ in order) + (plants[last[0]][1] + Wl[last[0]] if last else 0)
    assert need + 2 <= n, (need, n)
    gaps = rng.multinomial(n - need - 1, np.full(len(order) + 1, 1.0 / (len(order) + 1)))
    words = []
    for s, d, cls in plants:
        w = rng.integers(0, S, d)
        first = {None: not_mid, "lo": lo_set, "hi": hi_set, "mid": np.array([mid])}[cls]
        w[0] = first[rng.integers(0, first.size)]
        if cls == "mid":
            w[1:] = hi_set[rng.integers(0, hi_set.size, d - 1)]
        words.append(symbols[w])
    lg = [rng.permutation(S) for _ in plants]
    rg = [rng.permutation(S) for _ in plants]
    pos = [[0] * p[0] for p in plants]

    def guards(pi, ci, at, right):
        s, d, cls = plants[pi]
        if cls == "mid":   # every key that starts up to K - 1 symbols before the word starts with a "hi" symbol
            t[at - Wl[pi]:at] = symbols[hi_set[rng.integers(0, hi_set.size, Wl[pi])]]
        if s <= S:
            t[at - 1] = symbols[lg[pi][ci]]
            if right:
                t[at + d] = symbols[rg[pi][ci]]
    cur = 0
    for (pi, ci), gap in zip(order, gaps):
        d, W = plants[pi][1], Wl[pi]
        cur += int(gap)
        t[cur + W:cur + W + d] = words[pi]
        guards(pi, ci, cur + W, True)
        pos[pi][ci] = cur + W
        cur += d + W + 1
    if last:
        pi, ci = last
        d, W = plants[pi][1], Wl[pi]
        assert cur <= n - d - W
        t[n - d:] = words[pi]
        guards(pi, ci, n - d, False)
        pos[pi][ci] = n - d
    return np.ascontiguousarray(t), pos


# ---- groups -----------------------------------------------------------------------------------------------------------------

Groups = namedtuple("Groups", "sizes glue apos M G")


def adjacent_lcp(t, sa, cap):
    """min(cap, LCP) of the suffixes in neighbouring slots; the end of the text differs from every symbol"""
    t = np.asarray(t)
    sa = np.asarray(sa).astype(np.int64)
    n = int(t.size)
    tp = np.concatenate([t.astype(np.int32), np.full(cap + 1, -1, np.int32)])
    a, b = sa[:-1], sa[1:]
    lcp = np.zeros(max(n - 1, 0), np.int32)
    live = np.arange(max(n - 1, 0))
    for j in range(cap):
        live = live[tp[a[live] + j] == tp[b[live] + j]]   # (never both past the end: the shorter suffix ends first)
        if live.size == 0:
            break
        lcp[live] += 1
    return lcp


def groups_after_keys(t, sa, k, cap=256):
    """The tied groups a sort by k-symbol keys leaves, read off the suffix array sa of t: sizes in suffix-array order, glue
    (module docstring; capped at cap - k), the slots of the tied records, M records, G groups."""
    lcp = adjacent_lcp(t, sa, max(cap, k))
    same = lcp >= k
    act = np.zeros(len(sa), bool)
    act[:-1] |= same
    act[1:] |= same
    apos = np.flatnonzero(act)
    M = int(apos.size)
    glue = np.where(same[apos[:-1]], lcp[apos[:-1]].astype(np.int64) - k, -1) if M else np.zeros(0, np.int64)
    sizes = group_sizes(glue >= 0, M)[1]
    return Groups(sizes, glue, apos, M, int(sizes.size))


def group_sizes(tied, M):
    """(first record, size) of every maximal run of tied pairs among M records"""
    if M == 0 or not tied.any():
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    x = np.concatenate([[False], tied, [False]])
    d = np.diff(x.astype(np.int8))
    starts = np.flatnonzero(d == 1)
    ends = np.flatnonzero(d == -1)
    return starts.astype(np.int64), (ends - starts + 1).astype(np.int64)


# ---- the tile plan ----------------------------------------------------------------------------------------------------------

Plan = namedtuple("Plan", "tiles inside left")


def plan_tiles(sizes, TILE, CAP):
    """round_sort.hpp: loc_plan_kernel, and the one-tile case of its callers.  The list of sum(sizes) records is cut into
    tiles of whole groups: tile t = the groups that start in [t * TILE, (t + 1) * TILE); a tile longer than CAP leaves out the
    group that straddles (t + 1) * TILE.  A list of at most CAP records is one tile.
    -> tiles int64[T, 3] = (begin, local_end, end), records inside the tiles, records left out"""
    sizes = np.asarray(sizes, np.int64)
    M = int(sizes.sum())
    if M <= CAP:
        return Plan(np.array([[0, M, M]], np.int64), M, 0)
    gstart = np.concatenate([[0], np.cumsum(sizes)])
    nt = -(-M // TILE)
    p = np.arange(nt + 1, dtype=np.int64) * TILE
    g = np.searchsorted(gstart, np.minimum(p, M - 1), side="right") - 1        # the group that holds record p
    ts = np.where(p >= M, M, np.where(gstart[g] == p, p, gstart[g + 1]))
    begin, end = ts[:-1], np.maximum(ts[1:], ts[:-1])
    local_end = np.where(end - begin > CAP, gstart[g[1:]], end)
    tiles = np.stack([begin, local_end, end], axis=1)
    inside = int((local_end - begin).sum())
    return Plan(tiles, inside, int((end - local_end).sum()))


# ---- the stages -------------------------------------------------------------------------------------------------------------

def tiny_pass(glue, tied, limit, truncated):
    """tiny_groups_kernel: a group of at most TINY_MAX records is written when every neighbouring pair of its sorted members
    differs inside the next `limit` bytes (always, with ties in text order, in a truncated build).  -> records resolved; their
    pairs are cleared in tied"""
    starts, sizes = group_sizes(tied, tied.size + 1)
    resolved = 0
    for s, z in zip(starts, sizes):
        if z <= TINY_MAX and (truncated or int(glue[s:s + z - 1].max()) < limit):
            tied[s:s + z - 1] = False
            resolved += int(z)
    return resolved


def finish_tile(g, b, L, h):
    """group_finish_kernel on one tile.  g: glue - (h - key) of the tile's pairs (< 0: not tied).  Rounds of
    kc = min(8, (64 - 12 - bits(groups)) / b) symbols; a round without fewer tied records or more groups is a stall; after two
    stalls in a row or FIN_MAX_ROUNDS rounds every group that still holds a tied pair fails as a whole.
    -> bool per pair: belongs to a failed group"""
    cur = g >= 0
    orig = cur.copy()
    e = rounds = stall = 0
    while True:
        st, sz = group_sizes(cur, cur.size + 1)
        A, G = int(sz.sum()), int(sz.size)
        if A == 0:
            return np.zeros(cur.size, bool)
        if rounds == FIN_MAX_ROUNDS or stall >= 2:
            ost, osz = group_sizes(orig, orig.size + 1)
            failed = np.zeros(cur.size, bool)
            for s, z in zip(ost, osz):
                if cur[s:s + z - 1].any():
                    failed[s:s + z - 1] = True
            return failed
        kc = min(8, (64 - FIN_POS_BITS - bits_for(G)) // b)
        if L:
            kc = min(kc, L - h)
        e += kc
        h += kc
        new = cur & (g >= e)
        if L and h >= L:
            new[:] = False
        _, sz2 = group_sizes(new, new.size + 1)
        stall = 0 if (int(sz2.sum()) < A or int(sz2.size) > G) else stall + 1
        cur = new
        rounds += 1


def finisher_run(glue, tied, d, b, L, k):
    """run_group_finisher at depth k + d: plan, every tile finished, what failed or was left out stays.
    -> (records in tiles, records resolved, plan)"""
    starts, sizes = group_sizes(tied, tied.size + 1)
    plan = plan_tiles(sizes, FIN_TILE, FIN_CAP)
    # list position -> record: the active list is the tied records, compacted
    rec_of = np.concatenate([np.arange(s, s + z) for s, z in zip(starts, sizes)]) if sizes.size else np.zeros(0, np.int64)
    resolved = 0
    for begin, local_end, _ in plan.tiles:
        if local_end == begin:
            continue
        r0, r1 = int(rec_of[begin]), int(rec_of[local_end - 1])
        pairs = slice(r0, r1)
        g = np.where(tied[pairs], glue[pairs] - d, -1)
        failed = finish_tile(g, b, L, k + d)
        ok = tied[pairs] & ~failed
        _, zs = group_sizes(ok, ok.size + 1)
        resolved += int(zs.sum())
        tied[pairs] &= failed
    return plan.inside, resolved, plan


def round_sort_big(sizes, local_rounds=True):
    """Builder::round_sort: the records of a round that go through the global sort.  Everything when the tile-local sort is
    off, when an average group exceeds half a tile or when more than half the records sit in left-out groups; else the
    plan's left-out groups."""
    M, G = int(np.sum(sizes)), int(len(sizes))
    if not local_rounds or G == 0 or (M > LOC_CAP and M > G * (LOC_CAP // 2)):
        return M
    left = plan_tiles(sizes, LOC_TILE, LOC_CAP).left
    return M if left * 2 > M else left


def loc_sort_packed(gb, b, kc):
    """the record form loc_sort_kernel takes in a chunk round of kc symbols with gb group-id bits (Builder::round_sort:
    packed when top - begin_bit + LOC_GID_BITS <= 64, top = min(64, gid_shift + LOC_GID_BITS), gid_shift = 64 - gb)"""
    begin_bit = 64 - gb - b * kc
    gid_shift = 64 - gb
    top = gid_shift + LOC_GID_BITS if gid_shift < 64 - LOC_GID_BITS else 64
    return top - begin_bit + LOC_GID_BITS <= 64


def period_groups(t, sa, apos, tied):
    """the groups of the active list as period_finish.hpp sees them: per group (first record, size, members' text positions
    ascending, difference d or 0 when the members are no arithmetic progression)"""
    starts, sizes = group_sizes(tied, tied.size + 1)
    out = []
    for s0, z in zip(starts, sizes):
        pos = np.sort(np.asarray(sa)[apos[s0:s0 + z]].astype(np.int64))
        df = np.diff(pos)
        out.append((int(s0), int(z), pos, int(df[0]) if (df == df[0]).all() else 0))
    return out


def run_end(t, d, p0):
    """E: the first x >= p0 with x + d >= n or t[x] != t[x + d]"""
    n = int(t.size)
    stop = min(n - d, p0 + (1 << 16))
    while True:
        ne = np.flatnonzero(t[p0:stop] != t[p0 + d:stop + d])
        if ne.size:
            return p0 + int(ne[0])
        if stop >= n - d:
            return n - d
        p0, stop = stop, min(n - d, stop + (1 << 20))


def period_attempt(t, sa, apos, tied, M):
    """run_period_finisher: up to four times, the difference that covers the most records of arithmetic groups (the smaller
    one on a tie) is taken when it covers at least M / 8; a group of that difference is ordered (all its pairs cleared in tied)
    when the run from its first member reaches its last member but one: E + d >= last and E < n; else it is out of the
    histogram.  Nothing counts when all the tries together covered less than M / 8.
    -> (records resolved, [(d, records covered, [(p0, last, members, E, taken)])])"""
    gs = period_groups(t, sa, apos, tied)
    bad = [g[3] == 0 for g in gs]
    n = int(t.size)
    tries, covered, resolved = [], 0, 0
    for _ in range(4):
        hist = {}
        for g, bd in zip(gs, bad):
            if not bd:
                hist[g[3]] = hist.get(g[3], 0) + g[1]
        if not hist:
            break
        d, cnt = min(hist.items(), key=lambda kv: (-kv[1], kv[0]))
        if cnt * 8 < M:
            break
        covered += cnt
        rows = []
        for i, g in enumerate(gs):
            if bad[i] or g[3] != d:
                continue
            p0, last = int(g[2][0]), int(g[2][-1])
            E = run_end(t, d, p0)
            taken = E + d >= last and E < n
            rows.append((p0, last, g[1], E, taken))
            bad[i] = True
            if taken:
                tied[g[0]:g[0] + g[1] - 1] = False
                resolved += g[1]
        tries.append((d, cnt, rows))
    if covered * 8 < M:
        return 0, tries
    return resolved, tries


def simulate(gr, n, k, b, L=0, tiny=True, group_finish=True, period_finish=True, local_rounds=True, t=None, sa=None):
    """The host loop of Builder::build over the groups gr (groups_after_keys of the full suffix array) -> the BuildStats
    counts.  exact is False from the point where the build would start a doubling round, or where a try of the periodic-run
    shortcut leaves 64 or more records (it would be tried again after the rounds): the counts up to there are what the model
    vouches for (doubling_rounds, rounds, active_total are then lower bounds; handover = the records of the round the model
    stopped before).  t, sa: the text and its suffix array, needed once the shortcut is tried (period_attempt).
    Left out of the restatement, all unreachable at the default settings before exact turns False: per_fails < 8 and
    per_skip (set by a try that resolves too little: the model stops there), have_isa (set by the first doubling round)
    and round_sort's exit top <= begin_bit (no key bits to sort)."""
    glue = gr.glue.astype(np.int64)
    tied = glue >= 0
    st = dict(tiny_resolved=0, finisher_runs=0, finisher_records=0, finisher_resolved=0, rounds=0, chunk_rounds=0, active_total=0,
              big_records=0, big_passes_records=0, exact=True, plans=[], round_sizes=[], packed=[], period_resolved=0,
              period_tries=[], handover=0)
    if L and k >= L:
        return st
    d = 0

    def count():
        _, z = group_sizes(tied, tied.size + 1)
        return int(z.sum()), int(z.size), z
    M, G, sizes = count()
    if tiny and M and M * 16 <= n:
        st["tiny_resolved"] = tiny_pass(glue, tied, (L - k) if L else TINY_DEPTH, bool(L))
    fin_useful = True
    chunk_done = 0
    M_prev = 0
    while True:
        M, G, sizes = count()
        if not M or (L and k + d >= L):
            break
        if group_finish and fin_useful and M <= G * (FIN_CAP // 2):
            looked, res, plan = finisher_run(glue, tied, d, b, L, k)
            st["finisher_runs"] += 1
            st["finisher_records"] += looked
            st["finisher_resolved"] += res
            st["plans"].append(plan)
            if res * 4 < looked:
                fin_useful = False
            M, G, sizes = count()
            if not M:
                break
        if period_finish and L == 0 and M >= 64 and (not fin_useful or M > G * (FIN_CAP // 2)):
            res, tries = period_attempt(t, sa, gr.apos, tied, M)
            st["period_resolved"] += res
            st["period_tries"].append(tries)
            M, G, sizes = count()
            if not M:
                break
            if M >= 64:
                st["exact"] = False
                st["handover"] = M
                break
        shrinking = M_prev != 0 and M * 2 <= M_prev
        if not (L or chunk_done < CHUNK_ROUNDS_BEFORE_DOUBLING or shrinking):
            st["exact"] = False
            st["handover"] = M
            break
        gb = bits_for(G)
        kc = (64 - gb) // b
        if L:
            kc = min(kc, L - (k + d))
        big = round_sort_big(sizes, local_rounds)
        passes = -(-(gb + b * kc) // RADIX_BITS)
        st["big_records"] += big
        st["big_passes_records"] += big * passes
        st["round_sizes"].append(sizes)
        st["packed"].append(loc_sort_packed(gb, b, kc))
        st["active_total"] += M
        st["rounds"] += 1
        st["chunk_rounds"] += 1
        chunk_done += 1
        M_prev = M
        d += kc
        tied &= glue >= d
    return st


def tied_model(t, k):
    """M by the model the 64-bit build's tests use (cases.tied_after_keys): groups_after_keys must agree with it"""
    return cases.tied_after_keys(t, k)


# ---- the cases --------------------------------------------------------------------------------------------------------------
# name -> (n, plants, keyword arguments of planted_groups, L).  Seeds are fixed; tests/test_refine_cases_cpu.py checks what each
# case claims against the model.
Case = namedtuple("Case", "n plants kw L")
PAIR, TRIPLE = (2, K), (3, K)


def _c(n, plants, L=0, **kw):
    kw.setdefault("seed", 7)
    return Case(n, plants, kw, L)


def tiny_cases():
    M16 = [PAIR] * 8000   # 16 000 tied records
    c = {
        "sizes_2_9": _c(300_000, [(s, 14) for s in range(2, 10)] * 3),                      # three groups of every size 2..9
        "lcp_63_64_65": _c(300_000, [(s, K + e) for s in (2, 3) for e in (63, 64, 65)]),    # glue up to 65: 64 and 65 stay
        "ends_at_text_end": _c(300_000, [(2, 20), (3, 20)] + [PAIR] * 50, at_end=0),        # a member with 0..8 bytes beyond the key
        "M4096": _c(300_000, [PAIR] * 2048),
        "M4097": _c(300_000, [PAIR] * 2047 + [TRIPLE]),
        "sparse_16M_eq_n": _c(256_000, M16),                                                # 16 M == n: the tiny pass runs
        "sparse_16M_gt_n": _c(255_999, M16),                                                # 16 M == n + 1: it does not
    }
    for L in (13, 19, 20, 21):                                                              # L - h = 1, 7, 8, 9
        c["trunc_L%d" % L] = _c(300_000, [(s, 40) for s in range(2, 10)], L=L)
    return c


def finisher_cases():
    pow2 = [(1 << e, K) for e in range(1, 12)] + [((1 << e) + 1, K) for e in range(1, 12)]
    c = {
        "M4096": _c(300_000, [PAIR] * 2048),                                                # the one-tile shortcut
        "M4097": _c(300_000, [PAIR] * 2047 + [TRIPLE]),                                     # planned: two tiles
        # 3583 records sort before the "mid" group, which straddles record 3584: tile 0 is [0, 3583 + size)
        "tile_eq_cap": _c(400_000, [PAIR + ("lo",)] * 1790 + [TRIPLE + ("lo",)] + [(513, K, "mid")] + [PAIR + ("hi",)] * 600),
        "tile_cap_plus_1": _c(400_000, [PAIR + ("lo",)] * 1790 + [TRIPLE + ("lo",)] + [(514, K, "mid")] + [PAIR + ("hi",)] * 600),
        # the "mid" group starts tile 0: 4096 records are a tile of exactly FIN_CAP, 4097 can never fit
        "group_4096": _c(600_000, [(4096, K, "mid")] + [PAIR + ("hi",)] * 600),
        "group_4097": _c(600_000, [(4097, K, "mid")] + [PAIR + ("hi",)] * 600),
        "largest_96": _c(300_000, [(96, K)] + [PAIR] * 200),
        "largest_97": _c(300_000, [(97, K)] + [PAIR] * 200),
        "sizes_pow2": _c(900_000, pow2),
        # (a tile of 2048 pairs -- s_gq / s_gpos at CAP / 2 groups -- exists only as the one tile of M4096: a planned tile of
        #  pairs holds FIN_TILE / 2 of them)
        #  The issue's "2047 pairs plus a triple" is 4097 records, which cannot be one tile: this case has one pair less.
        "pairs_2046_and_a_triple": _c(300_000, [PAIR] * 2046 + [TRIPLE]),                   # one tile of 4095 records, 2047 groups
        "long_lcp": _c(400_000, [(2, K + 4100)] + [PAIR] * 3000 + [(5, 15)] * 40),          # pairs that share up to 4100 symbols
        "below_a_quarter": _c(300_000, [(2, K + 900)] + [PAIR] * 40),
        "above_a_quarter": _c(300_000, [(2, K + 900)] + [PAIR] * 400),
        "sigma4": _c(300_000, [(2, 24), (3, 25), (4, 22), (40, 21)] + [(2, 21)] * 500, symbols=np.array([65, 67, 71, 84], np.uint8)),
        "sigma256": _c(300_000, [(2, 9), (3, 10), (27, 8), (300, 7)] + [(2, 7)] * 500, symbols=np.arange(256, dtype=np.uint8)),
    }
    for L in (13, 20, 33):
        c["trunc_L%d" % L] = _c(300_000, [(s, 60) for s in (2, 3, 9, 27)] + [PAIR] * 100, L=L)
    return c


def round_sort_cases():
    c = {
        "tile_eq_cap": _c(400_000, [PAIR + ("lo",)] * 1790 + [TRIPLE + ("lo",)] + [(513, K, "mid")] + [PAIR + ("hi",)] * 600),
        "tile_cap_plus_1": _c(400_000, [PAIR + ("lo",)] * 1790 + [TRIPLE + ("lo",)] + [(514, K, "mid")] + [PAIR + ("hi",)] * 600),
        "M4096": _c(300_000, [PAIR] * 2048),
        "M4097": _c(300_000, [PAIR] * 2047 + [TRIPLE]),
        "one_big_between_small": _c(600_000, [PAIR + ("lo",)] * 3000 + [(5000, K, "mid")] + [PAIR + ("hi",)] * 3000),
        "two_big_groups": _c(900_000, [PAIR + ("lo",)] * 6000 + [(4500, K, "mid"), (4700, K, "mid")] + [PAIR + ("hi",)] * 6000),
        # one big group whose copy to the global sort's list is cut into slices.  (A group of 10^5 records brings shifted groups of
        # 10^5 / 27 records with it, 2 * 10^5 more records that no tile holds: the tile-local sort is only taken when fewer than
        # half the records are left out, which would need a text of about 10^7 symbols.  20 000 is what fits 2 * 10^6.)
        "big_20000": _c(2_000_000, [PAIR] * 50_000 + [(20_000, K)]),
        "packed_L20": _c(400_000, [(s, 40) for s in (2, 3, 9, 27)] * 8 + [PAIR] * 3000, L=20),   # kc = 8: 40 key bits, packed
        "sigma256": _c(300_000, [(2, 9), (3, 10), (27, 8), (300, 7)] + [(2, 7)] * 3000, symbols=np.arange(256, dtype=np.uint8)),
    }
    return c


def periodic_runs(n, runs, seed, plants=(), symbols=D1_SYMBOLS):
    """planted_groups(n // 2, plants) followed by random text with periodic runs.  A run (pos, d, length, end[, edits]) is a
    random word of d symbols repeated over [pos, pos + length) (pos counts from n // 2; "eot": the run ends the text); the
    symbol after it is below ("lt") or above ("gt") the one d before it: the pairs of the run's groups come out in
    descending or ascending order of position.  edits: offsets into the run whose symbol is replaced by another one."""
    rng = np.random.default_rng(seed)
    symbols = np.asarray(symbols)
    S = symbols.size
    head = planted_groups(n // 2, list(plants), seed + 1, symbols)[0] if plants else symbols[rng.integers(0, S, n // 2)]
    t = np.concatenate([head, symbols[rng.integers(0, S, n - n // 2)]])
    at = []
    for pos, d, length, end, *edits in runs:
        w = rng.integers(1, S - 1, d)                       # neither the smallest nor the largest symbol: both ends possible
        p = n - length if end == "eot" else n // 2 + pos
        t[p:p + length] = symbols[w[np.arange(length) % d]]
        if end != "eot":
            j = int(w[length % d])
            t[p + length] = symbols[j - 1 if end == "lt" else j + 1]
        j = int(w[(d - 1) % d])
        t[p - 1] = symbols[(j + 1) % S] if t[p - 1] == symbols[j] else t[p - 1]   # the run does not reach further left
        for e in (edits[0] if edits else ()):
            j = int(np.flatnonzero(symbols == t[p + e])[0])
            t[p + e] = symbols[j + 1 if j + 1 < S - 1 else j - 1]
        at.append(p)
    return np.ascontiguousarray(t), at


PCase = namedtuple("PCase", "n runs kw")
PER_D, PER_T = 200, 8
PER_LEN = 2 * PER_D + K + 64 + PER_T     # residues 0 .. 71 have three members, the others two; every group holds a pair that
#                                          shares 64 symbols or more beyond the key: neither the tiny pass nor the finisher take it


def period_cases():
    """Default settings.  The tiny pass leaves every group of the runs (a pair of each shares >= 64 symbols), the finisher
    stalls on them and gives up (fin_useful cleared), and the shortcut is tried on M >= 64 records."""
    D, LEN = PER_D, PER_LEN
    BD = 3000                            # most pairs share more than the finisher's 24 x 8 symbols: it gives up in its first run
    BLEN = 2 * BD + K + 64 + PER_T
    x0 = PER_T + 64 - 5                  # the triple of residue x0 and the four after it
    tile = lambda e, d, length: e - (length - d)   # noqa: E731  run start (from n // 2 = 2^17) that puts E at e
    c = {
        # E = p1 - 1 for residue x0 (one below p0 + (m - 2) d): the symbol before the third member is changed
        "E_one_less": PCase(1 << 18, [(5000, BD, BLEN, "lt", [x0 + 2 * BD - 1])], dict(seed=31)),
        # the smallest E a group can have at or above p0 + (m - 2) d: members share the key, so E >= p1 + K
        "E_first_reachable": PCase(1 << 18, [(5000, BD, BLEN, "gt", [x0 - 9 + 2 * BD + K])], dict(seed=32)),
        "ends_lt_gt_eot": PCase(1 << 18, [(5000, 200, LEN, "lt"), (20000, 210, LEN + 20, "gt"), (0, 220, LEN + 40, "eot")], dict(seed=33)),
        "tile_edges": PCase(1 << 18, [(tile(2 * 4096 + 4095, 200, LEN), 200, LEN, "lt"), (tile(5 * 4096, 210, LEN + 20), 210, LEN + 20, "gt"),
                                      (tile(8 * 4096 + 1, 220, LEN + 40), 220, LEN + 40, "lt")], dict(seed=34)),
        "three_tiles": PCase(1 << 18, [(4096 - 300, BD, BLEN, "gt")], dict(seed=35)),
        "M64": PCase(1 << 18, [(5000, D, D + K + 64 + 31, "lt")], dict(seed=36)),            # 32 pairs that share 64 .. 95 symbols
        "M63": PCase(1 << 18, [(5000, D, D + K + 64 + 29, "lt")], dict(seed=37, plants=[(3, K + 64)])),   # 30 pairs and a triple
    }
    return c


def narrow_cases():
    """27 symbols, keys of 8 symbols (40 bits: the narrow-record plan, which needs 2^22 symbols).  Plants of 8 symbols; the
    random part adds a few dozen accidental pairs, which the model counts."""
    return {"all_tiny": _c(4_400_000, [(s, 10) for s in range(2, 9)] * 4),
            "with_rest": _c(4_400_000, [(s, 10) for s in range(2, 10)] * 4 + [(27, 9)])}


def make_periodic(case):
    return periodic_runs(case.n, case.runs, **case.kw)[0]


def make(case):
    """-> the text of a case"""
    kw = dict(case.kw)
    return planted_groups(case.n, case.plants, kw.pop("seed"), **kw)[0]
