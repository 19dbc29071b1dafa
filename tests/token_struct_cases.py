"""Texts, patterns and the models of the two structures every token search starts from (test_token_struct_cases_cpu.py,
test_gpu_token_structs.py); plain NumPy, no GPU.

tq_range (csrc/token_query.hpp) takes two device arrays as given.  They are modelled whole here, from the comments that define
them and not from the kernels that write them:

  dir   "dir[v - min] = number of suffixes whose first symbol is < v, u32, max - min + 2 entries", when max - min + 1 <= 2^24:
        directory(t) = searchsorted(sort(t), arange(min, max + 2)); its last entry is n.
  K     "K[r] = ((T[p] + 1) << 32) | (p + 1 < n ? T[p + 1] + 1 : 0), p = SA[r], u64": keys(t, sa).

The writers and the edges the texts below stand on:
  tq_hist_kernel         counts bin T[i] - min in LDS below cap = min(bins, HIST_LDS) and by global atomics from cap on.  bins_B puts
                         the alphabet on both sides of HIST_LDS; hot_above puts half of 400 000 tokens on the first global bin and a
                         quarter on the last LDS bin; top_of_range does the subtraction at the top of int32.  Every text has min = 5,
                         so a kernel that forgets `- mn` shifts every bin.
  the scan (three steps) tiles of SC_TILE entries, SC_ITEMS per thread; the partial sums are scanned SC_BLOCK at a time.  tile_L puts
                         the directory's end one before, on and one behind a tile edge (one and two tiles); parts_1024 and parts_1025
                         put the number of partial sums on and one behind the second trip of the parts loop; cap_in is the largest
                         directory there is (2^24 + 1 entries), cap_out the smallest range without one.
  tq_keys_kernel         every text; top_of_range holds the key field 2^31.

The bounds texts are short (n = 1 .. 65 and around 128 and 256) over {6, 7, 8}, with every pattern of length 1 .. 4 over
{-1, 5, 6, 7, 8, 9}: tq_key_bounds and tq_text_bounds search the lower and the upper bound in one loop, and the sizes around a
power of two are where the two midpoints part and meet again.

bins_B, a decision: the list of bins that must be present (0, 12286, 12287, 12288, B - 1) and the bin that must be absent (B - 2)
collide for B = 12288 and 12289.  Presence wins -- the last LDS bin and the first global bin are what the texts are for -- and the
absent bin is the highest one below B - 1 that is not required: 12285 for all three B.
"""
import itertools

import numpy as np

import token_cases as tc
from test_int_cpu import model_sa

I32_MIN, I32_MAX = tc.I32_MIN, tc.I32_MAX

# restated from the headers; (file under suffixarray_amd/csrc, regular expression whose group 1 is the definition, value)
HEADER_CONSTANTS = [
    ("token_query.hpp", r"constexpr u32 HIST_LDS = (\d+);", "12288"),
    ("token_query.hpp", r"constexpr u64 DIR_CAP = (1ull << 24);", "1ull << 24"),
    ("token_query.hpp", r"constexpr int BLOCK = (\d+);", "256"),
    ("token_query.hpp", r"constexpr int STEPS = (\d+);", "32"),
    ("token_query.hpp", r"const u32 cap = (bins < HIST_LDS \? bins : HIST_LDS);", "bins < HIST_LDS ? bins : HIST_LDS"),
    ("token_query.hpp", r"if \(knobs.dir && range (<=) DIR_CAP\)", "<="),
    ("big_build.hpp", r"constexpr u32 SC_BLOCK = (\d+), SC_ITEMS = \d+, SC_TILE = SC_BLOCK \* SC_ITEMS;", "1024"),
    ("big_build.hpp", r"constexpr u32 SC_BLOCK = \d+, SC_ITEMS = (\d+), SC_TILE = SC_BLOCK \* SC_ITEMS;", "8"),
    ("big_build.hpp", r"constexpr u32 SC_BLOCK = \d+, SC_ITEMS = \d+, SC_TILE = (SC_BLOCK \* SC_ITEMS);", "SC_BLOCK * SC_ITEMS"),
]
HIST_LDS = 12288
DIR_CAP = 1 << 24
BLOCK = 256
STEPS = 32
SC_BLOCK = 1024
SC_ITEMS = 8
SC_TILE = SC_BLOCK * SC_ITEMS

MN = 5                                         # the smallest symbol of every directory text but top_of_range
N_TEXT = 40000


# ---- the models ----------------------------------------------------------------------------------------------------------------

def directory(t):
    """dir[j] = number of suffixes whose first symbol is < min + j, j in [0, max - min + 2); the last entry is n"""
    t = np.asarray(t, np.int64)
    mn, mx = int(t.min()), int(t.max())
    d = np.searchsorted(np.sort(t), np.arange(mn, mx + 2, dtype=np.int64), side="left").astype(np.uint32)
    assert d.size == mx - mn + 2 and int(d[-1]) == t.size
    return d


def keys(t, sa):
    """K[r] = ((t[p] + 1) << 32) | (t[p + 1] + 1 if p + 1 < n else 0), p = sa[r]"""
    t = np.asarray(t, np.int64)
    p = np.asarray(sa, np.int64)
    nxt = np.concatenate([t + 1, [0]])[p + 1] if t.size else np.zeros(0, np.int64)
    return ((t[p] + 1).astype(np.uint64) << np.uint64(32)) | nxt.astype(np.uint64)


def has_directory(t):
    t = np.asarray(t, np.int64)
    return bool(t.size) and int(t.max()) - int(t.min()) + 1 <= DIR_CAP


def describe(kind, t, sa, i):
    """what stands behind entry i of "dir" or "K": the symbol or rank, and a text position that holds it"""
    t = np.asarray(t, np.int64)
    i = int(i)
    if kind == "dir":
        mn = int(t.min())
        v = mn + i
        where = np.flatnonzero(t == v - 1)                             # the symbol whose count the entry adds to the one before it
        return "dir[%d]: suffixes below symbol %d (bin %d, scan tile %d, thread %d, item %d); symbol %d stands %d times%s" % (
            i, v, i, i // SC_TILE, i % SC_TILE // SC_ITEMS, i % SC_ITEMS, v - 1, where.size,
            ", first at text position %d" % int(where[0]) if where.size else "")
    p = int(sa[i])
    return "K[%d]: rank %d is suffix %d, T[p] = %d, T[p + 1] = %s" % (i, i, p, int(t[p]), int(t[p + 1]) if p + 1 < t.size else "(the end)")


def mismatch(kind, got, want, t, sa):
    """"" or the first five differing entries through describe()"""
    if got.shape == want.shape and np.array_equal(got, want):
        return ""
    if got.shape != want.shape:
        return "%s: %d entries, model %d" % (kind, got.size, want.size)
    bad = np.flatnonzero(got != want)
    return "%s: %d of %d entries differ\n" % (kind, bad.size, want.size) + "\n".join(
        "  got %d, model %d -- %s" % (int(got[i]), int(want[i]), describe(kind, t, sa, i)) for i in bad[:5])


# ---- texts for the directory and the histogram -----------------------------------------------------------------------------------

def _uniform(seed, n, bins, present, absent=(), mn=MN):
    """n symbols uniform over `bins` bins from mn on; the bins of `absent` are emptied (moved to bin 1), then one token of every
    bin of `present` is planted at a random position"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, bins, n, dtype=np.int64)
    for a in absent:
        b[b == a] = 1
    present = sorted(set(p for p in present if 0 <= p < bins))
    assert not set(present) & set(absent)
    b[rng.choice(n, len(present), replace=False)] = present
    return (b + mn).astype(np.int32)


def _bins_absent(B):
    need = {0, 12286, 12287, 12288, B - 1}
    return max(a for a in range(B - 1) if a not in need and a <= B - 2)


def _make(name):
    kind, _, arg = name.partition("_")
    if kind == "bins":
        B = int(arg)
        return _uniform(B, N_TEXT, B, [0, 12286, 12287, 12288, B - 1], [_bins_absent(B)])
    if name == "hot_above":
        rng = np.random.default_rng(41)
        n = 400000
        b = rng.integers(0, 20000, n, dtype=np.int64)
        b[:n // 2] = HIST_LDS
        b[n // 2:n // 2 + n // 4] = HIST_LDS - 1
        b[-2:] = (0, 19999)
        return (rng.permutation(b) + MN).astype(np.int32)
    if kind == "tile":
        L = int(arg)                                                   # directory entries: bins 0 .. L - 2
        return _uniform(L, N_TEXT, L - 1, [0, SC_TILE - 2, SC_TILE - 1, SC_TILE, SC_TILE + 1, L - 2])
    if kind == "parts":
        L = SC_BLOCK * SC_TILE + (int(arg) - SC_BLOCK)
        edge = [k * SC_TILE + j for k in (0, 1, SC_BLOCK - 1, SC_BLOCK) for j in (0, SC_TILE - 1)]
        return _uniform(int(arg), N_TEXT, L - 1, edge + [0, L - 2])
    if name == "cap_in":
        return _uniform(51, 3000, DIR_CAP, [0, DIR_CAP - 1])
    if name == "cap_out":
        return _uniform(52, 3000, DIR_CAP + 1, [0, DIR_CAP])
    if name == "top_of_range":
        return _uniform(53, N_TEXT, HIST_LDS + 1, [0, HIST_LDS - 1, HIST_LDS], mn=I32_MAX - HIST_LDS)
    raise KeyError(name)


BINS = ("bins_12287", "bins_12288", "bins_12289")
TILES = ("tile_8191", "tile_8192", "tile_8193", "tile_16384", "tile_16385")
PARTS = ("parts_1024", "parts_1025")
DIR_TEXTS = BINS + ("hot_above",) + TILES + PARTS + ("cap_in", "cap_out", "top_of_range")
SMALL_RANGE = 20000                            # texts of at most this range go through all four plans of the search
FAMILIES = ("bins_12288", "hot_above", "tile_8193", "parts_1025", "cap_in", "top_of_range")   # one per family also through build()
WALK_TEXTS = ("hot_above", "tile_8193")
WALK_RANKS = 4096

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def text(name):
    return _cached(("t", name), lambda: _make(name))


def sa_of(name):
    return _cached(("sa", name), lambda: model_sa(text(name)).astype(np.int32))


def dir_of(name):
    return _cached(("dir", name), lambda: directory(text(name)))


def keys_of(name):
    return _cached(("K", name), lambda: keys(text(name), sa_of(name)))


def range_of(name):
    t = text(name)
    return int(t.max()) - int(t.min()) + 1


def info_expected(name, plan):
    """the fields of info() that the model fixes"""
    t, sa = text(name), sa_of(name)
    switches = "".join(tc.PLANS[plan])
    return {"n": t.size, "min_symbol": int(t.min()), "max_symbol": int(t.max()),
            "dir_entries": range_of(name) + 1 if "DIR" not in switches and has_directory(t) else 0,
            "key_bytes": 8 if "KEYS" not in switches else 0, "last_rank": int(np.flatnonzero(sa == t.size - 1)[0])}


def singles_expected(name):
    """(v0, Q, first, count) of the length-1 patterns [v], v = v0 .. v0 + Q - 1 over [min - 1, max + 1] (cut at I32_MAX): first by
    searchsorted over the sorted text, count by bincount -- absent symbols keep the exact lower bound"""
    def make():
        t = np.asarray(text(name), np.int64)
        v0, v1 = int(t.min()) - 1, min(int(t.max()) + 1, I32_MAX)
        first = np.searchsorted(np.sort(t), np.arange(v0, v1 + 1, dtype=np.int64), side="left").astype(np.uint32)
        count = np.bincount(t - v0, minlength=v1 - v0 + 1).astype(np.uint32)
        return v0, v1 - v0 + 1, first, count
    return _cached(("singles", name), make)


# ---- texts and patterns for the bounds -------------------------------------------------------------------------------------------

ALPHABET = (6, 7, 8)
PATTERN_SYMBOLS = (-1, 5, 6, 7, 8, 9)
SMALL_N = tuple(range(1, 66))
EDGE_N = (127, 128, 129, 255, 256, 257)
SHORT = [list(p) for m in range(1, 5) for p in itertools.product(PATTERN_SYMBOLS, repeat=m)]     # 6 + 36 + 216 + 1296


def _bounds_texts():
    out = {}
    for n in SMALL_N:
        out["equal_%d" % n] = np.full(n, 7, np.int32)
        out["period2_%d" % n] = np.tile(np.array([7, 6], np.int32), n // 2 + 1)[:n].copy()
        out["random_%d" % n] = np.random.default_rng(1000 + n).choice(np.array(ALPHABET, np.int32), n)
    for n in EDGE_N:
        out["equal_%d" % n] = np.full(n, 7, np.int32)
        out["equal_but_last_%d" % n] = np.concatenate([np.full(n - 1, 7, np.int32), np.array([8], np.int32)])
    return out


BOUNDS_TEXTS = _bounds_texts()


def bounds_patterns(t):
    """every short pattern; the whole text, and with one more symbol; every suffix of at most 6 symbols with 5, 9, -1 and
    I32_MIN appended"""
    tl = [int(v) for v in t]
    pats = list(SHORT) + [tl, tl + [7]]
    for m in range(1, min(6, len(tl)) + 1):
        pats += [tl[len(tl) - m:] + [v] for v in (5, 9, -1, I32_MIN)]
    return pats


def span_contexts(t):
    """the contexts of the spans test: the short patterns and the whole text"""
    return list(SHORT) + [[int(v) for v in t]]


def bounds_expected(name):
    """(text, suffix array, patterns, first, count by model (a), count by model (b)) of one bounds text, once per process"""
    def make():
        t = BOUNDS_TEXTS[name]
        sa = model_sa(t).astype(np.int32)
        pats = bounds_patterns(t)
        first, count = tc.model_a(t, sa, pats)
        return t, sa, pats, first, count, tc.model_b(t, pats)
    return _cached(("bounds", name), make)


def packed_patterns(name):
    """the pattern set of one bounds text as (packed int32, uint64 offsets), once per process"""
    return _cached(("packed", name), lambda: tc.pack(bounds_expected(name)[2]))


def group_sizes(t, sa):
    """-> (sizes of the runs of ranks with an equal first symbol -- the windows tq_key_bounds is given behind the directory, and
    the high field of K --, sizes of the runs with an equal key -- the windows tq_text_bounds refines)"""
    k = keys(t, sa)
    return (set(np.unique(k >> np.uint64(32), return_counts=True)[1].tolist()), set(np.unique(k, return_counts=True)[1].tolist()))


# ---- what the lists have to reach ------------------------------------------------------------------------------------------------

def coverage(dir_texts=DIR_TEXTS, bounds=None):
    """asserts, from the texts alone, that the lists stand where their names say"""
    bounds = BOUNDS_TEXTS if bounds is None else bounds
    caps, lds_edge, global_edge, hot, tile_edge, nparts, ends = set(), False, False, False, False, set(), set()
    for name in dir_texts:
        t = np.asarray(text(name), np.int64)
        mn = int(t.min())
        assert mn == (I32_MAX - HIST_LDS if name == "top_of_range" else MN), name
        bins = range_of(name)
        if not has_directory(t):
            assert name == "cap_out" and bins == DIR_CAP + 1
            continue
        cnt = np.bincount(t - mn, minlength=bins)
        caps.add("bins" if bins < HIST_LDS else "lds" if bins > HIST_LDS else "both")
        lds_edge |= bins > HIST_LDS and cnt[HIST_LDS - 1] > 0 and cnt[HIST_LDS] > 0
        global_edge |= bins > HIST_LDS and cnt[HIST_LDS] > 0
        hot |= bins > HIST_LDS and cnt[HIST_LDS] * 2 >= t.size
        L = bins + 1
        nparts.add((L + SC_TILE - 1) // SC_TILE)
        ends.add(((L + SC_TILE - 1) // SC_TILE, L % SC_TILE))
        tile_edge |= bins > SC_TILE and cnt[SC_TILE - 1] > 0 and cnt[SC_TILE] > 0
        if name.startswith("bins_"):
            B = int(name[5:])
            assert bins == B and cnt[_bins_absent(B)] == 0 and all(cnt[b] > 0 for b in (0, 12286, 12287, 12288, B - 1) if b < B), name
        if name.startswith("tile_"):
            assert L == int(name[5:]) and all(cnt[b] > 0 for b in (8190, 8191, 8192, 8193) if b < bins), name
        if name.startswith("parts_"):
            assert (L + SC_TILE - 1) // SC_TILE == int(name[6:]), name
            assert all(cnt[k * SC_TILE + j] > 0 for k in (0, 1, SC_BLOCK - 1, SC_BLOCK) for j in (0, SC_TILE - 1) if k * SC_TILE + j < bins), name
        if name == "cap_in":
            assert bins == DIR_CAP
    assert {"bins", "both", "lds"} <= caps, caps                      # cap = bins, cap = bins = HIST_LDS, cap = HIST_LDS
    assert lds_edge and global_edge and hot                             # the last LDS bin and the first global one hold symbols
    assert tile_edge
    assert {SC_BLOCK, SC_BLOCK + 1} <= nparts, sorted(nparts)
    # (tiles, entries of the last one modulo SC_TILE): the directory ends one entry before the first tile edge -- a last thread with
    # 7 of its SC_ITEMS entries --, on it and one behind it -- a tile of one entry --, and on and behind the second edge
    assert {(1, SC_TILE - 1), (1, 0), (2, 1), (2, 0), (3, 1)} <= ends, sorted(ends)
    high, full, lengths = set(), set(), set()
    for name, t in bounds.items():
        h, f = group_sizes(t, model_sa(t))
        high |= h
        full |= f
        lengths.add(int(t.size))
    assert set(range(1, 66)) <= high and set(range(1, 65)) <= full, (sorted(set(range(1, 66)) - high), sorted(set(range(1, 65)) - full))
    assert set(SMALL_N) | set(EDGE_N) <= lengths
    assert len(SHORT) == 1554
