"""Models and case table of the integer-alphabet build's edge tests (tests/test_gpu_int_edges.py); plain NumPy, no GPU.

sa_hip_libsais_int / sa_hip_libsais64_long (csrc/int_build.hpp, int_core in csrc/capi_dropins.hpp) choose a code width b, a
number s of symbols per initial key and a route, then hand route B's keys to BigBuilder::build_with (csrc/big_build.hpp), whose
prefix doubling repairs every key that is merely shorter or wider than intended: the suffix array cannot show a plan that is
wrong.  The stats can.  This module restates, from the comments of those headers and DESIGN 9f and not from the kernels,
  plan(t, knobs)            min, max, compacted, sigma, route, bits, s
  keys(t, plan)             the u64 key of every suffix
  rounds_model(t, sa, plan) tied_after_sort, rounds, tied_total, sort_passes from the plain LCP of neighbouring ranks
and holds the texts that put n, sigma, max and the ties on the edges of the key, of the keygen's tile and halo, of the code
width, of the presence table and its scan, and of the refusal's "first position".  tests/test_int_cases_cpu.py checks the
constants against the headers, the models against brute force and that every case holds the edge it is named for."""
import functools
import zlib
from collections import namedtuple

import numpy as np

# restated from the headers: (file under suffixarray_amd/csrc, regular expression with one group, the group's text)
DENSE_CAP = 1 << 24
KG_TILE, KG_HALO = 2048, 64
SC_BLOCK, SC_ITEMS = 1024, 8
SC_TILE = SC_BLOCK * SC_ITEMS
BG_TILE = 512 * 16
GRID_CAP = 256 * 8            # stream_grid: at most this many workgroups
FIRST_BAD_PER_BLOCK = 256 * 16   # int_first_bad_kernel: stream_grid(n, 256 * 16) workgroups of 256 threads
CONSTANTS = [
    ("int_build.hpp", r"constexpr u64 DENSE_CAP = (1ull << 24);", "1ull << 24"),
    ("int_build.hpp", r"constexpr u32 KG_TILE = (\d+);", "2048"),
    ("int_build.hpp", r"constexpr u32 KG_HALO = (\d+);", "64"),
    ("int_build.hpp", r"__shared__ u64 s_c\[(KG_TILE \+ KG_HALO)\];", "KG_TILE + KG_HALO"),
    ("int_build.hpp", r"const u32 span = (KG_TILE \+ \(u32\)s - 1);", "KG_TILE + (u32)s - 1"),
    ("int_build.hpp", r"a->dense = (kn\.compact && range <= DENSE_CAP);", "kn.compact && range <= DENSE_CAP"),
    ("int_build.hpp", r"a->bits = (bits_for\(sigma \+ 1\));", "bits_for(sigma + 1)"),
    ("int_build.hpp", r"a->bits = (bits_for\(range \+ 1\));", "bits_for(range + 1)"),
    ("int_build.hpp", r"(int s = 64 / a->bits);", "int s = 64 / a->bits"),
    ("int_build.hpp", r"return (kn\.bytes && a\.dense && a\.sigma <= 256 && n <= 0xFFFFFFFEull);",
     "kn.bytes && a.dense && a.sigma <= 256 && n <= 0xFFFFFFFEull"),
    ("int_build.hpp", r"\*key_bits = (a\.bits \* a\.s);", "a.bits * a.s"),
    ("int_build.hpp", r"\*h0 = (\(u64\)a\.s);", "(u64)a.s"),
    ("int_build.hpp", r"int_first_bad_kernel<S>\), dim3\((stream_grid\(n, 256 \* 16\))\), dim3\(256\)", "stream_grid(n, 256 * 16)"),
    ("int_build.hpp", r"nparts = (\(range \+ big::SC_TILE - 1\) / big::SC_TILE);", "(range + big::SC_TILE - 1) / big::SC_TILE"),
    ("big_build.hpp", r"constexpr u32 SC_BLOCK = (\d+), SC_ITEMS = \d+, SC_TILE = SC_BLOCK \* SC_ITEMS;", "1024"),
    ("big_build.hpp", r"constexpr u32 SC_BLOCK = \d+, SC_ITEMS = (\d+), SC_TILE = SC_BLOCK \* SC_ITEMS;", "8"),
    ("big_build.hpp", r"for \(u64 base = 0; base < nparts; base \+= (SC_BLOCK)\)", "SC_BLOCK"),
    ("big_build.hpp", r"constexpr int BG_BLOCK = (\d+);", "512"),
    ("big_build.hpp", r"constexpr int BG_ITEMS = (\d+);", "16"),
    ("big_build.hpp", r"constexpr u32 BG_TILE = (BG_BLOCK \* BG_ITEMS);", "BG_BLOCK * BG_ITEMS"),
    ("big_build.hpp", r"(const int rbits = bits_for\(n \+ 2\));", "const int rbits = bits_for(n + 2)"),
    ("big_build.hpp", r"sort_pairs\(gk, p1, k1, pfree, M, (bits_for\(G \+ 1\)),", "bits_for(G + 1)"),
    ("big_build.hpp", r"for \(int shift = 0; shift < bits; shift \+= (8)\)", "8"),
    ("big_build.hpp", r"for \(u64 h = h0; M > 0; (h \*= 2)\)", "h *= 2"),
    ("sa_build.hpp", r"if \(g > (256u \* 8u)\) g = 256u \* 8u;", "256u * 8u"),
    ("common.hpp", r"(while \(b < 64 && \(1ull << b\) < count\) \+\+b;)", "while (b < 64 && (1ull << b) < count) ++b;"),
]

# the diagnostic switches of int_build.hpp (Knobs::read), by the name the tests give a plan
PLANS = {
    "default": {},
    "no_bytes": {"SA_HIP_INT_BYTES": "0"},
    "raw_codes": {"SA_HIP_INT_COMPACT": "0"},
    "keys4": {"SA_HIP_INT_BYTES": "0", "SA_HIP_INT_KEY_SYMBOLS": "4"},
    "keys1": {"SA_HIP_INT_KEY_SYMBOLS": "1"},
}
KNOB_ENV = ("SA_HIP_INT_BYTES", "SA_HIP_INT_COMPACT", "SA_HIP_INT_KEY_SYMBOLS")


def knobs(plan_name):
    env = PLANS[plan_name]
    return dict(bytes=env.get("SA_HIP_INT_BYTES", "1") != "0", compact=env.get("SA_HIP_INT_COMPACT", "1") != "0",
                key_symbols=int(env.get("SA_HIP_INT_KEY_SYMBOLS", "64")))


def bits_for(count):
    """smallest b with 2^b >= count (csrc/common.hpp)"""
    return 0 if count <= 1 else int(count - 1).bit_length()


def stream_grid(work_items, per_block):
    """workgroups of a streaming launch (csrc/sa_build.hpp): one per per_block items, at most GRID_CAP, at least one"""
    return max(1, min(GRID_CAP, -(-int(work_items) // per_block)))


def first_bad_stride(n):
    """positions this far apart are looked at by the same thread of int_first_bad_kernel"""
    return stream_grid(n, FIRST_BAD_PER_BLOCK) * 256


# ---- the models -------------------------------------------------------------------------------------------------------------

def plan(t, kn):
    """What the alphabet pass decides for the text t (n >= 2) under the knobs kn, from int_build.hpp's header comment: dense
    codes 1 + rank iff compaction is on and max + 1 <= 2^24, else raw codes v + 1; b bits hold the largest code; s symbols
    per key; route A (bytes) iff allowed, dense and sigma <= 256."""
    t = np.asarray(t)
    n = int(t.size)
    mn, mx = int(t.min()), int(t.max())
    compacted = bool(kn["compact"]) and mx + 1 <= DENSE_CAP
    sigma = int(np.unique(t).size) if compacted else 0
    b = max(1, bits_for(sigma + 1) if compacted else bits_for(mx + 2))
    s = max(1, min(64 // b, int(kn["key_symbols"]), n))
    route = "A" if (kn["bytes"] and compacted and sigma <= 256 and n <= 0xFFFFFFFE) else "B"
    return dict(min=mn, max=mx, compacted=int(compacted), sigma=sigma, route=route, bits=b, s=s)


def codes(t, p):
    """the code of every position as Python ints: 1 + rank (dense) or v + 1 (raw); 0 is kept for 'past the end'"""
    t = np.asarray(t)
    if p["compacted"]:
        return [int(x) + 1 for x in np.unique(t, return_inverse=True)[1].reshape(-1)]
    return [int(x) + 1 for x in t]


def keys(t, p, zero_last_code_at=()):
    """key[i] = the codes of t[i .. i + s), most significant first, b bits each, 0 past the end: np.uint64[n].
    zero_last_code_at: positions whose key loses its last code (reads 0 there) -- what a keygen tile sees whose halo is one
    code short; used by the CPU test to show that a case depends on that code."""
    c = codes(t, p)
    n, b, s = len(c), p["bits"], p["s"]
    assert b * s <= 64
    lose = set(int(x) for x in zero_last_code_at)
    out = np.zeros(n, np.uint64)
    for i in range(n):
        key = 0
        for j in range(s):
            x = c[i + j] if i + j < n else 0
            if j == s - 1 and i in lose:
                x = 0
            key = (key << b) | x
        assert key < 1 << 64
        out[i] = np.uint64(key)
    return out


def tied_of_keys(k):
    """number of keys that are not unique"""
    cnt = np.unique(k, return_counts=True)[1]
    return int(cnt[cnt > 1].sum())


def neighbour_lcp(t, sa):
    """lcp[r] = number of symbols the suffixes sa[r - 1] and sa[r] share (compared symbol by symbol), r in [1, n);
    lcp[0] = lcp[n] = 0: int64[n + 1]"""
    t = np.asarray(t, np.int64)
    sa = np.asarray(sa, np.int64)
    n = int(t.size)
    lcp = np.zeros(n + 1, np.int64)
    r, a, b = np.arange(1, n), sa[:-1].copy(), sa[1:].copy()
    while r.size:
        ok = (a < n) & (b < n)
        r, a, b = r[ok], a[ok], b[ok]
        eq = t[a] == t[b]
        r, a, b = r[eq], a[eq] + 1, b[eq] + 1
        lcp[r] += 1
    return lcp


def tied(lcp, d):
    """ranks whose suffix shares at least d symbols with a neighbour in rank"""
    return int((np.maximum(lcp[:-1], lcp[1:]) >= d).sum())


def groups(lcp, d):
    """maximal runs of ranks whose suffixes share their first d symbols (runs of two and more)"""
    x = lcp[1:-1] >= d
    return int(x[0]) + int((x[1:] & ~x[:-1]).sum()) if x.size else 0


def rounds_model(t, sa, p):
    """What BigBuilder::build_with does with keys of s symbols, from its header comment: the initial sort over b * s bits
    leaves the suffixes grouped by their first s symbols (a suffix shorter than that is alone: its padding is code 0); the
    round at depth h sorts the tied records by the rank of suffix + h (bits_for(n + 2) bits) and by group id
    (bits_for(groups + 1) bits), one 8-bit digit a pass, and leaves them grouped by their first 2 h symbols."""
    n = int(np.asarray(t).size)
    lcp = neighbour_lcp(t, sa)
    b, s = p["bits"], p["s"]
    out = dict(tied_after_sort=tied(lcp, s), rounds=0, tied_total=0, sort_passes=-(-b * s // 8), depths=[])
    d = s
    while True:
        m = tied(lcp, d)
        if m == 0:
            return out
        g = groups(lcp, d)
        out["rounds"] += 1
        out["tied_total"] += m
        out["sort_passes"] += -(-bits_for(n + 2) // 8) + -(-bits_for(g + 1) // 8)
        out["depths"].append((d, m, g))
        d *= 2


# ---- the texts --------------------------------------------------------------------------------------------------------------

# (b, s, route, compacted) per plan; meta: whatever the CPU test needs to show that the case is on its edge
Case = namedtuple("Case", "name family text k dtypes expect meta")
BOTH, LONG = (np.int32, np.int64), (np.int64,)

# bits of the dense code (1 + rank, 0 past the end) by the number of distinct symbols, written out
DENSE_BITS = {1: 1, 2: 2, 3: 2, 4: 3, 5: 3, 6: 3, 7: 3, 8: 4, 10: 4, 15: 4, 16: 5, 255: 8, 256: 9, 257: 9, 300: 9, 1000: 10,
              65535: 16, 65536: 17, 2 ** 21 - 1: 21, 2 ** 21: 22}
HALO_N = 3 * KG_TILE + 70


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def sample_all(rng, values, n):
    """n symbols drawn from values, every value at least once"""
    values = np.asarray(values, np.int64)
    assert n >= values.size
    t = np.concatenate([values, rng.choice(values, n - values.size)])
    rng.shuffle(t)
    return t


def plant(t, A, B, L, values):
    """t[B : B + L] = t[A : A + L] in place; the symbols before and behind the copy at B are changed where they would extend
    the match (only positions B - 1 and B + L are written besides the copy)"""
    values = np.asarray(values, np.int64)
    n = int(t.size)
    assert 1 <= A and A + L <= B - 1 and B + L < n and values.size >= 2
    t[B:B + L] = t[A:A + L]
    for x, y in ((B - 1, A - 1), (B + L, A + L)):
        if t[x] == t[y]:
            t[x] = values[(int(np.flatnonzero(values == t[x])[0]) + 1) % values.size]


def _halo_text(name, values, s, near):
    """Two planted pairs in a random text over values.  Copy A of the first pair starts on tile 0's last position (its key's
    last symbol is the last code of the halo), copy B on tile 1's; copy A of the second starts at 2048 - s + 1 (its key's last
    symbol is the first code of the halo), copy B at the same place of tile 2.  near = False: the copies share exactly s
    symbols (tied after the sort); True: exactly s - 1, the key's last symbol decides."""
    t = sample_all(_rng(name), values, HALO_N)
    L = s - 1 if near else s
    pairs = [(KG_TILE - 1, 2 * KG_TILE - 1), (KG_TILE - s + 1, 3 * KG_TILE - s + 1)]
    for A, B in pairs:
        plant(t, A, B, L, values)
    return t, pairs


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []

    def add(name, family, text, k, dtypes, expect, **meta):
        text = np.ascontiguousarray(text, dtype=np.int64)
        text.setflags(write=False)
        assert all(p in PLANS for p in expect)
        out.append(Case(name, family, text, int(k), dtypes, expect, meta))

    # -- n against the key: n below, on and above s
    for n in (2, 3, 63, 64, 65):
        add("key_equal_n%d" % n, "key", np.full(n, 5), 6, BOTH, {"no_bytes": (1, min(64, n), "B", 1)})
    for n in (31, 32, 33):
        add("key_sigma3_n%d" % n, "key", sample_all(_rng("key3_%d" % n), [0, 1, 2], n), 3, BOTH, {"no_bytes": (2, min(32, n), "B", 1)})

    # -- n against the keygen's tile of 2048 positions and its halo of s - 1 codes
    for s_ in (32, 7):
        for n in (2047, 2048, 2049, 2048 + s_ - 1, 2048 + s_, 4095, 4096, 4097, 3 * 2048 + 1):
            if s_ == 32:
                add("tile_sigma2_n%d" % n, "tile", sample_all(_rng("tile2_%d" % n), [0, 1], n), 2, BOTH,
                    {"no_bytes": (2, 32, "B", 1), "keys4": (2, 4, "B", 1), "default": (2, 32, "A", 1)})
            else:
                vals = np.arange(300) * 7 + 3                     # max 2096: raw codes take bits_for(2098) = 12 bits
                add("tile_sigma300_n%d" % n, "tile", sample_all(_rng("tile300_%d" % n), vals, n), 2097, BOTH,
                    {"default": (9, 7, "B", 1), "raw_codes": (12, 5, "B", 0), "keys1": (9, 1, "B", 1)})

    # -- a tie, or its absence, decided by a code of the halo
    for b, vals in ((10, np.arange(1000)), (2, np.arange(3))):
        s = 64 // b
        plans = {"default": (10, 6, "B", 1)} if b == 10 else {"no_bytes": (2, 32, "B", 1)}
        for near in (False, True):
            name = "halo_b%d_%s" % (b, "near" if near else "tied")
            t, pairs = _halo_text(name, vals, s, near)
            add(name, "halo", t, int(vals.max()) + 1, BOTH, plans, pairs=pairs, near=near)
    add("halo_b1_equal", "halo", np.full(HALO_N, 0), 1, BOTH, {"no_bytes": (1, 64, "B", 1)},
        pairs=[(KG_TILE - 1, 2 * KG_TILE - 1), (KG_TILE - 63, 3 * KG_TILE - 63)], near=None)

    # -- dense code width: sigma + 1 on both sides of a power of two; every value occurs
    for sigma in (1, 2, 3, 4, 7, 8, 15, 16, 255, 256, 257, 2 ** 16 - 1, 2 ** 16):
        b = DENSE_BITS[sigma]
        n = sigma + 70
        e = {"default": (b, 64 // b, "A", 1), "no_bytes": (b, 64 // b, "B", 1)} if sigma <= 256 else {"default": (b, 64 // b, "B", 1)}
        add("dense_sigma%d" % sigma, "dense", sample_all(_rng("dense%d" % sigma), np.arange(sigma), n), sigma, BOTH, e, sigma=sigma)
    for sigma, b, s in ((2 ** 21 - 1, 21, 3), (2 ** 21, 22, 2)):
        add("dense_sigma%d" % sigma, "dense", sample_all(_rng("dense%d" % sigma), np.arange(sigma), sigma + 2048), sigma, BOTH,
            {"default": (b, s, "B", 1)}, sigma=sigma)

    # -- raw code width: max + 2 on both sides of a power of two, the 64-bit-wide key, the ceilings of both symbol types
    def raw_text(name, mx, lo_vals=49):
        rng = _rng(name)
        vals = np.unique(np.concatenate([rng.integers(0, mx, lo_vals, dtype=np.int64), [0, mx]]))
        t = sample_all(rng, vals, 3000)
        plant(t, 100, 1500, 300, vals)
        t[7], t[8] = mx, mx                                        # the largest code in the key's upper half
        return t
    for name, mx, b, s in (("2p32m2", 2 ** 32 - 2, 32, 2), ("2p32m1", 2 ** 32 - 1, 33, 1), ("2p40", 2 ** 40, 41, 1),
                           ("2p62", 2 ** 62, 63, 1), ("2p63m2", 2 ** 63 - 2, 63, 1)):
        add("raw_max_" + name, "raw", raw_text("raw" + name, mx), mx + 1, LONG, {"default": (b, s, "B", 0)})
    for name, mx, b, s in (("2p24", 2 ** 24, 25, 2), ("2p31m2", 2 ** 31 - 2, 31, 2)):
        add("raw_max_" + name, "raw", raw_text("raw" + name, mx), mx + 1, BOTH, {"default": (b, s, "B", 0)})
    for mx, b, s in ((2, 2, 32), (3, 3, 21), (6, 3, 21), (7, 4, 16)):
        vals = np.arange(mx + 1)
        t = sample_all(_rng("rawsmall%d" % mx), vals, 3000)
        plant(t, 100, 1500, 300, vals)
        add("raw_small_max%d" % mx, "raw", t, mx + 1, BOTH, {"raw_codes": (b, s, "B", 0)})

    # -- the presence table and its scan: max + 1 at the scan's tile of 8192, beyond 1024 tiles, at the cap of the table
    for R in (8191, 8192, 8193, 16385, 2 ** 23, 2 ** 23 + 1, 2 ** 24, 2 ** 24 + 1):
        vals = np.unique([v for v in (0, 1, R // 2, R - 2, R - 1, SC_TILE - 1, SC_TILE) if v < R])
        t = sample_all(_rng("tables%d" % R), vals, 3000)
        plant(t, 100, 1500, 200, vals)
        if R <= DENSE_CAP:
            b = DENSE_BITS[vals.size]
            e = {"default": (b, 64 // b, "A", 1), "no_bytes": (b, 64 // b, "B", 1)}
        else:
            e = {"default": (25, 2, "B", 0)}
        add("tables_range%d" % R, "tables", t, R, BOTH, e, sigma=int(vals.size) if R <= DENSE_CAP else 0, parts=-(-R // SC_TILE))
    vals = np.arange(2 ** 24 - 10, 2 ** 24)
    t = sample_all(_rng("tables_high"), vals, 3000)
    plant(t, 100, 1500, 200, vals)
    add("tables_high_alphabet", "tables", t, 2 ** 24, BOTH, {"default": (4, 16, "A", 1), "no_bytes": (4, 16, "B", 1)}, sigma=10,
        parts=2048)
    add("tables_sigma256_n300", "tables", sample_all(_rng("t256"), np.arange(256), 300), 256, BOTH,
        {"default": (9, 7, "A", 1), "no_bytes": (9, 7, "B", 1)}, sigma=256, parts=1)
    add("tables_sigma257_n300", "tables", sample_all(_rng("t257"), np.arange(257), 300), 257, BOTH, {"default": (9, 7, "B", 1)},
        sigma=257, parts=1)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in all_cases() if c.name == name)


# one case per family for the host drop-ins
DROPIN_CASES = ("key_equal_n65", "tile_sigma300_n2049", "halo_b10_tied", "dense_sigma257", "raw_max_2p31m2", "tables_range8193")

# ---- refusals ---------------------------------------------------------------------------------------------------------------
Refusal = namedtuple("Refusal", "name text k dtypes")
REFUSAL_N, REFUSAL_K = 6200, 1000


def first_bad(t, k):
    """the smallest position whose symbol lies outside [0, k), or None"""
    bad = np.flatnonzero((np.asarray(t) < 0) | (np.asarray(t) >= k))
    return int(bad[0]) if bad.size else None


@functools.lru_cache(maxsize=None)
def refusal_cases():
    n, k = REFUSAL_N, REFUSAL_K
    base = np.random.default_rng(99).integers(0, k - 1, n)      # values 0 .. k - 2
    base[[4500, 300, 6000]] = k - 1                                # the largest symbol, three times
    stride = first_bad_stride(n)
    assert stride == 512 and 700 + 3 * stride < n
    out = [Refusal("k_is_max", base, k - 1, BOTH), Refusal("k_is_max_plus_1", base, k, BOTH)]
    edits = [("at_0", {0: -1}, BOTH), ("at_last", {n - 1: k}, BOTH), ("three", {4097: k, 5000: -5, n - 1: k + 7}, BOTH),
             ("negative_first", {1000: -3, 2000: k + 1}, BOTH), ("too_large_first", {1000: 5000, 2000: -1}, BOTH),
             ("same_thread", {700: -1, 700 + 3 * stride: 2000}, BOTH), ("same_thread_reverse", {700: 2 ** 31 - 1, 700 + stride: -2 ** 31}, BOTH),
             ("same_thread_and_an_earlier_thread", {700 + stride: k, 700 + 2 * stride: -1, 650 + stride: -9}, BOTH),
             ("beyond_int32", {123: 2 ** 40, 5: -2 ** 63}, LONG)]
    for name, ed, dtypes in edits:
        t = base.copy()
        for p, v in ed.items():
            t[p] = v
        out.append(Refusal(name, t, k, dtypes))
    for r in out:
        r.text.setflags(write=False)
    return tuple(out)
