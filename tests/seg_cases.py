"""Texts, model and expectations of the bucketed LSD sorts' tests (tests/test_gpu_seg.py); plain NumPy, no GPU.

csrc/radix_narrow.hpp (8-byte records: u32 narrow key + suffix) and csrc/radix_narrow48.hpp (10-byte records: u32 + u16 key
+ suffix) sort the top digit first and then run 256 LSD sorts side by side, one per top-digit bucket: seg_plan_kernel cuts
every bucket into tiles ("flat" tiles, bucket-major) and the flat range into NCHUNK ticket parts of whole buckets,
seg_hist_kernel counts the first digit per bucket, seg_onesweep_kernel / seg48_onesweep_kernel run one pass each with one
look-back chain per bucket.  Whole builds of random or word text give these kernels bucket sizes nobody chose.  Here the
bucket sizes are exact BY CONSTRUCTION:

  b = 8   128 .. 255 distinct bytes (byte = code): the top digit of a position is its symbol's code, a bucket's size is that
          symbol's count, the text is a seeded permutation of a prescribed multiset with the planted words written first;
  b = 5   the 27 symbols of refine_cases.D1_SYMBOLS plus reserved bytes (split_cases): the top digit is symbol 0 and the top
          three code bits of symbol 1; a reserved symbol occurs only in its plant, so its buckets hold the planted records
          and the buckets between them are empty.

plan(), bucket_of(), passes() restate the kernels' arithmetic; lsd_model() is one stable argsort of the sort keys;
stepwise_model() is the same sort done the way the device does it (top-digit pass by TEXT_TILE tiles, then pass by pass,
bucket by bucket, flat tile by flat tile with the digit bases of a per-bucket histogram) and takes the name of one
deliberate mistake.  tests/test_seg_cases_cpu.py holds every case against its claims, the two models against each other and
every mistake against lsd_model.  Everything takes a Geom: FULL is the device's geometry, SMALL the same divided by 128 (the
step-wise model runs there)."""
from collections import namedtuple
from math import gcd

import numpy as np

import split_cases as sc
from split_cases import codes_of, keys_of

# restated from the headers; (file under suffixarray_amd/csrc, regular expression whose group 1 is the value's definition, value)
SEG_ITEMS, SEG48_ITEMS, SPLIT_ITEMS, NCHUNK, RADIX_BITS, RADIX, INCL_MASK, TPB = 24, 14, 28, 8, 8, 256, 3, 4
TEXT_TILE = 512 * 16
NARROW_MIN_N = 1 << 22
N_MAX = (1 << 22) + (1 << 16)
HEADER_CONSTANTS = [
    ("radix_narrow.hpp", r"constexpr int SEG_ITEMS = (\d+);", "24"),
    ("radix_narrow48.hpp", r"#define SA_SEG48_ITEMS (\d+)", "14"),
    ("radix_narrow48.hpp", r"constexpr int SEG48_LAST_ITEMS = (SEG48_ITEMS);", "SEG48_ITEMS"),
    ("radix_sort.hpp", r"constexpr int NCHUNK = (\d+);", "8"),
    ("radix_sort.hpp", r"constexpr int RADIX_BITS = (\d+);", "8"),
    ("radix_sort.hpp", r"#define SA_INCL_MASK (\d+)u", "3"),
    ("radix_narrow.hpp", r"#define SA_TEXT_ITEMS (\d+)", "16"),
    ("radix_narrow.hpp", r"constexpr u32 TEXT_TILE = (512u \* TEXT_ITEMS);", "512u * TEXT_ITEMS"),
    ("radix_narrow.hpp", r"int split_items = (\d+);", "28"),
    ("radix_narrow.hpp", r"begin_bit >= 24 && begin_bit < 56 && n >= \(1u << (22)\)", "22"),
    ("radix_narrow48.hpp", r"begin_bit >= 8 && begin_bit < 24 && n >= \(1u << (22)\)", "22"),
    ("radix_narrow.hpp", r"const u32 tpb = (\d+);", "4"),            # (both launches of the header: split_hist_kernel, seg_hist_kernel)
    ("radix_narrow48.hpp", r"const u32 tpb = (\d+);", "4"),
    ("radix_narrow.hpp", r"if \(rest (>=) TILE\)\s+seg_tile<true", ">="),
    ("radix_narrow48.hpp", r"if \(rest (>=) TILE\)\s+seg48_tile<true", ">="),
    ("radix_narrow.hpp", r"const u32 target = \(u32\)\(\(\(u64\)F \* \(u32\)d\) (/) NCHUNK\);", "/"),
    ("radix_narrow.hpp", r"if \(s_tp\[mid\] (<) target\) lo = mid \+ 1; else hi = mid;", "<"),
    ("radix_narrow.hpp", r"if \(tprefix\[mid\] (<=) f\) lo = mid; else hi = mid;", "<="),
    ("radix_narrow48.hpp", r"const size_t off16 = (\(\(size_t\)n \* 4 \+ 63\) & ~\(size_t\)63);", "((size_t)n * 4 + 63) & ~(size_t)63"),
    ("radix_sort.hpp", r"max_tiles = div_up\(n_max \? n_max : 1, (256 \* SORT_ITEMS)\);", "256 * SORT_ITEMS"),
]
U64 = np.uint64

Geom = namedtuple("Geom", "n0 T8 T10 TS TT big copies")
FULL = Geom(NARROW_MIN_N, 512 * SEG_ITEMS, 512 * SEG48_ITEMS, 512 * SPLIT_ITEMS, TEXT_TILE, 16385, 300)
SMALL = Geom(NARROW_MIN_N >> 7, 4 * SEG_ITEMS, 4 * SEG48_ITEMS, 4 * SPLIT_ITEMS, TEXT_TILE >> 7, 129, 6)


# ---- the model --------------------------------------------------------------------------------------------------------------

def passes(b, k0, L=0):
    """What Builder::build and the two host drivers make of a key of k0 symbols of b bits (default switches, n >= 2^22):
    plan "narrow" (radix_sort_narrow) / "narrow48" (radix_sort_narrow48) / None, the characters and bits of the sort key
    (the 10-byte plan takes the top bits of one more character when L allows: Builder::build, partial_char), lo_bits /
    hi_bits, and every pass after the top-digit pass as (array, shift, mask)."""
    begin = 64 - b * k0
    out = {"b": b, "k0": k0, "plan": None, "chars": k0, "begin_bit": begin, "passes": []}
    if b <= 8 and 24 <= begin < 56:
        lo = 56 - begin
        np_ = -(-lo // RADIX_BITS)
        out.update(plan="narrow", lo_bits=lo, hi_bits=0, bits=8 + lo,
                   passes=[("k32", RADIX_BITS * p, (1 << (lo - RADIX_BITS * p if p == np_ - 1 else RADIX_BITS)) - 1) for p in range(np_)])
    elif b <= 8 and 8 <= begin < 24:
        if b * k0 < 56 and b * (k0 + 1) > 56 and (L == 0 or k0 + 1 <= L):
            out.update(chars=k0 + 1, begin_bit=8)
            begin = 8
        rem = 56 - begin
        hi = rem - 16
        np_hi = -(-hi // RADIX_BITS)
        ps = [("k16", 0, 255), ("k16", 8, 255)]
        ps += [("k32", RADIX_BITS * q, (1 << (hi - RADIX_BITS * q if q == np_hi - 1 else RADIX_BITS)) - 1) for q in range(np_hi)]
        out.update(plan="narrow48", lo_bits=16, hi_bits=hi, np_hi=np_hi, bits=8 + rem, passes=ps)
    return out


def sort_keys(t, spec, halo_tile=None):
    """The key the plan sorts by, right-aligned in spec["bits"] bits (its top 8 bits are the top digit): the first spec["chars"]
    symbols, cut to 56 bits.  halo_tile (a deliberate mistake): the symbols behind the position's tile of halo_tile positions
    read as 0, as if the top-digit pass staged no halo."""
    b, k = spec["b"], spec["chars"]
    c = np.concatenate([codes_of(t)[0], np.zeros(k, U64)])
    pos = np.arange(t.size)
    key = np.zeros(t.size, U64)
    for j in range(k):
        cj = c[j:j + t.size]
        if halo_tile is not None:
            cj = np.where((pos + j) // halo_tile == pos // halo_tile, cj, U64(0))
        key = (key << U64(b)) | cj
    return key >> U64(b * k - spec["bits"])


def top_digit(t, b, k0):
    """the top 8 key bits of every position: its first ceil(8 / b) symbols (k0 at least that many)"""
    c8 = -(-8 // b)
    assert k0 >= c8
    return (keys_of(t, c8)[0] >> U64(c8 * b - 8)).astype(np.int64)


Plan = namedtuple("Plan", "bstart tprefix cfirst")


def plan(sizes, tile, round_down=False):
    """seg_plan_kernel: bstart / tprefix = exclusive sums of the bucket sizes / of ceil(size / tile), [256] = the totals;
    cfirst[c] = tprefix of the FIRST bucket whose first tile lies at or beyond F * c / 8 (integer division), cfirst[8] = F.
    round_down (a deliberate mistake): the LAST bucket whose first tile lies at or before the target."""
    sizes = np.asarray(sizes, np.int64)
    assert sizes.size == RADIX
    tiles = -(-sizes // tile)
    bstart = np.concatenate([[0], np.cumsum(sizes)])
    tprefix = np.concatenate([[0], np.cumsum(tiles)])
    F = int(tprefix[RADIX])
    cfirst = []
    for d in range(NCHUNK + 1):
        target = F * d // NCHUNK
        if round_down:
            lo = max(b for b in range(RADIX + 1) if tprefix[b] <= target)
        else:
            lo, hi = 0, RADIX
            while lo < hi:
                mid = (lo + hi) >> 1
                if tprefix[mid] < target:
                    lo = mid + 1
                else:
                    hi = mid
        cfirst.append(F if d == NCHUNK else int(tprefix[lo]))
    return Plan(bstart, tprefix, np.array(cfirst, np.int64))


def bucket_of(tprefix, f, strict=False):
    """seg_bucket_of: eight bisection steps to the last b with tprefix[b] <= f.  strict (a deliberate mistake): < for <=."""
    lo, hi = 0, RADIX
    for _ in range(RADIX_BITS):
        mid = (lo + hi) >> 1
        if (tprefix[mid] < f) if strict else (tprefix[mid] <= f):
            lo = mid
        else:
            hi = mid
    return lo


def flat_tiles(pl, tile, strict=False):
    """every flat tile as the pass kernels see it: (bucket, first record, records; 0: nothing of its bucket is left there)"""
    F = int(pl.tprefix[RADIX])
    bucket = np.array([bucket_of(pl.tprefix, f, strict) for f in range(F)], np.int64)
    start = pl.bstart[bucket] + (np.arange(F) - pl.tprefix[bucket]) * tile
    rest = pl.bstart[bucket + 1] - start
    return bucket, start, np.clip(rest, 0, tile)


def lsd_model(keys):
    """the whole sort: one stable argsort of the sort keys -- ties stay in text order"""
    return np.argsort(keys, kind="stable")


WRONG = ("unstable", "padding", "bucket_of", "mask", "halo", "swap")   # (the seventh, cfirst rounded down, is plan(round_down=True))


def stepwise_model(t, spec, geom, wrong=None):
    """The sort as the device does it -> the suffix order.  Top-digit pass: keys made per TEXT_TILE tile, stable by the top 8
    bits.  Then every pass of spec["passes"]: per bucket the records of its flat tiles (flat_tiles), a histogram of the pass's
    digit, the digit bases bstart[b] + exclusive sum, every record to base[digit] + its rank among the records of that digit
    before it.  wrong: one of WRONG --
      unstable   pass 0 ranks the records of a digit run in reverse
      padding    the padding of a bucket's partial tile is counted and stored as records of the highest digit
      bucket_of  seg_bucket_of compares with < instead of <=
      mask       the last pass ranks with a mask one bit wider than the histogram it was given
      halo       the top-digit pass reads no symbols behind its tile's edge
      swap       the 10-byte plan's passes 2.. still rank by k16"""
    n = int(t.size)
    key = sort_keys(t, spec, geom.TT if wrong == "halo" else None)
    top = (key >> U64(spec["bits"] - 8)).astype(np.uint8)
    vals = np.argsort(top, kind="stable")
    key = key[vals]
    arrays = {"k32": ((key >> U64(16 if spec["plan"] == "narrow48" else 0)) & U64(0xFFFFFFFF)).astype(np.int64),
              "k16": (key & U64(0xFFFF)).astype(np.int64)}
    tile = geom.T8 if spec["plan"] == "narrow" else geom.T10
    pl = plan(np.bincount(top, minlength=RADIX), tile)
    tb, tstart, tn = flat_tiles(pl, tile, strict=(wrong == "bucket_of"))
    last = len(spec["passes"]) - 1
    for pi, (arr, shift, mask) in enumerate(spec["passes"]):
        if wrong == "swap" and pi >= 2:
            arr = "k16"
        smask = 2 * mask + 1 if (wrong == "mask" and pi == last) else mask
        out = {k: np.full(n, -1, np.int64) for k in arrays}
        vout = np.full(n, n, np.int64)
        clobber = []
        for bkt in np.unique(tb):
            fl = np.flatnonzero(tb == bkt)
            idx = np.concatenate([np.arange(tstart[f], tstart[f] + tn[f]) for f in fl])
            if idx.size == 0:
                continue
            d_h = (arrays[arr][idx] >> shift) & mask
            d_s = (arrays[arr][idx] >> shift) & smask
            hist = np.bincount(d_h, minlength=2 * RADIX)
            base = pl.bstart[bkt] + np.concatenate([[0], np.cumsum(hist)])[:-1]
            o = np.argsort(d_s, kind="stable")
            sd = d_s[o]
            if wrong == "unstable" and pi == 0:
                rank = np.searchsorted(sd, sd, side="right") - 1 - np.arange(sd.size)
            else:
                rank = np.arange(sd.size) - np.searchsorted(sd, sd, side="left")
            dest = np.empty(idx.size, np.int64)
            dest[o] = base[sd] + rank
            ok = dest < n
            for k in arrays:
                out[k][dest[ok]] = arrays[k][idx[ok]]
            vout[dest[ok]] = vals[idx[ok]]
            if wrong == "padding":
                pads = int(fl.size * tile - idx.size)
                first = int(base[mask] + hist[mask])
                clobber.append(np.arange(first, min(first + pads, n)))
        for c in clobber:
            vout[c] = n
        arrays, vals = out, vout
    return vals


def mismatch(got, exp, pl, tile):
    """None where the arrays are equal, else the first differing slot with its bucket, its flat tile and that tile's kind"""
    if got.shape == exp.shape and np.array_equal(got, exp):
        return None
    if got.shape != exp.shape:
        return "shape %s, expected %s" % (got.shape, exp.shape)
    bad = np.flatnonzero(got != exp)
    slot = int(bad[0])
    b = int(np.searchsorted(pl.bstart, slot, side="right") - 1)
    j = (slot - int(pl.bstart[b])) // tile
    left = int(pl.bstart[b + 1]) - (int(pl.bstart[b]) + j * tile)
    return "first differing slot %d (bucket %d, its tile %d = flat tile %d of %d, %s): got %d, expected %d; %d of %d slots differ" % (
        slot, b, j, int(pl.tprefix[b]) + j, int(pl.tprefix[RADIX]), "full" if left >= tile else "partial, %d records" % left,
        int(got[slot]), int(exp[slot]), bad.size, exp.size)


# ---- texts ------------------------------------------------------------------------------------------------------------------

Text = namedtuple("Text", "t b sigma info")


def _r(geom, r):
    """the text length's remainder r of the full geometry, scaled"""
    return r * geom.n0 >> 22


def spread(total, k):
    q, r = divmod(total, k)
    assert q >= 1
    return [q + (i < r) for i in range(k)]


def multiset_text(sizes, seed, plants=(), clean_from=None, clean=()):
    """b = 8: the text in which code c (the byte c) occurs exactly sizes[c - 1] times.  plants [(position, codes)] are written
    first, the rest of the multiset fills the free positions in a seeded random order.  clean_from / clean: the free positions
    from clean_from on hold none of the codes in clean (swapped with free positions before it)."""
    sizes = np.asarray(sizes, np.int64)
    n, sigma = int(sizes.sum()), sizes.size
    assert 128 <= sigma <= 255 and sizes.min() >= 1
    rng = np.random.default_rng(seed)
    t = np.zeros(n, np.uint8)
    left = sizes.copy()
    for pos, w in plants:
        w = np.asarray(w, np.uint8)
        assert pos >= 0 and pos + w.size <= n and not t[pos:pos + w.size].any()
        t[pos:pos + w.size] = w
        left -= np.bincount(w, minlength=sigma + 1)[1:]
    assert left.min() >= 0, "a planted symbol occurs more often than its bucket holds"
    free = np.flatnonzero(t == 0)
    fill = np.repeat(np.arange(1, sigma + 1, dtype=np.uint8), left)
    rng.shuffle(fill)
    if clean_from is not None:
        late = np.flatnonzero((free >= clean_from) & np.isin(fill, clean))
        early = np.flatnonzero((free < clean_from) & ~np.isin(fill, clean))[:late.size]
        fill[late], fill[early] = fill[early].copy(), fill[late].copy()
    t[free] = fill
    return t


def edge_list(T):
    return [T - 1, T, T + 1, 2 * T, 2 * T + 1, 4 * T, 4 * T + 1, 5 * T - 1]


SMALL_BUCKETS = [1, 1, 1, 1, 63, 64, 65]


def tile_sizes(geom, plan_):
    """the prescribed bucket sizes of the tile_edges texts, in bucket order"""
    T = geom.T8 if plan_ == 8 else geom.T10
    return SMALL_BUCKETS + edge_list(T) + (edge_list(geom.TS) if plan_ == 8 else [])


def t_tile_edges(geom, plan_):
    """b = 8, sigma 200: the codes 1.. hold tile_sizes(), the rest of the text is spread over the other codes"""
    n = geom.n0 + _r(geom, 1 if plan_ == 8 else 3)
    sizes = tile_sizes(geom, plan_)
    t = multiset_text(sizes + spread(n - sum(sizes), 200 - len(sizes)), 11 + plan_)
    return Text(t, 8, 200, {"buckets": {c + 1: s for c, s in enumerate(sizes)}})


def t_tile_edges5(geom, plan_):
    """b = 5, sigma 31: the buckets (R_i, g), i = 1..4, g = 1..7 -- reserved symbol i followed by an ordinary symbol whose code
    is 4 g .. 4 g + 3 -- hold tile_sizes() in bucket order; (R_i, 0) is empty: the codes 0..3 follow no reserved symbol"""
    n = geom.n0 + _r(geom, 1 if plan_ == 8 else 3)
    A = sc.alphabet(sc.RES_LO)
    o = sc.ordinary_codes(A)
    rng = np.random.default_rng(105 + plan_)
    sizes = tile_sizes(geom, plan_)
    slots = [(r, g) for r in (1, 2, 3, 4) for g in range(1, 8)]
    plants, buckets = [], {}
    for (r, g), s in zip(slots, sizes):
        plants.append(sc.free_plant(A, (r,), s, 1, rng, second=[c for c in range(4 * g, 4 * g + 4) if c in o]))
        buckets[(r << 3) | g] = s
    for r, g in slots[len(sizes):]:        # every reserved symbol occurs: sigma = 31
        if not any(rr == r for rr, _ in slots[:len(sizes)]):
            plants.append(sc.free_plant(A, (r,), 1, 1, rng, second=[c for c in range(4 * g, 4 * g + 4) if c in o]))
            buckets[(r << 3) | g] = 1
            break
    t, _ = sc.plant_text(n, 5 + plan_, plants)
    return Text(t, 5, 31, {"buckets": buckets})


def t_one_bucket(geom, high):
    """b = 8: one symbol holds 15/16 of the text, every other symbol one tile.  low: sigma 128, code 3; high: sigma 255, code
    255 -- bucket 255 in use.  (More than 7/8 of all TILES is out of reach in this family: 127 other symbols are 127 tiles, the
    large bucket would need 889 tiles, the longest text allowed has 594 of 7168 records.  7/8 of the records it is.)"""
    n = geom.n0 + _r(geom, 15)
    sigma, big = (255, 255) if high else (128, 3)
    small = (n // 16) // (sigma - 1)
    sizes = [small] * sigma
    sizes[big - 1] = n - small * (sigma - 1)
    return Text(multiset_text(sizes, 21 + high), 8, sigma, {"big": big, "small": small})


def _lcm(*xs):
    out = 1
    for x in xs:
        out = out * x // gcd(out, x)
    return out


def t_part_starts(geom, shifted):
    """b = 8, sigma 128: eight buckets of 6 lcm(tiles) records -- whole tiles of the 8-byte, the 10-byte and the split pass's
    plan alike -- each followed by 15 tiny buckets of one tile: F = 8 (m + 15) and F c / 8 is the first tile of the c-th large
    bucket.  shifted: the first group has 14 tiny buckets, the last 16 -- every target lies one tile inside a large bucket."""
    n = geom.n0 + _r(geom, 8191)
    big = 6 * _lcm(geom.T8, geom.T10, geom.TS)
    tiny = spread(n - 8 * big, 120)
    assert max(tiny) <= min(geom.T8, geom.T10)
    groups = [14] + [15] * 6 + [16] if shifted else [15] * 8
    sizes, bigs = [], []
    for g in groups:
        bigs.append(len(sizes) + 1)
        sizes += [big] + [tiny.pop() for _ in range(g)]
    return Text(multiset_text(sizes, 31 + shifted), 8, 128, {"bigs": bigs, "big": big})


def t_empties(geom):
    """b = 5, sigma 29 (two reserved bytes): R1 occurs once, followed by code 3 (bucket 8: one record), R2 once, followed by a
    code >= 28 (bucket 23: one record): the buckets 9..22 between them are empty, 0..7 before them (code 0 starts no key) and
    240..255 behind the last used one (the codes 30, 31 do not occur)"""
    A = sc.alphabet(sc.RES_LO[:2])
    rng = np.random.default_rng(141)
    plants = [sc.free_plant(A, (1,), 1, 7, rng, second=[3]), sc.free_plant(A, (2,), 1, 7, rng, second=[28, 29])]
    t, _ = sc.plant_text(geom.n0, 41, plants)
    return Text(t, 5, 29, {"ones": [8, 23], "run": (9, 22), "leading": 8, "trailing": 16})


PAD_X, PAD_Y, PAD_RUN = 100, 101, 8


def t_padding(geom, plan_):
    """b = 8, sigma 255: the words X 255^8 and Y 255^8, three times each; the last X and the last Y of the text are planted
    ones.  With keys of 5 (8-byte plan) or 7 (10-byte plan) symbols the planted X and Y positions carry all-ones narrow keys,
    the padding value, and in the top-digit order they are their buckets' last records: the last tile of bucket X holds
    tile_n = 1 mod 64 records, that of bucket Y 63 mod 64."""
    T = geom.T8 if plan_ == 8 else geom.T10
    n = geom.n0 + _r(geom, 3)
    half = (T // 64 // 2) * 64
    sizes = spread(n - (3 * T + 2 * half + 64), 253)
    sizes = sizes[:PAD_X - 1] + [2 * T + half + 1, T + half + 63] + sizes[PAD_X - 1:]
    w = lambda c: [c] + [255] * PAD_RUN
    plants = [(n // 4, w(PAD_X)), (n // 4 + 64, w(PAD_Y)), (n // 2, w(PAD_X)), (n // 2 + 64, w(PAD_Y)), (n - 40, w(PAD_X)), (n - 20, w(PAD_Y))]
    t = multiset_text(sizes, 51 + plan_, plants, clean_from=n - 40, clean=(PAD_X, PAD_Y))
    return Text(t, 8, 255, {"X": PAD_X, "Y": PAD_Y, "plants": {PAD_X: [p for p, x in plants if x[0] == PAD_X], PAD_Y: [p for p, x in plants if x[0] == PAD_Y]}})


TIE_WORDS = [list(range(50, 58)), list(range(60, 68)), list(range(70, 78)), list(range(80, 88))]   # eight symbols each: >= k0 for every plan


def t_ties(geom):
    """b = 8, sigma 200: four words of eight symbols; the first planted geom.big times (16385: no level of the three-pass plan
    fits the group), the others geom.copies times, one word per cell of 16 positions, the cells drawn from the whole text.  The
    words' first symbols have buckets of more than three tiles."""
    n = geom.n0 + _r(geom, 15)
    counts = [geom.big] + [geom.copies] * 3
    rng = np.random.default_rng(61)
    cells = np.sort(rng.choice(n // 16 - 1, sum(counts), replace=False))
    which = rng.permutation(np.repeat(np.arange(4), counts))
    at = cells * 16 + rng.integers(0, 8, cells.size)
    plants = [(int(p), TIE_WORDS[w]) for p, w in zip(at, which)]
    firsts = [w[0] for w in TIE_WORDS]
    rest = spread(n - 4 * (3 * geom.T8 + geom.big + 5), 196)
    sizes = [3 * geom.T8 + geom.big + 5 if c in firsts else rest.pop() for c in range(1, 201)]
    t = multiset_text(sizes, 62, plants)
    return Text(t, 8, 200, {"pos": [np.sort(at[which == w]) for w in range(4)], "counts": counts})


def t_ties5(geom):
    """b = 5, sigma 27: four words of twelve ordinary symbols (as long as the longest key, the partial character included),
    planted like those of t_ties by split_cases.plant_text: rows in one random order, random gaps"""
    n = geom.n0 + _r(geom, 15)
    rng = np.random.default_rng(161)
    counts = [geom.big] + [geom.copies] * 3
    words = [sc.D1_SYMBOLS[rng.integers(0, sc.D1_SYMBOLS.size, 12)] for _ in counts]
    t, pos = sc.plant_text(n, 81, [np.tile(w, (c, 1)) for w, c in zip(words, counts)])
    return Text(t, 5, 27, {"pos": [np.sort(p) for p in pos], "counts": counts})


EDGE_WORD = list(range(150, 164))   # 14 symbols


def t_text_edges(geom):
    """b = 8, sigma 200: the word EDGE_WORD starts j = 1 + (i - 1) mod 6 positions before the i-th multiple of TEXT_TILE, so 1 ..
    k0 - 1 of its symbols lie before every kind of edge (k0 <= 7); the text has TEXT_TILE - 1 positions behind the last edge and
    ends in the word's first three symbols: the keys of the last k0 - 1 positions end in code 0"""
    n = geom.n0 + _r(geom, 8191)
    edges = np.arange(1, (n - 1) // geom.TT + 1) * geom.TT
    plants = [(int(e) - 1 - (i % 6), EDGE_WORD) for i, e in enumerate(edges)] + [(n - 3, EDGE_WORD[:3])]
    rest = spread(n - 14 * (edges.size + 100), 186)
    sizes = [edges.size + 100 if c in EDGE_WORD else rest.pop() for c in range(1, 201)]
    return Text(multiset_text(sizes, 71, plants), 8, 200, {"edges": edges, "starts": np.array([p for p, _ in plants[:-1]])})


TEXTS = {
    "tile_edges_8": (t_tile_edges, (8,)), "tile_edges_10": (t_tile_edges, (10,)),
    "tile_edges5_8": (t_tile_edges5, (8,)), "tile_edges5_10": (t_tile_edges5, (10,)),
    "one_bucket_low": (t_one_bucket, (0,)), "one_bucket_high": (t_one_bucket, (1,)),
    "part_starts": (t_part_starts, (0,)), "part_starts_shifted": (t_part_starts, (1,)),
    "empties": (t_empties, ()),
    "padding_keys_8": (t_padding, (8,)), "padding_keys_10": (t_padding, (10,)),
    "ties": (t_ties, ()), "ties5": (t_ties5, ()),
    "text_edges": (t_text_edges, ()),
}


def make(name, geom=FULL):
    f, args = TEXTS[name]
    return f(geom, *args)


# ---- the cases --------------------------------------------------------------------------------------------------------------
# FORMS: name -> (plan, switches, what BuildStats must show).  The 8-byte plan's forms all carry SA_HIP_SPLIT=0 except
# "declined": SA_HIP_NARROW_K=0 would keep the three-pass plan out by itself, SA_HIP_TEXT_PASS=0 would not -- near-random text
# would take it and the LSD passes would not run.
FORMS = {
    "split=0": (8, {"SA_HIP_SPLIT": "0"}, dict(narrow48=0, narrow_k=1, text_top_pass=1, split_plan=0, top=1)),
    "declined": (8, {}, dict(narrow48=0, narrow_k=1, text_top_pass=1, split_plan=0, top=2)),
    "narrow_k=0": (8, {"SA_HIP_SPLIT": "0", "SA_HIP_NARROW_K": "0"}, dict(narrow48=0, narrow_k=0, text_top_pass=1, split_plan=0, top=1)),
    "text_pass=0": (8, {"SA_HIP_SPLIT": "0", "SA_HIP_TEXT_PASS": "0"}, dict(narrow48=0, narrow_k=1, text_top_pass=0, split_plan=0, top=1)),
    "default": (10, {}, dict(narrow48=1, narrow_k=0, text_top_pass=1, split_plan=0, top=1)),
    # the control: the same text and key length on 12-byte records (radix_sort_pairs), compared with the same model
    "12-byte": (12, {"SA_HIP_NARROW48": "0"}, dict(narrow48=0, narrow_k=0, text_top_pass=1, split_plan=0, top=None)),
}
SWITCHES = ("SA_HIP_SPLIT", "SA_HIP_INITIAL_CHARS", "SA_HIP_NARROW_K", "SA_HIP_TEXT_PASS", "SA_HIP_NARROW48", "SA_HIP_NARROW", "SA_HIP_TOP_CLAIMS",
            "SA_HIP_FUSE_HIST", "SA_HIP_FUSE_DIR", "SA_HIP_PARTIAL_CHAR", "SA_HIP_WIDE_TEXT_PASS", "SA_HIP_SPLIT_ITEMS", "SA_HIP_DIR_BITS",
            "SA_HIP_LITE_FLAGS", "SA_HIP_SORT_BLOCK", "SA_HIP_LOCAL_BIG", "SA_HIP_SPLIT_CAP", "SA_HIP_SECTOR_SEARCH")

# Case: text, case number of the issue's list, runs [(form, key lengths)], the run that also asks for the int64 array, claims.
# The b = 5 key lengths run on the b = 5 texts (the b = 5 variants of tile_edges and ties, and empties); padding_keys needs 32
# narrow or high bits of all ones (k0 = 5 / 7 at b = 8 only); the declined form needs the group of 16385 equal keys (ties only)
# and 32 narrow bits.
Case = namedtuple("Case", "text number runs sa64 claim")
K8, K5, K10, K10_5 = (5, 3, 2), (8, 7, 5), (6, 7), (11, 9)
CASES = {
    "tile_edges_8": Case("tile_edges_8", 1, [("split=0", K8), ("narrow_k=0", (5,)), ("text_pass=0", (5,))], ("split=0", 5),
                         dict(chains=[1, 1, 2, 2, 3, 4, 5, 5], tails=[12287, 0, 1, 0, 1, 0, 1, 12287])),
    "tile_edges_10": Case("tile_edges_10", 1, [("default", K10), ("12-byte", (7,))], ("default", 7),
                          dict(chains=[1, 1, 2, 2, 3, 4, 5, 5], tails=[7167, 0, 1, 0, 1, 0, 1, 7167])),
    "tile_edges5_8": Case("tile_edges5_8", 1, [("split=0", K5)], None, dict(chains=[1, 1, 2, 2, 3, 4, 5, 5], tails=[12287, 0, 1, 0, 1, 0, 1, 12287])),
    "tile_edges5_10": Case("tile_edges5_10", 1, [("default", K10_5)], None, dict(chains=[1, 1, 2, 2, 3, 4, 5, 5], tails=[7167, 0, 1, 0, 1, 0, 1, 7167])),
    # cfirst per plan tile (8-byte, 10-byte): read off plan() once; parts with equal bounds are empty, their tickets are stolen
    "one_bucket_low": Case("one_bucket_low", 2, [("split=0", (5,)), ("default", (7,))], None,
                           dict(big=3, cfirst={8: [0, 323, 323, 323, 323, 323, 336, 392, 448], 10: [0, 551, 551, 551, 551, 551, 551, 591, 676]},
                                chain={8: 321, 10: 549})),
    "one_bucket_high": Case("one_bucket_high", 2, [("split=0", (5,)), ("default", (7,))], None,
                            dict(big=255, cfirst={8: [0, 71, 143, 215, 575, 575, 575, 575, 575], 10: [0, 100, 200, 803, 803, 803, 803, 803, 803]},
                                 chain={8: 321, 10: 549})),
    "part_starts": Case("part_starts", 3, [("split=0", (5,)), ("default", (6,))], None, dict(offset=0)),
    "part_starts_shifted": Case("part_starts_shifted", 3, [("split=0", (5,)), ("default", (6,))], None, dict(offset=1)),
    "empties": Case("empties", 4, [("split=0", K5), ("default", K10_5)], None, dict()),
    "padding_keys_8": Case("padding_keys_8", 5, [("split=0", (5,)), ("narrow_k=0", (5,))], None, dict(k0=5, tail={PAD_X: 1, PAD_Y: 63})),
    "padding_keys_10": Case("padding_keys_10", 5, [("default", (7,))], None, dict(k0=7, tail={PAD_X: 1, PAD_Y: 63})),
    "ties": Case("ties", 6, [("split=0", K8), ("declined", (5,)), ("default", K10)], ("declined", 5), dict()),
    "ties5": Case("ties5", 6, [("split=0", K5), ("declined", (8,)), ("default", K10_5)], None, dict()),
    "text_edges": Case("text_edges", 7, [("split=0", (5,)), ("text_pass=0", (5,)), ("default", (7,))], None, dict()),
}
# the deliberate mistake of stepwise_model (or of plan()) that every case of the issue's list must tell from lsd_model:
# (case, key length, mistake).  "cfirst" changes no record's place -- see tests/test_seg_cases_cpu.py.
SENSITIVITY = {1: ("tile_edges5_8", 7, "mask"), 2: ("one_bucket_low", 7, "swap"), 3: ("part_starts_shifted", 5, "cfirst"),
               4: ("empties", 8, "bucket_of"), 5: ("padding_keys_8", 5, "padding"), 6: ("ties", 5, "unstable"), 7: ("text_edges", 5, "halo")}


def tile_of(plan_, geom=FULL):
    return {8: geom.T8, 10: geom.T10, 12: geom.T10}[plan_]


def spec_of(T, form, k0, L):
    """passes() of a run; the 12-byte control sorts the same key in one piece (no partial character: not the 10-byte plan)"""
    if FORMS[form][0] == 12:
        return {"b": T.b, "k0": k0, "plan": None, "chars": k0, "bits": T.b * k0, "passes": []}
    return passes(T.b, k0, L)
