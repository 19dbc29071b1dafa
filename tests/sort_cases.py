"""Model and case generator of the one-sweep radix sort's direct tests (tests/test_gpu_sort.py); plain NumPy, no GPU.

csrc/radix_sort.hpp cuts the input of every pass into tiles of 16 * block records and the tiles into 8 chunks of
tpc = ceil(tiles / 8) tiles, each with a look-back chain of its own; pass p counts pass p + 1's per-chunk histogram from a
{base chunk, threshold} word per digit.  The cases below sit where that geometry changes (geom()), and the key families aim
at what uniform random keys never hit: a digit run that ends on a chunk's first record, keys equal to the padding of a partial
tile, one odd record among equal ones, keys already ordered by their high part.  tests/test_sort_cases_cpu.py checks that
the lists really contain what they claim."""
from collections import namedtuple

import numpy as np

NCHUNK = 8            # look-back chains per pass
RADIX_BITS = 8
SORT_ITEMS = 16       # records per thread: tile = 16 * block
HIST_GRID = 2048      # workgroups of radix_hist_kernel at most
BLOCKS = (512, 256)
U64 = np.uint64
ALL_ONES = 0xFFFFFFFFFFFFFFFF

# (begin_bit, end_bit).  The issue's list gives 1, 2, 3, 4, 5, 6 and 8 passes -- (0,57) is 57 bits = 8 passes -- so (8,57) is
# added: 49 bits, 7 passes, a 1-bit last digit.
WINDOWS = [(0, 1), (63, 64), (0, 8), (0, 9), (7, 9), (8, 16), (31, 33), (0, 24), (20, 52), (4, 37), (0, 40), (3, 51), (8, 57),
           (0, 57), (1, 64), (0, 64)]


def npasses(lo, hi):
    return (hi - lo + RADIX_BITS - 1) // RADIX_BITS


def pass_bits(lo, hi):
    """width of every pass's digit, lowest pass first (the last one may be narrower: SortPlan.last_mask)"""
    w = hi - lo
    return [min(RADIX_BITS, w - RADIX_BITS * p) for p in range(npasses(lo, hi))]


def window_mask(lo, hi):
    return (((1 << (hi - lo)) - 1) << lo) & ALL_ONES


def sort_model(keys, vals, lo, hi):
    """np.argsort(keys & window_mask, kind="stable") applied to both arrays.  Windows of up to 16 bits are shifted down and
    narrowed first: the same order, and NumPy's stable sort of 8- and 16-bit integers is a radix sort."""
    keys = np.asarray(keys, dtype=U64)
    m = keys & U64(window_mask(lo, hi))
    if hi - lo <= 16:
        m = (m >> U64(lo)).astype(np.uint8 if hi - lo <= 8 else np.uint16)
    order = np.argsort(m, kind="stable")
    return keys[order], (None if vals is None else np.asarray(vals)[order])


def geom(n, block):
    """make_geom() and the launch of radix_hist_kernel restated: tile, tiles, tpc, chunks in use, tiles per histogram workgroup"""
    tile = SORT_ITEMS * block
    tiles = -(-n // tile)
    tpc = -(-max(tiles, 1) // NCHUNK)
    used = -(-tiles // tpc)
    hist_per = -(-tiles // min(tiles, HIST_GRID)) if tiles else 0
    return {"tile": tile, "tiles": tiles, "tpc": tpc, "chunks": used, "hist_per": hist_per}


def chunk_of_tile(t, tpc):
    return min(t // tpc, NCHUNK - 1)


def small_sizes(T):
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]


def large_sizes(T):
    return [8 * T - 1, 8 * T, 8 * T + 1, 9 * T, 16 * T, 16 * T + 1, 33 * T + 1, 41 * T + 5, 65 * T + 1]


def boundary_sizes(T):
    return [9 * T, 17 * T, 33 * T + 1, 41 * T + 5]


# -- key families: window values first (w < 2^W as uint64), the bits outside the window filled in afterwards ------------------
def _rand64(rng, n):
    return rng.integers(0, ALL_ONES, n, dtype=U64, endpoint=True)


def _rand_bits(rng, n, W):
    return _rand64(rng, n) >> U64(64 - W)


def embed(w, lo, hi, rng):
    """window values -> keys: the bits outside [lo, hi) are random, a kernel that looks at them fails"""
    noise = _rand64(rng, w.size) & U64(ALL_ONES ^ window_mask(lo, hi))
    return (w << U64(lo)) | noise


def _from_digits(digits):
    w = np.zeros(digits[0].size, dtype=U64)
    for p, d in enumerate(digits):
        w |= d.astype(U64) << U64(RADIX_BITS * p)
    return w


def _ascending(n, W):
    i = np.arange(n, dtype=U64)
    if (1 << W) > n:
        return i * U64(((1 << W) - 1) // n)  # (n - 1) * step < 2^W: no overflow at W = 64
    return (i << U64(W)) // U64(n)           # long runs of equal values


def f_uniform(n, W, rng, tile):
    return _rand_bits(rng, n, W)


def f_all_zero(n, W, rng, tile):
    return np.zeros(n, dtype=U64)


def f_all_ones(n, W, rng, tile):
    """with the window (0, 64) these are the keys a partial last tile is padded with"""
    return np.full(n, (1 << W) - 1, dtype=U64)


def f_ascending(n, W, rng, tile):
    return _ascending(n, W)


def f_descending(n, W, rng, tile):
    return _ascending(n, W)[::-1].copy()


def _odd(pos):
    def f(n, W, rng, tile):
        p = pos(n, tile)
        if not 0 <= p < n or n < 2:
            return None
        a = int(_rand_bits(rng, 1, W)[0])
        w = np.full(n, a, dtype=U64)
        w[p] = a ^ (1 << int(rng.integers(0, W)))    # differs from the rest in one bit of one digit
        return w
    return f


def f_digit_shares(n, W, rng, tile, bits=None):
    """every digit of the window: its 2^bits values in equal shares, permuted on their own"""
    return _from_digits([rng.permutation(np.arange(n, dtype=np.uint32) % (1 << b)) for b in bits])


def f_digit0_low(n, W, rng, tile, bits=None):
    return _rand_bits(rng, n, W) & U64(((1 << W) - 1) ^ ((1 << bits[0]) - 1))


def f_digit255_low(n, W, rng, tile, bits=None):
    return _rand_bits(rng, n, W) | U64((1 << bits[0]) - 1)


def f_round_keys(n, W, rng, tile):
    """the keys of a refinement round: gid << s | low.  Group ids ascend along the input, group sizes run 1, 2, 4 .. 4096 and
    start over, the low part takes one of 3 values -- ordered by the high part already, many equal low parts."""
    s = W // 2
    sizes = []
    total = 0
    while total < n:
        sizes.append(1 << (len(sizes) % 13))
        total += sizes[-1]
    gid = np.repeat(np.arange(len(sizes), dtype=U64), sizes)[:n]
    gid = np.minimum(gid, U64((1 << (W - s)) - 1))                # the last id takes what does not fit
    three = np.array([0, 1, (1 << s) - 1], dtype=U64) & U64((1 << s) - 1)
    return (gid << U64(s)) | three[rng.integers(0, 3, n)]


FAMILIES = {
    "uniform": f_uniform,
    "all_zero": f_all_zero,
    "all_ones": f_all_ones,
    "ascending": f_ascending,
    "descending": f_descending,
    "odd_first": _odd(lambda n, T: 0),
    "odd_tile_end": _odd(lambda n, T: T - 1),
    "odd_tile_start": _odd(lambda n, T: T),
    "odd_last": _odd(lambda n, T: n - 1),
    "digit_shares": f_digit_shares,
    "digit0_low": f_digit0_low,
    "digit255_low": f_digit255_low,
    "round_keys": f_round_keys,
}
_NEEDS_BITS = ("digit_shares", "digit0_low", "digit255_low")


def make_keys(family, n, lo, hi, seed, tile=SORT_ITEMS * 512):
    """keys of one case, or None where the family does not apply (an odd record at an index the size does not have)"""
    rng = np.random.default_rng([list(FAMILIES).index(family), n, lo, hi, seed])
    kw = {"bits": pass_bits(lo, hi)} if family in _NEEDS_BITS else {}
    w = FAMILIES[family](n, hi - lo, rng, tile, **kw)
    return None if w is None else embed(w, lo, hi, rng)


def boundary_count(n, block, which, delta):
    """records with lowest digit 0 in the chunk-boundary family: B + delta, B the first record of chunk 1 ("first") or of the
    last chunk in use ("last")"""
    g = geom(n, block)
    c = 1 if which == "first" else g["chunks"] - 1
    return c * g["tpc"] * g["tile"] + delta


def boundary_keys(n, lo, hi, seed, block, which, delta):
    """Chunk-boundary family: the lowest digit is 0 in exactly B + delta records and 1 in the rest, at random positions, so
    that after pass 0 the run of digit 0 ends one short of, on, or one past a chunk's first record; the higher digits are
    uniform, so pass 1 goes wrong if pass 0 counted a record into the wrong chunk's histogram."""
    assert npasses(lo, hi) >= 2
    zeros = boundary_count(n, block, which, delta)
    assert 0 < zeros < n
    rng = np.random.default_rng([99, n, lo, hi, seed, block, which == "last", delta + 1])
    d0 = np.ones(n, dtype=U64)
    d0[rng.permutation(n)[:zeros]] = 0
    w = (_rand_bits(rng, n, hi - lo) & U64(((1 << (hi - lo)) - 1) ^ 0xFF)) | d0
    return embed(w, lo, hi, rng)


def make_values(n, kind, seed):
    """"iota": arange(n); "random": u32 drawn from a pool of n / 3 values, so most of them occur more than once"""
    if kind is None:
        return None
    if kind == "iota":
        return np.arange(n, dtype=np.uint32)
    rng = np.random.default_rng([7, n, seed])
    pool = rng.integers(0, 1 << 32, max(1, n // 3), dtype=np.uint32)
    return pool[rng.integers(0, pool.size, n)]


# -- case lists ---------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "family n lo hi seed vals")
Boundary = namedtuple("Boundary", "n lo hi seed which delta vals")

ONE_PASS = [w for w in WINDOWS if npasses(*w) == 1]
TWO_PASS = [w for w in WINDOWS if npasses(*w) == 2]
LONG = [w for w in WINDOWS if npasses(*w) >= 3]
BOUNDARY_WINDOWS = [(0, 9), (3, 19), (0, 24)]     # two passes (a 1-bit and a full second digit), three passes
KEYS_ONLY_WINDOWS = [(7, 9), (0, 9), (0, 24), (20, 52), (4, 37), (3, 51), (8, 57), (1, 64)]   # 1 .. 8 passes
BIG_CASE = {"block": 256, "n": 2049 * 4096 + 1, "windows": [(0, 8), (5, 21)]}


def sweep_cases(block, family):
    """One family's cases at one block size: every window at the sizes up to 2T + 1; above that a one-pass, a two-pass and a
    long window per size, rotating so that the families between them take every window to the large sizes."""
    T = SORT_ITEMS * block
    fi = list(FAMILIES).index(family)
    out = []
    for n in small_sizes(T):
        for lo, hi in WINDOWS:
            out.append((n, lo, hi))
    for si, n in enumerate(large_sizes(T)):
        out += [(n,) + ONE_PASS[(fi + si) % len(ONE_PASS)], (n,) + TWO_PASS[(fi + si) % len(TWO_PASS)],
                (n,) + LONG[(fi + si) % len(LONG)]]
    cases = []
    for n, lo, hi in out:
        if family.startswith("odd_") and make_keys(family, min(n, 2 * T + 1), 0, 8, 0, T) is None:
            continue
        cases.append(Case(family, n, lo, hi, 1, "iota" if len(cases) % 2 == 0 else "random"))
    return cases


def boundary_cases(block):
    T = SORT_ITEMS * block
    out = []
    for n in boundary_sizes(T):
        for which in ("first", "last"):
            for delta in (-1, 0, 1):
                for lo, hi in BOUNDARY_WINDOWS:
                    out.append(Boundary(n, lo, hi, 1, which, delta, "iota" if len(out) % 2 == 0 else "random"))
    return out


def keys_only_cases(block):
    T = SORT_ITEMS * block
    return [Case("uniform", n, lo, hi, 2, None) for n in (T + 1, 9 * T, 33 * T + 1) for lo, hi in KEYS_ONLY_WINDOWS]


def count_calls():
    """sort calls of the sweep, the boundary family, the keys-only cases and the big case, both block sizes"""
    c = sum(len(sweep_cases(b, f)) for b in BLOCKS for f in FAMILIES)
    c += sum(len(boundary_cases(b)) + len(keys_only_cases(b)) for b in BLOCKS)
    return c + len(BIG_CASE["windows"])


def mismatch(got, exp, n, block):
    """None where the arrays are equal, else the first differing slot with its tile and chunk (geom)"""
    if got.shape == exp.shape and np.array_equal(got, exp):
        return None
    if got.shape != exp.shape:
        return "shape %s, expected %s" % (got.shape, exp.shape)
    slot = int(np.flatnonzero(got != exp)[0])
    g = geom(n, block)
    tile = slot // g["tile"]
    return "first differing slot %d (tile %d of %d, chunk %d of %d in use, tpc %d): got %#x, expected %#x" % (
        slot, tile, g["tiles"], chunk_of_tile(tile, g["tpc"]), g["chunks"], g["tpc"], int(got[slot]), int(exp[slot]))
