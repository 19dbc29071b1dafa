"""Generator and phase model of the LCP edge tests (tests/test_gpu_lcp_edges.py); plain NumPy, no GPU.

csrc/lcp.hpp compares every irreducible pair (i, Phi[i]) in three phases: a lane loop of 8-byte steps up to d0 + lane_bytes,
one wave per pair up to wave_bytes more, then split rounds whose segments double, cut into 4096-byte chunks.  Whichever
phase closes a pair, the array is the same, so a hand-off that is one byte off shows only when a PLCP value lies on it, and
a phase that quietly passes everything on shows only in the stage counters.  This module plants common prefixes of exact
lengths (planted_prefixes), restates the host loop of lcp::run (edges) and the closing rule of every phase (classify), and
so gives the expected arrays and counters.  tests/test_lcp_cases_cpu.py checks that the case lists reach the edges they
name and that the constants below are the header's.

Depths and budgets are in bytes, PLCP values in symbols (sym_bytes = 1 or 4), as in the header."""
from collections import namedtuple

import numpy as np

# restated from the headers; (file under suffixarray_amd/csrc, regular expression whose group 1 is the definition, value)
BLOCK, SCAN_ITEMS, WAVE = 256, 16, 64
SCAN_TILE = BLOCK * SCAN_ITEMS
SPLIT_CHUNK = BLOCK * 16
WAVE_STEP = WAVE * 16
LANE_STEP = 8
MAX_ROUNDS = 64
LANE_BYTES, WAVE_BYTES = 64, 16384
HEADER_CONSTANTS = [
    ("common.hpp", r"constexpr int WAVE = (\d+);", "64"),
    ("lcp.hpp", r"constexpr u32 BLOCK = (\d+);", "256"),
    ("lcp.hpp", r"constexpr u32 SCAN_ITEMS = (\d+);", "16"),
    ("lcp.hpp", r"constexpr u32 SCAN_TILE = (BLOCK \* SCAN_ITEMS);", "BLOCK * SCAN_ITEMS"),
    ("lcp.hpp", r"constexpr u32 SPLIT_CHUNK = (BLOCK \* 16);", "BLOCK * 16"),
    ("lcp.hpp", r"constexpr u32 WAVE_STEP = (WAVE \* 16);", "WAVE * 16"),
    ("lcp.hpp", r"constexpr u32 MAX_ROUNDS = (\d+);", "64"),
    ("lcp.hpp", r"u32 lane_bytes = (\d+);", "64"),
    ("lcp.hpp", r"u64 wave_bytes = (\d+);", "16384"),
    ("lcp.hpp", r"bytes \+= 8;\s+if \(x\) \{[^\n]*\n\s+d \+= (\d+);", "8"),
    ("lcp.hpp", r"u64 seg = (\(\(kn.wave_bytes \+ SPLIT_CHUNK - 1\) / SPLIT_CHUNK\) \* SPLIT_CHUNK);",
     "((kn.wave_bytes + SPLIT_CHUNK - 1) / SPLIT_CHUNK) * SPLIT_CHUNK"),
    ("lcp.hpp", r"d_lo \+= seg;\s+seg \*= (\d+);", "2"),
    ("lcp.hpp", r"for \(u32 j = 0; (j < MAX_ROUNDS && d_lo < n \* SB); \+\+j\)", "j < MAX_ROUNDS && d_lo < n * SB"),
]
assert SCAN_TILE == 4096 and SPLIT_CHUNK == 4096 and WAVE_STEP == 1024

# the knob settings of the case lists: name -> (lane_bytes, wave_bytes); the default pair leaves the environment unset
KNOBS = {"default": (LANE_BYTES, WAVE_BYTES), "small": (8, 1024), "waves_splits": (0, 16),
         "int_6_10": (6, 10), "int_default": (LANE_BYTES, WAVE_BYTES), "int_0_1": (0, 1)}


def knob_env(name):
    lane, wave = KNOBS[name]
    if (lane, wave) == (LANE_BYTES, WAVE_BYTES):
        return {}
    return {"SA_HIP_LCP_LANE_BYTES": str(lane), "SA_HIP_LCP_WAVE_BYTES": str(wave)}


# ---- the host loop ----------------------------------------------------------------------------------------------------------
Edges = namedtuple("Edges", "k0 d_lane d_wave_end rounds lane_steps wave_steps chunks split_rounds")


def edges(n, sym_bytes=1, k0=0, lane_bytes=LANE_BYTES, wave_bytes=WAVE_BYTES):
    """The hand-off depths of lcp::run in bytes: d_lane = k0 + lane_bytes (lane loop -> wave), d_wave_end = d_lane +
    wave_bytes (wave -> split), rounds = [D_0, D_1, ..] with D_0 = d_wave_end and D_{j+1} = D_j + seg_j (round j covers
    [D_j, D_{j+1})), the 8-byte steps of the lane loop, the 1024-byte steps of the wave and the 4096-byte chunks of the first
    three rounds.  split_rounds: the rounds the host launches for a text of n symbols.  rounds always holds at least D_0..D_3."""
    d_lane = k0 + lane_bytes
    d_wave_end = d_lane + wave_bytes
    seg = (wave_bytes + SPLIT_CHUNK - 1) // SPLIT_CHUNK * SPLIT_CHUNK
    d_lo, rounds, launched, chunks = d_wave_end, [d_wave_end], 0, []
    for j in range(MAX_ROUNDS):
        more = d_lo < n * sym_bytes
        if not more and len(rounds) >= 4:
            break
        if j < 3:
            chunks += list(range(d_lo, d_lo + seg, SPLIT_CHUNK))
        launched += more
        d_lo += seg
        seg *= 2
        rounds.append(d_lo)
    return Edges(k0, d_lane, d_wave_end, rounds, list(range(k0, d_lane, LANE_STEP)),
                 list(range(d_lane, d_wave_end, WAVE_STEP)), chunks, launched)


def edge_depths(lane_bytes, wave_bytes):
    """the nine depths d a list plants d - 1, d, d + 1 for: one lane step, the lane hand-off and one step beyond it, one
    wave step, the wave hand-off, a chunk bound inside round 0, the round bound D_1, a chunk bound inside round 1, D_2"""
    e = edges(1 << 40, 1, 0, lane_bytes, wave_bytes)
    D = e.rounds
    ds = [LANE_STEP, e.d_lane, e.d_lane + LANE_STEP, e.d_lane + WAVE_STEP, e.d_wave_end, D[0] + SPLIT_CHUNK, D[1],
          D[1] + SPLIT_CHUNK, D[2]]
    return sorted(set(d for d in ds if d > 0))


def lengths_around(depths, sym_bytes=1):
    """PLCP values (symbols) on and one either side of every depth (bytes); for 4-byte symbols the nearest symbol counts"""
    out = set()
    for d in depths:
        for v in (d // sym_bytes - 1, d // sym_bytes, d // sym_bytes + 1):
            if v >= 1:
                out.add(v)
    return sorted(out)


# ---- texts ------------------------------------------------------------------------------------------------------------------
def planted_prefixes(lengths, seed, alphabet, at_end=None, sym_bytes=1, high_only=False, filler=40):
    """A random word W longer than every length, in full once (the source), and for every L of lengths a copy W[:L] followed
    by a symbol different from W[L].  The symbols to the left of the source and of the copies are pairwise distinct, so every
    copy starts an irreducible position.  The copy of length L shares exactly L symbols with every longer copy and with the
    source, and nothing else in the text begins with W[:L] and its follower: in suffix order it lies directly before or
    after the suffixes that share W[:L + 1], which gives one irreducible pair of PLCP exactly L.  Copies and source lie in a
    random order, `filler` random symbols apart.  at_end = L puts the copy of length L last and leaves out its follower:
    its pair ends at n - max(i, k) with PLCP L.
    alphabet: the symbol values (ascending; more of them than copies).  sym_bytes = 4: int32 symbols; high_only: the values
    are v << 24, so that two different symbols differ only in bits 24-30 (their highest byte).
    -> (text, {L: start of its copy}, start of the source)"""
    rng = np.random.default_rng(seed)
    alphabet = np.asarray(alphabet, np.int64)
    if high_only:
        assert sym_bytes == 4 and alphabet.max() < 128
        alphabet = alphabet << 24
    A = alphabet.size
    lengths = sorted(set(int(x) for x in lengths))
    assert A > len(lengths) + 2 and lengths[0] >= 1
    W = alphabet[rng.integers(0, A, lengths[-1] + 2)]
    left = rng.permutation(A)[:len(lengths) + 1]
    parts = [("src", W)] + [(L, W[:L]) for L in lengths if L != at_end]
    parts = [parts[j] for j in rng.permutation(len(parts))]
    if at_end is not None:
        assert at_end in lengths
        parts.append((at_end, W[:at_end]))
    out, pos, cur = [], {}, 0
    for j, (tag, w) in enumerate(parts):
        gap = alphabet[rng.integers(0, A, filler)]
        gap[-1] = alphabet[left[j]]
        out += [gap, w]
        cur += filler
        pos[tag] = cur
        cur += w.size
        if tag != "src" and tag != at_end:
            other = alphabet[alphabet != W[tag]]
            out.append(other[rng.integers(0, other.size, 1)])
            cur += 1
    if at_end is None:
        out.append(alphabet[rng.integers(0, A, filler)])
    t = np.concatenate(out)
    src = pos.pop("src")
    return t.astype(np.uint8 if sym_bytes == 1 else np.int32), pos, src


def as_bytes_order(t):
    """an order-preserving byte text with the suffix array of t (the alphabets here have at most 256 values)"""
    u, inv = np.unique(np.asarray(t), return_inverse=True)
    assert u.size <= 256
    return inv.reshape(-1).astype(np.uint8)


# ---- the PLCP model ---------------------------------------------------------------------------------------------------------
def irreducible_pairs(t, sa):
    """(i, k) for every position i with a predecessor k = Phi[i] in suffix order and i == 0, k == 0 or t[i-1] != t[k-1]"""
    t = np.asarray(t)
    sa = np.asarray(sa, np.int64)
    n = t.size
    phi = np.full(n, -1, np.int64)
    phi[sa[1:]] = sa[:-1]
    i = np.nonzero(phi >= 0)[0]
    k = phi[i]
    irr = (i == 0) | (k == 0)
    rest = ~irr
    irr[rest] = t[i[rest] - 1] != t[k[rest] - 1]
    return i[irr], k[irr]


def pair_lcps(t, i, k, start=None, quick=24):
    """common prefix lengths (symbols) of the suffix pairs (i, k), each bounded by n - max(i, k)"""
    t = np.asarray(t)
    n = t.size
    m = n - np.maximum(i, k)
    l = np.zeros(i.size, np.int64) if start is None else np.minimum(np.asarray(start, np.int64), m)
    act = np.nonzero(l < m)[0]
    for _ in range(quick):
        act = act[t[i[act] + l[act]] == t[k[act] + l[act]]]
        l[act] += 1
        act = act[l[act] < m[act]]
        if act.size == 0:
            break
    for j in act:
        a, b, lo, hi = int(i[j]), int(k[j]), int(l[j]), int(m[j])
        ne = np.nonzero(t[a + lo:a + hi] != t[b + lo:b + hi])[0]
        l[j] = lo + (int(ne[0]) if ne.size else hi - lo)
    return l


def model_plcp(t, sa):
    """PLCP (int64, text order) from the irreducible pairs and PLCP[i] >= PLCP[i-1] - 1; checked against kasai_plcp and the
    reference in tests/test_lcp_cases_cpu.py"""
    n = np.asarray(t).size
    i, k = irreducible_pairs(t, sa)
    w = np.zeros(n, np.int64)
    w[i] = i + pair_lcps(t, i, k)
    if n:
        w[int(sa[0])] = max(w[int(sa[0])], int(sa[0]))
    return np.maximum.accumulate(np.maximum(w, 0)) - np.arange(n) if n else w


# ---- the phase model --------------------------------------------------------------------------------------------------------
LANE, WAVE_PHASE = -2, -1          # phase codes; a split round is its number j >= 0
Phases = namedtuple("Phases", "i k plcp first mb phase by_end compared_positions wave_compares split_compares split_rounds tied")


def classify(t, sa, plcp, e, sym_bytes=1):
    """Which phase closes every irreducible pair under the edges e, and how.  first = the first differing byte of the pair
    (little-endian symbols), mb = (n - max(i, k)) * sym_bytes when there is none.  phi closes by a mismatch before
    lim = min(d_lane, mb), or by the end when lim == mb; the wave by a mismatch before end = min(d_wave_end, mb), or by the
    end when end == mb; round j by a mismatch before min(D_{j+1}, mb), or by the end when D_{j+1} >= mb.  With a key depth
    e.k0 only the pairs of tied ranks (PLCP >= k0) are compared; tied counts every such rank, reducible or not."""
    t = np.asarray(t)
    sa = np.asarray(sa, np.int64)
    plcp = np.asarray(plcp, np.int64)
    n = t.size
    i, k = irreducible_pairs(t, sa)
    tied = 0
    if e.k0:
        tied = int((plcp[sa[1:]] >= e.k0).sum())
        keep = plcp[i] >= e.k0
        i, k = i[keep], k[keep]
    L = plcp[i]
    m = n - np.maximum(i, k)
    mb = m * sym_bytes
    first = mb.copy()
    ne = np.nonzero(L < m)[0]
    x = (t[i[ne] + L[ne]].astype(np.int64) ^ t[k[ne] + L[ne]].astype(np.int64)) & 0xFFFFFFFF
    assert (x != 0).all()
    low = np.zeros(ne.size, np.int64)              # index of the lowest differing byte
    for b in range(sym_bytes - 1, -1, -1):
        low[(x >> (8 * b)) & 0xFF != 0] = b
    first[ne] = L[ne] * sym_bytes + low
    by_end = first == mb
    phase = np.full(i.size, 1 << 30, np.int64)
    lim = np.minimum(e.d_lane, mb)
    lane = (first < lim) | (lim == mb)
    phase[lane] = LANE
    end = np.minimum(e.d_wave_end, mb)
    wave = ~lane & ((first < end) | (end == mb))
    phase[wave] = WAVE_PHASE
    open_ = ~lane & ~wave
    for j in range(len(e.rounds) - 1, 0, -1):      # descending: the smallest round that closes wins
        hit = open_ & ((first < np.minimum(e.rounds[j], mb)) | (e.rounds[j] >= mb))
        phase[hit] = j - 1
    assert (phase < (1 << 30)).all(), "a pair beyond the restated rounds"
    return Phases(i, k, L, first, mb, phase, by_end, int(i.size), int((~lane).sum()), int(open_.sum()), e.split_rounds, tied)


# ---- case lists -------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name knobs text sym_bytes lengths at_end")
BYTE_ALPHABET = np.arange(48, 48 + 64)
INT_ALPHABET = np.arange(1, 120)


def _knob_edges(knobs, n, sym_bytes=1, k0=0):
    return edges(n, sym_bytes, k0, *KNOBS[knobs])


def byte_list(knobs, seed=1):
    """the one long text of a byte list: d - 1, d, d + 1 for every depth of edge_depths"""
    ls = lengths_around(edge_depths(*KNOBS[knobs]))
    t, _, _ = planted_prefixes(ls, seed, BYTE_ALPHABET)
    return Case("%s_edges" % knobs, knobs, t, 1, ls, None)


def end_depths(knobs):
    e = _knob_edges(knobs, 1 << 40)
    return [e.d_lane, e.d_wave_end, e.rounds[1]]


def end_cases(knobs, seed=100, sym_bytes=1, high_only=False):
    """one short text per at_end in d - 1, d, d + 1 for d = d_lane, d_wave_end, D_1 (symbols: the nearest counts)"""
    out = []
    alph = BYTE_ALPHABET if sym_bytes == 1 else INT_ALPHABET
    for L in lengths_around(end_depths(knobs), sym_bytes):
        t, _, _ = planted_prefixes([L], seed + L, alph, at_end=L, sym_bytes=sym_bytes, high_only=high_only)
        out.append(Case("%s_end%d%s" % (knobs, L, "_hi" if high_only else ""), knobs, t, sym_bytes, [L], L))
    return out


def int_list(knobs, high_only, seed=7):
    ls = lengths_around(edge_depths(*KNOBS[knobs]), 4)
    t, _, _ = planted_prefixes(ls, seed, INT_ALPHABET, sym_bytes=4, high_only=high_only)
    return Case("%s_edges%s" % (knobs, "_hi" if high_only else ""), knobs, t, 4, ls, None)


TILE_SIZES = (4095, 4096, 4097, 8192, 8193)


def tile_text(n, seed=5):
    """n random bytes with a 400-byte word at 100 and, 150 bytes before 2000 and before every multiple of 4096 below n - 1,
    a copy of its first 300 bytes (cut before the text's last byte) followed by the byte 255, which no other position holds:
    the copy sorts after the word, so its positions carry the common prefix -- the irreducible position of the copy lies in
    one scan tile and the reducible positions after it, whose values come from it through the max-scan, run into the next.
    (The text's last position always has PLCP 0: a bound at n - 1 cannot be crossed.)"""
    rng = np.random.default_rng(seed + n)
    t = BYTE_ALPHABET[rng.integers(0, BYTE_ALPHABET.size, n)].astype(np.uint8)
    W = t[100:500].copy()
    left = rng.permutation(BYTE_ALPHABET)
    t[99] = left[0]
    for j, b in enumerate([2000] + list(range(SCAN_TILE, n - 1, SCAN_TILE))):
        s = b - 150
        ln = min(300, n - 1 - s)
        t[s:s + ln] = W[:ln]
        t[s - 1] = left[j + 1]
        t[s + ln] = 255
    return t


def tile_list():
    return [Case("tile_%d" % n, "default", tile_text(n), 1, [], None) for n in TILE_SIZES]


SCAN_CARRY_N = (1 << 24) + SCAN_TILE + 1
SCAN_CARRY_COPY = 6000
SCAN_CARRY_STARTS = ((1 << 24) - 3000, (1 << 24) - 1)


def scan_carry_text(start, seed=9):
    """2^24 + 4097 random bytes with a copy of 6000 bytes (cut one byte before the end) at `start` whose source lies in the
    first megabyte.  The byte after the copy is larger than the byte after the source's part, so the copy sorts after the
    source and its positions, not the source's, carry the common prefix: the values of the reducible positions after `start`
    reach the tiles from 2^24 on only through lcp_tile_scan_kernel's carry (that kernel scans the tile maxima 4096 at a
    time: 4096 tiles are 2^24 positions)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, SCAN_CARRY_N, dtype=np.uint8)
    src = 500_000
    ln = min(SCAN_CARRY_COPY, SCAN_CARRY_N - 1 - start)
    t[start:start + ln] = t[src:src + ln]
    t[start - 1] = t[src - 1] ^ 1
    t[src + ln], t[start + ln] = 0x10, 0xF0
    return t


def plcp_window(t, sa, lo, hi):
    """PLCP[lo:hi] from the two suffixes themselves"""
    phi = np.full(t.size, -1, np.int64)
    phi[sa[1:]] = sa[:-1]
    i = np.arange(lo, hi)
    k = phi[i]
    ok = k >= 0
    out = np.zeros(hi - lo, np.int64)
    out[ok] = pair_lcps(t, i[ok], k[ok], quick=8)
    return out


def byte_lists():
    """name of the knob setting -> its cases (byte texts)"""
    out = {}
    for knobs in ("default", "small", "waves_splits"):
        out[knobs] = [byte_list(knobs)] + end_cases(knobs)
    out["default"] = out["default"] + tile_list()
    return out


def int_lists():
    out = {}
    for knobs in ("int_6_10", "int_default", "int_0_1"):
        cs = []
        for hi in (False, True):
            cs.append(int_list(knobs, hi))
            cs += end_cases(knobs, sym_bytes=4, high_only=hi)
        out[knobs] = cs
    return out


def all_cases():
    return [c for cs in list(byte_lists().values()) + list(int_lists().values()) for c in cs]


def solve(text, oracle):
    """(suffix array, PLCP) of a text of the lists, both int64: the suffix array from the oracle's SA-IS on an
    order-preserving byte image, the PLCP from model_plcp"""
    text = np.asarray(text)
    tb = text if text.dtype == np.uint8 else as_bytes_order(text)
    sa = oracle.sais(tb).astype(np.int64)
    return sa, model_plcp(text, sa)


def case_edges(case, k0=0, n=None):
    return edges(case.text.size if n is None else n, case.sym_bytes, k0, *KNOBS[case.knobs])


def end_phase(case):
    """the phase that closes, by reaching the end, a pair of at_end symbols: the first whose bound reaches its last byte"""
    e = case_edges(case)
    mb = case.at_end * case.sym_bytes
    if mb <= e.d_lane:
        return LANE
    if mb <= e.d_wave_end:
        return WAVE_PHASE
    return next(j for j in range(len(e.rounds) - 1) if e.rounds[j + 1] >= mb)


def keyed_counts(plcp, sa, irreducible_plcp, k0):
    """(tied, compared_positions) of a keyed pass with key depth k0"""
    return int((plcp[sa[1:]] >= k0).sum()), int((irreducible_plcp >= k0).sum())
