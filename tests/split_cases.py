"""Texts, key model and expectations of the three-pass narrow sort's tests (tests/test_gpu_split.py); plain NumPy, no GPU.

The plan of csrc/radix_split.hpp -- top digit, split pass (seg_split_kernel), local pass (local_finish_kernel /
local_persist_kernel) -- is only ever fed random text by the other tests: sub-buckets of about 6 000 records, bins of one or two,
a few dozen tied pairs.  Here the texts carry PLANTS: M copies of a word that starts with reserved bytes (bytes the random part
never uses), spread over the whole text.  A reserved symbol occurs only inside its plant, so the records that start with it are
the plant's alone: a prefix of reserved symbols fixes the top digit and the next key bits, the sub-bucket holds exactly the M
planted records, the chosen tails give every record its slot (their sorted order) and its bin, and a duplicated tail is a tied
pair at a known slot.  Nothing is taken from the recipe: measure() restates keygen, the level rule, sub-buckets, bins, tied slots
and staging rows from the text, every case carries its claims as data, and tests/test_split_cases_cpu.py checks the claims
against measure() and measure()'s core (vector_model) against pipeline_model.three_pass_model.

Alphabet: the 27 symbols of refine_cases.D1_SYMBOLS plus up to four reserved bytes: sigma <= 31, 5 bits per symbol.  Keys of
k = 8 symbols (40 bits, 32 narrow bits; SA_HIP_INITIAL_CHARS=8) or 7 (27 narrow bits); the top digit is symbol 0 and the top
three code bits of symbol 1.  Codes are 1..sigma in byte order, 0 past the end of the text."""
from collections import namedtuple

import numpy as np

from pipeline_model import choose_split_level, split_levels
from refine_cases import D1_SYMBOLS

# restated from the headers; (file under suffixarray_amd/csrc, regular expression whose group 1 is the value's definition, value)
LOCAL_CAP, LOCAL_CAP_BIG, LOCAL_BLOCK, LOCAL_BLOCK_BIG, LOCAL_RUN, LOCAL_BIN_BITS, SPLIT_BITS = 8192, 16384, 512, 1024, 8, 11, 10
LITE_CAP, BLD_TILE = 256, 4096
TEXT_TILE = 512 * 16
SPLIT_ITEMS = 28
NARROW_MIN_N = 1 << 22
HEADER_CONSTANTS = [
    ("radix_split.hpp", r"constexpr u32 LOCAL_CAP = (\d+);", "8192"),
    ("radix_split.hpp", r"constexpr u32 LOCAL_CAP_BIG = (\d+);", "16384"),
    ("radix_split.hpp", r"constexpr int LOCAL_BLOCK = (\d+);", "512"),
    ("radix_split.hpp", r"constexpr int LOCAL_BLOCK_BIG = (\d+);", "1024"),
    ("radix_split.hpp", r"constexpr u32 LOCAL_RUN = (\d+);", "8"),
    ("radix_split.hpp", r"constexpr int LOCAL_BIN_BITS = (\d+);", "11"),
    ("radix_split.hpp", r"constexpr int SPLIT_BITS = (\d+);", "10"),
    ("radix_split.hpp", r"if \(m (>) cap\) \{", ">"),
    ("radix_split.hpp", r"\(starts \? 2u : 1u\) (>) LITE_CAP\)", ">"),
    ("radix_split.hpp", r"if \(rest (>=) TILE\) split_tile<true", ">="),
    ("flags_common.hpp", r"constexpr u32 LITE_CAP = (\d+);", "256"),
    ("radix_narrow.hpp", r"#define SA_TEXT_ITEMS (\d+)", "16"),
    ("radix_narrow.hpp", r"constexpr u32 TEXT_TILE = (512u \* TEXT_ITEMS);", "512u * TEXT_ITEMS"),
    ("radix_narrow.hpp", r"int split_items = (\d+);", "28"),
    ("radix_narrow.hpp", r"n >= \(1u << (22)\)", "22"),
    ("radix_narrow.hpp", r"host_word\[k\] <= LOCAL_CAP_BIG && lo_bits - k >= (12)\)", "12"),
    ("radix_narrow.hpp", r"const int bb = \(big \|\| \(rest_bits >= (12) && nw.local_bin_bits == 12\)\) \? 12 : 11;", "12"),
    ("sa_build.hpp", r"int d = lg - (3);", "3"),
    ("sa_build.hpp", r"constexpr int BLD_TILE = (BLD_BLOCK \* BLD_ITEMS);", "BLD_BLOCK * BLD_ITEMS"),
    ("sa_build.hpp", r"if \(r \+ c (>) LITE_CAP\)", ">"),
]
RES_LO = (1, 2, 3, 4)            # reserved bytes below the 27 symbols: codes 1..4, the table's first sub-buckets
RES_HI = (251, 252, 253, 254)    # ... above them: the highest codes, the table's last sub-buckets
B = 5


def alphabet(reserved):
    """the text's bytes in code order: code c is alphabet[c - 1]"""
    return np.array(sorted(set(D1_SYMBOLS.tolist()) | set(reserved)), np.uint8)


def ordinary_codes(A):
    return np.flatnonzero(np.isin(A, D1_SYMBOLS)) + 1


def codes_of(t):
    """keygen's code map: the bytes present get the codes 1..sigma in byte order"""
    present = np.flatnonzero(np.bincount(t, minlength=256))
    code = np.zeros(256, np.uint64)
    code[present] = np.arange(1, present.size + 1, dtype=np.uint64)
    b = 0
    while (1 << b) < present.size + 1:
        b += 1
    return code[t], int(present.size), b


def keys_of(t, k):
    """the k-symbol key of every position, right-aligned (b * k bits), zero padding past the end -> (keys, b)"""
    c, sigma, b = codes_of(t)
    c = np.concatenate([c, np.zeros(k, np.uint64)])
    key = np.zeros(t.size, np.uint64)
    for j in range(k):
        key = (key << np.uint64(b)) | c[j:j + t.size]
    return key, b


# ---- the plan, vectorised ---------------------------------------------------------------------------------------------------

def vector_model(keys, lo_bits, dbits, cap=LOCAL_CAP, cap_big=LOCAL_CAP_BIG, force_big=False, bins=12, directory=False):
    """pipeline_model.three_pass_model without its loop over the sub-buckets (equal keys share a sub-bucket, so the tied slots
    and the order inside the sub-buckets are those of one stable sort of all keys): levels, the level rule (force_big:
    SA_HIP_LOCAL_BIG=1, only the large form is asked), sorted keys and order, sub-bucket sizes, tied slots with their head
    bit, staged entries per sub-bucket.  rb None: declined."""
    hb = min(SPLIT_BITS, lo_bits - LOCAL_BIN_BITS)
    out = {"rb": None, "big": False, "levels": None, "hb": hb}
    if hb < 1:
        return out
    levels = split_levels(keys, lo_bits, hb)
    if force_big:
        rb = next((k for k in range(1, hb + 1) if levels[k] <= cap_big and lo_bits - k >= 12), None)
        big = rb is not None
    else:
        rb, big = choose_split_level(levels, lo_bits, cap, cap_big)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    eq = ks[1:] == ks[:-1]
    eq_prev = np.concatenate([[False], eq])
    eq_next = np.concatenate([eq, [False]])
    tied = np.flatnonzero(eq_prev | eq_next)
    out.update(levels=levels, rb=rb, big=big, keys=ks, sa=order, tied=tied, head=~eq_prev[tied],
               split_max=levels[rb if rb else hb])
    if rb is None:
        return out
    bb = 12 if (big or (lo_bits - rb >= 12 and bins == 12)) else 11
    sub = (ks >> np.uint64(lo_bits - rb)).astype(np.int64)
    nsub = 256 << rb
    counts = np.bincount(sub, minlength=nsub)
    out.update(bb=bb, g2=dbits - 8 - rb, sub_counts=counts, sub_starts=np.concatenate([[0], np.cumsum(counts)]),
               staged_per_sub=np.bincount(sub[tied], minlength=nsub))
    if directory:
        top = (ks >> np.uint64(lo_bits + 8 - dbits)).astype(np.int64)
        out["dir"] = np.concatenate([np.searchsorted(top, np.arange(1 << dbits), side="left"), [keys.size]])
    return out


def default_dir_bits(n):
    """Builder::directory_layout"""
    lg = 0
    while (1 << lg) < n:
        lg += 1
    return min(max(lg - 3, 8), 27)


def measure(t, k, env=None):
    """What a build of t with SA_HIP_SPLIT=1, SA_HIP_INITIAL_CHARS=k and the switches of env must report: vector_model plus
    the host's decisions around it (narrow_sort_applies, the fused flags work and its fallbacks) -> dict; m["plan"] is
    BuildStats.split_plan, m["lite"] lite_flags, m["passes"] radix_passes (None: not claimed)."""
    env = env or {}
    n = int(t.size)
    keys, b = keys_of(t, k)
    lo_bits = b * k - 8
    dbits = int(env.get("SA_HIP_DIR_BITS", default_dir_bits(n)))
    m = {"n": n, "b": b, "k": k, "lo_bits": lo_bits, "dbits": dbits, "key_of": keys}
    if n < NARROW_MIN_N:          # narrow_sort_applies: no narrow-record sort, the plan is not considered
        m.update(rb=None, big=False, plan=0, split_max=0, narrow_k=0, lite=0, passes=None, considered=False)
        return m
    m.update(vector_model(keys, lo_bits, dbits, force_big=env.get("SA_HIP_LOCAL_BIG") == "1", bins=int(env.get("SA_HIP_LOCAL_BINS", 12))))
    m.update(considered=True, narrow_k=1, plan=m["rb"] or 0)
    fused = (m["rb"] is not None and env.get("SA_HIP_SPLIT_FLAGS", "1") != "0" and 0 <= m["g2"] <= m["bb"] and dbits - 8 <= lo_bits)
    if fused:                      # the local pass stages per sub-bucket; a row of more than LITE_CAP entries: the full flags pass
        m["lite"] = 2 if int(m["staged_per_sub"].max()) <= LITE_CAP else 0
    else:                          # flags_lite_kernel stages per tile of BLD_TILE slots
        per_tile = np.bincount(m["tied"] // BLD_TILE, minlength=1)
        m["lite"] = 1 if int(per_tile.max()) <= LITE_CAP else 0
    m["fused"] = fused
    m["lite_unfused"] = m["lite"] if not fused else (1 if int(np.bincount(m["tied"] // BLD_TILE, minlength=1).max()) <= LITE_CAP else 0)
    m["passes"] = 3 if m["rb"] is not None else 1 + -(-lo_bits // 8)
    return m


def sub_of(m, word):
    """index of the sub-bucket that holds the keys starting with the bytes of word (two symbols at least)"""
    return int(m["key_of"][word] >> np.uint64(m["lo_bits"] - m["rb"]))


def sub_view(m, sb):
    """sub-bucket sb of a measured text: size, the neighbours' sizes, bin populations, tied slots (from its start), staged"""
    lo, hi = int(m["sub_starts"][sb]), int(m["sub_starts"][sb + 1])
    ks = m["keys"][lo:hi]
    rest = m["lo_bits"] - m["rb"]
    bins = ((ks >> np.uint64(rest - m["bb"])) & np.uint64((1 << m["bb"]) - 1)).astype(np.int64)
    tied = m["tied"][(m["tied"] >= lo) & (m["tied"] < hi)] - lo
    return {"start": lo, "size": hi - lo, "before": int(m["sub_counts"][sb - 1]) if sb else 0,
            "after": int(m["sub_counts"][sb + 1]) if sb + 1 < m["sub_counts"].size else 0,
            "bins": np.bincount(bins, minlength=1 << m["bb"]), "tied": tied.tolist(), "staged": int(m["staged_per_sub"][sb]),
            "last_bin_of_last_slot": int(bins[-1]) if hi > lo else -1}


def runs(slots):
    """[(first slot, length)] of the maximal runs of consecutive slots"""
    out = []
    for s in slots:
        if out and out[-1][0] + out[-1][1] == s:
            out[-1][1] += 1
        else:
            out.append([s, 1])
    return [tuple(x) for x in out]


# ---- texts ------------------------------------------------------------------------------------------------------------------

def plant_text(n, seed, plants, end=None):
    """Random text over the 27 symbols with every row of every plant (uint8[M, w]) written once: rows of all plants in one
    random order, random gaps of at least one symbol, so the copies of a plant fall into different tiles of every pass.  end:
    a word that ends on the text's last symbol.  -> (text, [start positions per plant])"""
    rng = np.random.default_rng(seed)
    t = D1_SYMBOLS[rng.integers(0, D1_SYMBOLS.size, n)]
    which = np.concatenate([np.full(p.shape[0], i) for i, p in enumerate(plants)]) if plants else np.zeros(0, np.int64)
    row = np.concatenate([np.arange(p.shape[0]) for p in plants]) if plants else np.zeros(0, np.int64)
    perm = rng.permutation(which.size)
    which, row = which[perm], row[perm]
    width = np.array([p.shape[1] for p in plants], np.int64)[which] if plants else np.zeros(0, np.int64)
    tail = len(end) if end is not None else 0
    need = int(width.sum()) + which.size + tail
    assert need + 1 <= n, (need, n)
    gaps = rng.multinomial(n - need, np.full(which.size + 1, 1.0 / (which.size + 1)))[:-1] + 1
    start = np.cumsum(gaps + np.concatenate([[0], width[:-1]]))
    pos = []
    for i, p in enumerate(plants):
        sel = which == i
        at = start[sel]
        t[at[:, None] + np.arange(p.shape[1])[None, :]] = p[row[sel]]
        pos.append(at[np.argsort(row[sel])])
    if end is not None:
        t[n - tail:] = np.frombuffer(bytes(end), np.uint8)
    return np.ascontiguousarray(t), pos


def _digits(vals, w, base):
    out = np.empty((vals.size, w), np.int64)
    for j in range(w - 1, -1, -1):
        out[:, j] = vals % base
        vals = vals // base
    return out


def slot_plant(A, prefix, m, w, rng, ties=(), first=None):
    """m words of len(prefix) + w symbols: the codes of prefix, then a tail over the ordinary symbols.  The tails ascend with
    the row number, so row i sorts into slot i of the words; ties = [(slot, length)]: the words of slots slot .. slot + length - 1
    are equal.  first: the codes the tail's first symbol is drawn from (default: every ordinary symbol)."""
    o = ordinary_codes(A)
    f = o if first is None else np.asarray(first)
    new = np.ones(m, np.int64)
    for p, r in ties:
        assert p + r <= m and new[p + 1:p + r].all()
        new[p + 1:p + r] = 0
    gid = np.cumsum(new) - 1
    space = f.size * o.size ** (w - 1)
    vals = np.sort(rng.choice(space, int(gid[-1]) + 1, replace=False))[gid]
    d = _digits(vals, w, o.size)            # (the first digit is < f.size: vals < f.size * o.size^(w - 1))
    codes = np.concatenate([np.tile(np.asarray(prefix, np.int64), (m, 1)), np.sort(f)[d[:, :1]], o[d[:, 1:]]], axis=1)
    return A[codes - 1]


def free_plant(A, prefix, m, w, rng, second=None):
    """m words: the codes of prefix, then w random ordinary symbols (second: the codes the first of them is drawn from)"""
    o = ordinary_codes(A)
    codes = np.concatenate([np.tile(np.asarray(prefix, np.int64), (m, 1)), o[rng.integers(0, o.size, (m, w))]], axis=1)
    if second is not None:
        codes[:, len(prefix)] = np.asarray(second)[rng.integers(0, len(second), m)]
    return A[codes - 1]


Text = namedtuple("Text", "t words k A")   # words: the first copy of every plant (its sub-bucket is looked up by it)
N = 4_400_000
X = 16                                      # the fixed ordinary symbol that ends a four-symbol prefix (a code)


def t_sub(M, k=8, n=N, seed=1, ties=()):
    """one plant of M words R1 R2 R3 X + chosen tail: 20 key bits fixed, the group keeps M records at every level 0..10"""
    A = alphabet(RES_LO[:3])
    rng = np.random.default_rng(seed + 100)
    p = slot_plant(A, (1, 2, 3, X), M, k - 4, rng, ties)
    t, pos = plant_text(n, seed, [p])
    return Text(t, [pos[0][0]], k, A)


def t_sizes(sizes, seed=2):
    """four plants R_i X + six free symbols: the sub-bucket (R_i, X) holds exactly sizes[i] records at every level >= 2, and
    -- R_i is followed by X only -- the sub-buckets next to it are empty"""
    A = alphabet(RES_LO)
    rng = np.random.default_rng(seed + 100)
    t, pos = plant_text(N, seed, [free_plant(A, (i + 1, X), s, 6, rng) for i, s in enumerate(sizes)])
    return Text(t, [p[0] for p in pos], 8, A)


def t_one_bin(parity, seed=3):
    """LOCAL_CAP words R1 R2 R3 R4 s4 + three chosen symbols, s4 from eight codes that share their top two bits: at rb = 2 all
    8192 records of the sub-bucket (R1, R2) fall into ONE bin of 12 bits, R3 R4 (s4 >> 3); codes 8..15 make it odd (the high
    half of a counter word), 16..23 even.  (The words behind the first two symbols start with reserved symbols as well: tails
    of ordinary symbols with twelve bits fixed would add 8192 records to one sub-bucket of the random part.)"""
    A = alphabet(RES_LO)
    rng = np.random.default_rng(seed + 100)
    p = slot_plant(A, (1, 2, 3, 4), LOCAL_CAP, 4, rng, first=np.arange(8, 16) if parity else np.arange(16, 24))
    t, pos = plant_text(N, seed, [p])
    return Text(t, [pos[0][0]], 8, A)


def t_bins(k=8, seed=4):
    """The sub-bucket (R1, R2) with chosen bins (rb = 2: the bin is symbols 2, 3 and the top bits of symbol 4): three records
    in the LAST bin (z z and a code >= 24: all ones), bins of exactly two and exactly three members, 700 records with random
    tails -- and one in bin 0, which only a word that ends the text can reach (code 0 is the padding): R1 R2 are the text's
    last two symbols.  R3 R4 occur once, so that sigma is 31 and z has the code of all ones."""
    A = alphabet(RES_LO)
    rng = np.random.default_rng(seed + 100)
    o = ordinary_codes(A)
    fill = free_plant(A, (1, 2), 700, k - 2, rng, second=[c for c in o if c not in (10, 11, 12, 13, 31)])
    last = slot_plant(A, (1, 2, 31, 31), 3, k - 4, rng, first=np.arange(24, 32))
    two = slot_plant(A, (1, 2, 10, 20), 2, k - 4, rng, first=np.arange(8, 16))
    three = slot_plant(A, (1, 2, 12, 20), 3, k - 4, rng, first=np.arange(16, 24))
    once = A[np.array([[3, 4, 9, 9]]) - 1]
    t, pos = plant_text(N, seed, [fill, last, two, three, once], end=bytes(A[[0, 1]]))
    return Text(t, [pos[0][0], pos[1][0], pos[2][0], pos[3][0]], k, A)


TIES = {
    # (0, 1): the p == 0 guard; (15, 16): the row edge, seen by the pre-loop; (511, 512): lane 511 of item 0 and lane 0 of item
    # 1; (m - 2, m - 1): the p + 1 < m guard
    "a": (1030, [(0, 2), (15, 2), (511, 2), (1028, 2)]),
    # (16, 17): the DPP compare; (512, 513); a triple and a pair with no untied slot between them
    "b": (1030, [(16, 2), (100, 3), (103, 2), (512, 2)]),
    # five equal keys over slots 13..17: the row-edge pair (15, 16) is not a head
    "c": (1030, [(13, 5)]),
}


def t_stage(tied, where, seed=6):
    """a sub-bucket of 600 records whose tied slots number exactly `tied`: pairs from slot 0 on, the last group a triple when
    tied is odd; where = "first" / "last": the first / last non-empty sub-bucket of the table"""
    res = RES_LO[:3] if where == "first" else RES_HI[1:]
    A = alphabet(res)
    prefix = (1, 2, 3, X + 3) if where == "first" else (30, 29, 28, X)
    npairs = tied // 2 - (tied & 1)
    ties = [(2 * i, 2) for i in range(npairs)] + ([(2 * npairs, 3)] if tied & 1 else [])
    rng = np.random.default_rng(seed + 100)
    t, pos = plant_text(N, seed, [slot_plant(A, prefix, 600, 4, rng, ties)])
    return Text(t, [pos[0][0]], 8, A)


def t_tiles(T, seed=7):
    """top-digit buckets of exactly T - 1, T, T + 1, 2 T and 1 records: R1 followed by one of the four ordinary symbols whose
    codes share their top three bits g (the bucket (R1, g)), then six free symbols; four sub-buckets each, far below the cap"""
    A = alphabet(RES_LO[:1])
    rng = np.random.default_rng(seed + 100)
    sizes = {2: T - 1, 3: T, 4: T + 1, 5: 2 * T, 6: 1}
    plants = [free_plant(A, (1,), s, 7, rng, second=np.arange(4 * g, 4 * g + 4)) for g, s in sizes.items()]
    t, pos = plant_text(N, seed, plants)
    return Text(t, [p[0] for p in pos], 8, A)


def t_length(n, seed=8):
    """64 words R1 R2 R3 X + tail, the last of them ending on the text's last symbol: the keys of its last seven positions
    run into the zero padding"""
    A = alphabet(RES_LO[:3])
    rng = np.random.default_rng(seed + 100)
    p = slot_plant(A, (1, 2, 3, X), 64, 4, rng)
    t, pos = plant_text(n, seed, [p[:-1]], end=bytes(p[-1]))
    return Text(t, [pos[0][0]], 8, A)


TEXTS = {
    "sub_8192": (t_sub, (8192,)), "sub_8191": (t_sub, (8191,)), "sub_8193": (t_sub, (8193,)), "sub_16384": (t_sub, (16384,)),
    "sub_16385": (t_sub, (16385,)),
    "sizes_a": (t_sizes, ((1, 2, 511, 512),)), "sizes_b": (t_sizes, ((513, 1023, 1024, 1025),)),
    "one_bin_odd": (t_one_bin, (1,)), "one_bin_even": (t_one_bin, (0,)), "bins": (t_bins, ()),
    "ties_a": (t_sub, (TIES["a"][0], 8, N, 5, TIES["a"][1])), "ties_b": (t_sub, (TIES["b"][0], 8, N, 5, TIES["b"][1])),
    "ties_c": (t_sub, (TIES["c"][0], 8, N, 5, TIES["c"][1])),
    "stage_256_first": (t_stage, (256, "first")), "stage_257_first": (t_stage, (257, "first")),
    "stage_256_last": (t_stage, (256, "last")), "stage_257_last": (t_stage, (257, "last")),
    "tiles_24": (t_tiles, (512 * 24,)), "tiles_28": (t_tiles, (512 * 28,)), "tiles_32": (t_tiles, (512 * 32,)),
    "len_m1": (t_length, (NARROW_MIN_N - 1,)), "len_0": (t_length, (NARROW_MIN_N,)), "len_p1": (t_length, (NARROW_MIN_N + 1,)),
    "len_p8191": (t_length, (NARROW_MIN_N + 8191,)),
    "sub_8192_k7": (t_sub, (8192, 7)), "ties_a_k7": (t_sub, (TIES["a"][0], 7, N, 5, TIES["a"][1])), "bins_k7": (t_bins, (7,)),
}


def make(name):
    f, args = TEXTS[name]
    return f(*args)


# ---- the cases --------------------------------------------------------------------------------------------------------------
# Case: the text, the switches on top of SA_HIP_SPLIT=1 / SA_HIP_INITIAL_CHARS, and the claims -- all of them numbers read off
# measure() once and written down here; tests/test_split_cases_cpu.py holds measure() against them.
#   plan, form, split_max, lite: BuildStats.split_plan, "small" / "big" / None, split_max, lite_flags of the default form
#   subs: per planted word (Text.words) the size of its sub-bucket; every one has an empty sub-bucket before and after it
#   tied: the tied slots of the first planted sub-bucket as [(first slot, length)]; staged: its staged entries
#   bins: bb and what the bin populations of the first planted sub-bucket must show (see the CPU test)
#   buckets: sizes of the planted top-digit buckets
Case = namedtuple("Case", "text env claim")


def _c(text, env=None, **claim):
    return Case(text, env or {}, claim)


BIG = {"SA_HIP_LOCAL_BIG": "1"}
B11 = {"SA_HIP_LOCAL_BINS": "11"}
CASES = {}
FAMILIES = {}


def _family(name, cases):
    FAMILIES[name] = list(cases)
    CASES.update(cases)


_family("caps", {   # sub-bucket size against LOCAL_CAP / LOCAL_CAP_BIG; the planted group keeps its size at every level
    "sub_8192": _c("sub_8192", plan=2, form="small", split_max=8192, lite=2, subs=[8192], staged=0),
    "sub_8191": _c("sub_8191", plan=2, form="small", split_max=8191, lite=2, subs=[8191], staged=0),
    # no level fits 8192: the large form at level 1, whose largest sub-bucket is one of the random part
    "sub_8193": _c("sub_8193", plan=1, form="big", split_max=12783, lite=2, subs=[8193], staged=0),
    "sub_16384": _c("sub_16384", plan=1, form="big", split_max=16384, lite=2, subs=[16384], staged=0),
    "sub_16385": _c("sub_16385", plan=0, form=None, split_max=16385, lite=1),
})
_family("sizes", {  # the workgroup's item loop: 512 threads (1024 in the large form), sixteen items
    "sizes_a": _c("sizes_a", plan=2, form="small", split_max=6300, lite=2, subs=[1, 2, 511, 512]),
    "sizes_a_big": _c("sizes_a", BIG, plan=1, form="big", split_max=12484, lite=2, subs=[1, 2, 511, 512]),
    "sizes_b": _c("sizes_b", plan=2, form="small", split_max=6289, lite=2, subs=[513, 1023, 1024, 1025]),
    "sizes_b_big": _c("sizes_b", BIG, plan=1, form="big", split_max=12501, lite=2, subs=[513, 1023, 1024, 1025]),
})
# bins of the first planted sub-bucket: {bin: members}; "only": no other bin is populated.  bin 0 holds the one record that
# ends the text; the last bin three, the sub-bucket's last slot among them.  At 11 bin bits two neighbouring bins merge.
_BINS12 = {0: 1, (10 << 7) | (20 << 2) | 1: 2, (12 << 7) | (20 << 2) | 2: 3, 4095: 3}
_BINS11 = {0: 1, (10 << 6) | (20 << 1): 2, (12 << 6) | (20 << 1) | 1: 3, 2047: 3}
_family("bins", {
    "one_bin_odd": _c("one_bin_odd", plan=2, form="small", split_max=8192, lite=2, subs=[8192], bb=12, bins={401: 8192}, only=True),
    "one_bin_odd_11": _c("one_bin_odd", B11, plan=2, form="small", split_max=8192, lite=2, subs=[8192], bb=11, bins={200: 8192}, only=True),
    "one_bin_even": _c("one_bin_even", plan=2, form="small", split_max=8192, lite=2, subs=[8192], bb=12, bins={402: 8192}, only=True),
    "one_bin_even_11": _c("one_bin_even", B11, plan=2, form="small", split_max=8192, lite=2, subs=[8192], bb=11, bins={201: 8192}, only=True),
    "bins": _c("bins", plan=2, form="small", split_max=6253, lite=2, subs=[709], bb=12, bins=_BINS12, last_slot_bin=4095),
    "bins_11": _c("bins", B11, plan=2, form="small", split_max=6253, lite=2, subs=[709], bb=11, bins=_BINS11, last_slot_bin=2047),
})
_family("ties", {   # tied: [(first slot, length)] inside the planted sub-bucket; every tied slot is staged
    "ties_a": _c("ties_a", plan=2, form="small", split_max=6274, lite=2, subs=[1030], tied=[(0, 2), (15, 2), (511, 2), (1028, 2)], staged=8),
    # (the triple 100..102 and the pair 103, 104 are two groups that runs() reports as one run of five tied slots)
    "ties_b": _c("ties_b", plan=2, form="small", split_max=6275, lite=2, subs=[1030], tied=[(16, 2), (100, 5), (512, 2)], staged=9, groups=4),
    "ties_c": _c("ties_c", plan=2, form="small", split_max=6273, lite=2, subs=[1030], tied=[(13, 5)], staged=5, groups=1),
})
_family("staging", {   # a row of exactly LITE_CAP entries is staged; one more: the overflow path, lite_flags == 0
    "stage_256_first": _c("stage_256_first", plan=2, form="small", split_max=6283, lite=2, subs=[600], tied=[(0, 256)], staged=256, first=True),
    "stage_257_first": _c("stage_257_first", plan=2, form="small", split_max=6283, lite=0, subs=[600], tied=[(0, 257)], staged=257, first=True),
    "stage_256_last": _c("stage_256_last", plan=2, form="small", split_max=6283, lite=2, subs=[600], tied=[(0, 256)], staged=256, last=True),
    "stage_257_last": _c("stage_257_last", plan=2, form="small", split_max=6283, lite=0, subs=[600], tied=[(0, 257)], staged=257, last=True),
})


def _tiles(T):
    return {(1 << 3) | g: s for g, s in {2: T - 1, 3: T, 4: T + 1, 5: 2 * T, 6: 1}.items()}


_family("tiles", {  # buckets: top digit -> records; texts made for the tile of the split pass they run with
    "tiles_28": _c("tiles_28", plan=2, form="small", split_max=7331, lite=2, buckets=_tiles(512 * 28)),
    "tiles_24": _c("tiles_24", {"SA_HIP_SPLIT_ITEMS": "24"}, plan=2, form="small", split_max=6229, lite=2, buckets=_tiles(512 * 24)),
    # (the bucket of 2 T = 32 768 records has four sub-buckets of about 8192 at level 2: level 3 is taken)
    "tiles_32": _c("tiles_32", {"SA_HIP_SPLIT_ITEMS": "32"}, plan=3, form="small", split_max=4325, lite=2, buckets=_tiles(512 * 32)),
})
_family("length", {  # n against the top-digit pass's tiles of TEXT_TILE positions; below 2^22 no narrow-record sort at all
    "len_m1": _c("len_m1", plan=0, form=None, split_max=0, lite=0, narrow_k=0),
    "len_0": _c("len_0", plan=2, form="small", split_max=5978, lite=2, subs=[64], text_tiles=(512, 0)),
    "len_p1": _c("len_p1", plan=2, form="small", split_max=5978, lite=2, subs=[64], text_tiles=(512, 1)),
    "len_p8191": _c("len_p8191", plan=2, form="small", split_max=5990, lite=2, subs=[64], text_tiles=(512, 8191)),
})
_family("directory", {   # g2 = dbits - 8 - rb entries bits per sub-bucket, rb = 2, 12 bin bits
    "dir_g2_0": _c("bins", {"SA_HIP_DIR_BITS": "10"}, plan=2, form="small", split_max=6253, lite=2, g2=0),
    "dir_g2_bb": _c("bins", {"SA_HIP_DIR_BITS": "22"}, plan=2, form="small", split_max=6253, lite=2, g2=12),
    "dir_g2_bb1": _c("bins", {"SA_HIP_DIR_BITS": "23"}, plan=2, form="small", split_max=6253, lite=1, g2=13),   # declined: the flags pass on its own
})
_family("short_key", {   # SA_HIP_INITIAL_CHARS=7: 27 narrow bits
    "sub_8192_k7": _c("sub_8192_k7", plan=2, form="small", split_max=8192, lite=2, subs=[8192], staged=0),
    "ties_a_k7": _c("ties_a_k7", plan=2, form="small", split_max=6277, lite=2, subs=[1030], tied=[(0, 2), (15, 2), (511, 2), (1028, 2)], staged=8),
    "bins_k7": _c("bins_k7", plan=2, form="small", split_max=6251, lite=2, subs=[709], bb=12, bins=_BINS12, last_slot_bin=4095),
})
FORMS = [("", {}), ("+wg_per_sub", {"SA_HIP_LOCAL_PERSIST": "0"}), ("+grid1", {"SA_HIP_LOCAL_GRID": "1"}), ("+flags_pass", {"SA_HIP_SPLIT_FLAGS": "0"})]
