"""Texts, forms and the model of the two structures every byte-pattern query starts from (tests/test_gpu_query_structs.py);
plain NumPy, no GPU.

query_one (csrc/sa_query.hpp) takes two device arrays as truth: K, the sorted packed keys, and dir, the bucket directory
over K's top dbits.  Five code paths write them and the build plan picks one (WRITERS below).  The other GPU tests reach the
two arrays only through a few thousand queries; here they are modelled whole, from the comments that define them:

  K    sa_query.hpp: "the packed first-k0-characters key of every SA slot ... b bits per character after alphabet compaction";
       sa_build.hpp, gather_keys_kernel: "keys[j] = packed first k0 characters of suffix sa[j]", codes MSB first, left-aligned
       in 64 bits, 0 past the end of the text.  This is full[r].
       key_bytes == 8: the stored key is full[r].
       key_bytes == 4: (full[r] >> lo_shift) & 0xFFFFFFFF, lo_shift = 64 - b * k0 (sa_query.hpp: "K is u32[n] instead: ... the key
       without (all of) its top 8 bits"; sa_build.hpp: "key of slot j = (bucket(j) << 56) | (qkeys32[j] << q_lo_shift)").
       10-byte-record plan with the partial character (sa_build.hpp, Builder::build, the `partial_char && b * k0 < 56 &&
       b * (k0 + 1) > 56 && ...` branch: "The 56 key bits hold k0 whole characters and, when the next one does not fit, its TOP
       bits: the key is the first 56 bits of the (k0 + 1)-character key"): the stored u64 is the (k0 + 1)-character key with its
       low 8 bits cleared.  partial_applies() restates the branch's condition.
  dir  flags_common.hpp: "dir[bkt] = first slot whose key has top-dbits >= bkt"; dir[2^dbits] = n.

Beside dir the model computes the OWNER DECOMPOSITION that writers 1-3 imply (flags_common.hpp: "Slot j owns the buckets
(top(K[j-1]), top(K[j])]"): per head slot its run of buckets -- slot 0's run starts at bucket 0 (the leading run), the last
slot also owns the trailing run up to the end marker -- the run's span, and whether dir_emit writes it inline (span <=
DIR_INLINE) or queues it, in how many pieces of DIR_PIECE buckets.  It serves error messages and the preconditions of the
crafted text (tests/test_query_struct_cases_cpu.py); writers 4 and 5 do not work by owners.

The crafted text ("markov") is a chain over the bytes 1..100 (codes 1..100, b = 7) with a follower table: a background symbol
is followed by any background symbol; a symbol of FOLLOW only by the words listed for it.  The table plants exact spans:
  dbits 14 (two symbols per bucket): X = 30 is followed by 1, 41 or 82 only -- the first slot of (30, 41) owns exactly 40
    buckets (inline), the first slot of (30, 82) exactly 41 (queued).
  dbits 21 (three symbols per bucket): Y = 20 always continues 1 1 and the smallest continuation of 21 is 1 1: the first slot of
    (21, 1, 1) owns 128 * 128 = 16384 buckets, one piece.  Z = 60 always continues 1 1 and the smallest continuation of 61 is
    1 2: 16385 buckets, two pieces.  The unused codes 101..127 make the trailing run 27 pieces and more; code 0 (never a
    key's first symbol) makes the leading run longer than 16384 buckets.
The text ends in three fixed background symbols: a suffix that ends inside a planted word would add a key with code 0 inside
the planted run."""
from collections import namedtuple

import numpy as np

from refine_cases import D1_SYMBOLS

# restated from the headers; (file under suffixarray_amd/csrc, regular expression whose group 1 is the definition, value)
DIR_INLINE, DIR_PIECE, BLD_TILE, NARROW_MIN_N, TEXT_HALO = 40, 1 << 14, 4096, 1 << 22, 64
HEADER_CONSTANTS = [
    ("flags_common.hpp", r"constexpr u32 DIR_INLINE = (\d+);", "40"),
    ("flags_common.hpp", r"constexpr u32 DIR_PIECE = (1u << 14);", "1u << 14"),
    ("flags_common.hpp", r"if \(last - first (<) DIR_INLINE\)", "<"),
    ("sa_build.hpp", r"constexpr int BLD_TILE = (BLD_BLOCK \* BLD_ITEMS);", "BLD_BLOCK * BLD_ITEMS"),
    ("sa_build.hpp", r"const u32 first = \(j == 0\) \? 0u : \(u32\)\(kprev >> ds\) (\+ 1u);", "+ 1u"),
    ("sa_build.hpp", r"static int dir_coarse_bits\(int d\) \{ return (d > 16 \? 14 : 0); \}", "d > 16 ? 14 : 0"),
    ("sa_build.hpp", r"if \(partial_char && (b \* k0 < 56 && b \* \(k0 \+ 1\) > 56 && \(L == 0 \|\| \(u32\)\(k0 \+ 1\) <= L\)) && text_pass_applies\(b, k0 \+ 1\)\)",
     "b * k0 < 56 && b * (k0 + 1) > 56 && (L == 0 || (u32)(k0 + 1) <= L)"),
    ("radix_narrow.hpp", r"return ws.block == 512 && (begin_bit >= 24 && begin_bit < 56 && n >= \(1u << 22\)) &&", "begin_bit >= 24 && begin_bit < 56 && n >= (1u << 22)"),
    ("radix_narrow.hpp", r"constexpr int TEXT_HALO = (\d+);", "64"),
    ("radix_narrow.hpp", r"inline bool text_pass_applies\(int b, int k0\) \{ return (b <= 8 && k0 - 1 <= TEXT_HALO); \}", "b <= 8 && k0 - 1 <= TEXT_HALO"),
    ("radix_narrow48.hpp", r"return ws.block == 512 && (begin_bit >= 8 && begin_bit < 24 && n >= \(1u << 22\)) && text_pass_applies", "begin_bit >= 8 && begin_bit < 24 && n >= (1u << 22)"),
]
U64 = np.uint64


# ---- the model --------------------------------------------------------------------------------------------------------------

def code_map(t):
    """keygen's code map: the bytes present get the codes 1..sigma in byte order -> (code[256], sigma, b)"""
    present = np.flatnonzero(np.bincount(t, minlength=256))
    code = np.zeros(256, np.uint16)
    code[present] = np.arange(1, present.size + 1, dtype=np.uint16)
    return code, int(present.size), max(1, int(present.size).bit_length())


def full_keys(t, sa, code, b, k):
    """full[r]: the codes of T[sa[r] .. sa[r] + k), b bits each, MSB first, left-aligned in 64 bits, 0 past the end"""
    assert 1 <= b * k <= 64
    c = np.concatenate([np.asarray(code, U64)[t], np.zeros(k, U64)])
    sa = np.asarray(sa, np.int64)
    key = np.zeros(sa.size, U64)
    sh = 64
    for j in range(k):
        sh -= b
        key |= c[sa + j] << U64(sh)
    return key


def partial_applies(b, k0, L, narrow48):
    """the partial_char branch of Builder::build, default switches: only on the 10-byte-record plan (stats narrow48 == 1)"""
    return bool(narrow48) and b * k0 < 56 and b * (k0 + 1) > 56 and (L == 0 or k0 + 1 <= L) and b <= 8 and k0 <= TEXT_HALO


def stored_keys(t, sa, code, b, k0, key_bytes, lo_shift, partial=False):
    """-> (K as the device holds it: u64[n] or u32[n]; the u64 keys the directory is made over)"""
    if partial:
        assert key_bytes == 8
        k = full_keys(t, sa, code, b, k0 + 1) & ~U64(0xFF)
        return k, k
    full = full_keys(t, sa, code, b, k0)
    if key_bytes == 8:
        return full, full
    assert key_bytes == 4
    return ((full >> U64(lo_shift)) & U64(0xFFFFFFFF)).astype(np.uint32), full


def tops(keys, dbits):
    return (keys >> U64(64 - dbits)).astype(np.int64)


def directory(keys, dbits):
    """dir[bkt] = first slot whose key has top-dbits >= bkt; dir[2^dbits] = n"""
    top = tops(keys, dbits)
    return np.concatenate([np.searchsorted(top, np.arange(1 << dbits), side="left"), [keys.size]]).astype(np.uint32)


Owners = namedtuple("Owners", "first last slot span pieces")


def owners(keys, dbits):
    """The runs of buckets dir_emit is called with, in bucket order: slot 0 owns [0, top(K[0])] (the leading run), a slot j whose
    top bits differ from its predecessor's owns (top(K[j-1]), top(K[j])], the last slot also owns (top(K[n-1]), 2^dbits] with
    the value n (the trailing run: slot == n in the result).  pieces: 0 = written inline, else the queue entries."""
    top = tops(keys, dbits)
    n = top.size
    head = np.flatnonzero(np.concatenate([[True], top[1:] != top[:-1]]))
    first = np.concatenate([[0], top[head[1:] - 1] + 1, [top[-1] + 1]])
    last = np.concatenate([top[head], [1 << dbits]])
    slot = np.concatenate([head, [n]])
    span = last - first + 1
    pieces = np.where(span <= DIR_INLINE, 0, -(-span // DIR_PIECE))
    return Owners(first, last, slot, span, pieces)


def describe(own, bkt):
    """which run holds bucket bkt, and how the emit path writes it"""
    i = int(np.searchsorted(own.first, bkt, side="right") - 1)
    f, l, s, sp, pc = (int(x[i]) for x in (own.first, own.last, own.slot, own.span, own.pieces))
    kind = "inline" if pc == 0 else ("queued, piece %d of %d" % ((bkt - f) // DIR_PIECE + 1, pc))
    name = "leading run, " if i == 0 else ("trailing run, " if i == own.first.size - 1 else "")
    return "%sowner slot %d, buckets %d..%d (span %d), %s" % (name, s, f, l, sp, kind)


def dir_mismatch(got, want, own):
    """None, or the report of the first bad entry"""
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    if got.shape != want.shape:
        return "directory of %d entries, model %d" % (got.size, want.size)
    bad = np.flatnonzero(got != want)
    k = int(bad[0])
    return "dir[%d] = %d, model %d (%d of %d entries differ); %s" % (k, int(got[k]), int(want[k]), bad.size, want.size, describe(own, k))


def default_dir_bits(n):
    """Builder::directory_layout"""
    lg = 0
    while (1 << lg) < n:
        lg += 1
    return min(max(lg - 3, 8), 27)


def kmax(b, n, narrow48=True):
    """Builder::choose_initial_chars: 56 bits where the 10-byte-record plan is possible, else 64"""
    return 56 // b if (narrow48 and b <= 8 and n >= NARROW_MIN_N and 56 // b >= 6) else 64 // b


def expected_key_bytes(b, k0, n, env, adopted):
    """narrow keys: a build of n >= 2^22 with a key of at most 40 bits, unless a switch asks for the u64 array"""
    begin = 64 - b * k0
    narrow = n >= NARROW_MIN_N and 24 <= begin < 56
    keep = narrow and not adopted and env.get("SA_HIP_NARROW_K") != "0" and env.get("SA_HIP_FUSE_DIR") != "0"
    return 4 if keep else 8


def writer_of(st, env, adopted):
    """1..5 as in WRITERS, from BuildStats and the form; None: the lite pass overflowed (lite_flags == 0 without the switch) and
    the stats no longer tell whether flags_lite_kernel or the local pass wrote the directory"""
    if adopted or env.get("SA_HIP_FUSE_DIR") == "0":
        return 5
    if not st["narrow_k"]:
        return 1
    if env.get("SA_HIP_LITE_FLAGS") == "0":
        return 2
    return {2: 4, 1: 3}.get(st["lite_flags"])


WRITERS = {1: "flags_kernel<false>", 2: "flags_kernel<true>", 3: "flags_lite_kernel", 4: "local pass of the three-pass plan",
           5: "gather_keys_kernel + dir_build_kernel"}


# ---- texts ------------------------------------------------------------------------------------------------------------------

X, Y, Z = 30, 20, 60
FOLLOW = {          # planted symbol -> the words that may follow it
    X: [(1,), (41,), (82,)],
    Y: [(1, 1)],
    Y + 1: [(1, 1)],          # (also a background symbol: anything may follow it; this word makes sure 1 1 does)
    Z: [(1, 1)],
    Z + 1: [(1, 2), (50, 50)],
}
ONLY_PLANTED = (X, Y, Z, Z + 1)
TAIL = (90, 91, 92)
COPIES = 48


def markov(n, seed=11):
    rng = np.random.default_rng(seed)
    bg = np.setdiff1d(np.arange(1, 101), ONLY_PLANTED).astype(np.uint8)
    t = bg[rng.integers(0, bg.size, n)]
    p0 = int(rng.integers(0, n // 2))
    t[p0:p0 + bg.size] = rng.permutation(bg)           # every background symbol occurs
    words = [(s,) + w for s, ws in FOLLOW.items() for w in ws for _ in range(COPIES)]
    # word slots of four symbols, none over the permutation or the tail; a background symbol stands before every word
    slots = np.setdiff1d(np.arange(1, (n - 8) // 4), np.arange(p0 // 4 - 1, (p0 + bg.size) // 4 + 2))
    at = rng.choice(slots, len(words), replace=False) * 4
    for p, w in zip(at, words):
        t[p:p + len(w)] = w
    t[n - len(TAIL):] = TAIL
    return np.ascontiguousarray(t)


def all_equal(n):
    return np.full(n, 97, np.uint8)


def far2(n, seed=12):
    t = np.array([1, 255], np.uint8)[np.random.default_rng(seed).integers(0, 2, n)]
    t[:2] = (1, 255)
    return np.ascontiguousarray(t)


def uniform27(n, seed=13):
    t = D1_SYMBOLS[np.random.default_rng(seed).integers(0, D1_SYMBOLS.size, n)]
    if n >= 2 * D1_SYMBOLS.size:
        t[n // 2:n // 2 + D1_SYMBOLS.size] = D1_SYMBOLS
    return np.ascontiguousarray(t)


def words(n):
    from suffixarray_amd import synth
    return np.ascontiguousarray(synth.d2_words(n)[:n])


GENERATORS = {"markov": markov, "equal": all_equal, "far2": far2, "uni27": uniform27, "words": words}


def make(name, n):
    t = GENERATORS[name](n)
    assert t.size == n and t.dtype == np.uint8
    return t


# ---- forms ------------------------------------------------------------------------------------------------------------------
# Form: tag, switches, adopted (idx.load of the oracle's array instead of a build), L (max_suffix_length)
Form = namedtuple("Form", "tag env adopted L")


def _f(tag, env=None, adopted=False, L=0):
    return Form(tag, dict(env or {}), adopted, L)


def _with(forms, **env):
    return [Form(f.tag + "".join("+%s=%s" % (k[7:].lower(), v) for k, v in env.items()), dict(f.env, **env), f.adopted, f.L) for f in forms]


SMALL_FORMS = [_f("default"), _f("fuse_dir=0", {"SA_HIP_FUSE_DIR": "0"}), _f("adopted", adopted=True)]
ADOPTED_WIDTHS = [_f("adopted+dir_bits=%d" % d, {"SA_HIP_DIR_BITS": str(d)}, adopted=True) for d in (8, 16, 17, 21)]
TRUNCATED = [_f("L12", L=12), _f("adopted+L12", adopted=True, L=12)]
NARROW_FORMS = [_f("default"), _f("lite_flags=0", {"SA_HIP_LITE_FLAGS": "0"}), _f("narrow_k=0", {"SA_HIP_NARROW_K": "0"}),
                _f("split=1", {"SA_HIP_SPLIT": "1"}), _f("split=0", {"SA_HIP_SPLIT": "0"}), _f("split_flags=0", {"SA_HIP_SPLIT_FLAGS": "0"}),
                _f("fuse_dir=0", {"SA_HIP_FUSE_DIR": "0"})]
NARROW_FEW = [NARROW_FORMS[i] for i in (0, 1, 2, 5)]
K5 = {"SA_HIP_INITIAL_CHARS": "5"}          # b = 7: a 35-bit key, the narrow plans

# Case: id, text, n, forms, what the coverage table is to note.  One test per case: text, oracle array and models are shared by
# its forms.
Case = namedtuple("Case", "id text n forms")
SMALL_N = (2, 3, 4, 5, 4095, 4096, 4097, 8193)     # the four-slot vector load against its scalar tail; the tile edge BLD_TILE
MID_N = 60_001
BIG_N = tuple(NARROW_MIN_N + i for i in range(4))
CASES = []
for _n in SMALL_N:
    CASES.append(Case("uni27_%d" % _n, "uni27", _n, SMALL_FORMS + TRUNCATED[:1]))
    CASES.append(Case("equal_%d" % _n, "equal", _n, SMALL_FORMS[:2]))
CASES += [
    # writers 1 and 5 on the crafted spans, both forced widths; every adopted width (one level up to 16 bits, two above)
    Case("markov_mid", "markov", MID_N, SMALL_FORMS + _with(SMALL_FORMS, SA_HIP_DIR_BITS="14") + _with(SMALL_FORMS[:2], SA_HIP_DIR_BITS="21")
         + ADOPTED_WIDTHS + TRUNCATED),
    Case("equal_mid", "equal", MID_N, SMALL_FORMS + _with(SMALL_FORMS[:2], SA_HIP_DIR_BITS="21") + ADOPTED_WIDTHS + TRUNCATED),
    Case("far2_mid", "far2", MID_N, SMALL_FORMS + _with(SMALL_FORMS[:2], SA_HIP_DIR_BITS="14") + TRUNCATED[:1]),
    Case("uni27_mid", "uni27", MID_N, SMALL_FORMS + ADOPTED_WIDTHS[2:3] + TRUNCATED[:1]),
    Case("words_mid", "words", MID_N, SMALL_FORMS + ADOPTED_WIDTHS[1:3] + TRUNCATED),
    # writers 2-4 (and 1, 5 again) at the first size the narrow plans run at, on the crafted spans
    Case("markov_big_d14", "markov", BIG_N[0], _with(NARROW_FORMS, SA_HIP_DIR_BITS="14", **K5)),
    Case("markov_big_d21", "markov", BIG_N[0], _with(NARROW_FORMS, SA_HIP_DIR_BITS="21", **K5) + _with(ADOPTED_WIDTHS[3:], **K5)),
    Case("markov_big", "markov", BIG_N[0], _with(NARROW_FORMS[:2] + [_f("L12", L=12)], **K5)
         + [_f("narrow48", {"SA_HIP_NARROW48": "1", "SA_HIP_INITIAL_CHARS": "6", "SA_HIP_DIR_BITS": "21"}),
            _f("narrow48_56", {"SA_HIP_NARROW48": "1", "SA_HIP_INITIAL_CHARS": "8"})]),
]
for _n in BIG_N[1:]:
    CASES.append(Case("markov_%d" % _n, "markov", _n, _with(NARROW_FEW, SA_HIP_DIR_BITS="21", **K5) + _with(NARROW_FEW[:1] + NARROW_FEW[3:], SA_HIP_DIR_BITS="14", **K5)))
CASES += [
    # near-random text at the default width: the lite and the three-pass plans as the benchmark runs them; the 10-byte plan with
    # the partial character (11 symbols of 5 bits and one bit of the twelfth), without it (9 symbols), the 12-byte plan
    Case("uni27_big", "uni27", BIG_N[1], NARROW_FORMS[:3] + NARROW_FORMS[4:6] + [
        _f("narrow48_partial", {"SA_HIP_NARROW48": "1", "SA_HIP_INITIAL_CHARS": "11"}),
        _f("narrow48_partial+L12", {"SA_HIP_NARROW48": "1", "SA_HIP_INITIAL_CHARS": "11"}, L=12),
        _f("narrow48_45", {"SA_HIP_NARROW48": "1", "SA_HIP_INITIAL_CHARS": "9"}),
        _f("narrow48=0", {"SA_HIP_NARROW48": "0", "SA_HIP_INITIAL_CHARS": "12"}), _f("L12", L=12)]),
    Case("words_big", "words", BIG_N[3], [_f("default"), _f("narrow48=0", {"SA_HIP_NARROW48": "0"}), _f("fuse_dir=0", {"SA_HIP_FUSE_DIR": "0"}),
                                          ADOPTED_WIDTHS[2], _f("L12", L=12)]),
    Case("equal_big", "equal", BIG_N[2], [_f("k40", {"SA_HIP_INITIAL_CHARS": "40"}), _f("k40+lite_flags=0", {"SA_HIP_INITIAL_CHARS": "40", "SA_HIP_LITE_FLAGS": "0"})]),
]
CASE_BY_ID = {c.id: c for c in CASES}
SWITCHES = ("SA_HIP_DIR_BITS", "SA_HIP_INITIAL_CHARS", "SA_HIP_LITE_FLAGS", "SA_HIP_NARROW_K", "SA_HIP_SPLIT", "SA_HIP_SPLIT_FLAGS", "SA_HIP_NARROW48",
            "SA_HIP_FUSE_DIR", "SA_HIP_SECTOR_SEARCH", "SA_HIP_PARTIAL_CHAR", "SA_HIP_LOCAL_BIG", "SA_HIP_LOCAL_PERSIST", "SA_HIP_LOCAL_GRID",
            "SA_HIP_LOCAL_BINS", "SA_HIP_SPLIT_CAP", "SA_HIP_SPLIT_ITEMS")

# the spans the crafted text must show at the forced widths (checked without a GPU, and again on the device's own K)
PLANTED_SPANS = {14: (40, 41), 21: (16384, 16385)}


# ---- patterns ---------------------------------------------------------------------------------------------------------------

def bucket_pattern(bkt, dbits, b, alph):
    """the symbols whose codes are the b-bit digits of bucket number bkt, up to the first digit that is no symbol's code"""
    out = []
    for j in range(dbits // b):
        c = (bkt >> (dbits - b * (j + 1))) & ((1 << b) - 1)
        if not 1 <= c <= len(alph):
            break
        out.append(int(alph[c - 1]))
    return bytes(out)


def structure_patterns(t, keys, dbits, b, rng, k0, L):
    """every 1- and 2-symbol string over the alphabet; for the longest runs of the owner decomposition and the runs on the
    inline / queue / piece edges, the prefixes on both sides of the run and next to them; cases.edge_patterns"""
    import itertools

    import cases
    alph = np.flatnonzero(np.bincount(t, minlength=256)).astype(np.uint8)
    pats = [bytes(p) for r in (1, 2) for p in itertools.product(alph.tolist(), repeat=r)]
    own = owners(keys, dbits)
    pick = set(np.argsort(own.span)[-12:].tolist()) | {0, own.span.size - 1}
    for s in (DIR_INLINE, DIR_INLINE + 1, DIR_PIECE, DIR_PIECE + 1):
        pick |= set(np.flatnonzero(own.span == s)[:2].tolist())
    for i in sorted(pick):
        f, l = int(own.first[i]), int(own.last[i])
        for bkt in {f - 1, f, f + 1, (f + l) // 2, l - 1, l, l + 1}:
            if 0 <= bkt < (1 << dbits):
                p = bucket_pattern(bkt, dbits, b, alph)
                if p:
                    pats += [p, p + bytes(alph[:1]), p + bytes(alph[-1:])]
    pats += cases.edge_patterns(t, alph, k0, min(64 // b, 16), L, rng)
    return pats
