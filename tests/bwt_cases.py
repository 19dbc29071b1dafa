"""Generator and ruler model of the BWT edge tests (tests/test_gpu_bwt_edges.py); plain NumPy, no GPU.

Forward (csrc/bwt.hpp: bwt_gather_kernel): texts whose primary index is chosen (text_with_primary), at sizes around the
16-byte output groups and the 4096-byte tiles.  Inverse: psi as the header defines it (psi_of; decode walks it back to the
text, which tests/test_bwt_cases_cpu.py compares with model_unbwt), the hash rulers (mix64 and the salt restated) and the
host loop of run_unbwt round by round (simulate), which gives the counts of sa_hip_bwt_stats exactly."""
from collections import namedtuple

import numpy as np

# restated from the header; (file under suffixarray_amd/csrc, regular expression whose group 1 is the definition, value)
BLOCK, ITEMS = 256, 16
TILE = BLOCK * ITEMS
WALK, RULER, AUX_MIN = 2048, 1024, 1 << 18
SALT = 0x5851f42d4c957f2d
MIX = ((30, 0xbf58476d1ce4e5b9), (27, 0x94d049bb133111eb), (31, None))
HEADER_CONSTANTS = [
    ("bwt.hpp", r"constexpr u32 BLOCK = (\d+);", "256"),
    ("bwt.hpp", r"constexpr u32 ITEMS = (\d+);", "16"),
    ("bwt.hpp", r"constexpr u32 TILE = (BLOCK \* ITEMS);", "BLOCK * ITEMS"),
    ("bwt.hpp", r"u32 walk = (\d+);", "2048"),
    ("bwt.hpp", r"u32 ruler = (\d+);", "1024"),
    ("bwt.hpp", r"u64 aux_min = (1ull << 18);", "1ull << 18"),
    ("bwt.hpp", r"x \^= x >> (\d+); x \*= 0xbf58476d1ce4e5b9ull;", "30"),
    ("bwt.hpp", r"x \^= x >> (\d+); x \*= 0x94d049bb133111ebull;", "27"),
    ("bwt.hpp", r"return x \^ \(x >> (\d+)\);", "31"),
    ("bwt.hpp", r"return (\(mix64\(x \^ salt\) & smask\) == 0);", "(mix64(x ^ salt) & smask) == 0"),
    ("bwt.hpp", r"const u64 salt = (0x5851f42d4c957f2dull \^ n);", "0x5851f42d4c957f2dull ^ n"),
    ("bwt.hpp", r"const u64 smask = (\(u64\)kn.ruler - 1);", "(u64)kn.ruler - 1"),
    ("bwt.hpp", r"const u64 cap = (m \+ hash_count \+ \(n \+ B - 1\) / B \+ 2);", "m + hash_count + (n + B - 1) / B + 2"),
    ("bwt.hpp", r"const u64 max_rounds = (\(n \+ B - 1\) / B \+ 1);", "(n + B - 1) / B + 1"),
    ("bwt.hpp", r"const u32 steps = (\(u32\)bits_for\(S \+ 1\) \+ 1);", "(u32)bits_for(S + 1) + 1"),
    ("bwt.hpp", r"const bool direct = (h.aux_active >= kn.aux_min && r_aux <= 8 \* B);", "h.aux_active >= kn.aux_min && r_aux <= 8 * B"),
    ("bwt.hpp", r"if \(is_r\) \{ succ = \(u64\)R.mark\[y\] - 1; break; \}\s+if \((k >= B)\)", "k >= B"),
]
assert TILE == 4096
M64 = (1 << 64) - 1


def bits_for(count):
    """smallest b with 2^b >= count (csrc/common.hpp)"""
    return 0 if count <= 1 else int(count - 1).bit_length()


def mix64(x):
    x &= M64
    for shift, mul in MIX:
        x ^= x >> shift
        if mul:
            x = x * mul & M64
    return x


def hash_rulers(n, ruler):
    """the ranks the hash selects: mix64(x ^ salt) & (ruler - 1) == 0, salt = 0x5851f42d4c957f2d ^ n"""
    x = np.arange(n, dtype=np.uint64) ^ np.uint64(SALT ^ n)
    for shift, mul in MIX:
        x = x ^ (x >> np.uint64(shift))
        if mul:
            x = x * np.uint64(mul)
    return np.nonzero(x & np.uint64(ruler - 1) == 0)[0]


# ---- texts ------------------------------------------------------------------------------------------------------------------
A256 = np.arange(256)
A254 = np.arange(1, 255)                               # empty buckets at both ends of the byte range


def text_with_primary(n, p, seed, alphabet=A256):
    """t[0] = c, which occurs nowhere else, and exactly p - 1 of the other n - 1 symbols are below c: exactly p - 1 suffixes
    sort before suffix 0, so the primary index is p (1 <= p <= n)"""
    assert 1 <= p <= n
    rng = np.random.default_rng(seed)
    alphabet = np.sort(np.asarray(alphabet))
    need_lo, need_hi = p > 1, p < n
    ok = [j for j in range(alphabet.size) if (j > 0 or not need_lo) and (j < alphabet.size - 1 or not need_hi)]
    assert ok, "the alphabet has no symbol with others on the sides p asks for"
    j = ok[len(ok) // 2]
    lo, hi = alphabet[:j], alphabet[j + 1:]
    rest = np.concatenate([lo[rng.integers(0, max(lo.size, 1), p - 1)] if need_lo else np.zeros(0, np.int64),
                           hi[rng.integers(0, max(hi.size, 1), n - p)] if need_hi else np.zeros(0, np.int64)])
    return np.concatenate([[alphabet[j]], rng.permutation(rest)]).astype(np.uint8)


SIZES = (2, 3, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8191, 8192, 8193, 12289)
Case = namedtuple("Case", "name text primary")


def primaries(n):
    return sorted(set(p for p in (1, 2, 15, 16, 17, 4095, 4096, 4097, n - 1, n) if 1 <= p <= n))


def primary_cases():
    out = []
    for n in SIZES:
        for j, p in enumerate(primaries(n)):
            out.append(Case("n%d_p%d" % (n, p), text_with_primary(n, p, 1000 * n + p, A254 if j % 2 else A256), p))
    return out


def alphabet_cases():
    """(name, text): one symbol, {0, 255}, 256 symbols, 1..254, only 0, only 255"""
    rng = np.random.default_rng(4)
    out = []
    for n in (17, 4097):
        out += [("one_symbol_%d" % n, np.full(n, 97, np.uint8)), ("only_0_%d" % n, np.zeros(n, np.uint8)),
                ("only_255_%d" % n, np.full(n, 255, np.uint8)),
                ("two_0_255_%d" % n, np.array([0, 255], np.uint8)[rng.integers(0, 2, n)]),
                ("all_256_%d" % n, rng.integers(0, 256, n).astype(np.uint8)),
                ("mid_1_254_%d" % n, rng.integers(1, 255, n).astype(np.uint8))]
    out.append(("two_0_255_p1", text_with_primary(33, 1, 5, [0, 255])))
    out.append(("two_0_255_pn", text_with_primary(33, 33, 6, [0, 255])))
    return out


def all_texts():
    """name -> text, every forward case"""
    out = {c.name: c.text for c in primary_cases()}
    out.update(alphabet_cases())
    return out


def inverse_names():
    """the texts the inverse plans run on: per size the first, a middle and the last primary index, and every alphabet"""
    out = []
    for n in SIZES:
        ps = primaries(n)
        out += ["n%d_p%d" % (n, p) for p in sorted({ps[0], ps[len(ps) // 2], ps[-1]})]
    return out + [name for name, _ in alphabet_cases()]


def next_pow2(n):
    return max(2, 1 << bits_for(n))


# ---- psi and the ruler model ------------------------------------------------------------------------------------------------
def psi_of(U, primary):
    """psi[cum[U[u]] + #{u' < u: U[u'] = U[u]}] = row(u), row(0) = primary - 1, row(u) = u - 1 below primary, u from it on;
    -> (psi, F) with F[d] the first character of rank d"""
    U = np.asarray(U, np.uint8)
    order = np.argsort(U, kind="stable")
    row = np.where(order == 0, primary - 1, np.where(order < primary, order - 1, order))
    return row.astype(np.int64), U[order]


def decode(U, primary):
    """T[k] = F(psi^k(primary - 1))"""
    psi, F = psi_of(U, primary)
    out = np.empty(U.size, np.uint8)
    x = primary - 1
    for k in range(U.size):
        out[k] = F[x]
        x = psi[x]
    return out


Sim = namedtuple("Sim", "aux_only rulers ruler_rounds longest_walk rank_rounds max_rounds cap stops_at_B_on_ruler claims")


def simulate(U, I, r_aux, walk=WALK, ruler=RULER, aux_min=AUX_MIN):
    """The host loop of run_unbwt: aux rulers (duplicates keep their id and never walk), the aux-only decision, hash rulers,
    then rounds of walks of at most B = walk steps -- a walk stops on a ruler, or after B steps claims the row it has
    reached, which walks in the next round.  stops_at_B_on_ruler: walks whose B-th step reached a ruler (no claim)."""
    U = np.asarray(U, np.uint8)
    n = U.size
    B = walk
    m = (n - 1) // r_aux + 1
    assert len(I) == m
    psi = psi_of(U, int(I[0]))[0].tolist()
    is_r = [False] * n
    starts, aux_active = [], 0
    for t in range(m):
        x = int(I[t]) - 1
        assert 0 <= x < n
        if is_r[x]:
            starts.append(None)
        else:
            is_r[x] = True
            starts.append(x)
            aux_active += 1
    direct = aux_active >= aux_min and r_aux <= 8 * B
    hashed = hash_rulers(n, ruler)
    cap = m + hashed.size + (n + B - 1) // B + 2
    if not direct:
        for x in hashed.tolist():
            if not is_r[x]:
                is_r[x] = True
                starts.append(x)
    max_rounds = (n + B - 1) // B + 1
    lo, hi, rounds, longest, exact, claims = 0, len(starts), 0, 0, 0, 0
    while lo < hi:
        assert rounds < max_rounds, "more walk rounds than the bound"
        new = []
        for x in starts[lo:hi]:
            if x is None:
                continue
            k = 0
            while True:
                k += 1
                y = psi[x]
                if is_r[y]:
                    exact += k == B
                    break
                if k >= B:
                    is_r[y] = True
                    new.append(y)
                    break
                x = y
            longest = max(longest, k)
        starts += new
        claims += len(new)
        rounds += 1
        lo, hi = hi, len(starts)
    S = len(starts)
    assert S <= cap
    return Sim(int(direct), S, rounds, longest, 0 if direct else bits_for(S + 1) + 1, max_rounds, cap, exact, claims)


# ---- plans ------------------------------------------------------------------------------------------------------------------
PLANS = {
    "default": {},
    "rounds": {"SA_HIP_UNBWT_WALK": "8", "SA_HIP_UNBWT_RULER": "64"},
    "one_ruler": {"SA_HIP_UNBWT_WALK": "8", "SA_HIP_UNBWT_RULER": str(1 << 30)},
    "all_rulers": {"SA_HIP_UNBWT_RULER": "1"},
    "aux_only_8": {"SA_HIP_UNBWT_AUX_MIN": "1", "SA_HIP_UNBWT_WALK": "8"},
    "aux_only_16": {"SA_HIP_UNBWT_AUX_MIN": "1", "SA_HIP_UNBWT_WALK": "16"},
}


def plan_knobs(plan):
    e = PLANS[plan]
    return dict(walk=int(e.get("SA_HIP_UNBWT_WALK", WALK)), ruler=int(e.get("SA_HIP_UNBWT_RULER", RULER)),
                aux_min=int(e.get("SA_HIP_UNBWT_AUX_MIN", AUX_MIN)))


def plan_runs(plan, names=None):
    """(name of the text, r_aux or None for the plain form) of a plan.  one_ruler waits on the host once per 8 characters:
    beyond 33 characters it keeps one text per size.  The aux-only plans take every r_aux up to 8 B and the next one,
    which must fall back to the ranked plan."""
    names = inverse_names() if names is None else names
    texts = all_texts()
    out = []
    for name in names:
        n = texts[name].size
        if plan == "one_ruler":
            mid = "n%d_p%d" % (n, primaries(n)[len(primaries(n)) // 2])
            if n > 33 and name != mid:
                continue
            rs = [None, 16]
        elif plan.startswith("aux_only"):
            B = plan_knobs(plan)["walk"]
            rs = [r for r in (2, 4, 8, 16, 64, 128, 256) if r <= 16 * B]
        elif plan == "all_rulers":
            rs = [None]
        else:
            rs = [None, 2, 16]
        out += [(name, r) for r in rs]
    return out
