"""A model of query_one (csrc/sa_query.hpp) that records WHERE a bound was found, the texts and pattern sets that put a bound on
every slot the kernel steps by, and the deliberate mistakes the sets must catch (tests/test_query_cases_cpu.py,
tests/test_gpu_query_edges.py); plain NumPy / Python, no GPU.

query_one finds the range of a pattern in stages, and every stage has a fallback: the window walk of sector_bound hands [lo, hi]
to the every-64th-key samples, the samples to a plain bisection, the second-level keys (phase 1b) to the text search.  A stage
that wrongly shrinks [lo, hi] is wrong only for the patterns whose bound sits on that one slot, and a few thousand random
patterns over millions of slots do not ask it.  So the model follows the kernel step by step -- written from the header's
comments and the contract (the inclusive range of the suffixes whose first c = min(len, L) bytes equal the pattern; lb == n ->
{~0, ~0}) -- and its TRACE says what the result cannot show: the branch, the bucket against the window grid, per bound the
windows loaded and the stage it ended in, phase 1b's group and phase 2's form.  The model is never the judge: expected ranges
come from the oracle, the model's own ranges are checked against the oracle for every pattern, and the traces only MEASURE
which edges a case's patterns reach (CLAIMS below; a claim no pattern reaches fails the CPU test).

K and dir come from query_struct_cases.stored_keys / directory, pinned equal to the device's by test_gpu_query_structs.py.  The
two arrays of the deep keys get models here:
  K2   sa_query.hpp, k2_build_kernel: "K2[j] = the k2n characters that follow the key of slot j (codes of b bits, MSB first, left
       aligned; 0 past the end of the text or of a truncated index's depth), for every slot whose key equals a neighbour's";
       "a key group = the slots that share the key's first k0 CHARACTERS" (the stored key of the 10-byte plan holds one bit more).
  S    skeys_kernel: S[i] = K[64 i].

Texts: query_struct_cases.GENERATORS, and one more, `sized`: no text of that list gives directory buckets of a chosen size at a
chosen place of the window grid.  sized() uses 200 byte values (b = 8), so that with an 8-bit directory a bucket is the set of
suffixes that start with one byte; the bytes 1..D ("designated") occur exactly as often as SPEC says, in code order, so the
first slot of every designated bucket is the sum of the sizes before it -- chosen -- and a part of a bucket's occurrences is
followed by one fixed word, which makes a run of equal keys of a chosen length inside it (and a key group for phase 1b)."""
from collections import namedtuple

import numpy as np

import query_struct_cases as qs

SKEY_STRIDE, QC_DIGIT_BITS, QC_TILE, K2_AUTO_BATCH, CLUSTER_MIN, GRID_CAP = 64, 11, 4096, 32768, 1 << 20, 256 * 16
# restated from the sources; (file under suffixarray_amd/csrc, regular expression whose group 1 is the definition, value)
SOURCE_CONSTANTS = [
    ("sa_query.hpp", r"#define SA_SKEY_STRIDE (\d+)", "64"),
    ("sa_query.hpp", r"constexpr int QC_DIGIT_BITS = (\d+);", "11"),
    ("sa_query.hpp", r"constexpr u32 QC_TILE = (\d+);", "4096"),
    ("sa_capi.hip", r"constexpr u64 K2_AUTO_BATCH = (\d+);", "32768"),
    ("sa_capi.hip", r"u64 cluster_min = (1ull << 20);", "1ull << 20"),
    ("sa_capi.hip", r"if \(g > (256u \* 16u)\) g = 256u \* 16u;", "256u * 16u"),
    ("sa_capi.hip", r"bool cluster = (Q >= cluster_min && Q >= QC_TILE && Q < 0xFFFFFFFFull && a.keys && idx->k2_auto);",
     "Q >= cluster_min && Q >= QC_TILE && Q < 0xFFFFFFFFull && a.keys && idx->k2_auto"),
    ("sa_capi.hip", r"if \((Q >= K2_AUTO_BATCH && idx->k2_auto)\) \{ int rc = ensure_k2", "Q >= K2_AUTO_BATCH && idx->k2_auto"),
    ("sa_capi.hip", r"int k2n = (64 / \(b.q_b > 0 \? b.q_b : 1\));\s*if \(k2n > 16\) k2n = 16;", "64 / (b.q_b > 0 ? b.q_b : 1)"),
    ("sa_query.hpp", r"if \(MODE == 2\) \{   // 32-byte windows\s*SectorWindow<KT, (32)> w;", "32"),
    ("sa_query.hpp", r"\} else \{\s*SectorWindow<KT, (64)> w;", "64"),
    ("sa_query.hpp", r"const KT\* __restrict__ S = nullptr, int window_steps = (3)\)", "3"),
    ("sa_query.hpp", r"lo = sector_bound<false>\(K, l, h, t_lo, est, w, false, S, (big \? 0 : 3)\);", "big ? 0 : 3"),
    ("sa_query.hpp", r"sector_bound<true>\(K, lo, h, t_hi2, lo, w, (!big, S, big \? 2 : 3)\)", "!big, S, big ? 2 : 3"),
    ("sa_query.hpp", r"const bool big = (S && h - l > 64 \* SKEY_STRIDE);", "S && h - l > 64 * SKEY_STRIDE"),
    ("sa_query.hpp", r"if \((S && hi - lo > 2 \* SKEY_STRIDE)\) \{", "S && hi - lo > 2 * SKEY_STRIDE"),
    ("sa_query.hpp", r"if \(ia < ib0\) (hi = ia \* SKEY_STRIDE);", "hi = ia * SKEY_STRIDE"),
    ("sa_query.hpp", r"if \(ia > ia0\) (lo = \(ia - 1\) \* SKEY_STRIDE \+ 1);", "lo = (ia - 1) * SKEY_STRIDE + 1"),
    ("sa_query.hpp", r"if \(!NARROW && a.keys2 && !exact && (hi - lo > 1 && P == a.k0)\)", "hi - lo > 1 && P == a.k0"),
]
U64 = np.uint64
M64 = (1 << 64) - 1
NONE = 0xFFFFFFFF


def window_slots(key_bytes, mode):
    """W of sector_bound: 32-byte windows under mode 2, 64-byte windows under mode 1"""
    return (32 if mode == 2 else 64) // key_bytes


def k2n_of(b):
    return min(16, 64 // b)


# ---- the two arrays of the deep keys -------------------------------------------------------------------------------------------

def k2_keys(t, sa, code, b, k0, k2n, L, stored=None):
    """K2[j] for the slots tied with a neighbour in their first k0 characters, 0 elsewhere (never read) -> (K2, tied).
    stored: MISTAKE "k2_group_by_stored_key" -- the group taken from the stored keys (which differ inside a k0-character group
    under the 10-byte plan's partial character)"""
    n = int(sa.size)
    g = qs.full_keys(t, sa, code, b, k0) if stored is None else np.asarray(stored, U64)
    same = g[1:] == g[:-1]
    tied = np.concatenate([[False], same]) | np.concatenate([same, [False]])
    depth = (L - k0 if L > k0 else 0) if L else 1 << 40
    c = np.concatenate([np.asarray(code, U64)[t], np.zeros(k0 + k2n + 1, U64)])
    pos = np.asarray(sa, np.int64) + k0
    key = np.zeros(n, U64)
    for j in range(k2n):
        cj = c[np.minimum(pos + j, n)] if j < depth else np.zeros(n, U64)
        key = (key << U64(b)) | cj
    key <<= U64(64 - k2n * b)
    return np.where(tied, key, U64(0)), tied


def skeys(K):
    return np.ascontiguousarray(K[::SKEY_STRIDE])


# ---- the model -----------------------------------------------------------------------------------------------------------------

class Index:
    """what query_one reads: text, array, code map, plan, K, dir and (deep) K2, S"""

    def __init__(self, t, sa, L, k0, dbits, key_bytes=8, partial=False, deep=False, k2_mistake=None):
        self.t, self.tb, self.n, self.L = t, t.tobytes(), int(t.size), L
        self.sa = np.asarray(sa, np.int64)
        self.code_arr, self.sigma, self.b = qs.code_map(t)
        self.code = self.code_arr.tolist()
        self.k0, self.dbits, self.key_bytes, self.partial = k0, dbits, key_bytes, partial
        self.lo_shift = 64 - self.b * k0 if key_bytes == 4 else 0
        self.K, self.dkeys = qs.stored_keys(t, sa, self.code_arr, self.b, k0, key_bytes, self.lo_shift, partial)
        self.dir = qs.directory(self.dkeys, dbits).astype(np.int64)
        self.k2n, self.K2, self.S, self.tied = 0, None, None, None
        if deep:
            assert key_bytes == 8
            self.k2n = k2n_of(self.b)
            cut = 0 if k2_mistake == "k2_not_cut_at_L" else L
            self.K2, self.tied = k2_keys(t, sa, self.code_arr, self.b, k0, self.k2n, cut, self.K if k2_mistake == "k2_group_by_stored_key" else None)
            self.S = skeys(self.K)


def _cmp(ix, pos, qc):
    """cmp_suffix: the suffix against the c pattern bytes; a suffix that ends before c bytes compares less"""
    s = ix.tb[pos:pos + len(qc)]
    return 0 if s == qc else (-1 if s < qc else 1)


def sector_bound(ix, strict, l, h, tk, est, win, have_window, S, window_steps, W, tr, mistake=None):
    """first slot in [l, h) whose key is >= tk (strict: > tk), h if none; l < h.  win: [base of the window held]"""
    K = ix.K
    lo, hi = l, h
    base = est & ~(W - 1)
    seq = ""
    for _ in range(window_steps):
        if not lo < hi:
            break
        if have_window and win[0] == base:
            tr["saved"] = True
        else:
            tr["loads"] += 1
            win[0] = base
        have_window = False
        a, e = max(base, lo), min(base + W, hi)
        x0, x1 = (max(base, 0), min(base + W, ix.n)) if mistake == "in_mask_dropped" else (a, e)
        ks = K[x0:x1]
        if strict:
            below = int((ks <= tk).sum()) if mistake != "strict_lt" else int((ks < tk).sum())
        else:
            below = int((ks < tk).sum())
        if mistake is None and (a > base or e < base + W):
            # would the keys of the window outside [a, e) change the count?  (they belong to another bucket, or lie below lo)
            o = K[max(base, 0):min(base + W, ix.n)]
            if int((o <= tk).sum() if strict else (o < tk).sum()) != below:
                tr["mask_matters"] = True
        if below == 0:
            hi = a
            if a == lo:
                seq += "L"
                break
            seq += "l"
            base = base + W if mistake == "base_wrong_way" else base - W
        elif below == e - a:
            lo = e
            if e == hi:
                seq += "R"
                break
            seq += "r"
            base = base - W if mistake == "base_wrong_way" else base + W
        else:
            lo = hi = a + below
            seq += "i"
        if base < 0 or base >= ix.n + W:      # (only a mistaken walk leaves the array)
            break
    tr["seq"] = seq
    tr["end"] = "window"
    if lo < hi:
        tr["ran_out"] = window_steps > 0
        tr["end"] = "bisect"
        if S is not None:
            tr["span"] = hi - lo
        if S is not None and hi - lo > 2 * SKEY_STRIDE:
            ia, ib = (lo + SKEY_STRIDE - 1) // SKEY_STRIDE, (hi - 1) // SKEY_STRIDE + 1
            ia0, ib0 = ia, ib
            tr["lo64"], tr["hi64"] = lo % SKEY_STRIDE == 0, (hi - 1) % SKEY_STRIDE == 0
            tr["last_sample"] = ib0 == (ix.n - 1) // SKEY_STRIDE + 1
            while ia < ib:
                mid = (ia + ib) >> 1
                k = int(S[mid])
                if (k <= tk) if strict else (k < tk):
                    ia = mid + 1
                else:
                    ib = mid
            if ia < ib0:
                hi = ia * SKEY_STRIDE + {"sample_hi_plus_1": 1, "sample_hi_minus_1": -1}.get(mistake, 0)
            if ia > ia0:
                lo = (ia - 1) * SKEY_STRIDE + {"sample_lo_minus_1": 0, "sample_lo_plus_2": 2}.get(mistake, 1)
            tr["end"] = "samples"
            tr["ia"] = "ia0" if ia == ia0 else ("ib0" if ia == ib0 else "mid")
        tr["left"] = hi - lo
        while lo < hi:
            mid = (lo + hi) >> 1
            k = int(K[mid])
            if (k <= tk) if strict else (k < tk):
                lo = mid + 1
            else:
                hi = mid
    return lo


def _new_bound():
    return {"loads": 0, "saved": False, "seq": "", "end": None}


def query_model(ix, pattern, mode, mistake=None):
    """-> (first, second, trace) of one pattern on the Index ix under SA_HIP_SECTOR_SEARCH = mode"""
    n, b, k0, K = ix.n, ix.b, ix.k0, ix.K
    narrow = ix.key_bytes == 4
    c = len(pattern)
    if ix.L and c > ix.L:
        c = ix.L
    qc = pattern[:c]
    tr = {"c": c}
    lo, hi, exact, P = 0, n, False, 0
    pmax = min(c, k0)
    key_lo, sh = 0, 64
    while P < pmax:
        cd = ix.code[qc[P]]
        if cd == 0:
            tr["absent_in_key"] = P
            break
        sh -= b
        key_lo |= cd << sh
        P += 1
    tr["P"] = P
    if P == 0:
        tr["branch"] = "no_key"
    else:
        key_hi = key_lo | (((1 << sh) - 1) if sh > 0 else 0)
        ds = 64 - ix.dbits
        bl, bh = key_lo >> ds, key_hi >> ds
        d = ix.dir
        l, h = int(d[bl]), int(d[bl + 1])
        h_strict = h if bh == bl else int(d[bh + 1])
        h2_lo = 0 if bh == bl else int(d[bh])
        tr.update(bl=bl, bh=bh, l=l, h=h, last_bucket=bl == (1 << ix.dbits) - 1, at_n=l == n)
        if narrow:
            ls = ix.lo_shift
            t_lo, t_hi2 = (key_lo >> ls) & NONE, (key_hi >> ls) & NONE
            same_top = (key_lo >> 56) == (key_hi >> 56)
            t_hi1 = t_hi2 if (same_top or mistake == "t_hi1_not_widened") else NONE
            tr["same_top"] = same_top
            tr["key_bits"] = 64 - ls
        else:
            t_lo, t_hi1, t_hi2 = key_lo, key_hi, key_hi
        searched = False
        if bh != bl:
            tr["branch"] = "span"
            tr["span_buckets"] = bh - bl + 1
            tr["end_marker"] = bh == (1 << ix.dbits) - 1
            tr["empty_ends"] = l == h and h2_lo == h_strict
        else:
            tr["branch"] = "one_bucket" if l < h else "empty_bucket"
        if mode != 0 and bh == bl and l < h:
            W = window_slots(ix.key_bytes, mode)
            vs = ix.lo_shift if narrow else 0
            sb = ds - vs
            est = l
            tr["sb"] = sb
            if sb > 0:
                frac = (key_lo >> vs) & ((1 << sb) - 1)
                down = sb - 20 if sb > 20 else 0
                est = l + (((frac >> down) * (h - l)) >> (sb - down))
                if est >= h:
                    tr["clamped"] = True
                    if mistake != "estimate_not_clamped":
                        est = h - 1
            S = None if narrow else ix.S
            win = [-1]
            tr["W"], tr["est_window"] = W, (est & ~(W - 1))
            lb_tr, ub_tr = _new_bound(), _new_bound()
            if mode == 2:
                big = S is not None and h - l > 64 * SKEY_STRIDE
                tr["big"] = big
                lo = sector_bound(ix, False, l, h, t_lo, est, win, False, S, 0 if big else 3, W, lb_tr, mistake)
                hi = sector_bound(ix, True, lo, h, t_hi2, lo, win, not big, S, 2 if big else 3, W, ub_tr, mistake) if lo < h else lo
            else:
                lo = sector_bound(ix, False, l, h, t_lo, est, win, False, S, 3, W, lb_tr, mistake)
                hi = sector_bound(ix, True, lo, h, t_hi2, lo, win, True, S, 3, W, ub_tr, mistake) if lo < h else lo
            tr["lb"], tr["ub"] = lb_tr, (ub_tr if lo < h else None)
            searched = True
        if not searched:
            while l < h:
                mid = (l + h) >> 1
                k = int(K[mid])
                if k < t_lo:
                    l = mid + 1
                else:
                    h = mid
                    if k > t_hi1:
                        h_strict = mid
            lo = l
            l2 = lo if bh == bl else max(h2_lo, lo)
            h2 = h_strict
            while l2 < h2:
                mid = (l2 + h2) >> 1
                if int(K[mid]) <= t_hi2:
                    l2 = mid + 1
                else:
                    h2 = mid
            hi = l2
        exact = P == c
        tr["key_range"] = (lo, hi)
    # phase 1b
    if not narrow and ix.K2 is not None and not exact and hi - lo > 1 and P == k0:
        k2n = ix.k2n
        m2 = min(c - k0, k2n)
        if mistake == "m2_off_by_one":
            m2 = max(m2 - 1, 1)
        q2, absent = 0, False
        for i in range(m2):
            cd = ix.code[qc[k0 + i]]
            absent |= cd == 0
            q2 = (q2 << b) | cd
        tr["p1b"] = {"m2": m2, "k2n": k2n, "group": hi - lo, "absent": absent}
        if not absent:
            sh2 = 64 - m2 * b
            q2_lo = (q2 << sh2) & M64
            q2_hi = q2_lo | ((1 << sh2) - 1)
            K2 = ix.K2 if mistake != "k2_zero_group" else np.zeros(n, U64)
            assert ix.tied is None or bool(ix.tied[lo:hi].all()) or mistake, "phase 1b read a slot outside every key group"
            g = K2[lo:hi]
            tr["p1b"]["all_equal"] = bool((g == g[0]).all())
            tr["p1b"]["zero_entries"] = bool((g == 0).any())
            tr["p1b"]["stored_differ"] = bool(K[lo] != K[hi - 1])
            l, h, h_strict = lo, hi, hi
            while l < h:
                mid = (l + h) >> 1
                k2 = int(K2[mid])
                if k2 < q2_lo:
                    l = mid + 1
                else:
                    h = mid
                    if k2 > q2_hi:
                        h_strict = mid
            lb2 = l
            h = h_strict
            while l < h:
                mid = (l + h) >> 1
                if int(K2[mid]) <= q2_hi:
                    l = mid + 1
                else:
                    h = mid
            lo, hi = lb2, l
            exact = c <= k0 + k2n
            tr["p1b"]["exact"] = exact
            tr["p1b"]["range"] = (lo, hi)
    # phase 2
    lb, ub = lo, hi
    if not exact and hi - lo == 1:
        pos = int(ix.sa[lo])
        r = _cmp(ix, pos, qc)
        tr["p2"] = ("single", r)
        if r < 0 and qc.startswith(ix.tb[pos:pos + c]):
            tr["short_suffix"] = True
        lb = hi if r < 0 else lo
        if mistake == "single_ub_from_ge":
            ub = lo if r >= 0 else hi
        else:
            ub = lo if r > 0 else hi
    elif not exact:
        tr["p2"] = ("double", hi - lo)
        l, h, h_strict = lo, hi, hi
        while l < h:
            mid = (l + h) >> 1
            pos = int(ix.sa[mid])
            r = _cmp(ix, pos, qc)
            if r < 0:
                if qc.startswith(ix.tb[pos:pos + c]):
                    tr["short_suffix"] = True
                l = mid + 1
            else:
                h = mid
                if r > 0:
                    h_strict = mid
        lb = l
        h = h_strict
        while l < h:
            mid = (l + h) >> 1
            if _cmp(ix, int(ix.sa[mid]), qc) <= 0:
                l = mid + 1
            else:
                h = mid
        ub = l
    else:
        tr["p2"] = ("exact", 0)
    if lb == n:
        return NONE, NONE, tr
    return lb, (ub - 1) & NONE, tr


def query_trace(t, sa, code, b, k0, dbits, key_bytes, lo_shift, L, mode, K, dir, pattern, K2=None, S=None, k2n=0):
    """the model over arrays given one by one (the device's own K and dir, read back, for a report)"""
    ix = Index.__new__(Index)
    ix.t, ix.tb, ix.n, ix.L, ix.sa = t, t.tobytes(), int(t.size), L, np.asarray(sa, np.int64)
    ix.code, ix.b, ix.k0, ix.dbits, ix.key_bytes, ix.lo_shift = list(code), b, k0, dbits, key_bytes, lo_shift
    ix.K, ix.dir, ix.K2, ix.S, ix.k2n, ix.tied = K, np.asarray(dir, np.int64), K2, S, k2n, None
    return query_model(ix, pattern, mode)


def describe(tr):
    """one line for an error message: bucket, window walk, the stage each bound was found in"""
    out = ["branch %s, P = %d, c = %d" % (tr.get("branch"), tr.get("P", 0), tr["c"])]
    if "l" in tr:
        out.append("bucket %d [%d, %d) of %d slots" % (tr["bl"], tr["l"], tr["h"], tr["h"] - tr["l"]))
    if "W" in tr:
        out.append("W = %d, l %% W = %d, h %% W = %d, estimate's window %d%s%s" % (
            tr["W"], tr["l"] % tr["W"], tr["h"] % tr["W"], tr["est_window"], ", clamped" if tr.get("clamped") else "", ", big" if tr.get("big") else ""))
        for name in ("lb", "ub"):
            bt = tr.get(name)
            if bt:
                out.append("%s: walk '%s', %d loads%s, ended in %s%s%s" % (
                    name, bt["seq"], bt["loads"], " (one saved)" if bt["saved"] else "", bt["end"],
                    " (%s)" % bt["ia"] if "ia" in bt else "", ", %d slots bisected" % bt["left"] if "left" in bt else ""))
    if "key_range" in tr:
        out.append("key range [%d, %d)" % tr["key_range"])
    if "p1b" in tr:
        out.append("phase 1b %s" % tr["p1b"])
    out.append("phase 2 %s" % (tr["p2"],))
    return "; ".join(out)


# ---- texts ---------------------------------------------------------------------------------------------------------------------

SIGMA = 200                      # bytes 1..200: b = 8
WORD = (150, 120, 180, 120, 199, 101, 170, 130, 130, 160, 110)     # the symbols that follow a planted occurrence (all fillers)


def sized_spec(W2, W1):
    """(bucket size, planted run) of the designated bytes 1..D, in code order.  W2, W1: window slots under mode 2 and 1.  Sizes
    1, W - 1, W, W + 1, 2W, 3W + 1 for both W; 128, 129, 4096, 4097; pads of 1..3 slots move the buckets over the window grid;
    runs of W, W + 1, 3W + 1, 129 and 4097 equal keys: a whole bucket, or inside a larger one (the fixed word sorts in the middle
    of the fillers)."""
    spec = []
    for W in (W2, W1):
        for s in (1, W - 1, W, W + 1, 2 * W, 3 * W + 1):
            spec += [(s, 0), (s, 0)]
        spec += [(1, 0), (W, W), (W + 1, W + 1), (3 * W + 1, 3 * W + 1), (2, 0), (4 * W, W), (4 * W + 1, W + 1), (6 * W, 3 * W + 1), (1, 0)]
    spec += [(128, 0), (129, 0), (129, 129), (3, 0), (4096, 0), (4097, 0), (1, 0), (4096, 129), (4097, 4097), (2, 0), (300, 129)]
    return spec


def sized(n, spec, seed=21, tail=0.0):
    """tail: that share of the text is the LAST byte of the alphabet, half of the time followed by the smallest filler -- one
    bucket of thousands of unevenly spread keys that ends at slot n (the last sample of the array)"""
    rng = np.random.default_rng(seed)
    D = len(spec)
    assert D < 100 and all(D < w <= SIGMA for w in WORD)
    fill = np.arange(D + 1, SIGMA + 1).astype(np.uint8)
    planted = sum(r for _, r in spec)
    m = n - len(WORD) * planted
    sym = np.zeros(m, np.uint8)
    pl = np.zeros(m, bool)
    at = 0
    for i, (s, r) in enumerate(spec):
        sym[at:at + s] = i + 1
        pl[at:at + r] = True
        at += s
    assert at + fill.size + 3 <= m, "n too small for the spec"
    order = np.concatenate([rng.permutation(m - 3), [m - 3, m - 2, m - 1]])      # the text ends in three fillers
    sym, pl = sym[order], pl[order]
    length = 1 + len(WORD) * pl.astype(np.int64)
    off = np.cumsum(length) - length
    t = fill[rng.integers(0, fill.size, n)]
    if tail:
        t[rng.random(n) < tail] = fill[-1]
    free = np.flatnonzero(sym == 0)[:fill.size]
    t[off[free]] = fill                                                            # every filler occurs
    t[off[sym > 0]] = sym[sym > 0]
    for j, w in enumerate(WORD):
        t[off[pl] + 1 + j] = w
    if tail:
        at = np.flatnonzero((t[:-1] == fill[-1]) & (t[1:] > D) & (rng.random(n - 1) < 0.5))
        at = at[at + 1 < n - 3]
        t[at + 1] = np.where(t[at + 1] == fill[-1], fill[-1], fill[0])
    return np.ascontiguousarray(t)


def make_text(name, n):
    if name == "sized_wide":
        return sized(n, sized_spec(4, 8))
    if name == "sized_tail":
        return sized(n, [(1, 0), (2, 0)], tail=0.6)
    if name == "sized_narrow":
        return sized(n, sized_spec(8, 16))
    if name == "abc3":
        return abc3(n)
    return qs.make(name, n)


def abc3(n, seed=23):
    """the bytes a, b, c at random, every c that would be the fourth of a run replaced by a: sigma = 3, b = 2, the code of c is 3"""
    t = np.array([97, 98, 99], np.uint8)[np.random.default_rng(seed).integers(0, 3, n)]
    run = 0
    for i in range(n):
        run = run + 1 if t[i] == 99 else 0
        if run == 4:
            t[i], run = 97, 0
    t[:3] = (97, 98, 99)
    return np.ascontiguousarray(t)


# ---- pattern sets --------------------------------------------------------------------------------------------------------------

def every_bound(t, sa, m, L=0):
    """the distinct m-byte prefixes of all suffixes: every slot that starts a run of equal m-prefixes is a lower bound, every
    slot that ends one an upper bound.  -> (rows u8[k, m], first, second): the ranges read off the sorted array itself (one
    flatnonzero; the CPU test checks this shortcut against the oracle).  m <= L on a truncated array."""
    assert L == 0 or m <= L
    n = int(t.size)
    sa = np.asarray(sa, np.int64)
    tp = np.concatenate([t, np.zeros(m, np.uint8)]).astype(np.int16)
    tp[n:] = -1                                                  # past the end: unlike any byte
    pre = tp[sa[:, None] + np.arange(m)[None, :]]
    new = np.concatenate([[True], (pre[1:] != pre[:-1]).any(axis=1)])
    start = np.flatnonzero(new)
    end = np.concatenate([start[1:], [n]]) - 1
    whole = pre[start, m - 1] >= 0                               # suffixes shorter than m are no m-byte pattern
    return pre[start[whole]].astype(np.uint8), start[whole].astype(np.uint32), end[whole].astype(np.uint32)


def between(t, sa, k0, alph, pre=None):
    """for every pair of adjacent distinct k0-prefixes A < B: the k0-byte strings just above A and just below B (last byte moved
    to the next / previous byte of the alphabet) when they lie strictly between -- misses whose bound is B's first slot; at the
    two ends of a directory bucket they are the patterns below its first and above its last key, and those that fall into an
    empty bucket ask that one.  Also below the first and above the last key of the text.  -> (rows u8[k, k0], the bound's slot)"""
    rows, f, s = pre if pre is not None else every_bound(t, sa, k0)      # (pre: every_bound(t, sa, k0), already made)
    if rows.shape[0] == 0:
        return np.zeros((0, k0), np.uint8), np.zeros(0, np.int64)
    alph = np.asarray(alph, np.int64)
    nxt = np.full(256, -1, np.int64)
    prv = np.full(256, -1, np.int64)
    nxt[alph[:-1]] = alph[1:]
    prv[alph[1:]] = alph[:-1]
    A, B = rows[:-1], rows[1:]
    same_head = (A[:, :-1] == B[:, :-1]).all(axis=1)
    up = nxt[A[:, -1]]
    ok = (up >= 0) & (~same_head | (up < B[:, -1]))
    above = A[ok].copy()
    above[:, -1] = up[ok]
    dn = prv[B[:, -1]]
    ok2 = (dn >= 0) & (~same_head | (dn > A[:, -1]))
    below = B[ok2].copy()
    below[:, -1] = dn[ok2]
    ends, at = [], []
    for r, x, slot in ((rows[0], prv[rows[0][-1]], 0), (rows[-1], nxt[rows[-1][-1]], int(s[-1]) + 1)):
        if x >= 0:
            e = r.copy()
            e[-1] = x
            ends.append(e)
            at.append(slot)
    out = np.concatenate([above, below] + ([np.stack(ends)] if ends else []))
    slot = np.concatenate([f[1:][ok], f[1:][ok2], np.asarray(at, np.int64)]).astype(np.int64)
    return out, slot


def beyond_key(t, sa, code, b, k0, k2n, limit=None, seed=5, first_max=0):
    """for every slot of every key group of two or more slots: the prefixes of its suffix of k0 + 1, k0 + k2n - 1, k0 + k2n,
    k0 + k2n + 1 and 33 bytes, and each with its last byte raised, lowered and replaced by an absent byte; an absent byte at
    k0 and inside the second key as well.  limit: None takes every slot (the device test); the CPU test traces a fixed draw of
    that many slots.  first_max: only the groups whose suffixes start with a byte up to that one (the designated buckets of a
    sized text: the planted runs)."""
    n = int(t.size)
    g = qs.full_keys(t, sa, code, b, k0)
    same = g[1:] == g[:-1]
    tied = np.flatnonzero(np.concatenate([[False], same]) | np.concatenate([same, [False]]))
    if first_max:
        tied = tied[t[np.asarray(sa, np.int64)[tied]] <= first_max]
    if limit is not None and tied.size > limit:
        tied = tied[np.sort(np.random.default_rng(seed).choice(tied.size, limit, replace=False))]
    absent = np.flatnonzero(np.asarray(code) == 0)
    absent = absent[absent > 0]
    ab = int(absent[absent.size // 2]) if absent.size else None
    tb = t.tobytes()
    out = set()
    for j in tied.tolist():
        p = int(sa[j])
        for m in sorted({k0 + 1, k0 + k2n - 1, k0 + k2n, k0 + k2n + 1, 33}):
            w = tb[p:p + m]
            if len(w) <= k0:
                continue
            out.add(w)
            last = w[-1]
            if last < 255:
                out.add(w[:-1] + bytes([last + 1]))
            if last > 1:
                out.add(w[:-1] + bytes([last - 1]))
            if ab is not None:
                out.add(w[:-1] + bytes([ab]))
                out.add(w[:k0] + bytes([ab]) + w[k0 + 1:])           # an absent byte at k0
                if len(w) > k0 + 2:
                    out.add(w[:k0 + 1] + bytes([ab]) + w[k0 + 2:])   # ... inside the second key
    return sorted(out)


def long_patterns(t, sa, rng, count=40):
    """text windows of 33, 39, 40 and 41 bytes (past the four-word register window of cmp_suffix, tails of 1 and 7 bytes, none), as
    they are and with the last byte changed; patterns that run past the end of the text"""
    n = int(t.size)
    tb = t.tobytes()
    out = []
    for m in (33, 39, 40, 41):
        for p in rng.integers(0, max(n - m, 1), count).tolist():
            w = tb[p:p + m]
            out += [w, w[:-1] + bytes([(w[-1] % 255) + 1]), w[:32] + bytes([(w[32] % 255) + 1]) + w[33:]]
        out += [tb[n - m + 5:] + tb[:5], tb[max(n - m, 0):] + b"\x01", tb[max(n - 20, 0):] + bytes([255]) * (m - 20)]
    return out


def truncation_patterns(t, L, rng, count=60):
    """L > 0: patterns longer than L that differ only behind L are hits"""
    n = int(t.size)
    tb = t.tobytes()
    out = []
    for p in rng.integers(0, max(n - L - 8, 1), count).tolist():
        w = tb[p:p + L]
        out += [w + b"\x01", w + bytes([255]) * 5, w + tb[:9], w[:L - 1] + bytes([(w[-1] % 255) + 1]) + b"zz"]
    return out


def short_spans(ix):
    """patterns shorter than the directory bits: every 1-symbol string, and the 2-symbol strings over the first, middle and last eight symbols, present or not
    -- spans of 2 and of many buckets, the span that ends in the last bucket, spans with empty buckets at both ends"""
    alph = np.flatnonzero(np.asarray(ix.code) > 0)
    out = [bytes([int(a)]) for a in alph]
    if alph.size > 1:
        pick = alph if alph.size <= 40 else alph[np.r_[0:8, alph.size // 2 - 4:alph.size // 2 + 4, alph.size - 8:alph.size]]
        out += [bytes([int(a), int(c)]) for a in pick for c in pick]
    return out


def random_misses(ix, text, rng, count=600):
    """strings of 3 and of k0 symbols drawn from the alphabet (mostly absent: bounds anywhere, empty buckets); on the crafted chain
    the symbol 30 followed by what never follows it (the buckets between its three followers are empty); runs of the last symbol"""
    alph = np.flatnonzero(np.asarray(ix.code) > 0).astype(np.uint8)
    out = [bytes(alph[rng.integers(0, alph.size, m)]) for m in (3, max(ix.k0, 1)) for _ in range(count)]
    top = bytes(alph[-1:])                   # runs of the last symbol: the last buckets of the directory, used or empty
    out += [top * m + x for m in (3, 4, 5, 6, 8, 12) for x in (b"", bytes(alph[:1]), bytes(alph[-2:-1]))]
    if text == "markov":
        out += [bytes([qs.X, a, c]) for a in range(2, 101, 7) for c in (1, 50, 100)]
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------
# Case: id, text, n on the device, n of the CPU test (the claims hold there too, or it is the full size), forced switches, k0 and
# dbits that result (asserted against the device's layout), key bytes, the truncation depths, the claims (CLAIMS keys).
Case = namedtuple("Case", "id text n n_cpu env k0 dbits key_bytes Ls claims partial")

# A claim is a key of CLAIMS, or "key:item|item" for some of its items.
WINDOW = ("bucket_sizes", "grid", "bound_pos", "window_edge", "walk", "walk_runs_out", "runs", "have_window", "mask_matters", "phase2")
D8 = {"SA_HIP_INITIAL_CHARS": "12", "SA_HIP_DIR_BITS": "8"}
S8 = {"SA_HIP_INITIAL_CHARS": "8", "SA_HIP_DIR_BITS": "8"}
CASES = [
    # wide keys, an 8-bit directory over 8-bit symbols: a bucket = the suffixes that start with one byte; sizes and places chosen
    Case("sized_wide", "sized_wide", 80_001, 80_001, {"SA_HIP_DIR_BITS": "8", "SA_HIP_INITIAL_CHARS": "8"}, 8, 8, 8, (0, 12, 8),
         WINDOW + ("samples", "big", "long", "short_suffix", "truncated", "phase1b:group > 128|m2 = 1|m2 = k2n - 1|m2 = k2n|exact|absent byte|all K2 of the group equal"), False),
    # the same text, the key one symbol long: key bits = dbits, every bucket one run of equal keys, the estimate the bucket's first slot (with
    # fewer key bits than directory bits a pattern spans buckets and never reaches the windows)
    Case("sized_wide_k1", "sized_wide", 80_001, 80_001, {"SA_HIP_DIR_BITS": "8", "SA_HIP_INITIAL_CHARS": "1"}, 1, 8, 8, (0,), ("short_key",), False),
    # word text: key groups of 2, 3, ... slots, the second-level keys, the text search behind them
    Case("words_wide", "words", 60_001, 9_001, {"SA_HIP_INITIAL_CHARS": "12"}, 12, 13, 8, (0, 12, 20),
         ("phase1b:group of 2|group of 3|m2 = 1|m2 = k2n - 1|m2 = k2n|exact|not exact, phase 2 over the narrowed range|absent byte", "phase2", "long",
          "span:many buckets|empty buckets at both ends", "empty_bucket:l == h in the middle", "truncated"), False),
    # ... under an 8-bit directory: buckets of thousands of slots with keys that are anything but evenly spread
    Case("words_wide_d8", "words", 60_001, 9_001, D8, 12, 8, 8, (0,), ("walk_runs_out",), False),
    # a bucket of thousands of unevenly spread keys that ends at slot n: the last sample of the array for n % 64 = 0, 1 and 63
    Case("tail_n0", "sized_tail", 8_960, 8_960, S8, 8, 8, 8, (0,), ("samples_last",), False),
    Case("tail_n1", "sized_tail", 8_961, 8_961, S8, 8, 8, 8, (0,), ("samples_last",), False),
    Case("tail_n63", "sized_tail", 9_023, 9_023, S8, 8, 8, 8, (0,), ("samples_last",), False),
    # one symbol (b = 1, its code all ones): a pattern shorter than the directory bits ends in the last bucket; one key group of
    # n - 63 slots whose second-level keys are 0 where the text ended
    Case("equal_wide", "equal", 9_001, 9_001, {"SA_HIP_INITIAL_CHARS": "64"}, 64, 11, 8, (0, 70),
         ("span:2 buckets|many buckets|ends in the last bucket", "phase1b:group > 128|K2 entries of 0"), False),
    Case("far2_wide", "far2", 9_001, 9_001, {"SA_HIP_INITIAL_CHARS": "32"}, 32, 11, 8, (0,), ("span:many buckets|empty buckets at both ends",), False),
    # three symbols (b = 2, the top code all ones) and no run of four of the third: the last bucket of the directory is empty, a
    # pattern that starts with five of it finds l == h == n there and answers {~0, ~0}
    Case("abc3_wide", "abc3", 9_001, 9_001, {"SA_HIP_INITIAL_CHARS": "32"}, 32, 11, 8, (0,), ("empty_bucket",), False),
    # the 10-byte-record plan with the partial character: 11 symbols of 5 bits and one bit of the twelfth in the stored key; a key
    # group is still the first 11 characters
    Case("words_partial", "words", qs.NARROW_MIN_N + 3, qs.NARROW_MIN_N + 3, {"SA_HIP_NARROW48": "1", "SA_HIP_INITIAL_CHARS": "11"}, 11, 20, 8, (0,),
         ("partial", "phase1b:group of 2|group of 3|group > 128|m2 = 1|exact|not exact, phase 2 over the narrowed range"), True),
    # narrow keys: 40 bits (top digit cut off) over the sized text; a 16-bit key under a 16-bit directory (sb = 0: est = l; with fewer key
    # bits than directory bits a pattern spans buckets and never reaches the windows, so sb < 0 does not occur there)
    Case("sized_narrow", "sized_narrow", qs.NARROW_MIN_N + 1, qs.NARROW_MIN_N + 1, {"SA_HIP_DIR_BITS": "8", "SA_HIP_INITIAL_CHARS": "5"}, 5, 8, 4, (0,),
         WINDOW + ("narrow_40",), False),
    Case("sized_narrow_k2", "sized_narrow", qs.NARROW_MIN_N + 1, qs.NARROW_MIN_N + 1, {"SA_HIP_DIR_BITS": "16", "SA_HIP_INITIAL_CHARS": "2"}, 2, 16, 4, (0,),
         ("sb_le_0", "narrow_le32"), False),
    # narrow keys of 35 bits (part of the top digit kept) on the crafted chain; 1-symbol patterns have different top digits
    Case("markov_narrow", "markov", qs.NARROW_MIN_N, qs.NARROW_MIN_N, {"SA_HIP_INITIAL_CHARS": "5"}, 5, 19, 4, (0,),
         ("narrow_35", "top_digits", "span:many buckets|empty buckets at both ends", "empty_bucket:l == h in the middle"), False),
]
CASE_BY_ID = {c.id: c for c in CASES}
SWITCHES = qs.SWITCHES + ("SA_HIP_QCLUSTER_MIN", "SA_HIP_QCLUSTER", "SA_HIP_K2")


def effective_k0(case, L):
    return min(case.k0, L) if L else case.k0


_texts = {}


def text_and_array(oracle, case, n, L):
    """shared per (text, n): the text; per L: the oracle's (truncated) array"""
    key = (case.text, n)
    if key not in _texts:
        _texts.clear()
        _texts[key] = {"t": make_text(case.text, n)}
    e = _texts[key]
    if ("sa", L) not in e:
        e[("sa", L)] = (oracle.sais(e["t"]) if L == 0 else oracle.truncated_sa(e["t"], L)).astype(np.uint32)
    return e["t"], e[("sa", L)]


CPU_CAP = 1500


def _thin(ix, slot, first_byte, D):
    """which patterns the CPU test traces, by the slot of the pattern's bound: in the designated buckets of a sized text every
    slot of a bucket of up to 400 slots, and of the larger ones the 140 slots at either end and every 32nd; on the other texts
    every pattern up to CPU_CAP per set, a fixed stride beyond.  (The device is asked every pattern.)"""
    slot = np.asarray(slot, np.int64)
    if D:
        bk = np.searchsorted(ix.dir, slot, side="right") - 1
        bk = np.clip(bk, 0, ix.dir.size - 2)
        l, h = ix.dir[bk], ix.dir[bk + 1]
        keep = (h - l <= 400) | (slot - l < 140) | (h - slot <= 140) | (slot % 32 == 0)
        return np.flatnonzero(keep & (np.asarray(first_byte) <= D))
    step = max(-(-slot.size // CPU_CAP), 1)
    return np.arange(0, slot.size, step)


def pattern_sets(case, ix, cpu):
    """-> list of (name, patterns: list[bytes] or u8[k, m], expected (first, second) or None: ask the oracle).  cpu: thinned as
    _thin says; the device test passes cpu = False and asks everything."""
    import cases as gen_cases
    t, sa, k0, L = ix.t, ix.sa, ix.k0, ix.L
    rng = np.random.default_rng(77)
    alph = np.flatnonzero(np.asarray(ix.code) > 0)
    narrow = ix.key_bytes == 4
    big = ix.n >= qs.NARROW_MIN_N                # millions of rows per length: fewer lengths, and the sets that go through Python lists
    D = len(sized_spec(8, 16) if narrow else sized_spec(4, 8)) if case.text in ("sized_wide", "sized_narrow") else 0
    head = D + 1 if D else 10                    # ... only for the suffixes that start with a designated byte / with a newline
    sets = []
    for m in sorted({1, 2, k0} if big else {1, 2, max(k0 - 1, 1), k0}):
        rows, f, s = every_bound(t, sa, m, L)
        if m == k0:
            whole = (rows, f, s)
        if cpu:
            keep = _thin(ix, f, rows[:, 0], D)
            rows, f, s = rows[keep], f[keep], s[keep]
        sets.append(("every_bound_%d" % m, rows, (f, s)))
    if D or not narrow:
        rows, slot = between(t, sa, k0, alph, whole)
        if big:
            sel = rows[:, 0] <= head
            rows, slot = rows[sel], slot[sel]
        if cpu:
            rows = rows[_thin(ix, np.minimum(slot, ix.n - 1), rows[:, 0], D)]
        sets.append(("between", rows, None))
    if not narrow and k0 >= 2:
        sets.append(("beyond_key", beyond_key(t, sa, ix.code_arr, ix.b, k0, k2n_of(ix.b), limit=(200 if cpu else None), first_max=D or (head if big else 0)), None))
    sets.append(("short_spans", short_spans(ix), None))
    sets.append(("misses", random_misses(ix, case.text, rng), None))
    sets.append(("edge", gen_cases.edge_patterns(t, alph.astype(np.uint8), k0, k2n_of(ix.b), L, rng), None))
    sets.append(("long", long_patterns(t, sa, rng), None))
    if L:
        sets.append(("truncated", truncation_patterns(t, L, rng), None))
    return sets


def as_list(pats):
    return pats if isinstance(pats, list) else [bytes(r) for r in pats]


def as_packed(pats):
    """-> (packed u8, u64 offsets)"""
    if isinstance(pats, list):
        off = np.zeros(len(pats) + 1, np.uint64)
        off[1:] = np.cumsum([len(p) for p in pats], dtype=np.uint64)
        return np.frombuffer(b"".join(pats), np.uint8), off
    k, m = pats.shape
    return np.ascontiguousarray(pats.reshape(-1)), np.arange(k + 1, dtype=np.uint64) * np.uint64(m)


# ---- claims --------------------------------------------------------------------------------------------------------------------
# name -> function(list of traces of one (case, L, mode, deep)) -> dict item -> reached?  An item is one cell of the issue's table.

def _bounds(trs):
    for tr in trs:
        for nm in ("lb", "ub"):
            bt = tr.get(nm)
            if bt:
                yield tr, nm, bt


def _claim_bucket_sizes(trs, W, deep):
    sizes = {tr["h"] - tr["l"] for tr in trs if tr.get("branch") == "one_bucket"}
    want = [1, W - 1, W, W + 1, 2 * W, 3 * W + 1, 128, 129, 4096, 4097]
    return {"h-l=%d" % s: s in sizes for s in want}


def _claim_grid(trs, W, deep):
    one = [tr for tr in trs if tr.get("branch") == "one_bucket"]
    out = {}
    for x in (0, 1, W - 1):
        out["l%%W=%d" % x] = any(tr["l"] % W == x for tr in one)
        out["h%%W=%d" % x] = any(tr["h"] % W == x for tr in one)
    return out


def _claim_mask(trs, W, deep):
    return {"window keys of another bucket would change `below`": any(bt.get("mask_matters") for _, _, bt in _bounds(trs))}


def _claim_bound_pos(trs, W, deep):
    out = {"lb@l": False, "lb@l+1": False, "lb@h-1": False, "lb@h": False, "ub@l": False, "ub@l+1": False, "ub@h-1": False, "ub@h": False}
    for tr in trs:
        if tr.get("branch") != "one_bucket" or tr["h"] - tr["l"] < 4:
            continue
        lo, hi = tr["key_range"]
        for nm, v in (("lb", lo), ("ub", hi)):
            for tag, x in (("l", tr["l"]), ("l+1", tr["l"] + 1), ("h-1", tr["h"] - 1), ("h", tr["h"])):
                if v == x and (nm == "lb" or tr.get("ub") is not None or tag == "h"):
                    out["%s@%s" % (nm, tag)] = True
    del out["ub@l"]      # (an upper bound at l is an empty range at l: the lower bound's case)
    return out


def _claim_window_edge(trs, W, deep):
    seqs = {(nm, bt["seq"]) for _, nm, bt in _bounds(trs)}
    return {"lb from the left (rL)": any(s.endswith("rL") for nm, s in seqs if nm == "lb"),
            "lb from the right (lR)": any(s.endswith("lR") for nm, s in seqs if nm == "lb"),
            "ub from the left (rL)": any(s.endswith("rL") for nm, s in seqs if nm == "ub")}


def _claim_walk(trs, W, deep):
    seqs = {bt["seq"] for tr, nm, bt in _bounds(trs) if bt["end"] == "window" and not tr.get("big")}
    out = {}
    for k in (1, 2):
        out["%d left" % k] = any(s[:-1] == "l" * k for s in seqs)
        out["%d right" % k] = any(s[:-1] == "r" * k for s in seqs)
    return out


def _claim_walk_runs_out(trs, W, deep):
    out = {"3 left, ran out": False, "3 right, ran out": False}
    for tr, nm, bt in _bounds(trs):
        if bt.get("ran_out") and bt["seq"] in ("lll", "rrr"):
            out["3 %s, ran out" % ("left" if bt["seq"] == "lll" else "right")] = True
            out["then %s" % bt["end"]] = True
    out.setdefault("then samples" if deep else "then bisect", False)
    return out


def _claim_clamped(trs, W, deep):
    return {"est >= h": any(tr.get("clamped") for tr in trs)}


def _claim_sb(trs, W, deep):
    return {"sb <= 0": any(tr.get("sb", 1) <= 0 for tr in trs)}


def _claim_short_key(trs, W, deep):
    return {"key bits <= dbits: the estimate is the bucket's first slot": any("W" in tr and tr["est_window"] == tr["l"] & ~(W - 1) and tr["h"] - tr["l"] > 3 * W for tr in trs)}


def _claim_runs(trs, W, deep):
    out = {}
    runs = {}
    for tr in trs:
        if tr.get("branch") == "one_bucket" and tr.get("ub") is not None:
            lo, hi = tr["key_range"]
            runs.setdefault(hi - lo, []).append((hi, tr["h"]))
    for r in (1, W, W + 1, 3 * W + 1, 129, 4097):
        out["run of %d" % r] = r in runs
    ends = [e for v in runs.values() for e in v]
    out["run ends at a window edge"] = any(hi % W == 0 for hi, h in ends)
    out["run ends one slot short of it"] = any(hi % W == W - 1 for hi, h in ends)
    out["run ends at h"] = any(hi == h for hi, h in ends)
    return out


def _claim_have_window(trs, W, deep):
    ubs = [bt for _, nm, bt in _bounds(trs) if nm == "ub"]
    return {"ub in the lb's window (load saved)": any(bt["saved"] for bt in ubs), "ub loads a window of its own": any(not bt["saved"] and bt["loads"] for bt in ubs)}


def _claim_samples(trs, W, deep):
    if not deep:
        return {}
    b = [bt for _, _, bt in _bounds(trs)]
    s = [bt for bt in b if bt["end"] == "samples"]
    return {"lo on a multiple of 64": any(bt.get("lo64") for bt in s), "hi - 1 on a multiple of 64": any(bt.get("hi64") for bt in s),
            "ia == ib0": any(bt.get("ia") == "ib0" for bt in s), "ia == ia0": any(bt.get("ia") == "ia0" for bt in s),
            "hi - lo = 128 (not used)": any(bt.get("span") == 128 for bt in b), "hi - lo = 129 (used)": any(bt.get("span") == 129 and bt["end"] == "samples" for bt in b)}


def _claim_samples_last(trs, W, deep):
    if not deep:
        return {}
    return {"the last sample of the array": any(bt.get("last_sample") and bt["end"] == "samples" for _, _, bt in _bounds(trs))}


def _claim_big(trs, W, deep):
    one = [tr for tr in trs if tr.get("branch") == "one_bucket"]
    if not deep:
        return {"h-l=4097 without samples: windows": any(tr["h"] - tr["l"] == 4097 and tr["lb"]["loads"] for tr in one)}
    if W != 4:
        return {}
    return {"h-l=4096: windows first": any(tr["h"] - tr["l"] == 4096 and not tr["big"] and tr["lb"]["loads"] for tr in one),
            "h-l=4097: big": any(tr["h"] - tr["l"] == 4097 and tr["big"] for tr in one),
            "big: ub saved nothing, walked": any(tr.get("big") and tr["ub"] and tr["ub"]["loads"] for tr in one)}


def _claim_span(trs, W, deep):
    sp = [tr for tr in trs if tr.get("branch") == "span"]
    return {"2 buckets": any(tr["span_buckets"] == 2 for tr in sp), "many buckets": any(tr["span_buckets"] > 16 for tr in sp),
            "ends in the last bucket": any(tr["end_marker"] for tr in sp), "empty buckets at both ends": any(tr["empty_ends"] for tr in sp)}


def _claim_empty(trs, W, deep):
    e = [tr for tr in trs if tr.get("branch") == "empty_bucket"]
    return {"l == h in the middle": any(0 < tr["bl"] and not tr["last_bucket"] for tr in e),
            "l == h == n at the last bucket": any(tr["last_bucket"] and tr["at_n"] for tr in e)}


def _claim_top_digits(trs, W, deep):
    return {"same top digit": any(tr.get("same_top") is True for tr in trs), "different top digits": any(tr.get("same_top") is False for tr in trs)}


def _claim_p1b(trs, W, deep):
    if not deep:
        return {}
    p = [(tr, tr["p1b"]) for tr in trs if "p1b" in tr]
    k2n = p[0][1]["k2n"] if p else 0          # (the index's own k2n = min(16, 64 / b), carried in the trace)
    return {"group of 2": any(x["group"] == 2 for _, x in p), "group of 3": any(x["group"] == 3 for _, x in p), "group > 128": any(x["group"] > 128 for _, x in p),
            "m2 = 1": any(x["m2"] == 1 for _, x in p), "m2 = k2n - 1": any(x["m2"] == k2n - 1 for _, x in p), "m2 = k2n": any(x["m2"] == k2n for _, x in p),
            "exact": any(x.get("exact") is True for _, x in p), "not exact, phase 2 over the narrowed range": any(x.get("exact") is False and tr["p2"][0] != "exact" for tr, x in p),
            "absent byte": any(x["absent"] for _, x in p), "K2 entries of 0": any(x.get("zero_entries") for _, x in p),
            "all K2 of the group equal": any(x.get("all_equal") for _, x in p)}


def _claim_partial(trs, W, deep):
    if not deep:
        return {}
    return {"a key group (k0 characters) over more than one stored key": any(tr["p1b"].get("stored_differ") for tr in trs if "p1b" in tr)}


def _claim_phase2(trs, W, deep):
    r = {tr["p2"][1] for tr in trs if tr["p2"][0] == "single"}
    return {"single compare, r < 0": -1 in r, "r = 0": 0 in r, "r > 0": 1 in r, "double bisection": any(tr["p2"][0] == "double" for tr in trs)}


def _claim_long(trs, W, deep):
    cs = {tr["c"] for tr in trs if tr["p2"][0] != "exact"}
    return {"c = %d" % m: m in cs for m in (33, 39, 40, 41)}


def _claim_short_suffix(trs, W, deep):
    return {"a suffix shorter than the pattern that agrees as far as it goes": any(tr.get("short_suffix") for tr in trs)}


def _claim_truncated(trs, W, deep):
    return {}     # (judged per L in the CPU test: patterns longer than L that are hits)


def _narrow_one(trs):
    return [tr for tr in trs if tr.get("branch") == "one_bucket" and "key_bits" in tr]


def _claim_narrow_40(trs, W, deep):
    return {"one-bucket searches over 40-bit keys: the stored 32 bits end below the top digit": any(tr["key_bits"] == 40 for tr in _narrow_one(trs))}


def _claim_narrow_35(trs, W, deep):
    return {"one-bucket searches over 35-bit keys: three bits of the top digit dropped, five kept": any(tr["key_bits"] == 35 for tr in _narrow_one(trs))}


def _claim_narrow_le32(trs, W, deep):
    return {"one-bucket searches over keys of at most 32 bits: the whole key stored": any(tr["key_bits"] <= 32 for tr in _narrow_one(trs))}


CLAIMS = {"bucket_sizes": _claim_bucket_sizes, "grid": _claim_grid, "mask_matters": _claim_mask, "bound_pos": _claim_bound_pos, "window_edge": _claim_window_edge,
          "walk": _claim_walk, "walk_runs_out": _claim_walk_runs_out, "clamped": _claim_clamped, "sb_le_0": _claim_sb, "short_key": _claim_short_key, "runs": _claim_runs,
          "have_window": _claim_have_window, "samples": _claim_samples, "samples_last": _claim_samples_last, "big": _claim_big, "span": _claim_span, "empty_bucket": _claim_empty,
          "top_digits": _claim_top_digits, "phase1b": _claim_p1b, "partial": _claim_partial, "phase2": _claim_phase2, "long": _claim_long, "short_suffix": _claim_short_suffix,
          "truncated": _claim_truncated, "narrow_40": _claim_narrow_40, "narrow_35": _claim_narrow_35, "narrow_le32": _claim_narrow_le32}

# reached under one window width only (the other column is printed as it is): where the walk stops is the estimate's matter
ANY_COLUMN = {("samples", "hi - lo = 128 (not used)")}

# ---- mistakes ------------------------------------------------------------------------------------------------------------------
# name -> (case that must catch it, L, modes, deep keys, what the model does instead).  No mutated kernel is built or run: a wrong
# `base` or sample index reads outside K, and a fault is not provoked on a device.
MISTAKES = {
    "in_mask_dropped": ("sized_wide", 0, (2, 1), False, "`below` counts every key of the window, not those of [a, b)"),
    "strict_lt": ("sized_wide", 0, (2, 1), False, "the STRICT form counts k < t instead of k <= t"),
    "base_wrong_way": ("sized_wide", 0, (2, 1), False, "base += W where every key is >= t, base -= W where every key is < t"),
    "sample_hi_minus_1": ("sized_wide", 0, (2, 1), True, "hi = ia * 64 - 1"),
    "sample_lo_plus_2": ("sized_wide", 0, (2, 1), True, "lo = (ia - 1) * 64 + 2"),
    "m2_off_by_one": ("words_wide", 0, (2,), True, "one character fewer of the pattern goes into the second key"),
    "k2_zero_group": ("equal_wide", 0, (2,), True, "K2 = 0 for the whole key group (a group taken too small leaves its other slots unwritten)"),
    "k2_group_by_stored_key": ("words_partial", 0, (2,), True, "a slot's group is taken from the stored key, which holds one bit beyond the k0 characters"),
    "single_ub_from_ge": ("words_wide", 0, (2, 0), False, "the single compare takes ub = lo from r >= 0"),
}
# Mistakes of the list that cannot change a range, each with the reason.  They stay in the model (query_model takes
# their names), so the CPU test can show that no pattern of any case tells them apart from the kernel.
UNREACHABLE = {
    "sample_hi_plus_1": "hi = ia * 64 + 1 only widens [lo, hi] on the side where the condition is known to hold; a bisection over a wider bracket returns "
                        "the same slot.  The shrinking form (sample_hi_minus_1) is in MISTAKES instead",
    "sample_lo_minus_1": "lo = (ia - 1) * 64 only widens [lo, hi] by a slot known not to satisfy the condition; sample_lo_plus_2 is in MISTAKES instead",
    "estimate_not_clamped": "frac >> down < 2^(sb - down), so ((frac >> down) * (h - l)) >> (sb - down) < h - l: est >= h never holds, the clamp is never taken",
    "t_hi1_not_widened": "key_hi = key_lo | ones, so every bit field of key_hi is >= the same field of key_lo, and below bit 56 key_hi is all ones when "
                         "the top digits differ: no stored key of bucket bl exceeds t_hi2, with or without the widening",
    "k2_not_cut_at_L": "c <= L, so m2 <= L - k0: the bits of K2 beyond the cut lie below the m2 characters compared, inside [q2_lo, q2_hi] whatever they hold",
}
