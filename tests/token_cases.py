"""Texts, patterns and the two CPU models of the token-index tests (test_token_index_cpu.py, test_gpu_token_index.py).

An answer is (first, count): first = number of suffixes that sort before the pattern (a suffix that ends sorts before one that
continues), count = number of suffixes that have the pattern as a prefix.
  model (a)  bisection over the suffix array, comparing the Python list t[sa[r] : sa[r] + m] with the pattern -- list order is
             exactly that order (a proper prefix is smaller) -- for first and first + count;
  model (b)  count again as the number of windows of the text equal to the pattern: no suffix array involved.
"""
import numpy as np

from test_int_cpu import model_sa

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

PLANS = {
    "default": {},
    "no_keys": {"SA_HIP_TOKEN_KEYS": "0"},
    "no_dir": {"SA_HIP_TOKEN_DIR": "0"},
    "text_only": {"SA_HIP_TOKEN_KEYS": "0", "SA_HIP_TOKEN_DIR": "0"},
}


def set_plan(monkeypatch, plan):
    for k in ("SA_HIP_TOKEN_KEYS", "SA_HIP_TOKEN_DIR"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)


def _plant(t):
    """c = t[n-1] also occurs earlier, followed by 0 (texts whose alphabet holds 0)"""
    t[10], t[11] = t[-1], 0
    return t


def texts():
    """name -> int32 text.  Texts with a large alphabet are short: every present symbol is a pattern, and a batch stays at a few
    thousand patterns."""
    rng = np.random.default_rng(29)
    c = {
        "n0": np.zeros(0, np.int32),
        "n1": np.array([4], np.int32),
        "n2": np.array([1, 0], np.int32),
        "n2_same": np.array([3, 3], np.int32),
        "all_equal": np.full(20000, 7, np.int32),
        "period2": np.tile(np.array([5, 1], np.int32), 9000),
        "period3": np.tile(np.array([2, 0, 1], np.int32), 7000),
        "rand_k2": _plant(rng.integers(0, 2, 50000).astype(np.int32)),
        "rand_k4": _plant(rng.integers(0, 4, 50000).astype(np.int32)),
        "rand_k1000": _plant(rng.integers(0, 1000, 50000).astype(np.int32)),
        "rand_k2147483647": _plant(rng.integers(0, I32_MAX, 3000).astype(np.int32)),
        "repeat_block": np.tile(rng.integers(0, 3000, 2000).astype(np.int32), 15),
        "zero_and_max": _plant(rng.choice(np.array([0, 1, 77, I32_MAX - 1, I32_MAX], np.int32), 6000)),
        "dir_edge_in": _plant(rng.choice(np.array([0, 2 ** 24 - 1], np.int32), 3000)),      # max - min + 1 == 2^24: a directory
        "dir_edge_out": _plant(rng.choice(np.array([0, 2 ** 24], np.int32), 3000)),         # one more: none
    }
    c["zero_and_max"][5], c["zero_and_max"][6] = 0, I32_MAX
    return c


def _fits(p):
    return all(I32_MIN <= v <= I32_MAX for v in p)


def patterns(t, seed=3):
    """the pattern list of one text (lists of Python ints, all within int32)"""
    rng = np.random.default_rng(seed)
    tl = [int(v) for v in t]
    n = len(tl)
    pats = [[], [-1], [I32_MIN], [-1, 5], [I32_MIN, I32_MIN], [0], [I32_MAX], [5, 6]]
    if n == 0:
        return pats
    present = sorted(set(tl))
    mn, mx = present[0], present[-1]
    pats += [[v] for v in present]
    pats += [[mn - 1], [mn - 1, mn], [mx + 1], [mx + 1, 0]]
    holes = [a + 1 for a, b in zip(present, present[1:]) if b - a > 1]
    if holes:
        h = holes[len(holes) // 2]
        pats += [[h], [h, mn], [h, mx, mx]]
    starts = [0, n - 1, max(n - 2, 0)] + [int(p) for p in rng.integers(0, n, 6)]
    for m in (1, 2, 3, 8, 64):
        for p in starts:
            w = tl[p:p + m]
            pats += [w, w[:-1] + [w[-1] + 1], w[:-1] + [w[-1] - 1]]
        tail = tl[max(n - m, 0):]                        # ends at n; one more symbol runs the comparison off the text
        pats += [tail + [mn], tail + [mx], tail + [-3]]
    pats += [tl, tl + [mn], tl + [mx], tl + [tl[0]]]
    if mn == mx:                                         # all-equal text: count = n - m + 1, or 0
        pats += [[mn] * m for m in (1, 2, n - 1, n, n + 1) if m >= 1]
    c = tl[-1]                                           # around the last suffix
    follow = sorted({tl[i + 1] for i in range(n - 1) if tl[i] == c})
    pats += [[c], [c, 0], [c, -5], [c, -5, 7], [c, I32_MIN], [c, I32_MAX], [c, 0, 0]]
    if follow:
        pats += [[c, follow[0]], [c, follow[0] - 1], [c, follow[0], -1]]
    pats += [[tl[0], -1], [tl[0], I32_MIN], tl[:2] + [-1], tl[:2] + [I32_MIN, 3], tl[:3] + [-7]]
    return [p for p in pats if _fits(p)]


def model_a(t, sa, pats):
    """(first, count) of every pattern by bisection over sa with list comparison"""
    tl = [int(v) for v in t]
    sl = [int(v) for v in sa]
    n = len(tl)
    first, count = [], []
    for p in pats:
        m = len(p)
        lo, hi = 0, n
        while lo < hi:                                   # suffixes (cut to m symbols) < p
            mid = (lo + hi) // 2
            if tl[sl[mid]:sl[mid] + m] < p:
                lo = mid + 1
            else:
                hi = mid
        a, hi = lo, n
        while lo < hi:                                   # ... <= p
            mid = (lo + hi) // 2
            if tl[sl[mid]:sl[mid] + m] <= p:
                lo = mid + 1
            else:
                hi = mid
        first.append(a)
        count.append(lo - a)
    return np.array(first, np.uint32), np.array(count, np.uint32)


def model_b(t, pats):
    """count of every pattern as the number of text windows equal to it (the empty pattern: a prefix of all n suffixes)"""
    t = np.asarray(t, np.int64)
    n = t.size
    out = []
    for p in pats:
        m = len(p)
        if m == 0 or m > n:
            out.append(n if m == 0 else 0)
            continue
        idx = np.flatnonzero(t[:n - m + 1] == p[0])
        for j in range(1, m):
            if idx.size == 0:
                break
            idx = idx[t[idx + j] == p[j]]
        out.append(idx.size)
    return np.array(out, np.uint32)


def pack(pats):
    off = np.zeros(len(pats) + 1, np.uint64)
    if pats:
        off[1:] = np.cumsum([len(p) for p in pats], dtype=np.uint64)
    return np.array([v for p in pats for v in p], dtype=np.int32), off


_CACHE = {}


def expected(name):
    """(text, suffix array, patterns, first, count) of one text, computed once per process"""
    if name not in _CACHE:
        t = texts()[name]
        sa = model_sa(t)
        pats = patterns(t)
        first, count = model_a(t, sa, pats)
        _CACHE[name] = (t, sa.astype(np.int32), pats, first, count)
    return _CACHE[name]
