"""The planted-repeat generator and the tie model of tests/test_gpu_big_ties.py, checked without a GPU: the model counts
exactly 2 (R - k + 1) tied positions at the R values the GPU sweep uses, the copies match on exactly R symbols (brute-force
compare), and the oracle's suffix array holds suffix A+i and suffix B+i in adjacent slots for every i <= R - k, the side
decided by the symbols right after the copies -- the three facts the GPU tests lean on."""
import numpy as np
import pytest

import cases

D1_SYMBOLS = np.concatenate([[10], np.arange(97, 123)]).astype(np.uint8)   # the 27 bytes of the D1 text
K = 12                                                                     # the byte build's initial_chars at 27 symbols

# (R, n): the sweep's R values -- tied counts 2, 4, 8190, 8192, 8194, 16384, 16386 and 199 978
SWEEP_R = [(12, 300_000), (13, 300_000), (4106, 300_000), (4107, 300_000), (4108, 300_000), (8203, 300_000), (8204, 300_000),
           (100_000, 3_000_000)]


def brute_lcp(t, x, y):
    m = t.size - max(x, y)
    ne = np.flatnonzero(t[x:x + m] != t[y:y + m])
    return int(ne[0]) if ne.size else m


def test_tie_model_on_hand_counted_texts():
    f = lambda s, k: cases.tied_after_keys(np.frombuffer(s, np.uint8), k)   # noqa: E731
    assert f(b"abcabd", 2) == 2            # "ab" twice
    assert f(b"abcabd", 3) == 0
    assert f(b"abcab", 2) == 2             # the last "b" + nothing is its own key
    assert f(b"aaaa", 1) == 4
    assert f(b"aaaa", 2) == 3              # "aa" three times, "a" + nothing once
    assert f(b"aaaa", 4) == 0
    assert f(b"aaaa", 64) == 0             # keys longer than the text
    assert f(b"abababab", 2) == 7          # "ab" x 4, "ba" x 3, "b" + nothing
    assert f(b"abababab", 3) == 6
    assert f(b"x", 5) == 0
    assert cases.tied_after_keys(np.zeros(0, np.uint8), 3) == 0
    # packed keys and row keys (k * bits > 64) agree; symbol values do not matter, only their equality
    rng = np.random.default_rng(1)
    t = rng.integers(0, 3, 5000)
    for k in (1, 2, 7, 32):
        rows = np.lib.stride_tricks.sliding_window_view(np.concatenate([t + 1, np.zeros(k - 1, t.dtype)]), k)
        c = np.unique(rows, axis=0, return_counts=True)[1]
        assert cases.tied_after_keys(t, k) == int(c[c > 1].sum()), k
        assert cases.tied_after_keys(t * (2 ** 39) + 5, k) == cases.tied_after_keys(t, k)
    assert cases.tied_after_keys(np.zeros(100, np.int64), 64) == 37 and cases.tied_after_keys(np.zeros(100, np.int64), 70) == 31


@pytest.mark.parametrize("R,n", SWEEP_R)
def test_model_counts_two_per_shared_key(R, n):
    for A, B in ((n // 3, 2 * n // 3), (3, n // 2), (n // 5, n - 1 - R)):
        t = cases.planted_repeat(n, R, A, B, 1000 + R, D1_SYMBOLS)
        assert t.dtype == np.uint8 and t.size == n
        assert cases.tied_after_keys(t, K) == 2 * (R - K + 1), (R, A, B)
        assert cases.tied_after_keys(t, K + 1) == 2 * (R - K), (R, A, B)


def test_copies_match_on_exactly_R_symbols():
    n = 300_000
    for R, A, B in ((13, 5, 100), (4107, 1, 4108), (4107, 70_000, n - 1 - 4107), (8203, 100_000, 200_000)):
        t = cases.planted_repeat(n, R, A, B, R, D1_SYMBOLS)
        assert t[A - 1] != t[B - 1] and t[A + R] != t[B + R]
        for i in sorted({0, 1, R // 2, R - K, R - 1} | set(int(x) for x in np.random.default_rng(R).integers(0, R, 200))):
            assert brute_lcp(t, A + i, B + i) == R - i, (R, A, B, i)
    # the generator over other alphabets: two symbols (the guards have one other symbol to take), wide integers
    t = cases.planted_repeat(5000, 300, 1, 301, 7, np.array([0, 1], np.int32))
    assert t.dtype == np.int32 and brute_lcp(t, 1, 301) == 300 and t[0] != t[300]
    big = (np.arange(300, dtype=np.int64) * 3_600_000_007) + 11
    t = cases.planted_repeat(50_000, 2000, 17, 30_000, 8, big)
    assert t.dtype == np.int64 and int(t.max()) > 2 ** 39 and brute_lcp(t, 17, 30_000) == 2000


@pytest.mark.parametrize("R,n", [(13, 300_000), (4107, 300_000), (8203, 300_000), (100_000, 3_000_000)])
def test_oracle_puts_the_pairs_in_adjacent_slots(oracle, R, n):
    A, B = 7, n - 1 - R
    t = cases.planted_repeat(n, R, A, B, 2000 + R, D1_SYMBOLS)
    sa = oracle.sais(t).astype(np.int64)
    inv = np.empty(n, np.int64)
    inv[sa] = np.arange(n)
    i = np.arange(R - K + 1)
    side = 1 if t[A + R] < t[B + R] else -1          # the first symbols after the copies differ: they decide every pair
    assert np.array_equal(inv[B + i], inv[A + i] + side)
