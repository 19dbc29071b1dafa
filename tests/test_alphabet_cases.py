"""CPU: the alphabet generators of the code-width sweep (tests/test_gpu_alphabets.py) and the oracle on their inputs.  The
generators must give exactly the alphabet asked for -- every code width b from 1 to 9 at both of its ends, gap bytes between
present ones -- and the oracle, the judge of the GPU sweep, must be right on these texts and patterns: its suffix array equals
the naive sort, its query ranges equal a scan over Python's own order of the suffixes."""
import numpy as np
import pytest

import cases

CASES = cases.alphabet_cases()


def test_alphabet_cases_cover_every_code_width_at_both_ends():
    bs = {}
    for _, sigma, _ in CASES:
        bs.setdefault(cases.code_bits(sigma), []).append(sigma)
    assert sorted(bs) == list(range(1, 10))
    for b, sigmas in bs.items():
        assert max(sigmas) == min(2 ** b - 1, 256) and (b == 1 or min(sigmas) == 2 ** (b - 1)), (b, sigmas)
    # code_bits restates bits_for(sigma + 1): 2^b >= sigma + 1 > 2^(b-1)
    for sigma in range(1, 257):
        b = cases.code_bits(sigma)
        assert 2 ** b >= sigma + 1 and (b == 1 or 2 ** (b - 1) < sigma + 1), sigma
    has0 = [bool((cases.alphabet(s, v) == 0).any()) for _, s, v in CASES]
    has255 = [bool((cases.alphabet(s, v) == 255).any()) for _, s, v in CASES]
    assert any(has0) and not all(has0) and any(has255) and not all(has255)


@pytest.mark.parametrize("cid,sigma,variant", CASES, ids=[c[0] for c in CASES])
def test_alphabet_generators(cid, sigma, variant):
    alph = cases.alphabet(sigma, variant)
    assert alph.dtype == np.uint8 and np.unique(alph).size == sigma
    assert bool((alph == 0).any()) == (variant in ("lo", "ends") or sigma == 256)
    assert bool((alph == 255).any()) == (variant in ("hi", "ends") or sigma == 256)
    gaps = cases.gap_bytes(alph)
    if 2 <= sigma < 256:
        assert gaps.size and not np.isin(gaps, alph).any() and alph.min() < gaps.min() and gaps.max() < alph.max()
    else:
        assert gaps.size == 0
    for kind in ("uniform", "binary"):
        for n in (300, 20_000):
            t = cases.alphabet_text(alph, n, kind, seed=sigma)
            assert t.size == n and t.dtype == np.uint8
            assert np.array_equal(np.unique(t), np.sort(alph)), (kind, n)
            assert np.array_equal(t, cases.alphabet_text(alph, n, kind, seed=sigma))   # deterministic
        if kind == "binary" and sigma > 1:
            cnt = np.bincount(t, minlength=256)
            assert cnt.argmax() == alph.min()
            run = np.diff(np.flatnonzero(np.diff(np.concatenate([[-1], (t == alph.min()).astype(np.int8), [-1]])) != 0)).max()
            assert run >= 32, run


def test_edge_patterns_hold_what_they_promise():
    rng = np.random.default_rng(3)
    alph = cases.alphabet(31, "mid")
    t = cases.alphabet_text(alph, 5000, "uniform", 1)
    k0, k2n, L = 8, 12, 10
    pats = cases.edge_patterns(t, alph, k0, k2n, L, rng)
    lens = {len(p) for p in pats}
    assert b"" in pats and set(range(0, k0 + k2n + 3)) <= lens and set(cases.WORD_LENGTHS) <= lens
    assert any(len(p) > L for p in pats)
    gaps = set(cases.gap_bytes(alph).tolist())
    assert any(set(p) & gaps for p in pats)
    assert any(min(p) < alph.min() for p in pats if p) and any(max(p) > alph.max() for p in pats if p)
    assert bytes([alph.max()]) * k0 in pats and bytes([alph.min()]) * (k0 + 1) in pats
    tail = bytes(t[-k0:])
    assert any(p.startswith(tail) and len(p) > k0 for p in pats)   # runs past the end of the text


@pytest.mark.parametrize("cid,sigma,variant", CASES, ids=[c[0] for c in CASES])
def test_oracle_on_alphabet_texts(oracle, cid, sigma, variant):
    alph = cases.alphabet(sigma, variant)
    b = cases.code_bits(sigma)
    k0, k2n = max(40 // b, 1), min(64 // b, 16)
    rng = np.random.default_rng(sigma)
    for kind in ("uniform", "binary"):
        t = cases.alphabet_text(alph, 1500, kind, seed=7 * sigma)
        sa = oracle.sais(t).astype(np.uint32)
        assert np.array_equal(sa, oracle.sa_naive(t)), kind
        pats = cases.edge_patterns(t, alph, k0, k2n, 0, rng)
        got = oracle.query_batch(t, sa, 0xFFFFFFFF, pats)
        exp = cases.brute_ranges(t, 0, pats)
        assert [tuple(r) for r in got] == exp, kind
        for L in (1, k0, 12):
            pats = cases.edge_patterns(t, alph, k0, k2n, L, rng)
            tsa = oracle.truncated_sa(t, L)
            got = oracle.query_batch(t, tsa, L, pats)
            assert [tuple(r) for r in got] == cases.brute_ranges(t, L, pats), (kind, L)
