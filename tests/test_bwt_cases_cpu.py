"""The generator and the ruler model of tests/test_gpu_bwt_edges.py (tests/bwt_cases.py), checked without a GPU: the restated
constants are the header's, text_with_primary gives the primary index asked for, the forward and inverse models return
every text (and agree with the reference), psi decodes to the text, and the plans reach what they are named for -- both
values of aux_only, the round bound and one less, a walk that ends on a ruler with its last step, ruler counts around a
power of two."""
import os
import re

import numpy as np
import pytest

import bwt_cases as bc
from test_bwt_cpu import model_bwt, model_unbwt, ref_bwt, ref_unbwt

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "suffixarray_amd", "csrc")
TEXTS = bc.all_texts()


@pytest.fixture(scope="module")
def forward(oracle):
    out = {}
    for name, t in TEXTS.items():
        sa = oracle.sais(t).astype(np.int64)
        U, p, _ = model_bwt(t, sa)
        out[name] = (sa, U, p)
    return out


@pytest.mark.parametrize("fname,pattern,value", bc.HEADER_CONSTANTS)
def test_constants_are_the_headers(fname, pattern, value):
    with open(os.path.join(CSRC, fname)) as f:
        found = re.findall(pattern, f.read())
    assert found and all(x == value for x in found), (fname, pattern, found)


def test_hash_and_bits():
    assert bc.mix64(0) == 0 and bc.mix64(1) == 0x5692161D100B05E5   # the splitmix64 finaliser's published value
    for n in (2, 17, 4097, 12289):
        want = [x for x in range(n) if bc.mix64(x ^ bc.SALT ^ n) & 63 == 0]
        assert bc.hash_rulers(n, 64).tolist() == want
        assert bc.hash_rulers(n, 1).size == n
    assert [bc.bits_for(c) for c in (0, 1, 2, 3, 4, 5, 16, 17)] == [0, 0, 1, 2, 2, 3, 4, 5]
    assert bc.next_pow2(2) == 2 and bc.next_pow2(17) == 32 and bc.next_pow2(4096) == 4096


def test_text_with_primary(forward):
    cs = bc.primary_cases()
    assert sorted({c.text.size for c in cs}) == list(bc.SIZES)
    for c in cs:
        n = c.text.size
        assert forward[c.name][2] == c.primary and (c.text[1:] != c.text[0]).all(), c.name
        assert set(bc.primaries(n)) >= {1, n} | ({n - 1} if n > 1 else set())
    ps = {(c.text.size, c.primary) for c in cs}
    # the primary index on both sides of a 16-byte group and of a 4096-byte tile, and n on both sides of them
    assert {(33, 15), (33, 16), (33, 17), (8193, 4095), (8193, 4096), (8193, 4097), (4096, 4096), (4097, 4097), (16, 16)} <= ps
    assert {n % 16 for n in bc.SIZES} == {0, 1, 2, 3, 15}
    by = dict(bc.alphabet_cases())
    assert np.unique(by["two_0_255_4097"]).tolist() == [0, 255] and np.unique(by["all_256_4097"]).size == 256
    assert by["mid_1_254_4097"].min() == 1 and by["mid_1_254_4097"].max() == 254
    assert forward["two_0_255_p1"][2] == 1 and forward["two_0_255_pn"][2] == 33 and forward["one_symbol_17"][2] == 17


def test_models_return_every_text(forward):
    for name, t in TEXTS.items():
        sa, U, p = forward[name]
        assert np.array_equal(model_unbwt(U, p), t), name
        assert np.array_equal(bc.decode(U, p), t), name


def test_reference_agrees(ref, forward):
    for name, t in TEXTS.items():
        sa, U, p = forward[name]
        rU, rp, rf = ref_bwt(ref, t)
        assert rp == p and np.array_equal(rU, U) and np.array_equal(rf, np.bincount(t, minlength=256)), name
        for r in (2, 16, bc.next_pow2(t.size)):
            assert np.array_equal(ref_bwt(ref, t, r=r)[1], model_bwt(t, sa, r)[2]), (name, r)
        rc, back = ref_unbwt(ref, U, primary=p)
        assert rc == 0 and np.array_equal(back, t), name


def test_simulate_on_hand_counted_walks(forward):
    sa, U, p = forward["n16_p2"]
    s = bc.simulate(U, [p], 16, walk=8, ruler=1 << 30)          # one ruler: 8 steps and a claim, 8 steps back onto the ruler
    assert (s.aux_only, s.rulers, s.ruler_rounds, s.longest_walk, s.claims, s.stops_at_B_on_ruler) == (0, 2, 2, 8, 1, 1)
    assert s.rank_rounds == bc.bits_for(3) + 1 == 3 and s.max_rounds == 3 and s.cap == 1 + 0 + 2 + 2
    sa, U, p = forward["n17_p2"]
    s = bc.simulate(U, [p], 17, walk=8, ruler=1 << 30)          # 8 + 8 + 1
    assert (s.rulers, s.ruler_rounds, s.longest_walk, s.claims, s.stops_at_B_on_ruler) == (3, 3, 8, 2, 0)
    I = model_bwt(TEXTS["n17_p2"], sa, 16)[2]
    s = bc.simulate(U, I, 16, walk=8, ruler=1 << 30)            # rulers at text offsets 0 and 16: 8 + 8 and 1
    assert (s.rulers, s.ruler_rounds, s.claims, s.stops_at_B_on_ruler) == (3, 2, 1, 1)
    s = bc.simulate(U, [p], 17, ruler=1)                        # a ruler at every rank
    assert (s.rulers, s.ruler_rounds, s.longest_walk, s.claims, s.rank_rounds) == (17, 1, 1, 0, bc.bits_for(18) + 1)
    I = model_bwt(TEXTS["n17_p2"], sa, 2)[2]
    s = bc.simulate(U, I, 2, walk=8, aux_min=1)                 # aux-only: nine rulers two characters apart
    assert (s.aux_only, s.rulers, s.ruler_rounds, s.longest_walk, s.rank_rounds) == (1, 9, 1, 2, 0)
    I = model_bwt(TEXTS["n17_p2"], sa, 128)[2]
    assert bc.simulate(U, I, 128, walk=8, aux_min=1).aux_only == 0   # r_aux > 8 B: ranked
    assert bc.simulate(U, [p, p], 16, walk=8, ruler=1 << 30).rulers == 4   # a duplicate aux row keeps its id and never walks


def test_plans_reach_what_they_are_named_for(forward):
    seen = {plan: [] for plan in bc.PLANS}
    for plan in bc.PLANS:
        for name, r in bc.plan_runs(plan):
            t = TEXTS[name]
            sa, U, p = forward[name]
            I = [p] if r is None else model_bwt(t, sa, r)[2]
            seen[plan].append((t.size, r, bc.simulate(U, I, r or t.size, **bc.plan_knobs(plan))))
            assert plan != "one_ruler" or t.size <= 12289
    assert all(not s.aux_only and s.rulers > 1 or n < 1024 for n, r, s in seen["default"])
    assert any(s.ruler_rounds >= 3 for _, _, s in seen["rounds"])
    one = seen["one_ruler"]
    assert any(r is None and s.ruler_rounds == -(-n // 8) == s.max_rounds - 1 for n, r, s in one)
    assert any(r is None and n % 8 == 0 and s.stops_at_B_on_ruler == 1 for n, r, s in one)
    assert any(r is None and n % 8 == 1 and n > 4096 for n, r, s in one) and any(n % 8 == 7 for n, r, s in one)
    assert any(s.ruler_rounds == -(-n // 8) - 1 for n, r, s in one)
    assert all(s.rulers == (n - 1) // (r or n) + 1 + s.claims for n, r, s in one)
    S = {s.rulers for _, _, s in seen["all_rulers"]}
    assert all(s.rulers == n and s.ruler_rounds == 1 for n, r, s in seen["all_rulers"])
    assert {15, 16, 17} <= S and {4095, 4096, 4097} <= S          # 2^k - 1, 2^k, 2^k + 1
    assert {bc.bits_for(x + 1) + 1 for x in (15, 16, 17)} == {5, 6}
    for plan, B in (("aux_only_8", 8), ("aux_only_16", 16)):
        got = {(r, s.aux_only) for n, r, s in seen[plan]}
        assert got == {(r, int(r <= 8 * B)) for r in (2, 4, 8, 16, 64, 128, 256) if r <= 16 * B}, got
        assert any(s.aux_only and r < 8 and n % 8 for n, r, s in seen[plan])        # unaligned starts, an unaligned end
        assert any(s.aux_only and s.claims for n, r, s in seen[plan])             # r_aux > B: claims at known offsets
