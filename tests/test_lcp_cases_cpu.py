"""The generator and the phase model of tests/test_gpu_lcp_edges.py (tests/lcp_cases.py), checked without a GPU: the
restated constants are the header's, the PLCP model agrees with the Kasai model and with the reference, the model closes
hand-made pairs in the phase the header's code does, and every case list holds what it claims -- a PLCP value on every
hand-off depth and one either side, an end-of-text pair for every closing path, a pair for every phase, a reducible chain
across every scan tile bound."""
import os
import re

import numpy as np
import pytest

import lcp_cases as lc
from test_int_cpu import ref_plcp_int
from test_lcp_cpu import kasai_plcp, ref_plcp

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "suffixarray_amd", "csrc")
BYTE = lc.byte_lists()
INT = lc.int_lists()
ALL = lc.all_cases()


@pytest.fixture(scope="module")
def solved(oracle):
    return {c.name: lc.solve(c.text, oracle) for c in ALL}


@pytest.mark.parametrize("fname,pattern,value", lc.HEADER_CONSTANTS)
def test_constants_are_the_headers(fname, pattern, value):
    with open(os.path.join(CSRC, fname)) as f:
        found = re.findall(pattern, f.read())
    assert found and all(x == value for x in found), (fname, pattern, found)


def test_edges_restates_the_host_loop():
    e = lc.edges(600_000)
    assert (e.d_lane, e.d_wave_end) == (64, 16448) and e.rounds[:4] == [16448, 32832, 65600, 131136]
    assert e.split_rounds == 6 and e.rounds[6] >= 600_000 > e.rounds[5]
    assert e.lane_steps == list(range(0, 64, 8)) and e.wave_steps[:2] == [64, 1088] and len(e.wave_steps) == 16
    assert e.chunks[:5] == [16448, 20544, 24640, 28736, 32832] and len(e.chunks) == 4 + 8 + 16
    assert lc.edges(16448).split_rounds == 0 and lc.edges(16449).split_rounds == 1 and lc.edges(32833).split_rounds == 2
    e = lc.edges(5000, 4, 0, 6, 10)                       # bytes: 4 per symbol
    assert (e.d_lane, e.d_wave_end) == (6, 16) and e.rounds[:3] == [16, 4112, 12304] and e.split_rounds == 3
    e = lc.edges(100, 1, 12, 0, 16)                       # a key depth moves every hand-off
    assert (e.d_lane, e.d_wave_end) == (12, 28) and e.rounds[:2] == [28, 4124] and e.split_rounds == 1
    assert lc.edge_depths(64, 16384) == [8, 64, 72, 64 + 1024, 64 + 16384, 16448 + 4096, 32832, 32832 + 4096, 65600]
    assert lc.knob_env("default") == {} and lc.knob_env("int_6_10") == {"SA_HIP_LCP_LANE_BYTES": "6", "SA_HIP_LCP_WAVE_BYTES": "10"}


def _pair_text(L, tail_a, tail_b, sym_bytes=1):
    """two suffixes that share exactly L symbols and then differ (or, tail_b None, the second ends there)"""
    w = np.arange(L) % 7 + 10
    t = np.concatenate([[1], w, [tail_a], [2], w] + ([[tail_b]] if tail_b is not None else []))
    return t.astype(np.uint8 if sym_bytes == 1 else np.int32)


def test_classify_on_hand_made_pairs(oracle):
    """lane 8 / wave 16 (bytes): d_lane = 8, d_wave_end = 24, D_1 = 24 + 4096"""
    def phase_of(L, tail_a, tail_b, sym_bytes=1, lane=8, wave=16):
        t = _pair_text(L, tail_a, tail_b, sym_bytes)
        sa, plcp = lc.solve(t, oracle)
        ph = lc.classify(t, sa, plcp, lc.edges(t.size, sym_bytes, 0, lane, wave), sym_bytes)
        j = int(np.nonzero(ph.plcp == L)[0][0])
        assert ph.compared_positions == ph.i.size and ph.wave_compares == (ph.phase != lc.LANE).sum()
        assert ph.split_compares == (ph.phase >= 0).sum()
        return int(ph.phase[j]), bool(ph.by_end[j])
    assert phase_of(7, 30, 40) == (lc.LANE, False)        # mismatch in the last byte of the lane budget
    assert phase_of(8, 30, 40) == (lc.WAVE_PHASE, False)  # the first byte beyond it: left to the wave
    assert phase_of(8, 30, None) == (lc.LANE, True)       # ... unless the pair ends there: l == mb
    assert phase_of(9, 30, None) == (lc.WAVE_PHASE, True)
    assert phase_of(23, 30, 40) == (lc.WAVE_PHASE, False)
    assert phase_of(24, 30, 40) == (0, False)             # p + off >= end: left to the split rounds
    assert phase_of(24, 30, None) == (lc.WAVE_PHASE, True)   # end >= mb
    assert phase_of(25, 30, None) == (0, True)            # d_hi >= m
    assert phase_of(24 + 4095, 30, 40) == (0, False)
    assert phase_of(24 + 4096, 30, 40) == (1, False)      # p + off < hi: the next round's
    assert phase_of(24 + 4096, 30, None) == (0, True)
    assert phase_of(24 + 4097, 30, None) == (1, True)
    # 4-byte symbols, lane 6 / wave 10: symbol 1 spans bytes 4..7
    assert phase_of(1, 30, 40, 4, 6, 10) == (lc.LANE, False)                   # differs in byte 4
    assert phase_of(1, 1 << 24, 2 << 24, 4, 6, 10) == (lc.WAVE_PHASE, False)   # differs in byte 7 only
    assert phase_of(3, 1 << 24, 2 << 24, 4, 6, 10) == (lc.WAVE_PHASE, False)   # byte 15
    assert phase_of(4, 1 << 24, 2 << 24, 4, 6, 10) == (0, False)               # byte 19
    assert phase_of(4, 1 << 24, None, 4, 6, 10) == (lc.WAVE_PHASE, True)       # 16 bytes: end == mb


def test_keyed_counts_on_a_hand_made_text(oracle):
    t = np.frombuffer(b"abcxabcyabz", np.uint8)
    sa, plcp = lc.solve(t, oracle)
    for k0, tied in ((1, 5), (2, 3), (3, 1), (4, 0)):     # ab x3, b x3 (2 + 2 ranks tied at depth 1), c x2; abc x2, bc x2
        ph = lc.classify(t, sa, plcp, lc.edges(t.size, 1, k0), 1)
        assert ph.tied == tied, (k0, ph.tied)
        assert (ph.tied, ph.compared_positions) == lc.keyed_counts(plcp, sa, lc.classify(t, sa, plcp, lc.edges(t.size)).plcp, k0)
        assert (ph.plcp >= k0).all()


def test_models_agree_on_small_texts(solved):
    done = 0
    for c in ALL:
        if c.text.size < 70_000:
            sa, plcp = solved[c.name]
            assert np.array_equal(kasai_plcp(lc.as_bytes_order(c.text), sa), plcp), c.name
            done += 1
    assert done > 60


def test_reference_agrees(ref, solved):
    for c in ALL:
        sa, plcp = solved[c.name]
        if c.sym_bytes == 1:
            assert np.array_equal(ref.libsais(c.text), sa), c.name
            assert np.array_equal(ref_plcp(ref, c.text, sa)[0], plcp), c.name
        else:
            assert np.array_equal(ref_plcp_int(ref, c.text, sa), plcp), c.name


def _phases(c, solved):
    sa, plcp = solved[c.name]
    return lc.classify(c.text, sa, plcp, lc.case_edges(c), c.sym_bytes)


@pytest.mark.parametrize("knobs", list(BYTE) + list(INT))
def test_lists_reach_every_edge_and_phase(solved, knobs):
    cs = (BYTE.get(knobs) or INT[knobs])
    lists = [c for c in cs if c.name.startswith(knobs + "_edges")]
    assert len(lists) == (1 if knobs in BYTE else 2)
    for c in lists:
        assert c.text.size < 600_000
        ph = _phases(c, solved)
        have = set((ph.plcp[~ph.by_end]).tolist())
        SB = c.sym_bytes
        for d in lc.edge_depths(*lc.KNOBS[knobs]):
            for v in (d // SB - 1, d // SB, d // SB + 1):
                assert v < 1 or v in have, (c.name, d, v)
        e = lc.case_edges(c)
        res = None if SB == 1 else (3 if c.name.endswith("_hi") else 0)   # the byte of a symbol a mismatch can fall on
        can = lambda lo, hi: any(res is None or b % SB == res for b in range(lo, min(hi, lo + SB)))   # noqa: E731
        want = {0, 1, 2} | ({lc.LANE} if can(0, e.d_lane) else set()) | ({lc.WAVE_PHASE} if can(e.d_lane, e.d_wave_end) else set())
        assert set(ph.phase[~ph.by_end].tolist()) == want, c.name
        first = set(ph.first[~ph.by_end].tolist())
        if SB == 1:   # a mismatch in the last byte before and the first byte beyond every hand-off
            for d in (e.d_lane, e.d_wave_end, e.rounds[1], e.rounds[2]):
                assert (d - 1 in first or d == 0) and d in first, (c.name, d)
        elif c.name.endswith("_hi"):   # symbols that differ in their highest byte only
            assert all(f % 4 == 3 for f in first), c.name
            x = c.text[1:] ^ c.text[:-1]
            assert (x & 0x00FFFFFF == 0).all() and (c.text >> 24 < 128).all()
        else:
            assert all(f % 4 == 0 for f in first), c.name
        assert e.split_rounds >= 3 and ph.split_compares >= 9 and ph.wave_compares >= ph.split_compares


@pytest.mark.parametrize("knobs", list(BYTE) + list(INT))
def test_end_of_text_cases_close_by_the_end_in_their_phase(solved, knobs):
    cs = [c for c in (BYTE.get(knobs) or INT[knobs]) if c.at_end is not None]
    e = lc.case_edges(cs[0])
    SB = cs[0].sym_bytes
    per_variant = len(cs) // (1 if knobs in BYTE else 2)
    assert per_variant == len(lc.lengths_around([e.d_lane, e.d_wave_end, e.rounds[1]], SB))
    if SB == 1:
        assert per_variant == (9 if e.d_lane > 1 else 7)
    seen = set()
    for c in cs:
        ph = _phases(c, solved)
        n = c.text.size
        j = np.nonzero((np.maximum(ph.i, ph.k) == n - c.at_end) & (ph.plcp == c.at_end))[0]
        assert j.size == 1 and ph.by_end[j[0]], c.name
        assert ph.phase[j[0]] == lc.end_phase(c), (c.name, ph.phase[j[0]])
        seen.add(int(ph.phase[j[0]]))
    # a pair ends on a whole symbol: the lane loop can close one by its end when d_lane holds a symbol, the wave when
    # a multiple of the symbol size lies in (d_lane, d_wave_end]
    want = {0, 1} | ({lc.LANE} if e.d_lane >= SB else set()) | ({lc.WAVE_PHASE} if e.d_wave_end // SB > e.d_lane // SB else set())
    assert seen == want, (knobs, seen)


def test_tile_cases_carry_a_chain_across_every_tile_bound(solved):
    cs = [c for c in BYTE["default"] if c.name.startswith("tile_")]
    assert [c.text.size for c in cs] == list(lc.TILE_SIZES)
    for c in cs:
        sa, plcp = solved[c.name]
        irr = set(lc.irreducible_pairs(c.text, sa)[0].tolist())
        bounds = list(range(lc.SCAN_TILE, c.text.size - 1, lc.SCAN_TILE))   # the last position always has PLCP 0
        assert len(bounds) == (c.text.size - 2) // lc.SCAN_TILE
        for b in bounds:
            assert plcp[b] > 0 and plcp[b] == plcp[b - 1] - 1 and b not in irr and b - 1 not in irr, (c.name, b)
        assert plcp.max() >= 149


def test_scan_carry_layout():
    assert lc.SCAN_CARRY_N == (1 << 24) + 4097 and lc.SCAN_TILE * lc.SCAN_TILE == 1 << 24
    assert lc.SCAN_CARRY_STARTS == ((1 << 24) - 3000, (1 << 24) - 1)
    assert (lc.SCAN_CARRY_N + lc.SCAN_TILE - 1) // lc.SCAN_TILE > lc.SCAN_TILE   # the tile scan loops twice


@pytest.mark.parametrize("start", lc.SCAN_CARRY_STARTS)
def test_scan_carry_texts_carry_a_chain_over_2_24(oracle, start):
    """the copy, not its source, holds the common prefix, and its reducible positions run over position 2^24"""
    t = lc.scan_carry_text(start)
    sa = oracle.sais(t).astype(np.int64)
    ln = min(lc.SCAN_CARRY_COPY, t.size - 1 - start)
    assert start < 1 << 24 < start + ln - 1000
    w = lc.plcp_window(t, sa, start - 1, start + ln + 1)
    chain = np.arange(ln, 0, -1)                           # the last few positions may share more with some other suffix
    assert w[0] < 16 and w[-1] < 16 and np.array_equal(w[1:-17], chain[:-16]) and (w[-17:-1] >= chain[-16:]).all(), start
