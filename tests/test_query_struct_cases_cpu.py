"""The model and the cases of tests/test_gpu_query_structs.py (tests/query_struct_cases.py), checked without a GPU: the restated
constants and conditions are the headers', the models of K and dir agree with brute force on short texts, the owner
decomposition tiles the directory and reproduces it, and the crafted text shows the spans it claims at the forced widths."""
import os
import re

import numpy as np
import pytest

import query_struct_cases as qs
import split_cases as sc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "suffixarray_amd", "csrc")


@pytest.mark.parametrize("fname,pattern,value", qs.HEADER_CONSTANTS)
def test_constants_are_the_headers(fname, pattern, value):
    with open(os.path.join(CSRC, fname)) as f:
        found = re.findall(pattern, f.read())
    assert found and all(x == value for x in found), (fname, pattern, found)
    assert qs.BLD_TILE == 256 * 16 and qs.DIR_PIECE == 16384 and qs.NARROW_MIN_N == sc.NARROW_MIN_N


def _naive_sa(t):
    b = bytes(t)
    return np.array(sorted(range(len(b)), key=lambda i: b[i:]), np.int64)


SHORT = [("markov", 2000), ("uni27", 1999), ("far2", 777), ("equal", 300), ("words", 1500), ("uni27", 2), ("uni27", 5)]


@pytest.mark.parametrize("name,n", SHORT, ids=["%s_%d" % x for x in SHORT])
def test_models_against_brute_force(name, n):
    """K: every key packed symbol by symbol in plain Python, both stored forms and the partial-character form; dir: a count of the
    suffixes whose first symbols sort below every bucket bound"""
    t = qs.make(name, n)
    sa = _naive_sa(t)
    code, sigma, b = qs.code_map(t)
    assert sigma == np.unique(t).size and (1 << b) > sigma >= (1 << (b - 1))
    c = [int(code[x]) for x in t]
    for k0 in sorted({1, 2, min(5, 40 // b), 40 // b, 56 // b - (b * (56 // b) == 56), 64 // b}):
        direct = []
        for p in sa.tolist():
            key = 0
            for j in range(k0):
                key = (key << b) | (c[p + j] if p + j < n else 0)
            direct.append(key << (64 - b * k0))
        full = qs.full_keys(t, sa, code, b, k0)
        assert full.tolist() == direct, (name, k0)
        assert (np.diff(full.astype(object)) >= 0).all()
        k8, d8 = qs.stored_keys(t, sa, code, b, k0, 8, 0)
        assert k8.dtype == np.uint64 and k8.tolist() == direct and d8 is k8
        if 24 <= 64 - b * k0 < 56:
            k4, d4 = qs.stored_keys(t, sa, code, b, k0, 4, 64 - b * k0)
            assert k4.dtype == np.uint32 and d4.tolist() == direct
            assert k4.tolist() == [(x >> (64 - b * k0)) & 0xFFFFFFFF for x in direct]
            # (what query_one rebuilds: the bucket's top 8 bits and the narrow key)
            assert [((x >> 56) << 56) | (int(y) << (64 - b * k0)) for x, y in zip(direct, k4)] == direct
        if qs.partial_applies(b, k0, 0, True):
            kp, dp = qs.stored_keys(t, sa, code, b, k0, 8, 0, partial=True)
            longer = []
            for p in sa.tolist():
                key = 0
                for j in range(k0 + 1):
                    key = (key << b) | (c[p + j] if p + j < n else 0)
                longer.append(((key << (64 - b * (k0 + 1))) >> 8) << 8)
            assert kp.tolist() == longer and dp is kp
            assert [x >> (64 - b * k0) for x in longer] == [x >> (64 - b * k0) for x in direct]     # the same k0 symbols on top
        for dbits in (8, 11, 14):
            got = qs.directory(full, dbits)
            top = np.array([x >> (64 - dbits) for x in direct], np.int64)
            brute = [int((top < bkt).sum()) for bkt in range(1 << dbits)] + [n]
            assert got.dtype == np.uint32 and got.tolist() == brute, (name, k0, dbits)


def test_partial_condition():
    """5-bit symbols: 11 whole symbols and one bit of the twelfth; 7- and 8-bit symbols fill 56 bits exactly or leave a whole
    symbol's room: no partial character; a truncated index takes it only when L holds the longer key"""
    assert qs.partial_applies(5, 11, 0, True) and qs.partial_applies(5, 11, 12, True) and not qs.partial_applies(5, 11, 11, True)
    assert not qs.partial_applies(5, 11, 0, False) and not qs.partial_applies(5, 10, 0, True)
    assert not qs.partial_applies(7, 8, 0, True) and not qs.partial_applies(7, 7, 0, True) and not qs.partial_applies(8, 7, 0, True)
    assert qs.partial_applies(6, 9, 0, True) and qs.partial_applies(3, 18, 0, True)


@pytest.mark.parametrize("name,n,k0,dbits", [("markov", 3000, 4, 14), ("markov", 3000, 4, 21), ("equal", 500, 40, 21), ("far2", 900, 20, 16),
                                             ("uni27", 4097, 8, 9)])
def test_owner_runs_tile_the_directory(name, n, k0, dbits):
    """the runs are disjoint, cover 0 .. 2^dbits, and writing every run's value over its buckets gives the directory"""
    t = qs.make(name, n)
    sa = _naive_sa(t)
    code, sigma, b = qs.code_map(t)
    keys = qs.full_keys(t, sa, code, b, k0)
    own = qs.owners(keys, dbits)
    assert own.first[0] == 0 and own.last[-1] == 1 << dbits and (own.first[1:] == own.last[:-1] + 1).all() and (own.span >= 1).all()
    assert (own.slot[:-1] < n).all() and own.slot[-1] == n and (np.diff(own.slot) > 0).all()
    assert ((own.pieces == 0) == (own.span <= qs.DIR_INLINE)).all()
    q = own.pieces > 0
    assert ((own.pieces[q] - 1) * qs.DIR_PIECE < own.span[q]).all() and (own.span[q] <= own.pieces[q] * qs.DIR_PIECE).all()
    painted = np.repeat(own.slot, own.span)
    assert np.array_equal(painted, qs.directory(keys, dbits))
    for i in (0, own.span.size // 2, own.span.size - 1):
        text = qs.describe(own, int(own.last[i]))
        assert "span %d" % own.span[i] in text and ("inline" in text) == (own.span[i] <= 40), text
    bad = qs.directory(keys, dbits)
    assert qs.dir_mismatch(bad, bad.copy(), own) is None
    worse = bad.copy()
    worse[int(own.first[-1])] += 1
    assert "trailing run" in qs.dir_mismatch(worse, bad, own) and "1 of %d" % bad.size in qs.dir_mismatch(worse, bad, own)


_sa_cache = {}


def _markov(oracle, n):
    if n not in _sa_cache:
        t = qs.make("markov", n)
        _sa_cache[n] = (t, oracle.sais(t).astype(np.int64))
    return _sa_cache[n]


@pytest.mark.parametrize("n", [qs.MID_N, qs.BIG_N[0], qs.BIG_N[3]])
@pytest.mark.parametrize("dbits", [14, 21])
def test_crafted_text_reaches_the_emit_edges(oracle, n, dbits):
    """at the forced widths the owner decomposition holds runs of exactly 40 (inline) and 41 (queued) buckets, of 16384 (one piece)
    and 16385 (two pieces), a run of at least 3 pieces, and a leading run of more than one bucket; every byte 1..100 occurs (code ==
    byte, b = 7), planted symbols are followed by their words only, the text does not end in one"""
    t, sa = _markov(oracle, n)
    code, sigma, b = qs.code_map(t)
    assert (sigma, b) == (100, 7) and code[1:101].tolist() == list(range(1, 101))
    for s, ws in qs.FOLLOW.items():
        if s in qs.ONLY_PLANTED:
            at = np.flatnonzero(t == s)
            assert at.size == qs.COPIES * len(ws) and at.max() + 3 < n
            assert {tuple(t[p + 1:p + 1 + len(ws[0])].tolist()) for p in at} == set(ws)
    assert not set(t[-3:].tolist()) & (set(qs.FOLLOW) | {1})
    k0 = 5 if n >= qs.NARROW_MIN_N else 4
    own = qs.owners(qs.full_keys(t, sa, code, b, k0), dbits)
    spans = own.span.tolist()
    for s in qs.PLANTED_SPANS[dbits]:
        assert s in spans, (dbits, s)
    if dbits == 14:
        i40, i41 = spans.index(40), spans.index(41)
        assert own.pieces[i40] == 0 and own.pieces[i41] == 1
        assert own.last[i40] == (qs.X << 7) | 41 and own.last[i41] == (qs.X << 7) | 82
    else:
        i1, i2 = spans.index(16384), spans.index(16385)
        assert own.pieces[i1] == 1 and own.pieces[i2] == 2
        assert own.last[i1] == ((qs.Y + 1) << 14) | (1 << 7) | 1 and own.last[i2] == ((qs.Z + 1) << 14) | (1 << 7) | 2
        assert own.pieces[-1] >= 27 and own.pieces.max() >= 3          # the trailing run: codes 101..127
        assert own.span[0] > qs.DIR_PIECE and own.pieces[0] == 2      # the leading run: code 0
    assert own.span[0] > 1
    assert (own.pieces == 0).sum() > 1000 and (own.pieces > 0).sum() >= 3


def test_all_equal_text_gives_every_power_of_two():
    """b = 1: the keys 10..0, 110..0, ... put spans 2^(d-1) + 1, 2^(d-2), ..., 2, 1 and a trailing run of one bucket: both sides
    of 40 and of 16384"""
    n = 300
    t = qs.make("equal", n)
    sa = np.arange(n - 1, -1, -1)
    code, sigma, b = qs.code_map(t)
    assert (sigma, b) == (1, 1)
    own = qs.owners(qs.full_keys(t, sa, code, b, 40), 21)
    assert own.span.tolist() == [(1 << 20) + 1] + [1 << j for j in range(19, -1, -1)] + [1]
    assert own.pieces.tolist() == [65] + [max(1, (1 << j) >> 14) for j in range(19, 5, -1)] + [0] * 7


def test_case_table():
    """every form of the issue is there: both forced widths for every group of writers, the adopted widths on both sides of the
    two-level build, one truncated build per key width, the sizes around the vector load, the tile and 2^22"""
    ids = [c.id for c in qs.CASES]
    assert len(set(ids)) == len(ids)
    for c in qs.CASES:
        tags = [f.tag for f in c.forms]
        assert len(set(tags)) == len(tags), c.id
        for f in c.forms:
            assert set(f.env) <= set(qs.SWITCHES), (c.id, f.tag)
    by_n = {c.n for c in qs.CASES}
    assert set(qs.SMALL_N) | set(qs.BIG_N) | {qs.MID_N} == by_n
    env_of = lambda cid: [(f.env, f.adopted, f.L) for f in qs.CASE_BY_ID[cid].forms]
    for cid, d in (("markov_big_d14", "14"), ("markov_big_d21", "21")):
        es = [e for e, a, L in env_of(cid) if not a]
        assert all(e["SA_HIP_DIR_BITS"] == d and e["SA_HIP_INITIAL_CHARS"] == "5" for e in es)
        for sw in ("SA_HIP_LITE_FLAGS", "SA_HIP_NARROW_K", "SA_HIP_SPLIT_FLAGS", "SA_HIP_FUSE_DIR"):
            assert any(e.get(sw) == "0" for e in es), (cid, sw)
        assert {e.get("SA_HIP_SPLIT") for e in es} == {None, "0", "1"}
    mid = env_of("markov_mid")
    assert {e.get("SA_HIP_DIR_BITS") for e, a, L in mid if a} == {None, "8", "14", "16", "17", "21"}
    assert any(L == 12 and not a for e, a, L in mid) and any(L == 12 and a for e, a, L in mid)
    assert any(L == 12 for e, a, L in env_of("markov_big")) and any(L == 12 for e, a, L in env_of("uni27_big")) and any(L == 12 for e, a, L in env_of("words_big"))
    assert qs.expected_key_bytes(7, 5, 1 << 22, {}, False) == 4 and qs.expected_key_bytes(7, 5, (1 << 22) - 1, {}, False) == 8
    assert qs.expected_key_bytes(7, 6, 1 << 22, {}, False) == 8 and qs.expected_key_bytes(7, 5, 1 << 22, {}, True) == 8
    assert qs.expected_key_bytes(7, 5, 1 << 22, {"SA_HIP_NARROW_K": "0"}, False) == 8 and qs.expected_key_bytes(1, 40, 1 << 22, {}, False) == 4
    assert qs.default_dir_bits(1 << 22) == 19 and qs.default_dir_bits((1 << 22) + 1) == 20 and qs.default_dir_bits(2) == 8 == sc.default_dir_bits(2)
    st = {"narrow_k": 1, "lite_flags": 2}
    assert [qs.writer_of(st, {}, False), qs.writer_of(st, {"SA_HIP_LITE_FLAGS": "0"}, False), qs.writer_of(dict(st, lite_flags=1), {}, False),
            qs.writer_of(dict(st, narrow_k=0), {}, False), qs.writer_of(st, {}, True), qs.writer_of(st, {"SA_HIP_FUSE_DIR": "0"}, False),
            qs.writer_of(dict(st, lite_flags=0), {}, False)] == [4, 2, 3, 1, 5, 5, None]


def test_bucket_patterns():
    alph = np.arange(1, 101, dtype=np.uint8)
    assert qs.bucket_pattern((30 << 7) | 41, 14, 7, alph) == bytes([30, 41])
    assert qs.bucket_pattern((30 << 7) | 0, 14, 7, alph) == bytes([30]) and qs.bucket_pattern((101 << 7) | 5, 14, 7, alph) == b""
    assert qs.bucket_pattern((21 << 14) | (1 << 7) | 1, 21, 7, alph) == bytes([21, 1, 1])
