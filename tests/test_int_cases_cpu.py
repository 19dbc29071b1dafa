"""The models and the case table of tests/test_gpu_int_edges.py (tests/int_cases.py), checked without a GPU: the restated
constants are the headers', the key model orders like tuples of symbols, the tie model agrees with cases.tied_after_keys, with a
brute-force doubling over prefix tuples and with closed forms, test_int_cpu.model_sa is the reference's array on every case,
and every case holds the edge it is named for."""
import functools
import os
import re
from collections import Counter

import numpy as np
import pytest

import cases
import int_cases as ic
from test_int_cpu import model_sa, rank_remap, ref_int, ref_long

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "suffixarray_amd", "csrc")


@functools.lru_cache(maxsize=None)
def sa_of(name):
    """model_sa of a case, computed once for every test of the process that asks"""
    sa = model_sa(ic.case(name).text)
    sa.setflags(write=False)
    return sa


@pytest.mark.parametrize("fname,pattern,value", ic.CONSTANTS)
def test_constants_are_the_headers(fname, pattern, value):
    with open(os.path.join(CSRC, fname)) as f:
        found = re.findall(pattern, f.read())
    assert found and all(x == value for x in found), (fname, pattern, found)


def test_bits_for_and_stream_grid():
    assert [ic.bits_for(c) for c in (0, 1, 2, 3, 4, 5, 256, 257, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 63 + 1)] == [0, 0, 1, 2, 2, 3, 8, 9, 32, 33, 63, 64]
    assert [ic.stream_grid(n, 4096) for n in (0, 1, 4096, 4097, 6200, 4096 * 2048, 4096 * 2048 + 1, 10 ** 12)] == [1, 1, 1, 2, 2, 2048, 2048, 2048]
    assert ic.first_bad_stride(ic.REFUSAL_N) == 512


SMALL = [("all_equal", np.full(70, 4)), ("period2", np.tile([5, 1], 60)), ("sigma3", np.random.default_rng(1).integers(0, 3, 300)),
         ("sigma40", np.random.default_rng(2).integers(0, 40, 300) * 1000), ("repeat", np.tile(np.random.default_rng(3).integers(0, 9, 50), 6)),
         ("wide", np.random.default_rng(4).choice(np.array([0, 2 ** 32 - 2, 77, 2 ** 31]), 200))]


def _small_plans(t):
    for kn in (dict(bytes=True, compact=True, key_symbols=64), dict(bytes=False, compact=False, key_symbols=64),
               dict(bytes=False, compact=True, key_symbols=3), dict(bytes=False, compact=False, key_symbols=1)):
        yield ic.plan(t, kn)


def _tuples(t, s):
    """the first s symbols of every suffix, + 1, 0 past the end: what the key packs, as plain tuples"""
    v = [int(x) + 1 for x in t]
    return [tuple(v[i:i + s] + [0] * max(0, i + s - len(v))) for i in range(len(v))]


def test_keys_order_like_tuples():
    for name, t in SMALL:
        for p in _small_plans(t):
            k = ic.keys(t, p)
            tup = _tuples(t, p["s"])
            order = sorted(range(len(tup)), key=lambda i: (tup[i], i))
            assert np.argsort(k, kind="stable").tolist() == order, (name, p)
            ks = k[order]
            assert [bool(x) for x in ks[1:] == ks[:-1]] == [tup[a] == tup[b] for a, b in zip(order[1:], order[:-1])], (name, p)
            assert ic.tied_of_keys(k) == sum(c for c in Counter(tup).values() if c > 1), (name, p)


def brute_rounds(t, s):
    """groups of suffixes by their first d symbols as tuples (the end differs from every symbol), d = s, 2 s, ..."""
    out = []
    d = s
    while True:
        cnt = Counter(_tuples(t, d))
        m = sum(c for c in cnt.values() if c > 1)
        if m == 0:
            return out
        out.append((d, m, sum(1 for c in cnt.values() if c > 1)))
        d *= 2


def test_rounds_model_against_brute_force():
    for name, t in SMALL:
        sa = model_sa(t)
        lcp = ic.neighbour_lcp(t, sa)
        for d in (1, 2, 3, 5, 8, 21, 64, 65):
            assert ic.tied(lcp, d) == cases.tied_after_keys(t, d), (name, d)
        for p in _small_plans(t):
            m = ic.rounds_model(t, sa, p)
            br = brute_rounds(t, p["s"])
            assert m["depths"] == br, (name, p)
            assert m["tied_after_sort"] == ic.tied_of_keys(ic.keys(t, p)) == (br[0][1] if br else 0), (name, p)
            assert m["rounds"] == len(br) and m["tied_total"] == sum(x[1] for x in br), (name, p)
            rb = -(-ic.bits_for(t.size + 2) // 8)
            assert m["sort_passes"] == -(-p["bits"] * p["s"] // 8) + sum(rb + -(-ic.bits_for(g + 1) // 8) for _, _, g in br), (name, p)


def test_all_equal_closed_forms():
    for n in (2, 3, 64, 65, 200, 6145):
        t = np.full(n, 9)
        sa = model_sa(t)
        assert sa.tolist() == list(range(n - 1, -1, -1))
        lcp = ic.neighbour_lcp(t, sa)
        assert lcp[1:n].tolist() == list(range(1, n))
        for d in (1, 2, 63, 64, 65, 128, n - 1, n, n + 1):
            want = n - d + 1 if n - d + 1 >= 2 else 0
            assert ic.tied(lcp, d) == want and ic.groups(lcp, d) == (1 if want else 0), (n, d)
    p = ic.plan(np.full(6145, 9), ic.knobs("no_bytes"))
    m = ic.rounds_model(np.full(6145, 9), model_sa(np.full(6145, 9)), p)
    assert (p["bits"], p["s"]) == (1, 64) and m["rounds"] == 7 and m["tied_after_sort"] == 6145 - 63      # 64, 128, .. 4096
    assert m["sort_passes"] == 8 + 7 * (2 + 1)


def test_model_sa_is_the_reference_on_every_case(ref):
    for c in ic.all_cases():
        r, sigma = rank_remap(c.text)
        assert np.array_equal(ref_long(ref, r, sigma), sa_of(c.name)), c.name
        if c.text.size <= 70_000:
            assert np.array_equal(ref_int(ref, r, sigma), sa_of(c.name)), c.name


def test_every_case_has_the_plan_it_is_named_for():
    fam = Counter()
    for c in ic.all_cases():
        fam[c.family] += 1
        assert c.text.size >= 2 and 0 <= int(c.text.min()) and int(c.text.max()) < c.k, c.name
        assert c.text.size <= ic.HALO_N or c.name.startswith("dense_sigma") and c.text.size <= 2 ** 21 + 2048, c.name
        if np.int32 in c.dtypes:
            assert c.k <= 2 ** 31 - 1, c.name
        for pn, (b, s, route, compacted) in c.expect.items():
            p = ic.plan(c.text, ic.knobs(pn))
            assert (p["bits"], p["s"], p["route"], p["compacted"]) == (b, s, route, compacted), (c.name, pn, p)
            assert b * s <= 64 and (s + 1) * b > 64 or s == min(c.text.size, ic.knobs(pn)["key_symbols"]), (c.name, pn)
            if "sigma" in c.meta and compacted:
                assert p["sigma"] == c.meta["sigma"], (c.name, p)
    assert fam == {"key": 8, "tile": 18, "halo": 5, "dense": 15, "raw": 11, "tables": 11}
    assert all(ic.case(n) for n in ic.DROPIN_CASES) and len({ic.case(n).family for n in ic.DROPIN_CASES}) == 6


def test_width_edges_are_in_the_table():
    def p(name, plan):
        return ic.plan(ic.case(name).text, ic.knobs(plan))
    # dense: sigma + 1 = 2^b against sigma = 2^b
    for lo, hi in ((1, 2), (3, 4), (7, 8), (15, 16), (255, 256), (2 ** 16 - 1, 2 ** 16), (2 ** 21 - 1, 2 ** 21)):
        a, b = p("dense_sigma%d" % lo, "default"), p("dense_sigma%d" % hi, "default")
        assert lo + 1 == 1 << a["bits"] and b["bits"] == a["bits"] + 1, (lo, hi)
    assert p("dense_sigma2097151", "default")["bits"] * p("dense_sigma2097151", "default")["s"] == 63
    # raw: max + 2 = 2^b against 2^b + 1
    for lo, hi in (("raw_small_max2", "raw_small_max3"), ("raw_small_max6", "raw_small_max7")):
        a, b = p(lo, "raw_codes"), p(hi, "raw_codes")
        assert a["max"] + 2 == 1 << a["bits"] and b["max"] + 2 == (1 << a["bits"]) + 1 and b["bits"] == a["bits"] + 1
    a, b = p("raw_max_2p32m2", "default"), p("raw_max_2p32m1", "default")
    assert (a["max"], a["bits"], a["s"], b["max"], b["bits"], b["s"]) == (2 ** 32 - 2, 32, 2, 2 ** 32 - 1, 33, 1)
    # the key of 64 bits with its top bit set
    c = ic.case("raw_max_2p32m2")
    k = ic.keys(c.text[:40], a)
    assert a["bits"] * a["s"] == 64 and int(k.max()) >= 1 << 63 and int(k[7]) == ((2 ** 32 - 1) << 32) | (2 ** 32 - 1)
    assert p("raw_max_2p31m2", "default")["max"] == 2 ** 31 - 2 and ic.case("raw_max_2p31m2").k == 2 ** 31 - 1
    assert ic.case("raw_max_2p63m2").k == 2 ** 63 - 1 and p("raw_max_2p63m2", "default")["bits"] == 63
    # the rank table's cap, the scan's tile, more than SC_BLOCK scan parts, an alphabet far from 0
    assert p("tables_range16777216", "default")["compacted"] == 1 and p("tables_range16777217", "default")["compacted"] == 0
    assert p("raw_max_2p24", "default")["compacted"] == 0 and p("raw_max_2p24", "default")["max"] + 1 == ic.DENSE_CAP + 1
    parts = {c.name: c.meta["parts"] for c in ic.all_cases() if c.family == "tables"}
    assert [parts["tables_range%d" % r] for r in (8191, 8192, 8193, 16385, 2 ** 23, 2 ** 23 + 1, 2 ** 24)] == [1, 1, 2, 3, 1024, 1025, 2048]
    for name, np_ in parts.items():
        c = ic.case(name)
        assert np_ == -(-(int(c.text.max()) + 1) // ic.SC_TILE) or name.endswith("16777217"), name
    big = ic.case("tables_range8388609")
    assert parts[big.name] > ic.SC_BLOCK and int(big.text.max()) // ic.SC_TILE >= ic.SC_BLOCK      # a value in the scan's second loop
    assert p("tables_high_alphabet", "default")["min"] == 2 ** 24 - 10 and p("tables_high_alphabet", "default")["sigma"] == 10
    assert p("tables_sigma256_n300", "default")["route"] == "A" and p("tables_sigma257_n300", "default")["route"] == "B"
    assert p("dense_sigma256", "default")["route"] == "A" and p("dense_sigma257", "default")["route"] == "B"


def test_tile_cases_sit_on_the_tile():
    for sigma, s in ((2, 32), (300, 7)):
        ns = sorted(c.text.size for c in ic.all_cases() if c.name.startswith("tile_sigma%d_" % sigma))
        assert ns == sorted([2047, 2048, 2049, ic.KG_TILE + s - 1, ic.KG_TILE + s, 4095, 4096, 4097, 6145]), ns
    # the keys4 plan of the two-symbol texts: more than 255 tied groups in a round (two passes for the group ids)
    c = ic.case("tile_sigma2_n6145")
    m = ic.rounds_model(c.text, sa_of(c.name), ic.plan(c.text, ic.knobs("keys4")))
    assert m["rounds"] >= 3 and max(g for _, _, g in m["depths"]) > 255 and min(g for _, _, g in m["depths"]) <= 255, m["depths"]
    # one symbol per key on the 300-value texts: all records but the values that occur once go to the rounds, in more than 255 groups
    for c in (x for x in ic.all_cases() if x.name.startswith("tile_sigma300_")):
        m = ic.rounds_model(c.text, sa_of(c.name), ic.plan(c.text, ic.knobs("keys1")))
        d, recs, grps = m["depths"][0]
        once = int((np.unique(c.text, return_counts=True)[1] == 1).sum())
        assert (d, recs, grps) == (1, c.text.size - once, 300 - once) and grps > 255 and m["rounds"] >= 2, (c.name, m["depths"])


def test_halo_cases_depend_on_the_halo():
    for c in (x for x in ic.all_cases() if x.family == "halo"):
        (pn, (b, s, _, _)), = c.expect.items()
        p = ic.plan(c.text, ic.knobs(pn))
        t, n = c.text, int(c.text.size)
        lcp = ic.neighbour_lcp(t, sa_of(c.name))
        base = ic.tied(lcp, s)
        (A1, B1), (A2, B2) = c.meta["pairs"]
        assert A1 == ic.KG_TILE - 1 and A1 + s - 1 == ic.KG_TILE + s - 2            # its last symbol: the last code of the halo
        assert A2 + s - 1 == ic.KG_TILE                                              # its last symbol: the first code of the halo
        assert B1 % ic.KG_TILE == A1 and B2 % ic.KG_TILE == A2 and B1 // ic.KG_TILE == 1 and B2 // ic.KG_TILE == 2 and B2 + s < n
        if c.meta["near"] is None:
            # b = 1 is the all-equal text: every key of s symbols is tied.  A key that loses its last code leaves them and
            # becomes the key of the suffix of s - 1 symbols, which was alone: one record more, not two less
            assert base == n - s + 1 == ic.tied_of_keys(ic.keys(t, p))
            for A in (A1, A2):
                assert ic.tied_of_keys(ic.keys(t, p, zero_last_code_at=[A])) == base + 1
            continue
        shared = [int((np.cumprod(t[A:A + s + 1] == t[B:B + s + 1])).sum()) for A, B in c.meta["pairs"]]
        assert base == ic.tied_of_keys(ic.keys(t, p))
        if not c.meta["near"]:              # tied in truth: a key that loses its last code unties the pair
            assert shared == [s, s] and base == 4
            for A in (A1, A2):
                assert ic.tied_of_keys(ic.keys(t, p, zero_last_code_at=[A])) == base - 2, (c.name, A)
        else:                               # apart by the last symbol of the key alone: two keys that lose it are tied
            assert shared == [s - 1, s - 1] and base == 0
            for A, B in c.meta["pairs"]:
                assert ic.tied_of_keys(ic.keys(t, p, zero_last_code_at=[A])) == base, (c.name, A)
                assert ic.tied_of_keys(ic.keys(t, p, zero_last_code_at=[A, B])) == base + 2, (c.name, A)


def test_refusal_cases_hold_what_they_claim():
    rc = {r.name: r for r in ic.refusal_cases()}
    n, k, stride = ic.REFUSAL_N, ic.REFUSAL_K, ic.first_bad_stride(ic.REFUSAL_N)
    assert int(rc["k_is_max"].text.max()) == rc["k_is_max"].k and ic.first_bad(rc["k_is_max"].text, rc["k_is_max"].k) == 300
    assert ic.first_bad(rc["k_is_max_plus_1"].text, rc["k_is_max_plus_1"].k) is None
    want = {"at_0": 0, "at_last": n - 1, "three": 4097, "negative_first": 1000, "too_large_first": 1000, "same_thread": 700,
            "same_thread_reverse": 700, "same_thread_and_an_earlier_thread": 650 + stride, "beyond_int32": 5}
    for name, pos in want.items():
        assert ic.first_bad(rc[name].text, k) == pos and rc[name].text.size == n, name
    bad = lambda name: np.flatnonzero((rc[name].text < 0) | (rc[name].text >= k))   # noqa: E731
    assert (np.diff(bad("same_thread")) % stride == 0).all() and (np.diff(bad("same_thread_reverse")) % stride == 0).all()
    b = bad("same_thread_and_an_earlier_thread")
    assert (b[2] - b[1]) % stride == 0 and (b[1] - b[0]) % stride != 0 and b[0] % stride < b[1] % stride
    b = bad("three")                    # 4097 and 5000 are looked at by threads of different workgroups
    assert (b[0] % stride) // 256 != (b[1] % stride) // 256
