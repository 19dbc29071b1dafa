"""The generator and the model of tests/test_gpu_refine.py (tests/refine_cases.py), checked without a GPU: the restated
constants are the headers', the model counts hand-made texts right, plan_tiles agrees with a brute-force restatement, and
every case holds what its name claims -- group sizes, M on the stated edge, which group the plan leaves out."""
import os
import re

import numpy as np
import pytest

import cases
import refine_cases as rc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "suffixarray_amd", "csrc")
K = rc.K


@pytest.mark.parametrize("fname,pattern,value", rc.HEADER_CONSTANTS)
def test_constants_are_the_headers(fname, pattern, value):
    with open(os.path.join(CSRC, fname)) as f:
        found = re.findall(pattern, f.read())
    assert found and all(x == value for x in found), (fname, pattern, found)


def _groups(oracle, t, k, cap=256):
    sa = oracle.sais(t).astype(np.int64)
    g = rc.groups_after_keys(t, sa, k, cap)
    assert g.M == cases.tied_after_keys(t, k) and g.M == int(g.sizes.sum()) and g.G == g.sizes.size
    return g


def test_model_on_hand_counted_texts(oracle):
    f = lambda s, k: _groups(oracle, np.frombuffer(s, np.uint8), k)   # noqa: E731
    g = f(b"abcabd", 2)                      # "ab" twice; they share nothing beyond the key
    assert g.sizes.tolist() == [2] and g.glue.tolist() == [0]
    g = f(b"abcxabcy", 2)                    # "ab" (one more symbol shared) and "bc" (none)
    assert g.sizes.tolist() == [2, 2] and g.glue.tolist() == [1, -1, 0]
    g = f(b"aaaa", 1)                        # a, aa, aaa, aaaa: one group; the end differs from every symbol
    assert g.sizes.tolist() == [4] and g.glue.tolist() == [0, 1, 2]
    g = f(b"aaaa", 2)                        # the suffix "a" has the key "a" + nothing: alone
    assert g.sizes.tolist() == [3] and g.glue.tolist() == [0, 1]
    assert f(b"abcd", 1).M == 0
    assert rc.bits_for(0) == 0 and rc.bits_for(1) == 0 and rc.bits_for(2) == 1 and rc.bits_for(3) == 2 and rc.bits_for(4096) == 12
    # tiny pass: size <= 8 and every neighbouring pair apart within the limit
    glue = np.array([0, 63, -1, 64, -1] + [0] * 8 + [-1] + [0] * 7)
    tied = glue >= 0
    assert rc.tiny_pass(glue, tied, 64, False) == 3 + 8 and tied.sum() == 1 + 8      # the pair with glue 64 and the group of 9 stay
    tied = glue >= 0
    assert rc.tiny_pass(glue, tied, 1, True) == 3 + 2 + 8 and tied.sum() == 8        # truncated: every group of <= 8
    # one finisher tile: 8 symbols a round at b = 5; two rounds without a split end it
    assert not rc.finish_tile(np.array([0, -1, 7, -1, 8, 15]), 5, 0, 12).any()        # splits in round 1 and in round 2
    assert not rc.finish_tile(np.array([0, -1, 16]), 5, 0, 12).any()                     # round 2 splits nothing, round 3 does
    assert rc.finish_tile(np.array([0, -1, 24]), 5, 0, 12).tolist() == [False, False, True]   # rounds 2 and 3 split nothing
    assert not rc.finish_tile(np.array([0, -1, 8, -1, 16]), 5, 0, 12).any()           # every round splits something
    assert rc.finish_tile(np.array([7, 500, 3]), 5, 0, 12).all()                      # a group fails as a whole
    assert not rc.finish_tile(np.array([500, 500]), 5, 13, 12).any()                  # truncated at L: final after one symbol
    assert rc.loc_sort_packed(12, 5, 8) and not rc.loc_sort_packed(12, 5, 10) and rc.loc_sort_packed(0, 5, 8) and not rc.loc_sort_packed(5, 5, 11)


def brute_plan(sizes, TILE, CAP):
    M = sum(sizes)
    if M <= CAP:
        return [(0, M, M)]
    start_of, g0 = {}, 0
    for z in sizes:
        for r in range(g0, g0 + z):
            start_of[r] = g0
        g0 += z
    out = []
    for t in range(-(-M // TILE)):
        mine = sorted({s for s in start_of.values() if t * TILE <= s < (t + 1) * TILE})
        after = sorted({s for s in start_of.values() if s >= (t + 1) * TILE}) + [M]
        prev = out[-1][2] if out else 0
        if not mine:
            out.append((after[0], after[0], after[0]))
            continue
        begin, end = mine[0], after[0]
        assert begin == prev
        local_end = end
        if end - begin > CAP:
            local_end = start_of[(t + 1) * TILE]      # the group that straddles the nominal end
        out.append((begin, local_end, end))
    return out


def test_plan_tiles_against_brute_force():
    rng = np.random.default_rng(3)
    T, C = 28, 32
    lists = [[2] * 16, [2] * 15 + [3], [27, 5, 2], [27, 6, 2], [3] * 9 + [5] + [2] * 20, [3] * 9 + [6] + [2] * 20, [33, 2, 2], [2, 33, 2] * 3,
             [2, 70, 2, 2], [40, 40, 40], [2] * 14 + [33] + [2] * 30]
    for _ in range(300):
        lists.append(rng.choice([2, 2, 2, 3, 4, 5, 6, 9, 30, 33, 60], rng.integers(1, 60)).tolist())
    left_seen = 0
    for sizes in lists:
        p = rc.plan_tiles(sizes, T, C)
        assert [tuple(x) for x in p.tiles.tolist()] == brute_plan(sizes, T, C), sizes
        assert p.inside + p.left == sum(sizes) and (p.tiles[:, 1] - p.tiles[:, 0] <= C).all()
        left_seen += p.left > 0
    assert left_seen > 20
    assert rc.plan_tiles([27, 5, 2], T, C).left == 0 and rc.plan_tiles([27, 6, 2], T, C).left == 6    # tile of C kept, C + 1 not


def _sim(oracle, case, cap=256, **kw):
    t = rc.make(case)
    b = max(1, int(np.unique(t).size).bit_length())
    k = 64 // b
    g = _groups(oracle, t, k, cap)
    return t, g, rc.simulate(g, int(t.size), k, b, L=case.L, **kw)


def _count(g):
    u, c = np.unique(g.sizes, return_counts=True)
    return dict(zip(u.tolist(), c.tolist()))


def test_planted_groups_give_exact_group_counts(oracle):
    t, pos = rc.planted_groups(400_000, [(2, 13), (8, 20), (9, 20), (27, 150), (3, 1369)], 1)
    g = _groups(oracle, t, K, cap=1400)
    assert _count(g) == {2: 2, 8: 9, 9: 9, 27: 139, 3: 1358} and g.M == 7984
    assert int(g.glue.max()) == 1369 - K and [len(p) for p in pos] == [2, 8, 9, 27, 3]
    t, pos = rc.planted_groups(50_000, [(2, 20)], 2, at_end=0)
    assert pos[0][1] == 50_000 - 20 and np.array_equal(t[pos[0][0]:pos[0][0] + 20], t[-20:])


def test_tiny_cases_hold_what_they_claim(oracle):
    c = rc.tiny_cases()
    t, g, st = _sim(oracle, c["sizes_2_9"])
    assert _count(g) == {s: 9 for s in range(2, 10)}
    assert st["tiny_resolved"] == 9 * sum(range(2, 9)) and st["finisher_records"] == 81 and st["exact"] and st["rounds"] == 0
    t, g, st = _sim(oracle, c["lcp_63_64_65"])
    assert int(g.glue.max()) == 65 and (g.glue == 64).sum() == 2 + 2 * 2 and (g.glue == 63).sum() == 3 + 3 * 2
    assert g.M - st["tiny_resolved"] == 2 + 3 + 2 * 2 + 2 * 3      # the groups at glue 64 (two plants each size) and 65
    t, g, st = _sim(oracle, c["ends_at_text_end"])
    sa = oracle.sais(t)
    ends = [int(t.size - p) for p in sa[g.apos] if t.size - p <= K + 8]
    assert sorted(ends) == list(range(K, K + 9)) and st["tiny_resolved"] == g.M
    for name, M in (("M4096", 4096), ("M4097", 4097)):
        t, g, st = _sim(oracle, c[name])
        assert g.M == M and -(-M // rc.BLD_TILE) == (1 if M == 4096 else 2) and st["tiny_resolved"] == M
    t, g, st = _sim(oracle, c["sparse_16M_eq_n"])
    assert g.M * 16 == t.size and st["tiny_resolved"] == g.M
    t, g, st = _sim(oracle, c["sparse_16M_gt_n"])
    assert g.M * 16 == t.size + 1 and st["tiny_resolved"] == 0 and st["finisher_resolved"] == g.M
    for L in (13, 19, 20, 21):
        t, g, st = _sim(oracle, c["trunc_L%d" % L])
        assert int(g.glue.max()) >= L - K and st["tiny_resolved"] == g.M - 9 * (40 - K + 1) and st["finisher_resolved"] == 9 * (40 - K + 1)
        assert st["rounds"] == 0 and st["exact"]


def test_finisher_cases_hold_what_they_claim(oracle):
    c = rc.finisher_cases()
    kw = dict(tiny=False, period_finish=False)
    t, g, st = _sim(oracle, c["M4096"], **kw)
    assert g.M == 4096 and g.G == 2048 and st["plans"][0].tiles.tolist() == [[0, 4096, 4096]]
    t, g, st = _sim(oracle, c["M4097"], **kw)
    assert g.M == 4097 and len(st["plans"][0].tiles) == 2
    t, g, st = _sim(oracle, c["pairs_2046_and_a_triple"], **kw)
    assert g.M == 4095 and g.G == 2047 and len(st["plans"][0].tiles) == 1
    t, g, st = _sim(oracle, c["tile_eq_cap"], **kw)
    assert st["plans"][0].tiles[0].tolist() == [0, rc.FIN_CAP, rc.FIN_CAP] and st["plans"][0].left == 0 and g.sizes[1791] == 513
    assert st["rounds"] == 0 and st["finisher_resolved"] == g.M
    t, g, st = _sim(oracle, c["tile_cap_plus_1"], **kw)
    assert st["plans"][0].tiles[0].tolist() == [0, 3583, rc.FIN_CAP + 1] and st["plans"][0].left == 514
    assert st["finisher_records"] == g.M - 514 and st["finisher_resolved"] == g.M - 514 and st["rounds"] == 1 and st["active_total"] == 514
    t, g, st = _sim(oracle, c["group_4096"], **kw)
    assert g.sizes[0] == 4096 and st["plans"][0].tiles[0].tolist() == [0, 4096, 4096] and st["plans"][0].left == 0
    t, g, st = _sim(oracle, c["group_4097"], **kw)
    assert g.sizes[0] == 4097 and st["plans"][0].tiles[0].tolist() == [0, 0, 4097] and st["plans"][0].left == 4097
    assert st["rounds"] == 1 and st["active_total"] == 4097 and st["finisher_runs"] == 1
    for name, big in (("largest_96", 96), ("largest_97", 97)):
        t, g, st = _sim(oracle, c[name], **kw)
        assert int(g.sizes.max()) == big and st["finisher_resolved"] == g.M
    t, g, st = _sim(oracle, c["sizes_pow2"], **kw)
    have = set(g.sizes.tolist())
    assert all((1 << e) in have and (1 << e) + 1 in have for e in range(1, 12))
    t, g, st = _sim(oracle, c["long_lcp"], cap=4400, **kw)
    assert int(g.glue.max()) == 4100 and not st["exact"] and st["finisher_runs"] == 2
    first = st["plans"][0]
    assert len(first.tiles) > 2 and 0 < st["finisher_resolved"] < g.M and first.inside == g.M
    t, g, st = _sim(oracle, c["below_a_quarter"], cap=1000, **kw)
    assert st["finisher_runs"] == 1 and st["finisher_resolved"] * 4 < st["finisher_records"] and not st["exact"]
    t, g, st = _sim(oracle, c["above_a_quarter"], cap=1000, **kw)
    assert st["finisher_runs"] == 2 and st["finisher_resolved"] * 4 > g.M
    for name, b in (("sigma4", 3), ("sigma256", 9)):
        t, g, st = _sim(oracle, c[name], **kw)
        assert max(1, int(np.unique(t).size).bit_length()) == b and st["exact"] and st["finisher_resolved"] == g.M
    for L in (13, 20, 33):
        t, g, st = _sim(oracle, c["trunc_L%d" % L], **kw)
        assert int(g.glue.max()) == 60 - K and st["finisher_resolved"] == g.M and st["rounds"] == 0


def test_round_sort_cases_hold_what_they_claim(oracle):
    c = rc.round_sort_cases()
    kw = dict(tiny=False, period_finish=False, group_finish=False)
    want_big = {"tile_eq_cap": 0, "tile_cap_plus_1": 514, "M4096": 0, "M4097": 0, "one_big_between_small": 5000,
                "two_big_groups": 9200, "big_20000": None}
    for name, big in want_big.items():
        t, g, st = _sim(oracle, c[name], **kw)
        first = rc.plan_tiles(st["round_sizes"][0], rc.LOC_TILE, rc.LOC_CAP)
        got = rc.round_sort_big(st["round_sizes"][0])
        if big is None:   # the planted group and most of its shifted groups of 20 000 / 27 records; still the tile-local path
            assert 20_000 <= got and got * 2 <= g.M and int(g.sizes.max()) == 20_000, (name, got, g.M)
            big = got
        assert got == big and st["exact"], name
        assert not st["packed"][0] and st["active_total"] >= g.M, name
        if name == "tile_eq_cap":
            assert first.tiles[0].tolist() == [0, rc.LOC_CAP, rc.LOC_CAP]
        if name == "two_big_groups":
            out = first.tiles[first.tiles[:, 2] > first.tiles[:, 1]]
            assert len(out) == 2 and out[1, 0] >= out[0, 2]         # two tiles leave a group out: the second has a big_off
        if name in ("M4096", "M4097", "tile_eq_cap", "tile_cap_plus_1"):
            assert st["rounds"] == 1 and st["active_total"] == g.M
    t, g, st = _sim(oracle, c["packed_L20"], **kw)
    assert st["packed"] == [True] and st["rounds"] == 1 and st["active_total"] == g.M
    t, g, st = _sim(oracle, c["sigma256"], **kw)
    assert st["exact"] and st["rounds"] >= 1 and not st["packed"][0]


def test_period_cases_hold_what_they_claim(oracle):
    c = rc.period_cases()
    out = {}
    for name, case in c.items():
        t = rc.make_periodic(case)
        sa = oracle.sais(t).astype(np.int64)
        g = _groups(oracle, t, K, cap=512)
        st = rc.simulate(g, int(t.size), K, 5, t=t, sa=sa)
        rows = [(d,) + r for tries in st["period_tries"] for d, _, rs in tries for r in rs]   # (d, p0, last, members, E, taken)
        assert all(r[5] == (r[4] + r[0] >= r[2]) for r in rows)
        out[name] = (t, g, st, rows)
    t, g, st, rows = out["E_one_less"]
    left = [r for r in rows if not r[5]]
    assert left and any(r[4] == r[2] - r[0] - 1 and r[3] == 3 for r in left) and sum(r[3] for r in left) < 64   # E = p1 - 1
    assert st["period_resolved"] == sum(r[3] for r in rows if r[5]) > 5000
    t, g, st, rows = out["E_first_reachable"]
    assert min(r[4] - (r[2] - r[0]) for r in rows if r[5]) == K and any(r[5] and r[3] == 3 and r[4] == r[2] - r[0] + K for r in rows)
    t, g, st, rows = out["ends_lt_gt_eot"]
    assert [d for d, _, _ in st["period_tries"][0]] == [220, 210, 200] and all(r[5] for r in rows) and st["exact"]
    E = {d: next(r[4] for r in rows if r[0] == d) for d in (200, 210, 220)}
    assert t[E[200] + 200] < t[E[200]] and t[E[210] + 210] > t[E[210]] and E[220] + 220 == t.size
    t, g, st, rows = out["tile_edges"]
    assert {r[0]: r[4] % rc.PER_TILE for r in rows} == {200: 4095, 210: 0, 220: 1} and all(r[5] for r in rows)
    t, g, st, rows = out["three_tiles"]
    assert all(r[5] for r in rows) and st["exact"]
    assert max(r[2] + K for r in rows) // rc.PER_TILE - min(r[1] for r in rows) // rc.PER_TILE >= 2        # the run covers three tiles
    assert max(r[4] // rc.PER_TILE - r[1] // rc.PER_TILE for r in rows) >= 1                                # E from the tiles' carry
    t, g, st, rows = out["M64"]
    assert st["finisher_resolved"] == 0 and st["period_resolved"] == 64 and g.M - st["tiny_resolved"] == 64 and st["exact"]
    t, g, st, rows = out["M63"]
    assert st["finisher_resolved"] == 0 and st["period_resolved"] == 0 and g.M - st["tiny_resolved"] == 63 and not rows and st["handover"] == 63


def test_narrow_cases_hold_what_they_claim(oracle):
    for name, case in rc.narrow_cases().items():
        t = rc.make(case)
        g = _groups(oracle, t, 8)
        st = rc.simulate(g, int(t.size), 8, 5)
        assert t.size >= 1 << 22 and st["exact"] and st["rounds"] == 0
        if name == "all_tiny":
            assert int(g.sizes.max()) <= 8 and st["tiny_resolved"] == g.M
        else:
            assert int(g.sizes.max()) == 27 and 0 < st["tiny_resolved"] < g.M and st["finisher_resolved"] == g.M - st["tiny_resolved"]
