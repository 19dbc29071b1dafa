"""The case generator of the radix sort's direct tests (tests/sort_cases.py), checked without a GPU, so that
tests/test_gpu_sort.py cannot quietly stop covering what it claims: the sizes step the tile count across 8 -> 9 and 16 -> 17,
leave trailing chunks empty and reach chunks of five and more tiles, for both tile sizes; the windows give every pass count;
the chunk-boundary family's digit-0 run ends one short of, on and one past a chunk's first record; the model is stable."""
import numpy as np
import pytest

import sort_cases as sc


def all_sizes(block):
    T = sc.SORT_ITEMS * block
    return sc.small_sizes(T) + sc.large_sizes(T)


def test_geom_restates_make_geom():
    # hand-computed from csrc/radix_sort.hpp: make_geom, the ticket loop, radix_hist_kernel's `per`
    assert sc.geom(1, 512) == {"tile": 8192, "tiles": 1, "tpc": 1, "chunks": 1, "hist_per": 1}
    assert sc.geom(8 * 8192, 512) == {"tile": 8192, "tiles": 8, "tpc": 1, "chunks": 8, "hist_per": 1}
    assert sc.geom(8 * 8192 + 1, 512) == {"tile": 8192, "tiles": 9, "tpc": 2, "chunks": 5, "hist_per": 1}
    assert sc.geom(17 * 4096, 256) == {"tile": 4096, "tiles": 17, "tpc": 3, "chunks": 6, "hist_per": 1}
    assert sc.geom(41 * 4096 + 5, 256) == {"tile": 4096, "tiles": 42, "tpc": 6, "chunks": 7, "hist_per": 1}
    assert sc.geom(65 * 8192 + 1, 512) == {"tile": 8192, "tiles": 66, "tpc": 9, "chunks": 8, "hist_per": 1}
    assert sc.geom(2048 * 4096, 256)["hist_per"] == 1 and sc.geom(2048 * 4096 + 1, 256)["hist_per"] == 2
    assert [sc.chunk_of_tile(t, 3) for t in (0, 2, 3, 20, 21, 23, 24, 30)] == [0, 0, 1, 6, 7, 7, 7, 7]


@pytest.mark.parametrize("block", sc.BLOCKS)
def test_sizes_cover_the_chunk_geometry(block):
    T = sc.SORT_ITEMS * block
    swept = set()
    for fam in sc.FAMILIES:
        swept |= {c.n for c in sc.sweep_cases(block, fam)}
    assert swept == set(all_sizes(block))
    g = {n: sc.geom(n, block) for n in swept}
    tiles = {v["tiles"] for v in g.values()}
    assert {8, 9, 16, 17} <= tiles                                     # the tpc steps 1 -> 2 and 2 -> 3
    assert g[8 * T]["tpc"] == 1 and g[8 * T + 1]["tpc"] == 2 and g[16 * T]["tpc"] == 2 and g[16 * T + 1]["tpc"] == 3
    assert any(v["chunks"] < sc.NCHUNK and v["tiles"] > sc.NCHUNK for v in g.values())   # empty trailing chunks
    assert g[9 * T]["chunks"] == 5 and g[16 * T + 1]["chunks"] == 6 and g[41 * T + 5]["chunks"] == 7
    assert max(v["tpc"] for v in g.values()) >= 5
    assert g[33 * T + 1]["tpc"] == 5 and g[65 * T + 1]["tpc"] == 9       # a self-published inclusive prefix; > 2 look-back windows
    assert any(n % T not in (0, T - 1) and n > T for n in swept)          # partial last tiles
    assert {1, 2, 63, 64, 65, T - 1, T, T + 1} <= swept


def test_windows_hit_every_pass_count():
    assert {sc.npasses(*w) for w in sc.WINDOWS} == set(range(1, 9))
    assert {sc.npasses(*w) for w in sc.KEYS_ONLY_WINDOWS} == set(range(1, 9)) and len(sc.KEYS_ONLY_WINDOWS) == 8
    assert set(sc.KEYS_ONLY_WINDOWS) <= set(sc.WINDOWS)
    last = {w: sc.pass_bits(*w)[-1] for w in sc.WINDOWS}
    assert last[(0, 9)] == 1 and last[(0, 57)] == 1 and last[(1, 64)] == 7 and last[(0, 1)] == 1
    assert all(sum(sc.pass_bits(*w)) == w[1] - w[0] and 0 <= w[0] < w[1] <= 64 for w in sc.WINDOWS)
    # the result lands in either buffer: both parities of the pass count
    assert {sc.npasses(*w) % 2 for w in sc.WINDOWS} == {0, 1}
    for block in sc.BLOCKS:
        T = sc.SORT_ITEMS * block
        for fam in sc.FAMILIES:
            cs = sc.sweep_cases(block, fam)
            # every window at every small size the family applies to; three windows of 1, 2 and >= 3 passes above
            for n in {c.n for c in cs}:
                ws = [(c.lo, c.hi) for c in cs if c.n == n]
                if n <= 2 * T + 1:
                    assert ws == sc.WINDOWS, (fam, n)
                else:
                    assert [min(sc.npasses(*w), 3) for w in ws] == [1, 2, 3], (fam, n, ws)
            assert {c.vals for c in cs} == {"iota", "random"}
        # between them the families take every window to the large sizes
        big = {(c.lo, c.hi) for fam in sc.FAMILIES for c in sc.sweep_cases(block, fam) if c.n > 2 * T + 1}
        assert big == set(sc.WINDOWS)


def test_families_keep_to_their_window_and_fill_the_rest():
    T = 8192
    for fam in sc.FAMILIES:
        for lo, hi in sc.WINDOWS:
            k = sc.make_keys(fam, 2 * T + 1, lo, hi, 1, T)
            assert k.dtype == np.uint64 and k.size == 2 * T + 1
            again = sc.make_keys(fam, 2 * T + 1, lo, hi, 1, T)
            assert np.array_equal(k, again)                               # a function of (n, lo, hi, seed)
            outside = k & np.uint64(sc.ALL_ONES ^ sc.window_mask(lo, hi))
            free = 64 - (hi - lo)                                         # random bits outside the window
            assert np.unique(outside).size == (1 << free) if free <= 8 else np.unique(outside).size > T
            w = (k & np.uint64(sc.window_mask(lo, hi))) >> np.uint64(lo)
            bits0 = sc.pass_bits(lo, hi)[0]
            d0 = w & np.uint64((1 << bits0) - 1)
            if fam == "all_zero":
                assert not w.any()
            elif fam == "all_ones":
                assert (w == np.uint64((1 << (hi - lo)) - 1)).all()
            elif fam == "ascending":
                assert (np.diff(w.astype(object)) >= 0).all() and w[-1] > w[0]
            elif fam == "descending":
                assert (np.diff(w.astype(object)) <= 0).all() and w[-1] < w[0]
            elif fam.startswith("odd_"):
                u, cnt = np.unique(w, return_counts=True)
                assert sorted(cnt) == [1, 2 * T], fam
                p = int(np.flatnonzero(w == u[np.argmin(cnt)])[0])
                assert p == {"odd_first": 0, "odd_tile_end": T - 1, "odd_tile_start": T, "odd_last": 2 * T}[fam]
                assert bin(int(u[0]) ^ int(u[1])).count("1") == 1
            elif fam == "digit_shares":
                for p, b in enumerate(sc.pass_bits(lo, hi)):
                    c = np.bincount(((w >> np.uint64(8 * p)) & np.uint64((1 << b) - 1)).astype(np.int64), minlength=1 << b)
                    assert c.size == 1 << b and c.max() - c.min() <= 1
            elif fam == "digit0_low":
                assert not d0.any() and (hi - lo <= 8 or np.unique(w).size > 1)
            elif fam == "digit255_low":
                assert (d0 == np.uint64((1 << bits0) - 1)).all()
            elif fam == "round_keys":
                s = (hi - lo) // 2
                gid = w >> np.uint64(s)
                assert (np.diff(gid.astype(np.int64)) >= 0).all()         # ordered by the high part already
                assert np.unique(w & np.uint64((1 << s) - 1)).size <= 3
                if hi - lo >= 24:
                    assert np.unique(gid).size > 20
    # the all-ones family under the full window is the padding of a partial tile
    assert (sc.make_keys("all_ones", T + 1, 0, 64, 1, T) == np.uint64(sc.ALL_ONES)).all()
    # an odd record at an index the size does not have: no case
    assert sc.make_keys("odd_tile_start", T, 0, 8, 1, T) is None and sc.make_keys("odd_tile_end", T - 1, 0, 8, 1, T) is None
    assert all(c.n >= T for c in sc.sweep_cases(512, "odd_tile_end")) and all(c.n > T for c in sc.sweep_cases(512, "odd_tile_start"))
    assert all(c.n >= 2 for c in sc.sweep_cases(256, "odd_first"))


@pytest.mark.parametrize("block", sc.BLOCKS)
def test_boundary_family_counts(block):
    T = sc.SORT_ITEMS * block
    cs = sc.boundary_cases(block)
    assert {c.n for c in cs} == {9 * T, 17 * T, 33 * T + 1, 41 * T + 5}
    assert {sc.npasses(c.lo, c.hi) for c in cs} == {2, 3}
    seen = set()
    for c in cs:
        g = sc.geom(c.n, block)
        B = (1 if c.which == "first" else g["chunks"] - 1) * g["tpc"] * T      # a chunk's first record
        assert 0 < B < c.n and B % (g["tpc"] * T) == 0
        assert sc.chunk_of_tile(B // T, g["tpc"]) == sc.chunk_of_tile((B - 1) // T, g["tpc"]) + 1
        if (c.n, c.which, c.delta) in seen:
            continue
        seen.add((c.n, c.which, c.delta))
        k = sc.boundary_keys(c.n, c.lo, c.hi, c.seed, block, c.which, c.delta)
        d0 = (k >> np.uint64(c.lo)) & np.uint64(0xFF)
        assert int((d0 == 0).sum()) == B + c.delta and int((d0 == 1).sum()) == c.n - B - c.delta
        d1 = (k >> np.uint64(c.lo + 8)) & np.uint64((1 << sc.pass_bits(c.lo, c.hi)[1]) - 1)
        assert np.unique(d1).size == 1 << sc.pass_bits(c.lo, c.hi)[1]          # the second digit takes every value
        zeros = np.flatnonzero(d0 == 0)
        assert zeros[0] < T and zeros[-1] > c.n - T and (np.diff(zeros) > 1).any()   # scattered over the input
    assert {d for (_, _, d) in seen} == {-1, 0, 1} and {w for (_, w, _) in seen} == {"first", "last"}
    # "last" at 9T: chunk 4 holds the one tile past 8T; at 41T + 5 chunk 6 is short and chunk 7 empty
    assert sc.boundary_count(9 * T, block, "last", 0) == 8 * T and sc.boundary_count(9 * T, block, "first", 0) == 2 * T
    assert sc.boundary_count(41 * T + 5, block, "last", 1) == 36 * T + 1


def test_sort_model_is_stable():
    #                0     1     2     3     4     5     6     7     8     9
    keys = np.array([0x31, 0x10, 0x31, 0x20, 0x10, 0xF31, 0x00, 0x20, 0x31, 0x10], dtype=np.uint64)
    vals = np.arange(10, dtype=np.uint32) * 11
    k, v = sc.sort_model(keys, vals, 4, 8)          # window values 3 1 3 2 1 3 0 2 3 1; bits 8.. and 0..3 do not count
    assert v.tolist() == [66, 11, 44, 99, 33, 77, 0, 22, 55, 88]
    assert k.tolist() == [0x00, 0x10, 0x10, 0x10, 0x20, 0x20, 0x31, 0x31, 0xF31, 0x31]
    k, v = sc.sort_model(keys, vals, 0, 4)          # 1 0 1 0 0 1 0 0 1 0
    assert v.tolist() == [11, 33, 44, 66, 77, 99, 0, 22, 55, 88]
    k, v = sc.sort_model(keys, None, 0, 64)
    assert v is None and k.tolist() == sorted(keys.tolist())
    # the narrowed form of small windows orders like the plain form
    rng = np.random.default_rng(3)
    keys = rng.integers(0, sc.ALL_ONES, 5000, dtype=np.uint64, endpoint=True)
    vals = rng.integers(0, 50, 5000).astype(np.uint32)
    for lo, hi in sc.WINDOWS + [(5, 21), (3, 19), (48, 64)]:
        order = np.argsort(keys & np.uint64(sc.window_mask(lo, hi)), kind="stable")
        k, v = sc.sort_model(keys, vals, lo, hi)
        assert np.array_equal(k, keys[order]) and np.array_equal(v, vals[order]), (lo, hi)


def test_values_and_mismatch_report():
    v = sc.make_values(3000, "random", 1)
    assert v.dtype == np.uint32 and np.unique(v).size < 1500                   # duplicates
    assert np.array_equal(sc.make_values(5, "iota", 1), np.arange(5, dtype=np.uint32)) and sc.make_values(5, None, 1) is None
    a = np.arange(9 * 4096, dtype=np.uint64)
    b = a.copy()
    assert sc.mismatch(a, b, a.size, 256) is None
    b[2 * 4096 + 7] = 5
    msg = sc.mismatch(b, a, a.size, 256)
    assert "slot 8199 " in msg and "tile 2 of 9" in msg and "chunk 1 of 5" in msg and "tpc 2" in msg, msg


def test_big_case_straddles_a_chunk_in_the_histogram_kernel():
    g = sc.geom(sc.BIG_CASE["n"], sc.BIG_CASE["block"])
    assert g["tiles"] == 2050 and g["hist_per"] >= 2 and g["tpc"] % 2 == 1 and g["tpc"] == 257
    # workgroup 128 counts tiles 256 and 257: the last of chunk 0 and the first of chunk 1
    t = 128 * g["hist_per"]
    assert sc.chunk_of_tile(t, g["tpc"]) == 0 and sc.chunk_of_tile(t + 1, g["tpc"]) == 1
    assert sc.BIG_CASE["windows"] == [(0, 8), (5, 21)]


def test_call_count_stays_bounded():
    n = sc.count_calls()
    assert 3000 < n < 6000, n
