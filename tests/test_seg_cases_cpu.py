"""The generator and the model of tests/test_gpu_seg.py (tests/seg_cases.py), checked without a GPU: the restated constants are
the headers', plan() / bucket_of() agree with brute-force loops, every case holds what it claims -- measured from its text by
top_digit() and plan() -- the step-wise model agrees with lsd_model on every case and key length (at the reduced geometry),
and every deliberate mistake of the step-wise model shows on the case that is there to catch it."""
import os
import re

import numpy as np
import pytest

import seg_cases as sg
from pipeline_model import choose_split_level, split_levels

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "suffixarray_amd", "csrc")
U64 = np.uint64


@pytest.mark.parametrize("fname,pattern,value", sg.HEADER_CONSTANTS)
def test_constants_are_the_headers(fname, pattern, value):
    with open(os.path.join(CSRC, fname)) as f:
        found = re.findall(pattern, f.read())
    assert found and all(x == value for x in found), (fname, pattern, found)
    assert sg.FULL.T8 == 12288 and sg.FULL.T10 == 7168 and sg.FULL.TS == 14336 and sg.FULL.TT == sg.TEXT_TILE == 8192
    assert all(getattr(sg.FULL, x) == 128 * getattr(sg.SMALL, x) for x in ("n0", "T8", "T10", "TS", "TT"))


def test_plan_and_bucket_of_against_brute_force():
    """random size vectors, one used bucket (the first, one in the middle, the last), all 256 used, runs of empty buckets"""
    rng = np.random.default_rng(3)
    vectors = [np.where(rng.random(256) < p, rng.integers(1, 4000, 256), 0) for p in (0.02, 0.3, 0.9, 1.0) for _ in range(6)]
    for only in (0, 100, 255):
        v = np.zeros(256, np.int64)
        v[only] = 100000
        vectors.append(v)
    vectors.append(rng.integers(1, 3000, 256))
    vectors.append(np.full(256, 96))
    for v in vectors:
        for tile in (96, 97, 1000):
            if v.sum() == 0:
                continue
            pl = sg.plan(v, tile)
            tiles = [-(-int(s) // tile) for s in v]
            assert pl.bstart.tolist() == [int(v[:b].sum()) for b in range(257)]
            assert pl.tprefix.tolist() == [sum(tiles[:b]) for b in range(257)]
            F = sum(tiles)
            for c in range(9):
                first = next(b for b in range(257) if pl.tprefix[b] >= F * c // 8)
                assert pl.cfirst[c] == (F if c == 8 else pl.tprefix[first])
            assert (np.diff(pl.cfirst) >= 0).all() and pl.cfirst[0] == 0      # parts: whole buckets, in order
            assert set(pl.cfirst.tolist()) <= set(pl.tprefix.tolist())
            owner = [b for b in range(256) for _ in range(tiles[b])]             # the bucket of every flat tile, by enumeration
            assert [sg.bucket_of(pl.tprefix, f) for f in range(F)] == owner
            bucket, start, cnt = sg.flat_tiles(pl, tile)
            assert int(cnt.sum()) == int(v.sum()) and (cnt > 0).all()
            # the deliberate mistakes differ: < sends every bucket's first tile to the bucket before
            # (unless bucket 0 is the only one in use: the bisection starts there)
            assert [sg.bucket_of(pl.tprefix, f, strict=True) for f in range(F)] != owner or np.count_nonzero(v[1:]) == 0
    assert sg.passes(8, 5)["passes"] == [("k32", 0, 255), ("k32", 8, 255), ("k32", 16, 255), ("k32", 24, 255)]
    assert sg.passes(8, 3)["passes"] == [("k32", 0, 255), ("k32", 8, 255)] and sg.passes(8, 2)["passes"] == [("k32", 0, 255)]
    assert sg.passes(5, 7)["passes"][-1] == ("k32", 24, 7) and sg.passes(5, 5)["passes"] == [("k32", 0, 255), ("k32", 8, 255), ("k32", 16, 1)]
    assert sg.passes(8, 6)["np_hi"] == 3 and sg.passes(8, 7)["np_hi"] == 4 and sg.passes(8, 7)["passes"][2:] == [("k32", 8 * q, 255) for q in range(4)]
    assert sg.passes(5, 11, 11)["passes"][-1] == ("k32", 24, 127) and sg.passes(5, 11, 0)["chars"] == 12 and sg.passes(5, 11, 0)["passes"][-1] == ("k32", 24, 255)
    assert sg.passes(5, 9)["passes"][-1] == ("k32", 16, 31) and sg.passes(5, 9)["np_hi"] == 3
    assert sg.passes(8, 1)["plan"] is None and sg.passes(8, 8)["plan"] is None and sg.passes(5, 12)["plan"] is None


_texts = {}


def _text(name, geom=sg.FULL):
    key = (name, geom)
    if key not in _texts:
        for k in [k for k in _texts if k[1] == sg.FULL]:
            del _texts[k]
        _texts[key] = sg.make(name, geom)
    return _texts[key]


def _measured(T, plan_, k0):
    top = sg.top_digit(T.t, T.b, k0)
    sizes = np.bincount(top, minlength=256)
    tile = sg.tile_of(plan_)
    pl = sg.plan(sizes, tile)
    return top, sizes, tile, pl


def _chain(pl, b):
    return int(pl.tprefix[b + 1] - pl.tprefix[b])


@pytest.mark.parametrize("name", list(sg.CASES))
def test_case_holds_what_it_claims(name):
    case = sg.CASES[name]
    T = _text(case.text)
    t = T.t
    n = int(t.size)
    _, sigma, b = sg.codes_of(t)
    assert (b, sigma) == (T.b, T.sigma) and sg.NARROW_MIN_N <= n <= sg.N_MAX
    if T.b == 8:
        assert 128 <= sigma <= 255 and np.array_equal(np.unique(t), np.arange(1, sigma + 1))     # byte = code
    for form, k0s in case.runs:
        plan_, env, expect = sg.FORMS[form]
        for k0 in k0s:
            # the plan predicates admit the plan at this n (narrow_sort_applies / narrow48_applies, max_tiles = n / 4096 rounded up)
            spec = sg.passes(T.b, k0, 0)
            if plan_ != 12:
                assert spec["plan"] == {8: "narrow", 10: "narrow48"}[plan_], (name, form, k0)
                assert n // sg.tile_of(plan_) + sg.RADIX + 1 <= -(-n // 4096)
                assert spec["bits"] == 8 + spec["lo_bits"] + spec["hi_bits"] and len(spec["passes"]) == (-(-spec["lo_bits"] // 8) if plan_ == 8 else 2 + spec["np_hi"])
            top, sizes, tile, pl = _measured(T, 10 if plan_ == 12 else plan_, k0)
            key = sg.sort_keys(t, sg.spec_of(T, form, k0, 0))
            assert np.array_equal(top, (key >> U64(sg.spec_of(T, form, k0, 0)["bits"] - 8)).astype(np.int64))
            assert T.b == 5 or np.array_equal(sizes[1:sigma + 1], np.bincount(t, minlength=sigma + 1)[1:])   # a bucket's size is its symbol's count
            bucket, start, cnt = sg.flat_tiles(pl, tile)
            assert int(cnt.sum()) == n
            _claims(name, case, T, plan_, k0, top, sizes, tile, pl, bucket, cnt, key)


def _claims(name, case, T, plan_, k0, top, sizes, tile, pl, bucket, cnt, key):
    t, c, info, n = T.t, case.claim, T.info, int(T.t.size)
    number = case.number
    if number == 1:
        want = sg.tile_sizes(sg.FULL, 8 if plan_ == 8 else 10)
        at = sorted(info["buckets"])[:len(want)]
        assert [int(sizes[d]) for d in at] == want and [info["buckets"][d] for d in at] == want      # exact sizes, adjacent buckets
        assert at == list(range(at[0], at[0] + len(want))) or T.b == 5
        ones = at[:4]
        assert ones == list(range(ones[0], ones[0] + 4)) and sizes[:ones[0]].sum() == 0
        # flat tiles 0..3 are the four one-record buckets: one workgroup of seg_hist_kernel (TPB tiles) spans four buckets
        assert bucket[:sg.TPB].tolist() == ones and cnt[:sg.TPB].tolist() == [1, 1, 1, 1]
        assert [int(sizes[d]) for d in at[4:7]] == [63, 64, 65]
        edge = at[7:15]
        assert [_chain(pl, d) for d in edge] == c["chains"] and [int(sizes[d]) % tile for d in edge] == c["tails"]
        assert {1, sg.INCL_MASK + 1, sg.INCL_MASK + 2} <= set(c["chains"])                       # chains of 1, 4 and 5 tiles
        assert sorted({x % 64 for x in c["tails"]}) == [0, 1, 63]
        for d in edge:                                          # full tiles, then a partial one unless the size is a multiple
            mine = cnt[bucket == d]
            assert (mine[:-1] == tile).all() and int(mine[-1]) == (int(sizes[d]) % tile or tile)
        if plan_ == 8:    # the same list for the split pass's tile: the declined path's first plan call meets other tile counts
            second = at[15:23]
            assert [int(sizes[d]) for d in second] == sg.edge_list(sg.FULL.TS)
            p2 = sg.plan(sizes, sg.FULL.TS)
            assert [_chain(p2, d) for d in second] == c["chains"] and [_chain(pl, d) for d in second] == [2, 2, 2, 3, 3, 5, 5, 6]
            assert not np.array_equal(p2.tprefix, pl.tprefix)
    elif number == 2:
        big = c["big"]
        assert info["big"] == big and int(sizes[big]) * 8 > 7 * n and int(sizes.max()) == int(sizes[big])
        assert pl.cfirst.tolist() == c["cfirst"][plan_], (name, plan_, pl.cfirst.tolist())
        assert (np.diff(pl.cfirst) == 0).sum() >= 3                                  # empty parts: their tickets are stolen
        assert _chain(pl, big) == c["chain"][plan_] >= 300                           # a look-back chain of hundreds of tiles
        others = np.delete(sizes[1:T.sigma + 1], big - 1)
        assert (others == info["small"]).all() and info["small"] <= tile
        assert (sizes[255] > 0) == (big == 255) and T.sigma == (255 if big == 255 else 128)
    elif number == 3:
        F = int(pl.tprefix[256])
        bigs = info["bigs"]
        assert len(bigs) == 8 and all(int(sizes[d]) == info["big"] and info["big"] % tl == 0 for d in bigs for tl in (sg.FULL.T8, sg.FULL.T10, sg.FULL.TS))
        assert int(np.count_nonzero(sizes)) == 128 and int(np.delete(sizes, bigs).max()) <= tile
        for cc in range(1, 8):
            target = F * cc // 8
            assert F * cc % 8 == 0 and target == int(pl.tprefix[bigs[cc]]) + c["offset"]
            # on a bucket's first tile: the part starts there; one tile inside: at the next bucket
            assert int(pl.cfirst[cc]) == int(pl.tprefix[bigs[cc] + c["offset"]])
    elif number == 4:
        used = np.flatnonzero(sizes)
        assert used[0] == info["leading"] == 8 and 255 - used[-1] == info["trailing"] >= 8
        lo, hi = info["run"]
        assert sizes[lo:hi + 1].sum() == 0 and hi - lo + 1 >= 8 and int(sizes[lo - 1]) == 1 and int(sizes[hi + 1]) == 1 and info["ones"] == [lo - 1, hi + 1]
        assert len(set(pl.tprefix[lo:hi + 2].tolist())) == 1                       # the run shares its successor's prefix
    elif number == 5:
        assert k0 == c["k0"]
        spec = sg.passes(8, k0)
        ones = (1 << (spec["bits"] - 8)) - 1
        allones = (key & U64(ones)) == U64(ones)
        order0 = np.argsort(top.astype(np.uint8), kind="stable")
        final = sg.lsd_model(key)
        for d, mod in c["tail"].items():
            slots = np.flatnonzero(allones[order0] & (top[order0] == d))
            assert sorted(order0[slots].tolist()) == info["plants"][d] and len(slots) == 3     # the all-ones keys of the bucket: the plants
            assert int(slots[-1]) == int(pl.bstart[d + 1]) - 1                                  # the top-digit pass leaves one next to the padding
            tail = int(cnt[bucket == d][-1])
            assert tail < tile and tail % 64 == mod
            last3 = final[int(pl.bstart[d + 1]) - 3:int(pl.bstart[d + 1])]
            assert last3.tolist() == info["plants"][d]                                           # and every pass after it all three
        if plan_ == 8:
            assert ones == 0xFFFFFFFF
        else:
            assert ones == (1 << 48) - 1    # k16 = 0xFFFF and k32 = 0xFFFFFFFF
        assert int((allones & (top == 255)).sum()) == 6 * (sg.PAD_RUN - (k0 - 1))             # ... and inside the runs, in bucket 255
    elif number == 6:
        order0 = np.argsort(top.astype(np.uint8), kind="stable")
        slot_of = np.empty(n, np.int64)
        slot_of[order0] = np.arange(n)
        for w, (pos, cnt_w) in enumerate(zip(info["pos"], info["counts"])):
            same = np.flatnonzero(key == key[pos[0]])
            assert np.isin(pos, same).all() and pos.size == cnt_w                  # the copies share the key ...
            assert T.sigma ** k0 < 10 ** 11 or np.array_equal(same, pos)           # ... and nothing else does, once chance cannot repeat it
            assert np.unique(pos // sg.TEXT_TILE).size >= min(cnt_w, 512) // 2     # ... from different tiles of the top-digit pass
            d = int(top[pos[0]])
            in_tiles = np.unique((slot_of[pos] - pl.bstart[d]) // tile)
            assert in_tiles.size >= 2 and in_tiles.size == _chain(pl, d)           # ... into every tile of one bucket
        assert info["counts"][0] == 16385 and all(200 <= x <= 400 for x in info["counts"][1:])
        if plan_ == 8 and sg.passes(T.b, k0)["lo_bits"] == 32:   # default switches: the device declines the three-pass plan on its own count
            levels = split_levels(key, 32, 10)
            assert choose_split_level(levels, 32) == (None, False) and min(levels[1:]) > 16384 >= 16385 - 1
    elif number == 7:
        edges, starts = info["edges"], info["starts"]
        assert n % sg.TEXT_TILE == sg.TEXT_TILE - 1 and edges.size == n // sg.TEXT_TILE == 512
        before = edges - starts
        assert set(before.tolist()) == set(range(1, 7)) and k0 - 1 <= 6              # 1 .. k0 - 1 symbols before an edge, every edge
        for e, s in zip(edges, starts):
            assert t[s:s + 14].tolist() == sg.EDGE_WORD
        assert t[-3:].tolist() == sg.EDGE_WORD[:3]
        low = (key >> U64(sg.spec_of(T, "split=0", k0, 0)["bits"] - 8 * k0)) & U64(255)   # (b = 8: the key's last symbol)
        assert (low[n - (k0 - 1):] == 0).all() and (low[:n - (k0 - 1)] != 0).all()


def _small_runs():
    out = []
    for name, case in sg.CASES.items():
        for form, k0s in case.runs:
            if sg.FORMS[form][0] == 12:
                continue
            for k0 in k0s:
                if (name, sg.FORMS[form][0], k0) not in out:
                    out.append((name, sg.FORMS[form][0], k0))
    return out


@pytest.mark.parametrize("name,plan_,k0", _small_runs())
def test_stepwise_model_is_the_lsd_model(name, plan_, k0):
    """every case and key length at the reduced geometry, with and without the partial character of the 10-byte plan"""
    T = _text(sg.CASES[name].text, sg.SMALL)
    for L in (0, k0):
        spec = sg.passes(T.b, k0, L)
        want = sg.lsd_model(sg.sort_keys(T.t, spec))
        assert np.array_equal(sg.stepwise_model(T.t, spec, sg.SMALL), want), (name, k0, L)
        if spec["chars"] == k0:
            assert np.array_equal(sg.keys_of(T.t, k0)[0][want], np.sort(sg.keys_of(T.t, k0)[0]))


@pytest.mark.parametrize("number", sorted(sg.SENSITIVITY))
def test_a_wrong_step_shows_on_its_case(number):
    """One deliberate mistake per case of the list; the step-wise model with the mistake must leave another order than lsd_model
    on that case.  cfirst rounded the other way is the exception that cannot: either rounding cuts the flat range into parts of
    whole buckets, every tile is still handed out once and no record moves -- on the device the parts only decide which tickets
    are stolen.  What the case pins is the plan itself: the wrong rounding gives other part bounds on it (and the same bounds on
    the unshifted text, where every target is a bucket's first tile)."""
    name, k0, wrong = sg.SENSITIVITY[number]
    assert sg.CASES[name].number == number
    T = _text(sg.CASES[name].text, sg.SMALL)
    if wrong == "cfirst":
        for text, differs in (("part_starts_shifted", True), ("part_starts", False)):
            t = _text(text, sg.SMALL).t
            sizes = np.bincount(sg.top_digit(t, 8, k0), minlength=256)
            for tile in (sg.SMALL.T8, sg.SMALL.T10):
                assert (sg.plan(sizes, tile).cfirst.tolist() != sg.plan(sizes, tile, round_down=True).cfirst.tolist()) == differs
        return
    spec = sg.passes(T.b, k0, k0)
    want = sg.lsd_model(sg.sort_keys(T.t, spec))
    got = sg.stepwise_model(T.t, spec, sg.SMALL, wrong=wrong)
    assert not np.array_equal(got, want)
    pl = sg.plan(np.bincount(sg.top_digit(T.t, T.b, k0), minlength=256), sg.tile_of(8 if spec["plan"] == "narrow" else 10, sg.SMALL))
    print(number, name, wrong, sg.mismatch(got, want, pl, sg.tile_of(8 if spec["plan"] == "narrow" else 10, sg.SMALL)))
    if wrong == "unstable":   # only the tied keys move: the same keys in every slot
        k = sg.sort_keys(T.t, spec)
        assert np.array_equal(k[got], k[want])


def test_every_mistake_is_told_apart_somewhere():
    """all six mistakes of the step-wise model on one small text of each plan: none is a no-op of the model"""
    for name, k0 in (("tile_edges5_8", 7), ("tile_edges5_10", 11)):
        T = _text(name, sg.SMALL)
        spec = sg.passes(T.b, k0, k0)
        want = sg.lsd_model(sg.sort_keys(T.t, spec))
        for wrong in sg.WRONG:
            if wrong == "swap" and spec["plan"] == "narrow":
                continue
            differs = not np.array_equal(sg.stepwise_model(T.t, spec, sg.SMALL, wrong=wrong), want)
            assert differs or wrong == "unstable", (name, wrong)     # (no tied keys planted in these texts)


def test_every_form_runs_on_the_cases_the_table_names():
    """8-byte plan: split=0 on every case, declined on the ties, narrow_k=0 on tile_edges and padding_keys, text_pass=0 on
    tile_edges and text_edges; 10-byte plan: default on every case, the 12-byte control once; one int64 run per plan"""
    by_form = {}
    for name, case in sg.CASES.items():
        for form, k0s in case.runs:
            by_form.setdefault(form, set()).add(case.number)
            assert k0s and sg.FORMS[form][0] in (8, 10, 12)
    assert by_form["split=0"] == by_form["default"] == {1, 2, 3, 4, 5, 6, 7}
    assert by_form["declined"] == {6} and by_form["narrow_k=0"] == {1, 5} and by_form["text_pass=0"] == {1, 7} and len(by_form["12-byte"]) == 1
    wide = [sg.FORMS[c.sa64[0]][0] for c in sg.CASES.values() if c.sa64]
    assert sorted(wide) == [8, 8, 10]     # (the 8-byte plan under SA_HIP_SPLIT=0 and on the declined path)
    assert all(c.sa64 is None or c.sa64[1] in dict(c.runs)[c.sa64[0]] for c in sg.CASES.values())
