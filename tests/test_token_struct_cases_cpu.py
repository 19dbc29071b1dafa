"""The case module of the token-structure tests without a GPU: its constants against the headers, its two models against plain
Python loops, the two count models against each other on every bounds text, the assertions that the texts stand on the edges they
are named for, and the two read-back entry points: declared, exported, bound, and refusing NULL before any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import token_cases as tc
import token_struct_cases as sc
from test_int_cpu import model_sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "suffixarray_amd", "csrc")

NEW = ["sa_hip_token_index_get_dir_range", "sa_hip_token_index_get_key_range"]


@pytest.mark.parametrize("fname,pattern,value", sc.HEADER_CONSTANTS)
def test_constants_are_the_headers(fname, pattern, value):
    with open(os.path.join(CSRC, fname)) as f:
        found = re.findall(pattern, f.read())
    assert len(found) == 1 and found[0] == value, (fname, pattern, found)
    assert (sc.HIST_LDS, sc.DIR_CAP, sc.BLOCK, sc.STEPS, sc.SC_BLOCK, sc.SC_ITEMS, sc.SC_TILE) == (12288, 1 << 24, 256, 32, 1024, 8, 8192)


def _loop_directory(tl):
    mn, mx = min(tl), max(tl)
    return [sum(1 for x in tl if x < v) for v in range(mn, mx + 2)]


def _loop_keys(tl, sl):
    n = len(tl)
    return [((tl[p] + 1) << 32) | (tl[p + 1] + 1 if p + 1 < n else 0) for p in sl]


def test_models_are_the_plain_loops():
    """directory() and keys() against loops over Python ints, on texts of at most 300 tokens: the bounds texts, a cut of every
    directory text (its tokens of the 60 highest symbols, in text order) and the ends of int32"""
    small = [t for t in sc.BOUNDS_TEXTS.values() if t.size <= 300]
    for name in sc.BINS + sc.TILES + ("top_of_range",):
        t = sc.text(name)
        small.append(t[t > int(t.max()) - 60][:300])
    small += [np.array([0], np.int32), np.array([tc.I32_MAX], np.int32), np.array([tc.I32_MAX, tc.I32_MAX - 9, tc.I32_MAX, tc.I32_MAX - 3], np.int32)]
    assert len(small) > 200
    for t in small:
        tl = [int(v) for v in t]
        sa = model_sa(t)
        assert sorted(range(len(tl)), key=lambda p: tl[p:]) == sa.tolist()
        d = sc.directory(t)
        assert d.dtype == np.uint32 and d.tolist() == _loop_directory(tl), tl[:8]
        k = sc.keys(t, sa)
        assert k.dtype == np.uint64 and k.tolist() == _loop_keys(tl, sa.tolist()), tl[:8]
        assert (np.diff(k.astype(object)) >= 0).all()                        # "K is non-decreasing in r"
    top = sc.keys(np.array([tc.I32_MAX, tc.I32_MAX], np.int32), [1, 0])
    assert top.tolist() == [1 << 63, (1 << 63) | (1 << 31)]                  # "T[p] + 1 reaches 2^31: both fields are unsigned"


def test_describe_names_symbol_rank_and_position():
    t = np.array([7, 5, 9, 5, 7], np.int32)
    sa = model_sa(t)
    assert sa.tolist() == [3, 1, 4, 0, 2]
    s = sc.describe("dir", t, sa, 3)                                         # suffixes below 8: the entry that first counts the 7s
    assert "symbol 8" in s and "symbol 7 stands 2 times" in s and "text position 0" in s and "tile 0" in s
    assert "symbol 6 stands 0 times" in sc.describe("dir", t, sa, 2)
    s = sc.describe("K", t, sa, 2)
    assert "rank 2 is suffix 4" in s and "T[p] = 7" in s and "(the end)" in s
    want = sc.directory(t)
    got = want.copy()
    got[3] += 1
    msg = sc.mismatch("dir", got, want, t, sa)
    assert "1 of 6 entries differ" in msg and "got 5, model 4" in msg and "dir[3]" in msg
    assert sc.mismatch("dir", want, want, t, sa) == "" and "5 entries, model 6" in sc.mismatch("dir", want[:5], want, t, sa)
    k = sc.keys(t, sa)
    bad = k.copy()
    bad[[0, 4]] ^= np.uint64(1)
    msg = sc.mismatch("K", bad, k, t, sa)
    assert "2 of 5" in msg and "K[0]" in msg and "K[4]" in msg


def test_count_models_agree_on_the_bounds_texts():
    """model (a), bisection over the suffix array, and model (b), window counting, on every bounds text and its whole pattern set"""
    seen = 0
    for name in sc.BOUNDS_TEXTS:
        t, sa, pats, first, count, count_b = sc.bounds_expected(name)
        assert np.array_equal(count, count_b), (name, [pats[i] for i in np.flatnonzero(count != count_b)[:5]])
        assert len(pats) == 1554 + 2 + 4 * min(6, t.size) and all(tc.I32_MIN <= v <= tc.I32_MAX for p in pats for v in p), name
        assert int(first[len(sc.SHORT)]) + 1 <= t.size and count[len(sc.SHORT)] == 1 and count[len(sc.SHORT) + 1] == 0      # the whole text, and one more
        assert (first.astype(np.int64) + count <= t.size).all()
        seen += len(pats)
    assert len(sc.BOUNDS_TEXTS) == 3 * 65 + 2 * 6 and seen > 320000
    t = sc.BOUNDS_TEXTS["equal_64"]                                          # closed forms of the all-equal text
    _, _, pats, first, count, _ = sc.bounds_expected("equal_64")
    for m in (1, 2, 3, 4):
        i = pats.index([7] * m)
        assert (first[i], count[i]) == (m - 1, 64 - m + 1)
    assert (first[pats.index([6])], first[pats.index([8])], first[pats.index([7, -1])], first[pats.index([7, 7, -1])]) == (0, 64, 1, 2)


def test_singles_are_the_directory():
    """the expectation of the search over [min - 1, max + 1] restates the directory: first = dir, count = its differences"""
    for name in sc.BINS + sc.TILES + ("hot_above", "top_of_range"):
        v0, q, first, count = sc.singles_expected(name)
        d = sc.dir_of(name)
        t = sc.text(name)
        assert v0 == int(t.min()) - 1 and first[0] == 0 and count[0] == 0
        if name == "top_of_range":
            assert q == d.size and v0 + q - 1 == tc.I32_MAX and np.array_equal(first[1:], d[:-1]) and np.array_equal(count[1:], np.diff(d))
        else:
            assert q == d.size + 1 and np.array_equal(first[1:], d) and np.array_equal(count[1:-1], np.diff(d)) and count[-1] == 0
        assert int(count.sum()) == t.size


def test_info_expected_follows_the_plan():
    assert sc.info_expected("cap_out", "default")["dir_entries"] == 0 and sc.info_expected("cap_in", "default")["dir_entries"] == (1 << 24) + 1
    assert sc.info_expected("cap_in", "no_dir")["dir_entries"] == 0 and sc.info_expected("cap_in", "no_dir")["key_bytes"] == 8
    e = sc.info_expected("top_of_range", "no_keys")
    assert (e["key_bytes"], e["min_symbol"], e["max_symbol"], e["dir_entries"]) == (0, tc.I32_MAX - 12288, tc.I32_MAX, 12290)
    assert sc.sa_of("top_of_range")[e["last_rank"]] == e["n"] - 1
    assert set(sc.FAMILIES) <= set(sc.DIR_TEXTS) and set(sc.WALK_TEXTS) <= set(sc.DIR_TEXTS)
    assert [n for n in sc.DIR_TEXTS if sc.range_of(n) <= sc.SMALL_RANGE] == list(sc.BINS + ("hot_above",) + sc.TILES + ("top_of_range",))


def test_texts_stand_on_their_edges():
    sc.coverage()
    t = sc.text("hot_above")
    assert t.size == 400000 and int((t == sc.MN + 12288).sum()) >= 200000 and int((t == sc.MN + 12287).sum()) >= 100000 and sc.range_of("hot_above") == 20000
    assert sc.text("parts_1024").size == sc.N_TEXT and sc.range_of("parts_1024") + 1 == 1024 * 8192 and sc.range_of("parts_1025") + 1 == 1024 * 8192 + 1
    assert sc.text("cap_in").size == 3000 and np.unique(sc.text("cap_in")).size > 2900
    for n in (1, 2, 31, 32, 33, 63, 64, 65):
        assert sc.BOUNDS_TEXTS["period2_%d" % n].tolist() == ([7, 6] * 33)[:n] and set(sc.BOUNDS_TEXTS["random_%d" % n].tolist()) <= {6, 7, 8}
    assert sc.BOUNDS_TEXTS["equal_but_last_128"].tolist() == [7] * 127 + [8]


def test_coverage_fails_when_a_text_is_left_out():
    for gone in ("bins_12288", "parts_1025", "parts_1024", "hot_above", "tile_8192"):
        with pytest.raises(AssertionError):
            sc.coverage(dir_texts=[n for n in sc.DIR_TEXTS if n != gone])
    with pytest.raises(AssertionError):
        sc.coverage(bounds={k: v for k, v in sc.BOUNDS_TEXTS.items() if k != "equal_65"})


def test_read_backs_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int, name
    for name in ("dir_range", "key_range"):
        assert callable(getattr(capi.TokenIndex, name)), name
        for first, count in ((0, -1), (-1, 1)):                             # refused before the handle is looked at
            with pytest.raises(ValueError):
                getattr(capi.TokenIndex, name)(None, first, count)


def test_read_backs_refuse_null_before_any_device_call(capi):
    """the handle is an address that holds nothing: both calls must return before it is looked at"""
    lib = capi.lib()
    h = 0x1234
    d, k = np.zeros(2, np.uint32), np.zeros(2, np.uint64)
    assert lib.sa_hip_token_index_get_dir_range(None, 0, 1, d.ctypes.data) == -1
    assert b"sa_hip_token_index_get_dir_range" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_get_dir_range(h, 0, 1, None) == -1 and lib.sa_hip_token_index_get_dir_range(h, 0, 0, None) == -1
    assert lib.sa_hip_token_index_get_key_range(None, 0, 1, k.ctypes.data) == -1
    assert b"sa_hip_token_index_get_key_range" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_index_get_key_range(h, 0, 1, None) == -1 and lib.sa_hip_token_index_get_key_range(h, 0, 0, None) == -1
    assert not d.any() and not k.any()
