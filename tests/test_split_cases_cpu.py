"""The generator and the model of tests/test_gpu_split.py (tests/split_cases.py), checked without a GPU: the restated
constants are the headers', the vectorised model agrees with pipeline_model.three_pass_model on small keys, and every case
holds what it claims -- the level the rule takes and its form, the planted sub-buckets' sizes and empty neighbours, bin
populations, tied slots and staged entries per sub-bucket, the planted top-digit buckets."""
import os
import re

import numpy as np
import pytest

import split_cases as sc
from pipeline_model import three_pass_model

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "suffixarray_amd", "csrc")


@pytest.mark.parametrize("fname,pattern,value", sc.HEADER_CONSTANTS)
def test_constants_are_the_headers(fname, pattern, value):
    with open(os.path.join(CSRC, fname)) as f:
        found = re.findall(pattern, f.read())
    assert found and all(x == value for x in found), (fname, pattern, found)
    assert sc.TEXT_TILE == 512 * 16 and sc.BLD_TILE == 256 * 16 and sc.LOCAL_CAP == sc.LOCAL_BLOCK * 16 and sc.LOCAL_CAP_BIG == sc.LOCAL_BLOCK_BIG * 16


def test_vector_model_is_the_three_pass_model():
    """random keys with planted duplicates, caps small enough for every branch of the level rule: small form, large form, declined"""
    rng = np.random.default_rng(5)
    seen = set()
    for n, sigma, k0, cap, dbits, dup in ((60000, 27, 6, 64, 19, 0), (60000, 27, 5, 300, 17, 0), (50000, 4, 12, 40, 19, 0), (40000, 27, 6, 16, 19, 0),
                                          (60000, 27, 6, 64, 18, 100), (60000, 27, 6, 64, 18, 129), (30000, 3, 14, 8, 16, 0)):
        b = 1
        while (1 << b) < sigma + 1:
            b += 1
        p = [0.5] + [0.5 / (sigma - 1)] * (sigma - 1) if sigma == 3 else None
        codes = rng.choice(np.arange(1, sigma + 1), n + k0, p=p).astype(np.uint64)
        codes[n:] = 0
        key = np.zeros(n, np.uint64)
        for j in range(k0):
            key = (key << np.uint64(b)) | codes[np.arange(n) + j]
        key[n - dup:] = key[0]          # a group that no level makes smaller: the large form, or declined
        lo_bits = b * k0 - 8
        ref = three_pass_model(key, lo_bits, dbits, cap=cap, cap_big=2 * cap, seed=n)
        got = sc.vector_model(key, lo_bits, dbits, cap=cap, cap_big=2 * cap, directory=True)
        if ref is None:
            assert got["rb"] is None
            seen.add(None)
            continue
        seen.add(ref["big"])
        assert (got["rb"], got["big"], got["levels"]) == (ref["rb"], ref["big"], ref["levels"])
        assert np.array_equal(got["keys"], ref["keys"]) and np.array_equal(got["sa"], ref["sa"]) and np.array_equal(got["dir"], ref["dir"])
        assert list(zip(got["tied"].tolist(), got["head"].tolist())) == ref["staged"] and len(ref["staged"]) > 0
        pos = np.array([p for p, _ in ref["staged"]])
        per_sub = np.bincount(np.searchsorted(got["sub_starts"], pos, side="right") - 1, minlength=got["sub_counts"].size)
        assert np.array_equal(got["staged_per_sub"], per_sub) and int(got["sub_counts"].max()) == got["split_max"]
    assert seen == {False, True, None}
    assert sc.default_dir_bits(1 << 22) == 19 and sc.default_dir_bits((1 << 22) + 1) == 20 and sc.default_dir_bits(100) == 8
    assert sc.runs([0, 1, 5, 6, 7, 9]) == [(0, 2), (5, 3), (9, 1)]


_texts = {}


def _measured(name):
    """text and measure() of a case; the texts that several cases share are made once"""
    case = sc.CASES[name]
    if case.text not in _texts:
        _texts.clear()
        _texts[case.text] = sc.make(case.text)
    T = _texts[case.text]
    return case, T, sc.measure(T.t, T.k, case.env)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_holds_what_it_claims(name):
    case, T, m = _measured(name)
    c = case.claim
    t = T.t
    assert int(np.unique(t).size) == T.A.size <= 31 and m["b"] == 5 and np.array_equal(np.unique(t), T.A)
    form = None if not m["rb"] else ("big" if m["big"] else "small")
    assert (m["plan"], form, m["split_max"], m["lite"], m["narrow_k"]) == (c["plan"], c["form"], c["split_max"], c["lite"], c.get("narrow_k", 1)), \
        (name, m["plan"], form, m["split_max"], m["lite"], m.get("levels"))
    if name == "len_m1":
        assert t.size == sc.NARROW_MIN_N - 1 and not m["considered"]
    if "text_tiles" in c:
        assert divmod(int(t.size), sc.TEXT_TILE) == c["text_tiles"]
    if name.startswith("len_"):   # the last planted word ends the text: its shifted keys run into the zero padding
        assert int(m["key_of"][-8]) >> 20 == (((1 << 5 | 2) << 5 | 3) << 5 | sc.X) and int(m["key_of"][-1]) & ((1 << 35) - 1) == 0
        assert int(m["key_of"][-7]) & 31 == 0 and int(m["key_of"][-8]) & 31 != 0
    if c["form"] is None:
        if name == "sub_16385":   # declined on the device's own count: the group never shrinks
            assert m["levels"][1:] == [16385] * 10
        return
    assert m["levels"][m["rb"]] <= (sc.LOCAL_CAP_BIG if m["big"] else sc.LOCAL_CAP)
    if not m["big"]:
        assert m["rb"] == 1 or m["levels"][m["rb"] - 1] > sc.LOCAL_CAP
    elif not case.env.get("SA_HIP_LOCAL_BIG"):
        assert min(m["levels"][1:]) > sc.LOCAL_CAP
    for word, size in zip(T.words, c.get("subs", [])):
        v = sc.sub_view(m, sc.sub_of(m, word))
        assert (v["size"], v["before"], v["after"]) == (size, 0, 0), (name, v["size"], v["before"], v["after"])
    if name.startswith("sub_"):   # fixed through every level
        assert m["levels"][2:] == [c["subs"][0]] * 9
    if "subs" in c:
        sb = sc.sub_of(m, T.words[0])
        v = sc.sub_view(m, sb)
        nonempty = np.flatnonzero(m["sub_counts"])
        if c.get("first"):
            assert sb == nonempty[0]
        if c.get("last"):
            assert sb == nonempty[-1]
        if "tied" in c:
            assert sc.runs(v["tied"]) == c["tied"], (name, sc.runs(v["tied"]))
            # the slots' keys: equal inside a group; groups = the number of distinct keys among the tied slots
            ks = m["keys"][v["start"] + np.array(v["tied"])]
            if "groups" in c:
                assert np.unique(ks).size == c["groups"]
        if "staged" in c:
            assert v["staged"] == c["staged"] and (c["staged"] > sc.LITE_CAP) == (c["lite"] == 0)
            others = np.delete(m["staged_per_sub"], sb)
            assert int(others.max()) < sc.LITE_CAP      # no other row decides lite_flags
        if "bins" in c:
            assert m["bb"] == c["bb"]
            for bn, pop in c["bins"].items():
                assert int(v["bins"][bn]) == pop, (name, bn, int(v["bins"][bn]))
            if c.get("only"):
                assert np.count_nonzero(v["bins"]) == 1
            if "last_slot_bin" in c:
                last = c["last_slot_bin"]
                assert v["last_bin_of_last_slot"] == last == (1 << m["bb"]) - 1 and int(v["bins"][last]) % 2 == 1
                # empty and populated bins at both ends
                assert v["bins"][0] == 1 and v["bins"][1] == 0 and v["bins"][last - 1] == 0
    if "g2" in c:
        assert m["g2"] == c["g2"] and m["bb"] == 12 and m["fused"] == (c["g2"] <= 12)
    if "buckets" in c:
        top = np.bincount((m["key_of"] >> np.uint64(m["lo_bits"])).astype(np.int64), minlength=256)
        T_ = 512 * int(case.env.get("SA_HIP_SPLIT_ITEMS", sc.SPLIT_ITEMS))
        assert sorted(c["buckets"].values()) == [1, T_ - 1, T_, T_ + 1, 2 * T_]
        for d, size in c["buckets"].items():
            assert int(top[d]) == size, (name, d, int(top[d]))


def test_tied_pairs_sit_where_the_names_say():
    """the slots the tie cases are about, against the kernel's geometry: rows of 16 lanes, items of LOCAL_BLOCK slots"""
    a, b, c = (dict(sc.TIES[x][1]) for x in "abc")
    m = sc.TIES["a"][0]
    assert 0 in a and 15 in a and sc.LOCAL_BLOCK - 1 in a and m - 2 in a and all(v == 2 for v in a.values())
    assert 16 in b and sc.LOCAL_BLOCK in b and b[100] == 3 and b[103] == 2
    assert c == {13: 5} and 13 < 15 < 16 <= 13 + 5 - 1


@pytest.mark.parametrize("name", ["sub_8192", "sub_16384"])
def test_oracle_array_is_a_stable_sort_of_the_keys(oracle, name):
    """one small-form and one large-form case: the suffix array orders the model's keys, and equal keys by what follows them"""
    case, T, m = _measured(name)
    sa = oracle.sais(T.t).astype(np.int64)
    assert np.array_equal(m["key_of"][sa], m["keys"])
    assert np.array_equal(np.sort(sa), np.arange(T.t.size))
