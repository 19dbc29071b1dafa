"""CPU: the record-retrieval model and the row-table generators of cases.py (the yardstick of tests/test_gpu_rows.py) against a
brute-force scan, and -- on a machine without a device -- the library's host implementation against the model."""
import numpy as np
import pytest

import cases

SMALL = (1, 255, 256, 257, 512, 513)


@pytest.fixture(scope="module")
def row_cases(oracle):
    """name -> (text, starts, patterns, claims, oracle suffix array, oracle ranges of the patterns)"""
    out = {}
    made = {"main": cases.rows_main_case()}
    made.update({"rows%d" % n: cases.rows_small_case(n) for n in SMALL})
    for name, (text, starts, pats, claim) in made.items():
        sa = oracle.sais(text).astype(np.uint32)
        names = list(pats)
        rg = oracle.query_batch(text, sa, 0xFFFFFFFF, [pats[m] for m in names])
        out[name] = (text, starts, pats, claim, sa, dict(zip(names, rg)))
    return out


def _brute_rows(raw, rank, starts, pat):
    """every occurrence by bytes.find, ordered by the suffix array, mapped to rows; distinct rows in order of first hit"""
    pos = []
    i = raw.find(pat)
    while i >= 0:
        pos.append(i)
        i = raw.find(pat, i + 1)
    pos = np.array(sorted(pos, key=lambda p: rank[p]), dtype=np.uint64)
    rows = np.searchsorted(starts, pos, side="right").astype(np.int64) - 1
    _, first = np.unique(rows, return_index=True)
    return pos.size, rows[np.sort(first)]


def test_generators_plant_what_they_claim(row_cases):
    assert set(row_cases) == {"main"} | {"rows%d" % n for n in SMALL}
    for name, (text, starts, pats, claim, sa, rg) in row_cases.items():
        raw = bytes(text)
        assert raw.endswith(b"\n") and starts[0] == 0 and np.all(np.diff(starts.astype(np.int64)) > 0), name
        assert np.array_equal(starts[1:], np.flatnonzero(text == 10)[:-1] + 1), name          # one row per line
        assert set(np.unique(text).tolist()) <= set(range(97, 123)) | set(range(65, 91)) | {10}, name
        rank = np.empty(sa.size, np.int64)
        rank[sa] = np.arange(sa.size)
        for m, (hits, distinct) in claim.items():
            n, rows = _brute_rows(raw, rank, starts, pats[m])
            assert (n, rows.size) == (hits, distinct), (name, m)
            assert int(cases.range_hits(np.array([rg[m]]))[0]) == hits, (name, m)
    for n in SMALL:
        assert row_cases["rows%d" % n][1].size == n
    main = row_cases["main"][3]
    assert main["nl"] == (70_001, 70_001) and 70_001 % 256 != 0
    for h in (1, 2, 3, 4, 5, 6, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 20_000):
        assert main["h%d" % h][0] == h and main.get("u%d" % h, (h, h)) == (h, h)
    assert main["fill64"][1] == 163 and main["fill1536"][1] == 1855 and main["fill4096"][1] == 4455
    assert main["one20000"] == (20_000, 1) and main["one300"] == (300, 1)
    assert main["handoff4096"] == (4096, 10) and main["handoff4097"] == (4097, 11) and main["handoff5000"] == (5000, 914)
    # the three miss encodings: lb = n, a miss inside the array, a pattern below every suffix (second = first - 1 wraps)
    rg = row_cases["main"][5]
    assert tuple(rg["miss_end"]) == (0xFFFFFFFF, 0xFFFFFFFF)
    assert int(rg["miss_mid"]["second"]) == int(rg["miss_mid"]["first"]) - 1 > 0
    assert tuple(rg["miss_wrap"]) == (0, 0xFFFFFFFF)


def test_planted_order_and_row_edges(row_cases):
    """The tags put the hits of a marker in the planted order: the model's rows are the planted rows, first hit first; hits on
    a row's first byte, on its newline, in row 0 and in the last row land where they should."""
    text, starts, pats, claim, sa, rg = row_cases["main"]
    names = list(pats)
    ranges = np.array([rg[m] for m in names])
    _, rows = cases.rows_reference(sa, starts, ranges, 10 ** 9)
    got = dict(zip(names, rows))
    N = starts.size
    f, s = int(rg["head"]["first"]), int(rg["head"]["second"])
    assert set(sa[f:s + 1].tolist()) <= set(starts.tolist())                      # first bytes
    assert 0 in got["head"] and N - 1 in got["head"]
    f, s = int(rg["nl_head"]["first"]), int(rg["nl_head"]["second"])
    assert np.all(text[sa[f:s + 1]] == 10) and np.all(np.isin(sa[f:s + 1] + 1, starts))   # newlines: the row before
    assert sorted(got["nl_head"].tolist()) == sorted(r - 1 for r in got["head"].tolist() if r > 0)
    assert got["nl"][0] == N - 1                                                    # the final newline sorts first among "\n..."
    assert got["ends"].tolist()[:2] == [N - 1, 0] and got["ends"].size == 3
    assert got["rep_aba"].size == 2 and got["rep_abca"].size == 3 and got["rep_abcab"].size == 3


def test_rows_reference_equals_brute_force(row_cases):
    """rows_reference against bytes.find + the oracle's suffix array, every pattern of every case, for k up to past the rows,
    and on the zero-length-row table of every case (upper bound: the last of several rows at one offset)"""
    for name, (text, starts, pats, claim, sa, rg) in row_cases.items():
        raw = bytes(text)
        rank = np.empty(sa.size, np.int64)
        rank[sa] = np.arange(sa.size)
        names = list(pats)
        ranges = np.array([rg[m] for m in names])
        for table in (starts, cases.zero_length_rows(starts)):
            if table is not starts:
                assert table.size > starts.size and np.any(np.diff(table.astype(np.int64)) == 0) and table[1] == 0
            for k in (1, 2, 5, 64, 257, 4096, 10 ** 9):
                cnt, rows, fh = cases.rows_reference(sa, table, ranges, k, with_first_hits=True)
                for m, c, r, h in zip(names, cnt, rows, fh):
                    _, exp = _brute_rows(raw, rank, table, pats[m])
                    exp = exp[:k]
                    assert c == exp.size == r.size and np.array_equal(r, exp), (name, m, k)
                    assert np.all(np.diff(h) > 0)
    # zero-length rows: the row holding byte 0 is the LAST row that starts at 0
    text, starts, pats, claim, sa, rg = row_cases["rows257"]
    z = cases.zero_length_rows(starts)
    cnt, rows = cases.rows_reference(sa, z, np.array([rg["head"]]), 10 ** 9)
    last0 = int(np.flatnonzero(z == 0)[-1])
    assert last0 >= 1 and last0 in rows[0].tolist() and min(rows[0].tolist()) == last0


def test_host_rows_equal_the_model(capi, oracle, monkeypatch):
    """No device and SA_HIP_ALLOW_HOST=1: the library's host implementation (csrc/records.hpp: distinct_rows behind
    sa_hip_index_query_rows[_batch]) against the model -- every pattern of the small cases and of the main text, several
    k, both row tables, the batch and the one-query call, slots past every count untouched."""
    if capi.lib().sa_hip_device_count() >= 1:
        pytest.skip("a HIP device is present: the host path is never taken")
    monkeypatch.setenv("SA_HIP_ALLOW_HOST", "1")
    made = [cases.rows_small_case(n) for n in SMALL] + [cases.rows_main_case()]
    sentinel = np.uint64(0xDEADBEEFDEADBEEF)
    for text, starts, pats, claim in made:
        names = list(pats)
        plist = [pats[m] for m in names]
        with capi.DeviceIndex(text.size, 0) as idx:
            idx.build(text)
            assert idx.verify() == 0
            sa = idx.sa_u32()
            assert np.array_equal(sa, oracle.sais(text).astype(np.uint32))
            ranges = idx.query_batch(plist)
            assert np.array_equal(ranges, oracle.query_batch(text, sa, 0xFFFFFFFF, plist))
            for table in (starts, cases.zero_length_rows(starts)):
                idx.set_rows(table)
                for k in (0, 1, 4, 65, 4097, 10 ** 9):
                    if k <= 4097:
                        out = (np.full((len(plist), max(k, 1)), sentinel), np.zeros(len(plist), np.uint32),
                               np.zeros(len(plist), ranges.dtype))
                        (got, cnt), rg = idx.query_rows_batch_raw(plist, k, out=out)
                        assert np.array_equal(rg, ranges)
                        ecnt, erows = cases.rows_reference(sa, table, ranges, k)
                        assert np.array_equal(cnt, ecnt), k
                        for q in range(len(plist)):
                            assert np.array_equal(got[q, :cnt[q]], erows[q]), (names[q], k)
                            assert np.all(got[q, cnt[q]:] == sentinel), (names[q], k)
                    if k:
                        kq = min(k, 2 * table.size)   # (the one-query wrapper sizes its buffer by k; the library clamps k to the rows)
                        _, erows = cases.rows_reference(sa, table, ranges, kq)
                        for q in range(len(plist)):
                            one, rg1 = idx.query_rows(plist[q], kq)
                            assert np.array_equal(one, erows[q]) and rg1 == tuple(ranges[q]), (names[q], k)
