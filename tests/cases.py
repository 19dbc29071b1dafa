"""Shared input cases for the parity tests (same seeds on CPU and GPU)."""
import numpy as np
import pytest

from suffixarray_amd import synth


def small_texts():
    rng = np.random.default_rng(42)
    c = {
        "banana": np.frombuffer(b"banana", np.uint8),
        "mississippi": np.frombuffer(b"mississippi", np.uint8),
        "len1": np.frombuffer(b"z", np.uint8),
        "len2": np.frombuffer(b"ba", np.uint8),
        "aa": np.frombuffer(b"aa", np.uint8),
        "all_a_5000": synth.all_same(5000),
        "all_a_70000": synth.all_same(70000),
        "ab_3000": synth.periodic(6000, 2),
        "abc_2000": synth.periodic(6000, 3),
        "period7": synth.periodic(50001, 7),
        "fib": synth.fibonacci(46368),
        "perm256": np.tile(np.arange(256, dtype=np.uint8), 20),
        "highbit": np.tile(np.frombuffer(bytes([255, 0, 128, 255, 255, 0, 0, 1]), np.uint8), 300),
        "zeros": np.zeros(3000, np.uint8),
        "with_nul": np.frombuffer(b"ab\x00ab\x00\x00abab\x00", np.uint8),
    }
    for n in (3, 63, 64, 65, 4095, 4096, 4097, 8193, 65535, 65536, 65537):
        c[f"r27_{n}"] = rng.integers(97, 124, n, dtype=np.uint8)
    for sig in (2, 4, 256):
        c[f"r{sig}_30000"] = rng.integers(0, sig, 30000, dtype=np.uint8)
    c["d1_300k"] = synth.d1_uniform27(300_000)
    c["d2_300k"] = synth.d2_words(300_000)
    # long repeats: a random block repeated, forces doubling rounds on a large active set
    blk = rng.integers(97, 101, 5000, dtype=np.uint8)
    c["repeat_block"] = np.tile(blk, 12)
    return c


def reference_query_cases():
    """(alphabet size, text, patterns) of the oracle-against-the-reference query test: 100 000 characters with 4 % newlines,
    1500 patterns of 1..40 bytes, half of them text windows.  Their reference ranges are in tests/golden/golden_ref_cases.npz."""
    rng = np.random.default_rng(11)
    out = []
    for sig in (26, 4, 2):
        n = 100_000
        t = (rng.integers(0, sig, n) + 97).astype(np.uint8)
        t[rng.random(n) < 0.04] = 10
        pats = []
        for i in range(1500):
            m = int(rng.integers(1, 41))
            if i % 2 == 0:
                p = int(rng.integers(0, n - m))
                pats.append(bytes(t[p:p + m]).replace(b"\n", b"a"))
            else:
                pats.append(bytes((rng.integers(0, sig, m) + 97).astype(np.uint8)))
        out.append((sig, t, pats))
    return out


def query_patterns(text, count, rng, maxlen=40):
    n = text.size
    pats = []
    for i in range(count):
        m = int(rng.integers(1, maxlen + 1))
        if i % 2 == 0 and n > m:
            p = int(rng.integers(0, n - m))
            pats.append(bytes(text[p:p + m]))
        else:
            pats.append(bytes(rng.integers(97, 123, m, dtype=np.uint8)))
    pats += [b"", b"a", b"zzzzzzzz", bytes([255]) * 3, bytes([1]), bytes(text[-5:]), bytes(text[-1:]), bytes(text[:7])]
    return pats


def check_partitioned(SuffixArray, tmp_path):
    """documents cut into partitions of whole documents (the reference's scheme for inputs beyond one index, pyx:148-180,
    221-247): the same records as one index over everything, k honoured across partitions, save / load."""
    rng = np.random.default_rng(17)
    words = ["alpha", "beta", "gamma", "delta", "Milk", "store", "fox", "lazy dog", "quick", "brown"]
    docs = [" ".join(words[j] for j in rng.integers(0, len(words), rng.integers(2, 9))) + (" #%d" % i) for i in range(120)]
    one = SuffixArray(documents=docs, max_suffix_length=32)
    part = SuffixArray(documents=docs, max_suffix_length=32, partition_bytes=700)
    assert len(part.partitions) >= 5 and len(one.partitions) == 1
    for q in ("milk", "lazy dog", "FOX", "#7", "zzz", "a", "alpha beta"):
        exp = [d for d in docs if q.lower() in d.lower()]
        assert sorted(one.query_records(q, k=10**6)) == sorted(exp)
        assert sorted(part.query_records(q, k=10**6)) == sorted(exp), q
        few = part.query_records(q, k=3)
        assert len(few) == min(3, len(exp)) and all(r in exp for r in few)
    got = part.query_records_batch(["milk", "", "delta", "zzz"], k=5)
    assert got[1] == [] and got[3] == [] and len(got[0]) == min(5, sum("milk" in d.lower() for d in docs)) and all("delta" in r.lower() for r in got[2])
    with pytest.raises(RuntimeError):
        part.query_ranges(["milk"])
    part.save(str(tmp_path / "parts"))
    back = SuffixArray.load(str(tmp_path / "parts"))
    assert len(back.partitions) == len(part.partitions)
    assert sorted(back.query_records("quick", k=10**6)) == sorted(d for d in docs if "quick" in d.lower())
    for x in (one, part, back):
        x.close()


def check_partitioned_csv(SuffixArray, tmp_path):
    """a CSV column cut into partitions of whole rows (sa_hip_csv_index_create_partitioned; the reference cuts the file every
    2 GiB, engine.c:1437-1481, and answers from the partitions one after the other, pyx:221-247): the same rows as one index over
    the whole column, quoted fields and commas inside them included, k honoured across partitions, save / load."""
    import csv as _csv
    rng = np.random.default_rng(23)
    words = ["Acme", "Globex", "Initech", "Umbrella", "Hooli", "Vehement", "Massive Dynamic", "Stark", "Wayne", "Wonka"]
    tails = ["", " Inc", " LLC", ", Inc.", " Ltd", ' "The Best"']
    rows = [(str(i), words[int(rng.integers(0, len(words)))] + " " + words[int(rng.integers(0, len(words)))] + tails[int(rng.integers(0, len(tails)))],
             ["US", "DE", "FR"][i % 3]) for i in range(600)]
    path = str(tmp_path / "companies.csv")
    with open(path, "w", newline="") as f:
        w = _csv.writer(f)
        w.writerow(["id", "company_name", "country"])
        w.writerows(rows)
    one = SuffixArray(csv_file=path, search_column="company_name", max_suffix_length=32)
    part = SuffixArray(csv_file=path, search_column="company_name", max_suffix_length=32, partition_bytes=1500)
    assert len(one.partitions) == 1 and len(part.partitions) >= 6
    assert part.columns == ["id", "company_name", "country"]

    def ids(recs):
        return sorted(int(r["id"]) for r in recs)
    for q in ("acme", "INC", ", inc.", "massive dynamic", "the best", "zzz", "a", "hooli w"):
        exp = sorted(int(r[0]) for r in rows if q.lower() in r[1].lower())
        assert ids(one.query_records(q, k=10**6)) == exp, q
        got = part.query_records(q, k=10**6)
        assert ids(got) == exp, q
        assert all(set(r) == {"id", "company_name", "country"} for r in got)
        few = part.query_records(q, k=4)
        assert len(few) == min(4, len(exp)) and all(int(r["id"]) in exp for r in few)
    got = part.query_records_batch(["acme", "", "wonka", "zzz"], k=7)
    assert got[1] == [] and got[3] == [] and len(got[0]) == min(7, sum("acme" in r[1].lower() for r in rows))
    assert all("wonka" in r["company_name"].lower() for r in got[2])
    part.save(str(tmp_path / "csvparts"))
    back = SuffixArray.load(str(tmp_path / "csvparts"))
    assert len(back.partitions) == len(part.partitions) and back.columns == part.columns
    assert ids(back.query_records("stark", k=10**6)) == sorted(int(r[0]) for r in rows if "stark" in r[1].lower())
    for x in (one, part, back):
        x.close()


# -- alphabets of every code width ---------------------------------------------------------------------------------------------
# The build packs every byte into a code of b = bits_for(sigma + 1) bits (code 0 stays free), and b picks the key length and
# with it the sort plan.  These sigmas put every b from 1 to 9 at both of its ends: 2^(b-1) and the all-ones 2^b - 1.
ALPHABET_SIGMAS = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256)
_VARIANTS = ("mid", "lo", "hi", "ends")


def code_bits(sigma):
    """b of an alphabet of sigma bytes: the smallest b with 2^b >= sigma + 1 (csrc/common.hpp: bits_for)."""
    return max(1, int(sigma).bit_length())


def alphabet(sigma, variant):
    """sigma distinct byte values, evenly spaced so that absent ("gap") bytes lie between present ones wherever sigma < 256.
    variant: "mid" holds neither byte 0 nor byte 255, "lo" holds byte 0, "hi" holds byte 255, "ends" holds both."""
    lo = 0 if variant in ("lo", "ends") else 1
    hi = 255 if variant in ("hi", "ends") else 254
    if sigma > hi - lo + 1:
        raise ValueError("alphabet %d does not fit variant %s" % (sigma, variant))
    if sigma == 1:
        return np.array([hi if variant == "hi" else lo], dtype=np.uint8)
    vals = np.round(np.linspace(lo, hi, sigma)).astype(np.int64)
    assert np.unique(vals).size == sigma
    return vals.astype(np.uint8)


def alphabet_cases():
    """(id, sigma, variant) of the sweep: the variants rotate through the sigmas; 255 bytes are spaced only with both ends."""
    out = []
    for i, s in enumerate(ALPHABET_SIGMAS):
        v = "ends" if s >= 255 else _VARIANTS[i % 4]
        out.append(("s%d_b%d" % (s, code_bits(s)), s, v))
    return out


def gap_bytes(alph):
    """absent bytes strictly between the smallest and the largest present one"""
    present = np.zeros(256, bool)
    present[alph] = True
    return np.flatnonzero(~present[int(alph.min()):int(alph.max()) + 1]) + int(alph.min())


def alphabet_text(alph, n, kind, seed):
    """n bytes over exactly the bytes of alph (every one occurs).
    kind "uniform": i.i.d. uniform.  kind "binary": binary-like -- Zipf weights (the smallest byte the most frequent, the
    others in a random order of rank) and runs of the smallest byte (byte 0 where the alphabet has it) of geometric length,
    about a tenth of the text: skewed top-digit buckets and long ties."""
    rng = np.random.default_rng(seed)
    alph = np.sort(np.asarray(alph, dtype=np.uint8))
    s = alph.size
    if kind == "uniform":
        t = alph[rng.integers(0, s, n)]
    elif kind == "binary":
        order = np.concatenate([[0], 1 + rng.permutation(s - 1)])
        w = 1.0 / (np.arange(s) + 1.0) ** 1.1
        p = np.empty(s)
        p[order] = w / w.sum()
        t = alph[rng.choice(s, n, p=p)]
        runs = int(n * 0.1 / 64) + 1
        starts = rng.integers(0, n, runs)
        lens = rng.geometric(1.0 / 64, runs)
        for a, m in zip(starts, lens):
            t[a:a + m] = alph[0]
    else:
        raise ValueError(kind)
    if n >= s:   # every byte present: one shuffled copy of the alphabet somewhere
        p0 = int(rng.integers(0, n - s + 1))
        t[p0:p0 + s] = rng.permutation(alph)
    return np.ascontiguousarray(t, dtype=np.uint8)


WORD_LENGTHS = (8, 9, 16, 31, 32, 33, 40, 64)   # the word boundaries of the query's pattern_words / cmp_suffix


def edge_patterns(text, alph, k0, k2n, L, rng):
    """Patterns where a query over packed keys can go wrong: text windows of every length around the key and the second-level
    key (1 .. k0 + k2n + 2) and at the 8-byte word boundaries; runs of the largest and of the smallest present byte; windows
    with one byte replaced by an absent byte between present ones, a byte below the smallest or one above the largest, at
    positions 0, k0 - 1, k0, k0 + 1 and last; windows that run past the end of the text; the empty pattern; and, for a
    truncated build (L > 0), patterns longer than L."""
    n = int(text.size)
    alph = np.sort(np.asarray(alph, dtype=np.uint8))
    lo, hi = int(alph[0]), int(alph[-1])
    pats = [b""]

    def window(m):
        m = min(m, n)
        p = int(rng.integers(0, n - m + 1))
        return bytes(text[p:p + m])

    lengths = sorted(set(range(1, k0 + k2n + 3)) | set(WORD_LENGTHS))
    for m in lengths:
        pats += [window(m) for _ in range(3)]
    for m in sorted({1, 2, max(k0 - 1, 1), k0, k0 + 1, k0 + k2n + 1, 40, 65}):
        pats += [bytes([hi]) * m, bytes([lo]) * m]
    gaps = gap_bytes(alph)
    subs = []
    if gaps.size:
        subs += [int(gaps[0]), int(gaps[-1]), int(gaps[gaps.size // 2])]
    if lo > 0:
        subs += [lo - 1, 0]
    if hi < 255:
        subs += [hi + 1, 255]
    for m in (k0 + 2, k0 + k2n + 2, 33):
        for pos in sorted({0, max(k0 - 1, 0), k0, k0 + 1, m - 1}):
            if pos >= m:
                continue
            for c in subs:
                for _ in range(2):
                    w = bytearray(window(m))
                    if pos < len(w):
                        w[pos] = c
                    pats.append(bytes(w))
    for m in sorted({1, max(k0 - 1, 1), k0, k0 + 3, 40}):
        tail = bytes(text[max(n - m, 0):])
        pats += [tail, tail + bytes([lo]), tail + bytes([hi]), tail + bytes(text[:5])]
        if subs:
            pats.append(tail + bytes([subs[0]]))
    if L:
        for m in (L + 1, L + 5, 2 * L + 3, 70):
            w = bytearray(window(m))
            pats.append(bytes(w))
            if subs and len(w) > L:
                w[L] = subs[0]                # a change past L does not matter
                pats.append(bytes(w))
                w[L - 1] = subs[-1]           # a change at L - 1 does
                pats.append(bytes(w))
    return pats


def big_batch(text, edge, count, rng, maxlen=80):
    """the edge patterns followed by text windows of 1 .. maxlen bytes, count patterns in all (a batch this large builds the
    second-level keys of a wide-key index, csrc/sa_capi.hip: K2_AUTO_BATCH)"""
    n = int(text.size)
    out = list(edge)
    while len(out) < count:
        m = int(rng.integers(1, maxlen + 1))
        p = int(rng.integers(0, max(n - m, 0) + 1))
        out.append(bytes(text[p:p + m]))
    return out[:count]


def brute_ranges(text, max_suffix_length, patterns):
    """The query's result from Python's own order of the suffixes: {lb, ub - 1} over the suffixes whose first
    c = min(len, max_suffix_length) bytes compare below / not above the pattern's (a suffix that ends first is smaller),
    lb == n -> {UINT32_MAX, UINT32_MAX} (the conventions of test_oracle.py::test_query_edge_conventions).  Quadratic in n."""
    import bisect
    raw = bytes(text)
    n = len(raw)
    suffixes = sorted(raw[s:] for s in range(n))   # a suffix order sorts every prefix length the same way
    L = max_suffix_length if max_suffix_length else 1 << 32
    out = []
    for q in patterns:
        c = min(len(q), L)
        q = q[:c]
        lb = bisect.bisect_left(suffixes, q, key=lambda x: x[:c])
        ub = bisect.bisect_right(suffixes, q, key=lambda x: x[:c])
        out.append((0xFFFFFFFF, 0xFFFFFFFF) if lb == n else (lb, (ub - 1) & 0xFFFFFFFF))
    return out


# -- record retrieval: a row model and texts with planted hits ---------------------------------------------------------------
# Hits -> distinct rows runs as six pieces of code (csrc/rows_device.hpp: lane, wave, two workgroup tables, the fused single query;
# csrc/records.hpp: the host path).  The model below is plain NumPy over a suffix array that the caller has checked; the texts
# below put exact hit counts, row counts and suffix-array orders of the hits where those pieces switch and where their tables fill.
MISS = 0xFFFFFFFF


def range_hits(ranges):
    """hit counts of query ranges (structured first / second) under every miss encoding: {UINT32_MAX, UINT32_MAX} (lb = n) and
    second = first - 1, which wraps to UINT32_MAX when first = 0"""
    f = np.asarray(ranges["first"]).astype(np.int64)
    s = np.asarray(ranges["second"]).astype(np.int64)
    return np.where(f == MISS, 0, (s - f + 1) & 0xFFFFFFFF)


def rows_reference(sa, starts, ranges, k, with_first_hits=False):
    """The rows of every range: the hits sa[first .. second] (none for a miss), each mapped to the last row whose start is <= the
    hit (upper bound: of several zero-length rows at one offset the last wins), each row kept once in order of its first hit along
    the range (suffix-array order), the first min(k, num_rows) of them.  -> (counts int64[R], list of int64 row arrays) and, with
    with_first_hits, the index along its range of every kept row's first hit.  Vectorised: sort by (range, row, hit index), mark
    the first hit of every pair, order those by (range, hit index)."""
    sa = np.asarray(sa)
    starts = np.asarray(starts, dtype=np.uint64)
    cnt = range_hits(ranges)
    R = cnt.size
    first = np.where(cnt > 0, np.asarray(ranges["first"]).astype(np.int64), 0)
    total = int(cnt.sum())
    qid = np.repeat(np.arange(R, dtype=np.int64), cnt)
    hidx = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    pos = sa[np.repeat(first, cnt) + hidx].astype(np.uint64)
    row = np.searchsorted(starts, pos, side="right").astype(np.int64) - 1
    o = np.lexsort((hidx, row, qid))
    new = np.ones(total, dtype=bool)
    new[1:] = (qid[o][1:] != qid[o][:-1]) | (row[o][1:] != row[o][:-1])
    keep = np.sort(o[new])                       # (range, hit index) order: the order the hits were laid out in
    kq, kr, kh = qid[keep], row[keep], hidx[keep]
    nrows = np.bincount(kq, minlength=R)
    take = np.minimum(nrows, min(int(k), int(starts.size)))
    rank = np.arange(kq.size) - np.repeat(np.cumsum(nrows) - nrows, nrows)
    sel = rank < take[kq]
    cut = np.cumsum(take)[:-1]
    rows = np.split(kr[sel], cut)
    if with_first_hits:
        return take, rows, np.split(kh[sel], cut)
    return take, rows


def marker(i):
    """the i-th marker token: Q and three uppercase letters.  The texts below hold lowercase letters, newlines and markers, each
    marker followed by a lowercase tag, so a marker occurs exactly where it was planted.  QZZZ is never planted (a miss)."""
    assert 0 <= i < 26 ** 3 - 1
    return b"Q" + bytes(65 + (i // 26 ** e) % 26 for e in (2, 1, 0))


def _tag(j, width):
    return bytes(97 + (j // 26 ** e) % 26 for e in range(width - 1, -1, -1))


def planted_text(num_rows, plants, seed, start_marker=None, start_rows=()):
    """Rows of random lowercase filler, each ending in a newline, with planted marker tokens.
    plants: [(marker, rows)]: rows[j] is the row of the marker's j-th hit in suffix-array order -- the j-th token is followed by a
    fixed-width lowercase tag that sorts as j, so the tags decide the hits' order whatever their order in the text.
    start_rows: rows that begin with start_marker (the j-th of them tagged j): hits on a row's first byte; b"\\n" + start_marker hits
    the last byte (the newline) of the row before.  -> (text uint8, row starts uint64: one row per line)"""
    rng = np.random.default_rng(seed)
    width = 4
    per_row = [[] for _ in range(num_rows)]
    for m, rows in plants:
        assert len(rows) < 26 ** width
        for j, r in enumerate(rows):
            per_row[int(r)].append(m + _tag(j, width))
    head = {}
    for j, r in enumerate(start_rows):
        assert int(r) not in head
        head[int(r)] = start_marker + _tag(j, width)
    letters = rng.integers(97, 123, 16 * num_rows + 64, dtype=np.uint8).tobytes()
    fl = rng.integers(3, 11, 2 * num_rows + sum(len(t) for t in per_row) + 8)
    li = fi = 0
    out = []
    for r in range(num_rows):
        toks = per_row[r]
        if len(toks) > 1:
            toks = [toks[i] for i in rng.permutation(len(toks))]   # text order within a row is not the hits' order
        parts = [head.get(r, b"")]
        for t in toks + [b""]:
            m = int(fl[fi]); fi += 1
            if li + m > len(letters):
                li = 0
            parts.append(letters[li:li + m]); li += m
            parts.append(t)
        parts.append(b"\n")
        out.append(b"".join(parts))
    lens = np.fromiter((len(x) for x in out), dtype=np.int64, count=num_rows)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    return np.frombuffer(b"".join(out), dtype=np.uint8), starts


def _fresh(rng, pool, count):
    """count distinct rows out of pool, in a random order"""
    return rng.choice(np.asarray(pool), size=count, replace=False)


def _few_then_new(rng, num_rows, first, few, new):
    """first hits spread over exactly `few` rows (each of them at least once, the first `few` hits being those rows), then
    `new` hits in rows of their own: where a walk stops, or a wave hands a range on, is set by `first` and `few`"""
    rows = _fresh(rng, np.arange(num_rows), few + new)
    head = np.concatenate([rows[:few], rng.choice(rows[:few], first - few)]) if first > few else rows[:few][:first]
    return np.concatenate([head, rows[few:]])


def rows_main_case(num_rows=70_001, seed=5):
    """The main text of the record-retrieval sweep: num_rows rows (not a multiple of 256: the coarse table's last block is
    partial) and one marker per cell.  -> (text, starts, {name: pattern}, {name: (hits, distinct rows)} as planted).
    Names: h<count> (random rows, about half of them repeated), u<count> (every hit a row of its own), rep<...> (short ranges
    with a row repeated after another one: the lanes' seen-test), fill64 / fill1536 / fill4096 (the k-th new row lands on the
    last hit of a chunk: a wave / workgroup table holds k - 1 + chunk rows), mid64 (the 64th new row inside a wave chunk),
    handoff<count> (the first 4096 hits in 10 rows, the rest in rows of their own), one<count> (every hit in one row), ends
    (row 0 and the last row)."""
    rng = np.random.default_rng(seed)
    N = num_rows
    allrows = np.arange(N)
    spec = {}
    for h in (1, 2, 3, 4, 5, 6, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 20_000):
        d = max(1, (h + 1) // 2)
        rows = _fresh(rng, allrows, d)
        spec["h%d" % h] = rng.permutation(np.concatenate([rows, rng.choice(rows, h - d)]))
    for h in (2, 3, 4, 5, 6, 63, 64, 65, 127, 128, 255, 256, 257, 320, 1535, 1536, 1537, 1792, 4095, 4096, 4097, 4352, 20_000):
        spec["u%d" % h] = _fresh(rng, allrows, h)
    a, b, c = (int(x) for x in _fresh(rng, allrows, 3))
    spec["rep_aba"] = np.array([a, b, a])
    spec["rep_abab"] = np.array([a, b, a, b])
    spec["rep_abca"] = np.array([a, b, c, a])
    spec["rep_aaba"] = np.array([a, a, b, a])
    spec["rep_abcab"] = np.array([a, b, c, a, b])
    spec["fill64"] = _few_then_new(rng, N, 64, 63, 100)
    spec["mid64"] = _few_then_new(rng, N, 64, 30, 80)
    spec["fill1536"] = _few_then_new(rng, N, 256, 255, 1600)
    spec["fill4096"] = _few_then_new(rng, N, 256, 255, 4200)
    spec["mid1536"] = _few_then_new(rng, N, 1280, 1223, 600)
    for h in (4096, 4097, 4100, 5000):
        spec["handoff%d" % h] = _few_then_new(rng, N, 4096, 10, h - 4096)
    spec["one300"] = np.full(300, int(rng.integers(0, N)))
    spec["one20000"] = np.full(20_000, int(rng.integers(0, N)))
    spec["ends"] = np.array([N - 1, 0, N - 1, 0, int(rng.integers(1, N - 1)), N - 1])
    plants = [(marker(i), rows) for i, rows in enumerate(spec.values())]
    head_rows = np.concatenate([[0, N - 1], _fresh(rng, np.arange(1, N - 1), 3000)])
    rng.shuffle(head_rows)
    S = marker(len(plants))
    text, starts = planted_text(N, plants, seed, S, head_rows)
    pats = {name: m for name, (m, _) in zip(spec, plants)}
    pats.update({"head": S, "nl_head": b"\n" + S, "nl": b"\n", "miss_end": b"~", "miss_mid": b"QZZZ",
                 "miss_wrap": b"\x01"})
    claim = {name: (len(r), len(set(int(x) for x in r))) for name, r in spec.items()}
    claim["head"] = (len(head_rows), len(head_rows))
    claim["nl_head"] = (len(head_rows) - 1, len(head_rows) - 1)   # (row 0 has no newline before it)
    claim["nl"] = (N, N)
    for m in ("miss_end", "miss_mid", "miss_wrap"):
        claim[m] = (0, 0)
    return text, starts, pats, claim


def rows_small_case(num_rows, seed=9):
    """A small text of num_rows rows (1, 255, 256, 257, 512, 513: around the coarse table's 256-row blocks) -> as rows_main_case.
    every: one hit per row; twice: two per row; last: 70 hits in the last row and one in row 0; few: 5 hits over the ends."""
    rng = np.random.default_rng(seed + num_rows)
    N = num_rows
    spec = {"every": rng.permutation(N), "twice": rng.permutation(np.repeat(np.arange(N), 2)),
            "last": np.concatenate([np.full(70, N - 1), [0]]), "few": np.array([N - 1, 0, N - 1, N // 2, 0])}
    spec["last"] = rng.permutation(spec["last"])
    plants = [(marker(i), rows) for i, rows in enumerate(spec.values())]
    S = marker(len(plants))
    head_rows = rng.permutation(N)
    text, starts = planted_text(N, plants, seed, S, head_rows)
    pats = {name: m for name, (m, _) in zip(spec, plants)}
    pats.update({"head": S, "nl_head": b"\n" + S, "nl": b"\n", "miss_end": b"~", "miss_mid": b"QZZZ", "miss_wrap": b"\x01"})
    claim = {name: (len(r), len(set(int(x) for x in r))) for name, r in spec.items()}
    claim.update({"head": (N, N), "nl_head": (N - 1, N - 1), "nl": (N, N)})
    for m in ("miss_end", "miss_mid", "miss_wrap"):
        claim[m] = (0, 0)
    return text, starts, pats, claim


def zero_length_rows(starts, seed=3):
    """The same text under a row table with zero-length rows (equal consecutive starts, which sa_hip_index_set_rows accepts): row 0
    is empty, and empty rows sit at the coarse table's block edges and at random places."""
    rng = np.random.default_rng(seed)
    n = starts.size
    dup = {0, n - 1} | {i for i in (254, 255, 256, 511, 512) if i < n} | set(int(x) for x in rng.integers(0, n, max(n // 200, 3)))
    extra = starts[sorted(dup)]
    return np.sort(np.concatenate([starts, extra, starts[:1]])).astype(np.uint64)


# -- planted repeats with an exact tie model (the 64-bit-index build's flags pass and rounds) -----------------------------------
# csrc/big_build.hpp sorts the suffixes by a key of k symbols and hands every record whose key is not unique to the doubling
# rounds; BigStats.tied_after_sort is their number.  A random text with one planted copy of R symbols has exactly
# 2 (R - k + 1) of them (as long as the random part has no k-symbol tie of its own): the model below counts them, whatever they are.
def plant_copy(t, A, B, R, symbols):
    """t[B:B+R] = t[A:A+R] in place, then the guard symbols: the copies must not match one symbol further to the left or to
    the right (A >= 1, A + R <= B, B + R < n).  The left guard is t[B-1], or t[A-1] where B - 1 is the first copy's last symbol."""
    n = int(t.size)
    symbols = np.asarray(symbols)
    assert 1 <= A and A + R <= B and B + R < n and R >= 1 and symbols.size >= 2

    def other(v):
        return symbols[(int(np.flatnonzero(symbols == v)[0]) + 1) % symbols.size]
    t[B:B + R] = t[A:A + R]
    if t[B - 1] == t[A - 1]:
        g = B - 1 if B - 1 >= A + R else A - 1
        t[g] = other(t[g])
    if t[B + R] == t[A + R]:
        t[B + R] = other(t[B + R])
    assert t[A - 1] != t[B - 1] and t[A + R] != t[B + R] and np.array_equal(t[A:A + R], t[B:B + R])


def planted_repeat(n, R, A, B, seed, symbols):
    """Random text of n symbols over `symbols` (an array of values; its dtype is the text's) with t[B:B+R] = t[A:A+R] and guard
    symbols (plant_copy): the copies match on exactly R symbols, so LCP(suffix A+i, suffix B+i) = R - i for every i in [0, R)."""
    symbols = np.asarray(symbols)
    t = symbols[np.random.default_rng(seed).integers(0, symbols.size, n)]
    plant_copy(t, A, B, R, symbols)
    return np.ascontiguousarray(t)


def tied_after_keys(T, k):
    """The number of positions of T whose k-symbol key (symbols T[p .. p+k), 'nothing' past the end, which differs from every
    symbol) is shared with another position: the model of tied_after_sort.  Plain NumPy: the keys, np.unique with counts."""
    T = np.asarray(T)
    n = int(T.size)
    k = int(k)
    assert k >= 1
    if n == 0:
        return 0
    u, inv = np.unique(T, return_inverse=True)
    code = np.concatenate([inv.reshape(-1).astype(np.uint64) + np.uint64(1), np.zeros(k - 1, np.uint64)])   # 0 past the end
    b = max(1, int(u.size).bit_length())
    if k * b <= 64:
        keys = np.zeros(n, np.uint64)
        for c in range(k):
            keys = (keys << np.uint64(b)) | code[c:c + n]
        counts = np.unique(keys, return_counts=True)[1]
    else:
        counts = np.unique(np.lib.stride_tricks.sliding_window_view(code, k), axis=0, return_counts=True)[1]
    return int(counts[counts > 1].sum())


def pair_samples(R, k, count, seed, extra=()):
    """offsets i into a planted copy: 0, R - k (the last pair that shares a key), R - 1, `extra` and `count` random ones"""
    rng = np.random.default_rng(seed)
    return sorted({0, R - k, R - 1} | set(int(x) for x in extra) | set(int(x) for x in rng.integers(0, R, count)))


def check_planted_pairs(sa_d, A, B, R, k, a_first, samples):
    """Independent of the build's own checker: the slot j of suffix A+i is looked up in the device array (a torch tensor) by
    comparing every entry with A+i, in pieces of 2^30 entries; exactly one slot holds it, and for i <= R - k the slot next to it
    holds suffix B+i -- j + 1 where the first copy sorts first (a_first), j - 1 otherwise, the same side for every i.
    -> {i: j}"""
    import torch
    n = int(sa_d.numel())
    piece = 1 << 30
    slots = {}
    for i in samples:
        found = []
        for lo in range(0, n, piece):
            hit = torch.nonzero(sa_d[lo:lo + piece] == A + i).reshape(-1)
            found += [lo + int(x) for x in hit.cpu().numpy()]
        assert len(found) == 1, (i, found)
        j = found[0]
        if i <= R - k:
            jb = j + 1 if a_first else j - 1
            assert 0 <= jb < n and int(sa_d[jb].item()) == B + i, (i, j, a_first, sa_d[max(j - 1, 0):j + 2].cpu().numpy(), B + i)
        slots[i] = j
    return slots


def plant_copy_device(t, A, B, R, k):
    """plant_copy on a torch device tensor of integer symbols in [0, k): t[B:B+R] = t[A:A+R], guards to v + 1 mod k.
    -> a_first: the suffixes of the first copy sort before their partners (t[A+R] < t[B+R])"""
    n = int(t.numel())
    assert 1 <= A and A + R < B and B + R < n and k >= 2
    t[B:B + R] = t[A:A + R].clone()
    if int(t[B - 1].item()) == int(t[A - 1].item()):
        t[B - 1] = (int(t[B - 1].item()) + 1) % k
    if int(t[B + R].item()) == int(t[A + R].item()):
        t[B + R] = (int(t[B + R].item()) + 1) % k
    return int(t[A + R].item()) < int(t[B + R].item())
