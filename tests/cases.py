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
