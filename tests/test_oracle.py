"""CPU: the oracle (own restatement) against the golden vectors produced by the reference, and
against the reference itself where oracle/_ref is built."""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN
import cases


def _load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def test_golden_small_sa(oracle):
    g = _load("golden_small.npz")
    for name in g["names"]:
        t, sa = g[f"text__{name}"], g[f"sa__{name}"]
        got = oracle.sais(t)
        assert np.array_equal(got, sa), name
        assert np.array_equal(oracle.sais64(t), sa.astype(np.int64)), name
        if t.size <= 5000:
            assert np.array_equal(oracle.sa_naive(t), sa.astype(np.uint32)), name
        assert oracle.sufcheck(t, sa.astype(np.uint32)) == 0


def test_golden_readme(oracle):
    g = _load("golden_readme.npz")
    t, sa = g["text"], g["sa"]
    assert np.array_equal(oracle.sais(t), sa)
    L = int(g["max_suffix_length"][0])
    pats = [bytes(p) for p in g["patterns"]]
    got = oracle.query_batch(t, sa.astype(np.uint32), L, pats)
    assert np.array_equal(got, g["ranges"])
    # "zzz" is greater than every suffix: the reference's not-found sentinel
    assert tuple(got[3]) == (0xFFFFFFFF, 0xFFFFFFFF)


def test_golden_1mb(oracle):
    g = _load("golden_1mb.npz")
    L = int(g["max_suffix_length"][0])
    for name in g["names"]:
        t = g[f"text__{name}"]
        sa = oracle.sais(t)
        assert hashlib.sha256(sa.astype("<i4").tobytes()).hexdigest() == str(g[f"sa_sha256__{name}"][0]), name
        pats = [bytes(p) for p in g[f"patterns__{name}"]]
        got = oracle.query_batch(t, sa.astype(np.uint32), L, pats)
        assert np.array_equal(got, g[f"ranges__{name}"]), name
        # the reference's own truncated SA yields the same ranges, and so does
        # the oracle's truncated order
        assert np.array_equal(g[f"ranges__{name}"], g[f"ranges_truncated_ref__{name}"]), name
        tsa = oracle.truncated_sa(t, L)
        assert np.array_equal(oracle.query_batch(t, tsa, L, pats), g[f"ranges__{name}"]), name


def check_truncated_order(t, sa, L):
    """sa is a permutation ordered by the first L bytes (a suffix that ends sorts first), ties in text order."""
    n = t.size
    assert np.array_equal(np.sort(sa), np.arange(n, dtype=np.uint32))
    if n < 2:
        return
    L = min(L, n)
    pad = np.concatenate([t.astype(np.int16) + 1, np.zeros(L, np.int16)])
    keys = np.stack([pad[sa.astype(np.int64) + j] for j in range(L)], axis=1)
    diff = keys[1:] != keys[:-1]
    anyd = diff.any(axis=1)
    first = diff.argmax(axis=1)
    rows = np.nonzero(anyd)[0]
    assert np.all(keys[1:][rows, first[rows]] > keys[:-1][rows, first[rows]])
    assert np.all(sa[1:][~anyd] > sa[:-1][~anyd])


def test_truncated_contract(oracle):
    for name, t in cases.small_texts().items():
        if t.size > 70000:
            continue
        for L in (1, 3, 8, 32):
            check_truncated_order(t, oracle.truncated_sa(t, L), L)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _live_ref():
    """The reference itself where oracle/_ref is built; the stored outputs in golden_ref_cases.npz are checked either way."""
    from oracle.oracle import Ref
    return Ref() if Ref.available() else None


def test_oracle_vs_reference_build(oracle):
    g = _load("golden_ref_cases.npz")
    ref = _live_ref()
    names = [name for name, t in cases.small_texts().items() if t.size >= 1]
    assert names == list(g["names"])
    for name, t in cases.small_texts().items():
        if t.size < 1:
            continue
        assert _sha(t) == str(g[f"text_sha256__{name}"][0]), name   # the input the reference saw
        sa = oracle.sais(t)
        assert _sha(sa.astype("<i4")) == str(g[f"libsais_sha256__{name}"][0]), name
        assert _sha(sa.astype("<i4")) == str(g[f"libsais_omp4_sha256__{name}"][0]), name
        if t.size > 1:
            assert _sha(oracle.sais64(t).astype("<i8")) == str(g[f"libsais64_omp2_sha256__{name}"][0]), name
        if ref is not None:
            assert np.array_equal(sa, ref.libsais(t, threads=1)), name
            assert np.array_equal(sa, ref.libsais(t, threads=4)), name
            if t.size > 1:
                assert np.array_equal(oracle.sais64(t), ref.libsais64(t, threads=2)), name


def test_oracle_vs_reference_query(oracle):
    g = _load("golden_ref_cases.npz")
    ref = _live_ref()
    for sig, t, pats in cases.reference_query_cases():
        assert _sha(t) == str(g[f"query_text_sha256__{sig}"][0]), sig
        sa = oracle.sais(t).astype(np.uint32)
        got = oracle.query_batch(t, sa, 32, pats)
        exp = g[f"query_ranges__{sig}"]
        assert exp.size == len(pats) == got.size
        for q, a, e in zip(pats, got, exp):
            assert tuple(a) == tuple(e), q
        if ref is not None:
            tn = np.concatenate([t, np.zeros(64, np.uint8)])
            for q, a in zip(pats, got):
                assert tuple(a) == ref.query(tn, sa, 32, q), q


def test_query_edge_conventions(oracle):
    t = np.frombuffer(b"banana\nbandana\n", np.uint8)
    sa = oracle.sais(t).astype(np.uint32)
    n = t.size
    assert oracle.query(t, sa, 32, b"") == (0, n - 1)                   # empty pattern matches all
    assert oracle.query(t, sa, 32, b"zz") == (0xFFFFFFFF, 0xFFFFFFFF)    # greater than every suffix
    f, s = oracle.query(t, sa, 32, b"ban")
    assert s - f + 1 == 2
    f, s = oracle.query(t, sa, 32, b"bab")                               # miss: first = lb, last = lb - 1
    assert s == f - 1
    f, s = oracle.query(t, sa, 32, b"\x01")                              # smaller than every suffix
    assert (f, s) == (0, 0xFFFFFFFF)
    assert oracle.query(t, sa, 2, b"baXYZ") == oracle.query(t, sa, 32, b"ba")  # truncated to L
