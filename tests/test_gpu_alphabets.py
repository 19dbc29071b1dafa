"""Every alphabet code width through every build and query plan.  The build packs each byte into b = bits_for(sigma + 1) bits,
and b decides the initial key length k0, the sort (begin_bit = 64 - b * k0: <= 40 key bits -> 8-byte narrow records, 41..56
bits with b <= 8 -> 10-byte narrow48 records, otherwise 12-byte records), the directory and the second-level keys.  The narrow
plans only run from n = 2^22 on, so this sweep builds 4.5 M characters over alphabets of 1 .. 256 bytes -- every b at both
ends, the all-ones 2^b - 1 included, gap bytes between present ones -- with the default key and with forced keys on each plan
boundary, and judges the suffix arrays and the query ranges of edge patterns by the oracle (tests/cases.py: alphabet,
alphabet_text, edge_patterns)."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

N = 4_500_001
BIG_Q = 40_000                   # >= K2_AUTO_BATCH (32768): builds the second-level keys of a wide-key index on its way
SMALL_Q = 32_768                 # a batch below it does not
CASES = cases.alphabet_cases()
IDS = [c[0] for c in CASES]
COVER = {}                       # (b, plan) -> run names that took it; checked by test_plan_coverage_matrix


def _kind(variant):
    return "binary" if variant in ("lo", "ends") else "uniform"


def predicted_kmax(b, n, narrow48=True):
    """Builder::choose_initial_chars: the longest key -- 56 bits where the 10-byte-record plan is possible, else 64"""
    possible = narrow48 and b <= 8 and n >= 1 << 22
    return 56 // b if possible and 56 // b >= 6 else 64 // b


def predicted_plan(b, k0, n, narrow48=True):
    """the host predicates of Builder::build (narrow_sort_applies, narrow48_applies) restated for the default switches"""
    begin = 64 - b * k0
    if n >= 1 << 22 and 24 <= begin < 56:
        return "narrow"
    if narrow48 and b <= 8 and n >= 1 << 22 and 8 <= begin < 24 and k0 - 1 <= 64:
        return "narrow48"
    return "wide"


def observed_plan(st):
    """the 8- and 10-byte-record sorts launch segmented passes (pass kinds 2, 3); the 12-byte sort launches none"""
    seg = st["pass_launches"][2] + st["pass_launches"][3] > 0
    assert seg or not st["narrow48"], st
    return "narrow48" if st["narrow48"] else ("narrow" if seg else "wide")


def check_plan(st, sigma, b, k0, n, narrow48=True, run=""):
    assert (st["sigma"], st["bits_per_symbol"], st["initial_chars"]) == (sigma, b, k0), (run, st)
    plan = predicted_plan(b, k0, n, narrow48)
    assert observed_plan(st) == plan, (run, plan, st)
    # the top-digit pass reads the text (text_pass_applies: b <= 8); the 12-byte sort reads it in pass 0 when it has more than one
    assert st["text_top_pass"] == int(b <= 8 and (plan != "wide" or b * k0 > 8)), (run, st)
    assert st["narrow_k"] == int(plan == "narrow"), (run, st)
    COVER.setdefault((b, plan), []).append(run)
    return plan


def assert_sa(got, exp, what):
    if not np.array_equal(got, exp):
        d = np.flatnonzero(got != exp)
        pytest.fail("%s: suffix array differs in %d slots, first at %d: got %s, expected %s"
                    % (what, d.size, d[0], got[d[0]:d[0] + 4].tolist(), exp[d[0]:d[0] + 4].tolist()))


def assert_ranges(got, exp, pats, what):
    if not np.array_equal(got, exp):
        d = np.flatnonzero(got != exp)
        i = int(d[0])
        pytest.fail("%s: %d of %d ranges differ, first pattern %r (%d bytes): got %s, expected %s"
                    % (what, d.size, len(pats), pats[i][:80], len(pats[i]), tuple(got[i]), tuple(exp[i])))


def _text(sigma, variant, n=N):
    alph = cases.alphabet(sigma, variant)
    return alph, cases.alphabet_text(alph, n, _kind(variant), seed=1000 + sigma)


@pytest.mark.parametrize("cid,sigma,variant", CASES, ids=IDS)
def test_code_width_through_every_plan(gpu, oracle, monkeypatch, cid, sigma, variant):
    """The default key and forced keys on every plan boundary: the longest narrow key (40 // b characters), the shortest and
    the longest narrow48 key (40 // b + 1 and 56 // b, b <= 8), the longest 12-byte key with the narrow48 plan off (64 // b:
    63 bits for b = 9).  Each run: the stats report the alphabet and key asked for and the plan the predicates give, the
    device verifies the array, it equals the oracle's, and the edge patterns get the oracle's ranges in a small batch, in a
    batch that builds the second-level keys and in that batch again in the clustered order."""
    b = cases.code_bits(sigma)
    alph, t = _text(sigma, variant)
    ref = oracle.sais(t).astype(np.uint32)
    rng = np.random.default_rng(sigma)
    k2n = min(64 // b, 16)
    runs = [("default", 0, True), ("narrow_longest", 40 // b, True)]
    if b <= 8:
        runs += [("narrow48_shortest", 40 // b + 1, True), ("narrow48_longest", 56 // b, True)]
    runs.append(("wide_longest", 64 // b, False))
    for name, k, n48 in runs:
        run = "%s/%s" % (cid, name)
        monkeypatch.setenv("SA_HIP_NARROW48", "1" if n48 else "0")
        if k:
            monkeypatch.setenv("SA_HIP_INITIAL_CHARS", str(k))
        else:
            monkeypatch.delenv("SA_HIP_INITIAL_CHARS", raising=False)
        monkeypatch.delenv("SA_HIP_QCLUSTER_MIN", raising=False)
        with gpu.DeviceIndex(t.size, 0) as idx:
            idx.build(t)
            st = idx.build_stats()
            k0 = st["initial_chars"]
            if k:
                assert k0 == k, (run, "the forced key was capped", st)
            else:
                assert 1 <= k0 <= predicted_kmax(b, t.size, n48), (run, st)
            plan = check_plan(st, sigma, b, k0, t.size, n48, run)
            assert idx.verify() == 0, (run, st)
            assert_sa(idx.sa_u32(), ref, run)
            small = cases.edge_patterns(t, alph, k0, k2n, 0, rng)
            assert len(small) < SMALL_Q
            assert_ranges(idx.query_batch(small), oracle.query_batch(t, ref, 0xFFFFFFFF, small), small, run + " small batch")
            big = cases.big_batch(t, small, BIG_Q, rng)
            exp = oracle.query_batch(t, ref, 0xFFFFFFFF, big)
            assert_ranges(idx.query_batch(big), exp, big, run + " large batch (" + plan + ")")
            monkeypatch.setenv("SA_HIP_QCLUSTER_MIN", "4096")
            assert_ranges(idx.query_batch(big), exp, big, run + " large batch, clustered order")
            monkeypatch.delenv("SA_HIP_QCLUSTER_MIN")
    monkeypatch.delenv("SA_HIP_INITIAL_CHARS", raising=False)
    monkeypatch.delenv("SA_HIP_NARROW48", raising=False)
    # an index adopted from the text and the suffix array (keys gathered from the text, whatever plan built the array)
    with gpu.DeviceIndex(t.size, 0) as idx:
        idx.load(t, ref, 0)
        small = cases.edge_patterns(t, alph, 40 // b, k2n, 0, rng)
        assert_ranges(idx.query_batch(small), oracle.query_batch(t, ref, 0xFFFFFFFF, small), small, cid + " adopted, small batch")
        big = cases.big_batch(t, small, BIG_Q, rng)
        assert_ranges(idx.query_batch(big), oracle.query_batch(t, ref, 0xFFFFFFFF, big), big, cid + " adopted, large batch")


TRUNC = [(3, "hi"), (2, "lo"), (15, "hi"), (8, "lo"), (31, "mid"), (16, "ends"), (127, "mid"), (64, "ends"), (255, "ends"),
         (128, "lo"), (256, "ends")]


@pytest.mark.parametrize("sigma,variant", TRUNC, ids=["s%d_b%d" % (s, cases.code_bits(s)) for s, _ in TRUNC])
def test_truncated_builds_across_widths(gpu, oracle, sigma, variant):
    """b in {2, 4, 5, 7, 8, 9}, all-ones and power-of-two alphabets, L in {1, 2, k0 - 1, k0, k0 + 1, 32}: L < k0 shortens the key
    and with it can change the plan.  The suffix array keeps ties in text order (oracle.truncated_sa); the edge patterns,
    those longer than L included, get the oracle's ranges."""
    b = cases.code_bits(sigma)
    alph, t = _text(sigma, variant)
    rng = np.random.default_rng(100 + sigma)
    with gpu.DeviceIndex(t.size, 0) as idx:
        idx.build(t)
        kfull = idx.build_stats()["initial_chars"]
    for L in sorted({1, 2, kfull - 1, kfull, kfull + 1, 32} - {0}):
        run = "s%d_b%d/L%d" % (sigma, b, L)
        with gpu.DeviceIndex(t.size, 0) as idx:
            idx.build(t, L)
            st = idx.build_stats()
            k0 = min(kfull, L)
            check_plan(st, sigma, b, k0, t.size, True, run)
            tsa = oracle.truncated_sa(t, L)
            assert_sa(idx.sa_u32(), tsa, run)
            pats = cases.edge_patterns(t, alph, k0, min(64 // b, 16), L, rng)
            assert_ranges(idx.query_batch(pats), oracle.query_batch(t, tsa, L, pats), pats, run)


THRESHOLD = [(31, "mid"), (128, "lo")]


@pytest.mark.parametrize("sigma,variant", THRESHOLD, ids=["s%d_b%d" % (s, cases.code_bits(s)) for s, _ in THRESHOLD])
def test_plan_threshold(gpu, oracle, monkeypatch, sigma, variant):
    """n = 2^22 - 1, 2^22, 2^22 + 1: the narrow plans start exactly at 2^22, and below it the longest key is 64 bits, not 56
    (narrow48_possible), so the default and the capped key change too.  Default key, the longest key (override capped at
    kmax) and the longest narrow key; bit-exact arrays and the oracle's ranges on both sides."""
    b = cases.code_bits(sigma)
    alph = cases.alphabet(sigma, variant)
    full = cases.alphabet_text(alph, (1 << 22) + 1, "uniform", seed=2000 + sigma)
    rng = np.random.default_rng(7)
    seen = {}
    for n in ((1 << 22) - 1, 1 << 22, (1 << 22) + 1):
        t = np.ascontiguousarray(full[:n])
        assert np.unique(t).size == sigma
        ref = oracle.sais(t).astype(np.uint32)
        for k in (0, 99, 40 // b):
            run = "s%d_b%d/n%d/k%d" % (sigma, b, n, k)
            if k:
                monkeypatch.setenv("SA_HIP_INITIAL_CHARS", str(k))
            else:
                monkeypatch.delenv("SA_HIP_INITIAL_CHARS", raising=False)
            with gpu.DeviceIndex(n, 0) as idx:
                idx.build(t)
                st = idx.build_stats()
                k0 = st["initial_chars"]
                kmax = predicted_kmax(b, n)
                if k:
                    assert k0 == min(k, kmax), (run, st)
                else:
                    assert 1 <= k0 <= kmax, (run, st)
                seen[(n, k)] = check_plan(st, sigma, b, k0, n, True, run)
                assert idx.verify() == 0, (run, st)
                assert_sa(idx.sa_u32(), ref, run)
                pats = cases.edge_patterns(t, alph, k0, min(64 // b, 16), 0, rng)
                assert_ranges(idx.query_batch(pats), oracle.query_batch(t, ref, 0xFFFFFFFF, pats), pats, run)
    monkeypatch.delenv("SA_HIP_INITIAL_CHARS", raising=False)
    lo, at, hi = (1 << 22) - 1, 1 << 22, (1 << 22) + 1
    assert seen[(lo, 40 // b)] == "wide" and seen[(at, 40 // b)] == seen[(hi, 40 // b)] == "narrow", seen
    assert seen[(lo, 99)] == "wide" and seen[(at, 99)] == seen[(hi, 99)] == "narrow48", seen


def test_plan_coverage_matrix():
    """After the sweep above: the narrow plan ran for every b in 1..9, narrow48 for every b in 1..8, the 12-byte plan for every
    b -- a change of choose_initial_chars or of a predicate cannot quietly empty a cell."""
    ran = {b for b, _ in COVER}
    assert ran == set(range(1, 10)), "run the whole module: the matrix is filled by the sweep (%s)" % sorted(COVER)
    missing = [(b, p) for b in range(1, 10) for p in ("narrow", "narrow48", "wide") if (p != "narrow48" or b <= 8) and (b, p) not in COVER]
    for (b, p), runs in sorted(COVER.items()):
        print("b=%d %-8s %s" % (b, p, " ".join(runs)))
    assert not missing, missing


def _build_on_device(gpu, t):
    import torch
    n = int(t.size)
    text_d = torch.from_numpy(np.ascontiguousarray(t)).to("cuda:0")
    sa_d = torch.empty(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = gpu.libsais64_device(text_d.data_ptr(), sa_d.data_ptr(), n)
    bad = gpu.sufcheck64_device(text_d.data_ptr(), sa_d.data_ptr(), n)
    return sa_d.cpu().numpy(), st, bad


@pytest.mark.parametrize("cid,sigma,variant", CASES, ids=IDS)
def test_64bit_index_path_every_width(gpu, oracle, cid, sigma, variant):
    """The 64-bit-index build (csrc/big_build.hpp) has a code map of its own and keys of 64 // b characters: uniform and
    binary-like texts over every alphabet give the oracle's suffix array, and its on-device check agrees."""
    b = cases.code_bits(sigma)
    alph = cases.alphabet(sigma, variant)
    for kind in ("uniform", "binary"):
        t = cases.alphabet_text(alph, 300_000 + sigma, kind, seed=3000 + sigma)
        sa, st, bad = _build_on_device(gpu, t)
        assert (st["sigma"], st["bits_per_symbol"], st["initial_chars"]) == (sigma, b, 64 // b), (kind, st)
        assert bad == 0, (kind, st)
        assert_sa(sa, oracle.sais(t).astype(np.int64), "%s/%s" % (cid, kind))
