"""The 64-bit-index build (csrc/big_build.hpp) where its initial sort leaves ties: the flags pass (16 consecutive positions
per thread, 8192 per workgroup, aggregates scanned across waves, workgroups and tiles) and the doubling rounds on lists, for
bytes (sa_hip_libsais64_device) and for integer texts on route B (csrc/int_build.hpp, dense and raw codes).

Texts with one planted copy of R symbols (cases.planted_repeat) have an exact number of tied records after the sort, which a
NumPy model counts (cases.tied_after_keys): R puts that number on both sides of one and of two 8192-record tiles, on two
records, and on a few hundred thousand (many tiles, the last one partial).  Every build is compared whole with the oracle /
the reference AND its tied_after_sort with the model, exactly: a flags pass that loses or invents a record at a thread, wave or
tile edge fails here even where the rounds would still repair the order.  Then one int64 text of raw codes beyond 2^32 symbols
whose planted pairs have suffix indices on both sides of the 32-bit line."""
import numpy as np
import pytest

import cases
from test_big_ties_cpu import D1_SYMBOLS, SWEEP_R
from test_int_cpu import rank_remap, ref_long

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _give_back_hbm():
    """the large test leaves tens of GB in torch's caching allocator: hand it back so that later tests see the free HBM"""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()


# ~300 values spread up to 2^40 (int64 form) and up to 2^30 (int32 form): above the rank table's cap, so the codes are raw
SPREAD40 = np.random.default_rng(40).permutation(np.arange(300, dtype=np.int64) * 3_600_000_007 + 11)
SPREAD30 = np.random.default_rng(30).permutation(np.arange(300, dtype=np.int64) * 3_500_003 + 7).astype(np.int32)
assert int(SPREAD40.max()) < 2 ** 40 and int(SPREAD30.max()) < 2 ** 30

KEY_SYMBOLS = (None, "1", "5")   # SA_HIP_INT_KEY_SYMBOLS: the default (12 symbols of 5 bits), every record tied, in between


def placements(n, R):
    """(name, A, B): both copies inside the text, the first copy in the first 16 positions (the first thread of the keygen
    and, for the suffixes that sort there, of the flags pass), the second copy ending on the text's last symbol but one
    (B + R = n - 1: the rounds read ranks past the end, key2 = 0)"""
    return [("mid", n // 3, 2 * n // 3), ("head", 3, n // 2), ("tail", n // 5, n - 1 - R)]


def sweep_cases():
    out = []
    for R, n in SWEEP_R:
        for name, A, B in placements(n, R):
            if n > 1_000_000 and name != "tail":
                continue
            if n > 1_000_000:
                A = 7                                    # the large case: head and tail at once
            out.append(pytest.param(n, R, A, B, id="M%d_%s" % (2 * (R - 12 + 1), name)))
    return out


def _env(monkeypatch, key_symbols=None, bytes_route=False):
    for k in ("SA_HIP_INT_BYTES", "SA_HIP_INT_COMPACT", "SA_HIP_INT_KEY_SYMBOLS"):
        monkeypatch.delenv(k, raising=False)
    if not bytes_route:
        monkeypatch.setenv("SA_HIP_INT_BYTES", "0")      # route B (BigBuilder::build_with) whatever the alphabet
    if key_symbols:
        monkeypatch.setenv("SA_HIP_INT_KEY_SYMBOLS", key_symbols)


def build_bytes(gpu, t):
    import torch
    n = int(t.size)
    text_d = torch.from_numpy(np.ascontiguousarray(t).copy()).to("cuda:0")
    sa_d = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = gpu.libsais64_device(text_d.data_ptr(), sa_d.data_ptr(), n)
    bad = gpu.sufcheck64_device(text_d.data_ptr(), sa_d.data_ptr(), n)
    return sa_d.cpu().numpy(), st, bad


def build_ints(gpu, t, dtype, k):
    """the device form of the width: -> (suffix array, stats, sufcheck violations or None for the int32 form)"""
    import torch
    n = int(t.size)
    t_d = torch.from_numpy(np.ascontiguousarray(t.astype(dtype))).to("cuda:0")
    torch.cuda.synchronize()
    if dtype == np.int32:
        sa_d = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        st = gpu.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), n, k)
        return sa_d.cpu().numpy(), st, None
    sa_d = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = gpu.libsais64_long_device(t_d.data_ptr(), sa_d.data_ptr(), n, k)
    bad = gpu.sufcheck_long_device(t_d.data_ptr(), sa_d.data_ptr(), n)
    return sa_d.cpu().numpy(), st, bad


def check_bytes(gpu, t, want, model, tag):
    """the byte build of t: the expected array, no sufcheck violation, tied_after_sort == the model at the build's own key length"""
    sa, st, bad = build_bytes(gpu, t)
    m = model(st["initial_chars"])
    print(tag, "bytes: tied_after_sort %d model %d rounds %d tied_total %d" % (st["tied_after_sort"], m, st["rounds"], st["tied_total"]))
    assert np.array_equal(sa, want), (tag, st, int(np.flatnonzero(sa != want)[0]))
    assert bad == 0, (tag, st)
    assert st["tied_after_sort"] == m, (tag, st, m)
    assert st["tied_total"] >= st["tied_after_sort"], (tag, st)
    assert st["rounds"] >= 1 if m else st["rounds"] == 0, (tag, st)
    return st


def check_ints(gpu, monkeypatch, t, k, want, model, tag, key_symbols=KEY_SYMBOLS, widths=(np.int32, np.int64), compacted=1):
    for dtype in widths:
        for ks in key_symbols:
            _env(monkeypatch, ks)
            sa, st, bad = build_ints(gpu, t, dtype, k)
            m = model(st["symbols_per_key"])
            print(tag, np.dtype(dtype).name, "key symbols", ks, "->", st["symbols_per_key"], ": tied_after_sort %d model %d rounds %d"
                  % (st["tied_after_sort"], m, st["rounds"]))
            assert st["plan"] == 1 and st["compacted"] == compacted, (tag, dtype, ks, st)
            if ks:
                assert st["symbols_per_key"] == min(int(ks), 64 // st["bits_per_symbol"]), (tag, dtype, ks, st)
            assert np.array_equal(sa, want.astype(dtype)), (tag, dtype, ks, st, int(np.flatnonzero(sa != want)[0]))
            assert bad in (None, 0), (tag, dtype, ks, st)
            assert st["tied_after_sort"] == m, (tag, dtype, ks, st, m)
            assert st["tied_total"] >= st["tied_after_sort"] and (st["rounds"] >= 1 if m else st["rounds"] == 0), (tag, dtype, ks, st)


def _model_of(t):
    memo = {}

    def model(k):
        if k not in memo:
            memo[k] = cases.tied_after_keys(t, k)
        return memo[k]
    return model


@pytest.mark.parametrize("n,R,A,B", sweep_cases())
def test_planted_repeat_sweep(gpu, oracle, monkeypatch, n, R, A, B):
    """bytes, and the same text widened to int32 / int64 on route B with 12, 1 and 5 symbols per key"""
    t = cases.planted_repeat(n, R, A, B, 3000 + R, D1_SYMBOLS)
    model = _model_of(t)
    assert model(12) == 2 * (R - 12 + 1)                # the tied count this case was sized for
    want = oracle.sais(t).astype(np.int64)
    st = check_bytes(gpu, t, want, model, "R=%d A=%d B=%d" % (R, A, B))
    assert st["initial_chars"] == 12, st
    assert st["rounds"] >= int(np.ceil(np.log2(R / 12.0))) if R > 12 else st["rounds"] == 1, st   # doublings from 12 to beyond R
    check_ints(gpu, monkeypatch, t, 256, want, model, "R=%d A=%d B=%d" % (R, A, B))


@pytest.mark.parametrize("n,R,A,B", sweep_cases())
def test_planted_repeat_sweep_raw_codes(gpu, ref, monkeypatch, n, R, A, B):
    """the same planted structure over 300 values spread up to 2^40 (int64) / 2^30 (int32): no rank table, the codes are the
    values + 1, one or two symbols per key, so nearly every record goes to the rounds; expected from the reference through
    the order-preserving remap"""
    for dtype, spread, k in ((np.int64, SPREAD40, 2 ** 40), (np.int32, SPREAD30, 2 ** 30)):
        t = cases.planted_repeat(n, R, A, B, 4000 + R, spread)
        r, sigma = rank_remap(t)
        assert sigma == 300
        want = ref_long(ref, r, sigma)
        check_ints(gpu, monkeypatch, t, k, want, _model_of(t), "raw R=%d A=%d B=%d" % (R, A, B), key_symbols=(None,), widths=(dtype,),
                   compacted=0)


def test_two_repeats_and_a_three_copy_repeat(gpu, oracle, monkeypatch):
    """two planted repeats of different depth (the list compaction drops the short one's records rounds before the long one's)
    and one repeat with three copies (tied groups of three: the number of groups is not half the number of records)"""
    n = 400_000
    t = cases.planted_repeat(n, 5000, 1000, 200_000, 51, D1_SYMBOLS)
    cases.plant_copy(t, 50_000, 300_000, 37, D1_SYMBOLS)
    model = _model_of(t)
    assert model(12) == 2 * (5000 - 11) + 2 * (37 - 11)
    want = oracle.sais(t).astype(np.int64)
    check_bytes(gpu, t, want, model, "two repeats")
    check_ints(gpu, monkeypatch, t, 256, want, model, "two repeats")
    # three copies at A, B, C: six guards, pairwise different to the left and to the right of the copies
    R, A, B, C = 6000, 10, 150_000, n - 1 - 6000
    t = D1_SYMBOLS[np.random.default_rng(52).integers(0, 27, n)]
    t[B:B + R] = t[A:A + R]
    t[C:C + R] = t[A:A + R]
    t[[A - 1, B - 1, C - 1]] = D1_SYMBOLS[[3, 9, 20]]
    t[[A + R, B + R, C + R]] = D1_SYMBOLS[[14, 0, 7]]
    model = _model_of(t)
    assert model(12) == 3 * (R - 11)
    want = oracle.sais(t).astype(np.int64)
    check_bytes(gpu, t, want, model, "three copies")
    check_ints(gpu, monkeypatch, t, 256, want, model, "three copies")


@pytest.mark.parametrize("n", [8191, 8192, 8193, 16 * 512 * 3 + 1])
def test_every_record_tied_at_tile_edges(gpu, oracle, monkeypatch, n):
    """all-equal and period-2 texts of one tile less one, one tile, one tile and one, three tiles and one: every record (but
    the last k - 1, whose keys run past the end) is tied after the sort -- the count is the model's, not a formula's"""
    from suffixarray_amd import synth
    for name, t in (("all_equal", synth.all_same(n)), ("period2", synth.periodic(n, 2))):
        model = _model_of(t)
        want = oracle.sais(t).astype(np.int64)
        st = check_bytes(gpu, t, want, model, "%s n=%d" % (name, n))
        assert st["tied_after_sort"] >= n - 64, st
        check_ints(gpu, monkeypatch, t, 256, want, model, "%s n=%d" % (name, n), key_symbols=(None, "1"))


def test_raw_codes_beyond_2_32_device(gpu):
    """n = 2^32 + 2^24 int64 symbols, raw codes (values up to 2^40: above the rank table's cap), one symbol per key, a planted
    copy of R = 1e7 symbols from A = 1e9 + 7 to B = 2^32 + 12345: of every tied pair one suffix index lies below 2^32 and one
    above, and about 24 doubling rounds order them.

    Two sizes differ from the first sketch of this test, both for reasons of arithmetic, not of results.  (1) With 300 distinct
    values and one symbol per key the sort would leave all n records tied; the rounds keep 17 n + 90 bytes per tied record
    (big_build.hpp), 107 n = 460 GB here, more than the card has.  The values are therefore uniform over [0, 2^40): still raw
    codes, the first key nearly unique -- about n^2 / 2^41 = 8.4e6 accidental pairs, 1.7e7 records beside the 2e7 planted
    ones, 3.3 GB of lists.  (2) B > 2^32 and B + R < n need n > 2^32 + 1e7: n = 2^32 + 2^24, not 2^32 + 2^20.
    HBM: text 8 n + SA 8 n + 32 n during the initial sort = 48 n (207 GB), 8 n more for the sufcheck."""
    import torch
    n = (1 << 32) + (1 << 24)
    K = 1 << 40
    R, A, B = 10_000_000, 1_000_000_007, (1 << 32) + 12345
    gpu.release_workspace()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(0)
    if free < 56 * n:
        pytest.skip("needs %d GB of free HBM" % (56 * n >> 30))
    g = torch.Generator(device="cuda:0").manual_seed(11)
    t = torch.randint(0, K, (n,), device="cuda:0", dtype=torch.int64, generator=g)
    a_first = cases.plant_copy_device(t, A, B, R, K)
    sa = torch.empty(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = gpu.libsais64_long_device(t.data_ptr(), sa.data_ptr(), n, K)
    print("raw codes beyond 2^32:", st)
    assert st["compacted"] == 0 and st["plan"] == 1 and st["symbols_per_key"] == 1, st
    assert st["tied_after_sort"] >= 2 * R and st["rounds"] >= 20, st
    assert st["tied_after_sort"] <= 2 * R + 40_000_000, st      # accidental single-symbol ties: 1.7e7 expected (docstring)
    assert gpu.sufcheck_long_device(t.data_ptr(), sa.data_ptr(), n) == 0, st
    slots = cases.check_planted_pairs(sa, A, B, R, 1, a_first, cases.pair_samples(R, 1, 200, 12))
    assert len(slots) >= 200
