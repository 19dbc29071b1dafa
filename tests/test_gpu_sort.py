"""GPU: the one-sweep radix sort on its own (sa_hip_sort_pairs) against numpy's stable argsort."""
import numpy as np
import pytest

import sort_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 4095, 4096, 4097, 8192, 100_000, 1_000_003])
def test_sort_pairs_matches_stable_argsort(gpu, n):
    rng = np.random.default_rng(n)
    for bits in ((0, 64), (0, 8), (24, 64), (4, 37), (60, 64)):
        keys = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
        if bits == (0, 8):
            keys &= np.uint64(0xFFFF)   # heavy duplicates: stability matters
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        lo, hi = bits
        mask = np.uint64(((1 << (hi - lo)) - 1) << lo) if hi - lo < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
        order = np.argsort(keys & mask, kind="stable")
        k, v = gpu.sort_pairs(keys, vals, lo, hi)
        assert np.array_equal(k, keys[order]), (n, bits)
        assert np.array_equal(v, vals[order]), (n, bits)


def test_sort_skewed_digits(gpu):
    n = 300_000
    keys = np.zeros(n, dtype=np.uint64)
    keys[::7] = 1 << 40
    keys[::13] = 0xFFFFFFFFFFFFFFFF
    vals = np.arange(n, dtype=np.uint32)
    order = np.argsort(keys, kind="stable")
    k, v = gpu.sort_pairs(keys, vals)
    assert np.array_equal(k, keys[order]) and np.array_equal(v, vals[order])


# -- the sweep of tests/sort_cases.py: tile, chunk and digit edges, both pass kernels --------------------------------------------
def set_block(monkeypatch, block):
    """sa_hip_sort_pairs reads the switch on every call; 512 is the default (radix_onesweep_kernel<512>)"""
    if block == 512:
        monkeypatch.delenv("SA_HIP_SORT_BLOCK", raising=False)
    else:
        monkeypatch.setenv("SA_HIP_SORT_BLOCK", str(block))


def check_sort(gpu, keys, vals, n, lo, hi, block, what, failures):
    ek, ev = sc.sort_model(keys, vals, lo, hi)
    k, v = gpu.sort_pairs(keys, vals, lo, hi)
    bad = sc.mismatch(k, ek, n, block)
    if bad:
        bad = "keys: " + bad
    elif vals is None:
        bad = None if v is None else "a keys-only sort returned values"
    else:
        bad = sc.mismatch(v, ev, n, block)
        bad = bad and "values: " + bad
    if bad:
        failures.append("%s n=%d window=(%d,%d) passes=%d block=%d %s" % (what, n, lo, hi, sc.npasses(lo, hi), block, bad))


@pytest.mark.parametrize("family", list(sc.FAMILIES))
@pytest.mark.parametrize("block", sc.BLOCKS)
def test_sort_sweep(gpu, monkeypatch, block, family):
    """Every window at the sizes up to two tiles and one record, three windows at the sizes that step the chunk geometry
    (sort_cases.sweep_cases); keys and values exactly the stable model's."""
    set_block(monkeypatch, block)
    T = sc.SORT_ITEMS * block
    failures = []
    calls = 0
    for c in sc.sweep_cases(block, family):
        keys = sc.make_keys(c.family, c.n, c.lo, c.hi, c.seed, T)
        vals = sc.make_values(c.n, c.vals, c.seed)
        check_sort(gpu, keys, vals, c.n, c.lo, c.hi, block, "%s values=%s" % (family, c.vals), failures)
        calls += 1
    assert calls >= 59   # (an odd record at index T - 1 or T needs a size that has the index)
    assert not failures, "%d of %d sorts differ:\n%s" % (len(failures), calls, "\n".join(failures[:12]))


@pytest.mark.parametrize("block", sc.BLOCKS)
def test_sort_digit_run_ends_at_a_chunk_boundary(gpu, monkeypatch, block):
    """After pass 0 the run of digit 0 ends one short of, on, or one past the first record of chunk 1 and of the last chunk in
    use: which chunk's histogram pass 1 reads for the records around it hangs on the {base chunk, threshold} word."""
    set_block(monkeypatch, block)
    failures = []
    calls = 0
    for c in sc.boundary_cases(block):
        keys = sc.boundary_keys(c.n, c.lo, c.hi, c.seed, block, c.which, c.delta)
        vals = sc.make_values(c.n, c.vals, c.seed)
        what = "chunk_boundary(%s, zeros=%d=B%+d) values=%s" % (c.which, sc.boundary_count(c.n, block, c.which, c.delta), c.delta, c.vals)
        check_sort(gpu, keys, vals, c.n, c.lo, c.hi, block, what, failures)
        calls += 1
    assert calls == 72
    assert not failures, "%d of %d sorts differ:\n%s" % (len(failures), calls, "\n".join(failures[:12]))


@pytest.mark.parametrize("block", sc.BLOCKS)
def test_sort_keys_only(gpu, monkeypatch, block):
    """values == NULL: pass 0 makes the values from the record positions, nothing is returned for them; one window per
    pass count, so the result comes back from either buffer."""
    set_block(monkeypatch, block)
    T = sc.SORT_ITEMS * block
    failures = []
    for c in sc.keys_only_cases(block):
        keys = sc.make_keys(c.family, c.n, c.lo, c.hi, c.seed, T)
        check_sort(gpu, keys, None, c.n, c.lo, c.hi, block, "keys_only", failures)
    assert not failures, "\n".join(failures)


def test_sort_histogram_workgroup_straddles_a_chunk(gpu, monkeypatch):
    """2050 tiles of 4096: radix_hist_kernel gives every workgroup two tiles, chunks are 257 tiles long, so workgroup 128
    counts the last tile of chunk 0 and the first of chunk 1 and has to flush in between."""
    block, n = sc.BIG_CASE["block"], sc.BIG_CASE["n"]
    set_block(monkeypatch, block)
    rng = np.random.default_rng(2050)
    keys = rng.integers(0, sc.ALL_ONES, n, dtype=np.uint64, endpoint=True)
    vals = np.arange(n, dtype=np.uint32)
    failures = []
    for lo, hi in sc.BIG_CASE["windows"]:
        check_sort(gpu, keys, vals, n, lo, hi, block, "uniform", failures)
    assert not failures, "\n".join(failures)


def test_sort_noops_and_refusals(gpu):
    """begin_bit == end_bit sorts nothing and returns 0; a window outside 0 <= begin_bit <= end_bit <= 64 is refused with
    SA_HIP_EINVAL, the caller's arrays as they were, sa_hip_last_error naming the call."""
    lib = gpu.lib()
    rng = np.random.default_rng(5)
    keys0 = rng.integers(0, 1 << 63, 5000, dtype=np.uint64)
    vals0 = rng.integers(0, 1 << 32, 5000, dtype=np.uint32)

    def call(lo, hi, with_vals=True):
        k, v = keys0.copy(), vals0.copy()
        rc = lib.sa_hip_sort_pairs(k.ctypes.data, v.ctypes.data if with_vals else None, k.size, lo, hi, 0)
        assert np.array_equal(k, keys0) and np.array_equal(v, vals0), (lo, hi)   # untouched either way
        return rc

    # an empty window sorts nothing
    for b in (0, 5, 63, 64):
        assert call(b, b) == 0
        assert call(b, b, with_vals=False) == 0
    k, v = gpu.sort_pairs(keys0, vals0, 17, 17)
    assert np.array_equal(k, keys0) and np.array_equal(v, vals0)
    # refused windows: a code, the arrays untouched, the message names the call
    for lo, hi in ((-1, 8), (-64, 0), (0, 66), (0, 65), (60, 66), (9, 8), (64, 0)):
        assert call(lo, hi) == -1, (lo, hi)
        assert b"sa_hip_sort_pairs" in lib.sa_hip_last_error(), (lo, hi)
        with pytest.raises(gpu.SaHipError) as e:
            gpu.sort_pairs(keys0, vals0, lo, hi)
        assert e.value.code == -1 and "sa_hip_sort_pairs" in str(e.value)
    # and a good call still works afterwards
    k, v = gpu.sort_pairs(keys0, vals0, 0, 64)
    ek, ev = sc.sort_model(keys0, vals0, 0, 64)
    assert np.array_equal(k, ek) and np.array_equal(v, ev)


# -- radix_onesweep_kernel<256> under whole builds: every `block == 512` predicate turns the narrow, narrow48, split and
#    wide-text plans off, the build's sorts all run on the 4096-record tile ------------------------------------------------------
def test_build_on_the_256_thread_kernel_small_texts(gpu, oracle, monkeypatch):
    import cases
    monkeypatch.setenv("SA_HIP_SORT_BLOCK", "256")   # Builder::init reads it when the handle is created
    texts = cases.small_texts()                      # (d1_300k and d2_300k: D1 and word text at 300 000)
    assert texts["d1_300k"].size == 300_000 and texts["d2_300k"].size == 300_000
    nmax = max(t.size for t in texts.values())
    with gpu.DeviceIndex(nmax, 0) as idx:
        for name, t in texts.items():
            idx.build(t)
            st = idx.build_stats()
            assert np.array_equal(idx.sa_u32(), oracle.sais(t).astype(np.uint32)), (name, st)
            assert st["pass_launches"][1:] == [0, 0, 0], (name, st)


def test_build_on_the_256_thread_kernel_matches_default(gpu, oracle, monkeypatch):
    from suffixarray_amd import synth
    t = synth.d1_uniform27(1 << 22)
    monkeypatch.setenv("SA_HIP_SORT_BLOCK", "256")
    with gpu.DeviceIndex(t.size, 0) as idx:
        idx.build(t)
        st = idx.build_stats()
        # the switch was read and the narrow plans stood down: only radix_onesweep_kernel<256> sorted
        assert st["pass_launches"][1:] == [0, 0, 0] and st["pass_launches"][0] > 0, st
        assert st["narrow48"] == 0 and st["narrow_k"] == 0, st
        assert idx.verify() == 0, st
        a = idx.sa_u32().copy()
    assert np.array_equal(a, oracle.sais(t).astype(np.uint32)), st
    monkeypatch.delenv("SA_HIP_SORT_BLOCK")
    with gpu.DeviceIndex(t.size, 0) as idx:          # a fresh handle without the switch: the narrow plan of the default build
        idx.build(t)
        st0 = idx.build_stats()
        assert st0["pass_launches"][1:] != [0, 0, 0], st0
        b = idx.sa_u32().copy()
    assert np.array_equal(a, b), (st, st0)
