"""Texts beyond 2^32 - 2 bytes: the 64-bit-index build (csrc/big_build.hpp; the counterpart of libsais64's true 64-bit
path, libsais64.c:6684 -> libsais64_main).  At small sizes the same code is compared bit for bit with the oracle (the
entry point accepts any n); at n = 4.4e9 -- past every 32-bit index -- through the size-independent properties: the
on-device sufcheck with 64-bit indices and text spot checks."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _give_back_hbm():
    """the large tests leave tens of GB in torch's caching allocator: hand it back so that later tests see the free HBM"""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _build_on_device(gpu, t):
    import torch
    n = int(t.size)
    text_d = torch.from_numpy(np.ascontiguousarray(t)).to("cuda:0") if n else torch.empty(16, dtype=torch.uint8, device="cuda:0")
    sa_d = torch.empty(max(n, 1), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = gpu.libsais64_device(text_d.data_ptr(), sa_d.data_ptr(), n)
    bad = gpu.sufcheck64_device(text_d.data_ptr(), sa_d.data_ptr(), n)
    return sa_d[:n].cpu().numpy(), st, bad


def test_big_path_matches_oracle_at_small_sizes(gpu, oracle):
    """Every small text of the suite (classic, adversarial: all-a, Fibonacci, block repeats, two symbols, 256 symbols, NUL and
    high-bit bytes) + word text + a text with a long run: the 64-bit-index build gives the oracle's suffix array, its own
    sufcheck agrees, the doubling rounds run where the text has long repeats."""
    from suffixarray_amd import synth
    st = cases.small_texts()
    texts = dict(st)
    texts["words_2m"] = synth.d2_words(2_000_000)
    texts["d1_3m"] = synth.d1_uniform27(3_000_000)
    run = synth.d2_words(1_500_000).copy()
    run[400_000:470_000] = ord("q")
    texts["run"] = run
    rng = np.random.default_rng(5)
    texts["blocks"] = np.tile(rng.integers(97, 101, 50_000, dtype=np.uint8), 9)
    texts["one"] = np.frombuffer(b"x", np.uint8)
    texts["two_equal"] = np.frombuffer(b"aa", np.uint8)
    seen_rounds = 0
    for name, t in texts.items():
        if t.size == 0:
            continue
        sa, stats, bad = _build_on_device(gpu, t)
        assert bad == 0, (name, stats)
        assert np.array_equal(sa, oracle.sais(t).astype(np.int64)), (name, stats)
        seen_rounds += stats["rounds"]
    assert seen_rounds > 10   # all-a / Fibonacci / block repeats went through prefix doubling


def test_sufcheck64_sees_a_wrong_array(gpu, oracle):
    import torch
    from suffixarray_amd import synth
    t = synth.d2_words(300_000)
    sa = oracle.sais(t).astype(np.int64)
    text_d = torch.from_numpy(t).to("cuda:0")
    for kind in ("swap", "dup", "range"):
        bad = sa.copy()
        if kind == "swap":
            bad[1000], bad[1001] = bad[1001], bad[1000]
        elif kind == "dup":
            bad[5] = bad[6]
        else:
            bad[77] = t.size + 3
        sa_d = torch.from_numpy(bad).to("cuda:0")
        torch.cuda.synchronize()
        assert gpu.sufcheck64_device(text_d.data_ptr(), sa_d.data_ptr(), t.size) > 0, kind
    sa_d = torch.from_numpy(sa).to("cuda:0")
    torch.cuda.synchronize()
    assert gpu.sufcheck64_device(text_d.data_ptr(), sa_d.data_ptr(), t.size) == 0


def test_beyond_uint32_4p4e9_verified(gpu):
    """n = 4.4e9 > 2^32 - 2: D1 text generated on the host, built on the device with 64-bit suffix indices (41 bytes of HBM
    per character: 180 GB), checked by the on-device sufcheck (the suffix array is unique: verified <=> bit-exact) and by
    comparing sampled neighbours in the text on the host; entries beyond 2^32 occur."""
    import torch
    from suffixarray_amd import synth
    n = 4_400_000_000
    free, _ = torch.cuda.mem_get_info(0)
    if free < 46 * n:
        pytest.skip("needs %d GB of free HBM" % (46 * n >> 30))
    t = synth.d1_uniform27(n)
    text_d = torch.from_numpy(t).to("cuda:0")
    sa_d = torch.empty(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = gpu.libsais64_device(text_d.data_ptr(), sa_d.data_ptr(), n)
    assert st["initial_chars"] == 12 and st["sort_passes"] >= 8, st
    assert gpu.sufcheck64_device(text_d.data_ptr(), sa_d.data_ptr(), n) == 0, st
    assert int(sa_d.max().item()) == n - 1 and int((sa_d > 0xFFFFFFFF).sum().item()) == n - (1 << 32)
    rng = np.random.default_rng(1)
    js = torch.from_numpy(rng.integers(1, n, 2000)).to("cuda:0")
    a = sa_d[js - 1].cpu().numpy(); b = sa_d[js].cpu().numpy()
    for x, y in zip(a, b):
        assert bytes(t[int(x):int(x) + 64]) < bytes(t[int(y):int(y) + 64]) or int(x) + 64 > n
    print("4.4e9 characters, 64-bit indices: %.1f ms on the device (%s)" % (st["total_ms"], st))
    # the drop-in call (host text in, host int64 array out): the same array -- every 100 003rd entry and both ends compared
    # (the device array was verified above and a suffix array is unique), the byte histogram beside it
    import time
    t0 = time.time()
    sa_h, freq = gpu.libsais64(t, want_freq=True)
    print("sa_hip_libsais64(T, SA, 4.4e9) host to host: %.1f s" % (time.time() - t0))
    assert sa_h.dtype == np.int64 and sa_h.size == n
    assert np.array_equal(sa_h[::100_003], sa_d[::100_003].cpu().numpy())
    assert np.array_equal(sa_h[:4096], sa_d[:4096].cpu().numpy()) and np.array_equal(sa_h[-4096:], sa_d[-4096:].cpu().numpy())
    assert int(freq.sum()) == n and int((freq > 0).sum()) == 27


def _suffix_less(t, x, y):
    """suffix x < suffix y on the host, whatever their common prefix (compared in pieces of 1 MiB; the one that ends first is smaller)"""
    n = int(t.size)
    step = 1 << 20
    while True:
        a, b = t[x:x + step], t[y:y + step]
        m = min(a.size, b.size)
        ne = np.flatnonzero(a[:m] != b[:m])
        if ne.size:
            return bool(a[ne[0]] < b[ne[0]])
        if m < step:
            return x > y            # one of them ended: the shorter suffix (the larger index) sorts first
        x += step
        y += step


def test_beyond_uint32_4p4e9_planted_repeat(gpu):
    """The D1 text of test_beyond_uint32_4p4e9_verified with a copy of R = 2e7 characters planted from A = 1e9 + 7 to
    B = 2^32 + 12345 (cases.plant_copy: the copies match on exactly R characters).  The initial sort (12 characters) leaves
    2 (R - 11) records tied, in pairs (A+i, B+i) whose suffix indices lie on both sides of the 32-bit line and whose SA slots
    and ranks are spread over all of [0, n) -- D1's buckets are uniform -- so about 2.4 % of them sit at slots >= 2^32; the
    rounds need log2(2e7 / 12) = 20.7 doublings.  Checked: tied_after_sort within the planted count + 2000 (accidental
    12-character ties of the random text: about n^2 / (2 * 27^12) = 65 pairs), rounds >= 20, the on-device sufcheck, sampled
    neighbours compared on the host to the first difference, the planted pairs looked up directly in the array (adjacent slots,
    one side for all, the side the characters after the copies decide), PLCP and LCP of the pairs exactly R - i (the first large
    values these kernels produce beyond 2^32), and the sufcheck's sensitivity to one swapped pair at slots >= 2^32.
    HBM: 46 n for the build and its check + 90 bytes per tied record."""
    import torch
    n = 4_400_000_000
    R, A, B = 20_000_000, 1_000_000_007, (1 << 32) + 12345
    free, _ = torch.cuda.mem_get_info(0)
    if free < 46 * n + 90 * 2 * R:
        pytest.skip("needs %d GB of free HBM" % ((46 * n + 180 * R) >> 30))
    from suffixarray_amd import synth
    from test_big_ties_cpu import D1_SYMBOLS
    t = synth.d1_uniform27(n)
    cases.plant_copy(t, A, B, R, D1_SYMBOLS)
    a_first = bool(t[A + R] < t[B + R])
    assert a_first == _suffix_less(t, A + R, B + R)
    text_d = torch.from_numpy(t).to("cuda:0")
    sa_d = torch.empty(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = gpu.libsais64_device(text_d.data_ptr(), sa_d.data_ptr(), n)
    print("4.4e9 characters with a planted repeat of 2e7: %.1f ms on the device (%s)" % (st["total_ms"], st))
    assert st["initial_chars"] == 12 and st["sort_passes"] >= 8, st
    planted = 2 * (R - 12 + 1)
    assert planted <= st["tied_after_sort"] <= planted + 2000, st
    assert st["rounds"] >= 20 and st["tied_total"] >= st["tied_after_sort"], st
    assert gpu.sufcheck64_device(text_d.data_ptr(), sa_d.data_ptr(), n) == 0, st
    assert int(sa_d.max().item()) == n - 1 and int((sa_d > 0xFFFFFFFF).sum().item()) == n - (1 << 32)
    rng = np.random.default_rng(1)
    js = torch.from_numpy(rng.integers(1, n, 2000)).to("cuda:0")
    a = sa_d[js - 1].cpu().numpy(); b = sa_d[js].cpu().numpy()
    for x, y in zip(a, b):
        assert _suffix_less(t, int(x), int(y)), (x, y)
    # the planted pairs, looked up in the array: random offsets, both ends, and offsets whose suffixes begin with "zz" (the
    # last 1 / 729 of the slots: beyond 2^32)
    seg = t[A:A + R - 12]
    zz = np.flatnonzero((seg[:-1] == 122) & (seg[1:] == 122))[:8]
    assert zz.size == 8
    samples = cases.pair_samples(R, 12, 200, 2, extra=zz)
    slots = cases.check_planted_pairs(sa_d, A, B, R, 12, a_first, samples)
    paired = [i for i in samples if i <= R - 12]
    assert len(paired) >= 200
    high = [i for i in paired if min(slots[i], slots[i] + (1 if a_first else -1)) > 0xFFFFFFFF]
    assert high, "no sampled pair at slots beyond 2^32"
    # sufcheck up there: one swapped pair is seen, the restored array is clean
    j0 = slots[high[0]]
    j1 = j0 + (1 if a_first else -1)
    v0, v1 = int(sa_d[j0].item()), int(sa_d[j1].item())
    sa_d[j0], sa_d[j1] = v1, v0
    torch.cuda.synchronize()
    assert gpu.sufcheck64_device(text_d.data_ptr(), sa_d.data_ptr(), n) > 0
    sa_d[j0], sa_d[j1] = v0, v1
    torch.cuda.synchronize()
    assert gpu.sufcheck64_device(text_d.data_ptr(), sa_d.data_ptr(), n) == 0
    # PLCP at the later-sorted member of every sampled pair and LCP at its slot: exactly R - i
    torch.cuda.empty_cache()
    out_d = torch.empty(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ps = gpu.plcp64_device(text_d.data_ptr(), sa_d.data_ptr(), out_d.data_ptr(), n)
    print("plcp64_device, planted repeat:", ps)
    later = torch.tensor([(B if a_first else A) + i for i in paired], dtype=torch.int64, device="cuda:0")
    want = np.array([R - i for i in paired], np.int64)
    assert np.array_equal(out_d[later].cpu().numpy(), want)
    ls = gpu.lcp64_device(text_d.data_ptr(), sa_d.data_ptr(), out_d.data_ptr(), n)
    print("lcp64_device, planted repeat:", ls)
    at = torch.tensor([max(slots[i], slots[i] + (1 if a_first else -1)) for i in paired], dtype=torch.int64, device="cuda:0")
    assert np.array_equal(out_d[at].cpu().numpy(), want)
