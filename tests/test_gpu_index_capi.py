"""GPU: the byte-index handle of the C ABI (sa_hip_index_*, sa_hip_query_*) at the edges of its host code: the refusals that
differ on a device, the pinned block of the per-call paths (patterns of 0, 1, 48 959 and 48 960 bytes; small batches of 447 / 448 /
449 patterns and of 16 384 / 16 385 pattern bytes), every build entry point, and the handle's lifecycle.  One text of 65 536 bytes
over 4 symbols, built once; expected ranges from the oracle, expected rows from the row model of cases.py."""
import ctypes as C

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

EINVAL = -1
N = 65536
MAXU = 0xFFFFFFFF
MAX_HITS = 4096
LONG = 48961   # one byte more than the pinned block holds
SMALL_Q, SMALL_BYTES = 448, 16384


class Ctx:
    def __init__(self, gpu, oracle):
        import torch
        self.capi, self.L, self.oracle, self.torch = gpu, gpu.lib(), oracle, torch
        self.text = np.random.default_rng(5).integers(97, 101, N).astype(np.uint8)
        self.sa = oracle.sais(self.text).astype(np.uint32)
        self.starts = np.arange(0, N, 1000, dtype=np.uint64)           # 66 rows
        self.built, self.empty = gpu.DeviceIndex(N, 0), gpu.DeviceIndex(N, 0)
        self.built.build(self.text)
        self.built.set_rows(self.starts)
        self.empty.set_rows(self.starts)                                # a row table, no index
        self.big = np.full(N + 1, 97, np.uint8)                         # one byte more than the handles hold
        self.dev = torch.zeros(8 * (N + 1), dtype=torch.uint8, device="cuda:0")   # device memory for every pointer below
        torch.cuda.synchronize()
        self.d = self.dev.data_ptr()
        self.out = np.zeros(2 * (N + 1), np.uint64)
        self.off = np.array([0, 1], np.uint64)
        self.pair, self.u32, self.u64 = gpu.PairU32(), C.c_uint32(0), C.c_uint64(0)
        self.lay, self.bufs = gpu.ReplicaLayout(), gpu.ReplicaBuffers()
        self.lay_big, self.lay_width, self.lay_dir = gpu.ReplicaLayout(), gpu.ReplicaLayout(), gpu.ReplicaLayout()
        self.lay_big.n = N + 1
        self.lay_width.key_bytes = 3
        self.lay_dir.key_bytes, self.lay_dir.dir_bits = 8, 7
        self.long = np.full(LONG, 97, np.uint8).tobytes()

    def close(self):
        self.built.close()
        self.empty.close()


@pytest.fixture(scope="module")
def ctx(gpu, oracle):
    c = Ctx(gpu, oracle)
    yield c
    c.close()


def p(a):
    return a.ctypes.data


# (id, call(c) -> return code, expected code, expected text)
ROWS = [
    # ---- no index
    ("replica_layout/no index", lambda c: c.L.sa_hip_index_replica_layout(c.empty._h, C.byref(c.lay)), EINVAL, "sa_hip_index_replica_layout: no index"),
    ("replica_buffers/no index", lambda c: c.L.sa_hip_index_replica_buffers(c.empty._h, C.byref(c.bufs)), EINVAL, "sa_hip_index_replica_buffers: no index"),
    ("widen_device/no index", lambda c: c.L.sa_hip_index_widen_device(c.empty._h, c.d), EINVAL, "sa_hip_index_widen_device: no index"),
    ("query_batch_device/no index", lambda c: c.L.sa_hip_query_batch_device(c.empty._h, c.d, c.d, 1, c.d), EINVAL, "sa_hip_query_batch_device: no index"),
    ("query_batch_device_fixed/no index", lambda c: c.L.sa_hip_query_batch_device_fixed(c.empty._h, c.d, 1, 1, c.d), EINVAL, "sa_hip_query_batch_device_fixed: no index"),
    ("query_batch/no index", lambda c: c.L.sa_hip_query_batch(c.empty._h, p(c.text), p(c.off), 1, p(c.out)), EINVAL, "sa_hip_query_batch: no index"),
    ("query_hits/no index", lambda c: c.L.sa_hip_index_query_hits(c.empty._h, b"a", 1, 4, C.byref(c.pair), p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_query_hits: no index"),
    ("query_rows/no index", lambda c: c.L.sa_hip_index_query_rows(c.empty._h, b"a", 1, 1, p(c.out), C.byref(c.u32), None), EINVAL, "sa_hip_index_query_rows: no index"),
    ("query_rows_batch/no index", lambda c: c.L.sa_hip_index_query_rows_batch(c.empty._h, p(c.text), p(c.off), 1, 1, p(c.out), p(c.out), None), EINVAL, "sa_hip_index_query_rows_batch: no index"),
    ("rows_for_range/no index", lambda c: c.L.sa_hip_index_rows_for_range(c.empty._h, c.pair, 1, p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_rows_for_range: no index"),
    ("verify/no index", lambda c: c.L.sa_hip_index_verify(c.empty._h, C.byref(c.u64)), EINVAL, "sa_hip_index_verify: no index"),
    ("get_sa_u32/no index", lambda c: c.L.sa_hip_index_get_sa_u32(c.empty._h, p(c.out)), EINVAL, "sa_hip_index_get_sa_u32: no index"),
    ("get_sa_i64/no index", lambda c: c.L.sa_hip_index_get_sa_i64(c.empty._h, p(c.out)), EINVAL, "sa_hip_index_get_sa_i64: no index"),
    ("get_text/no index", lambda c: c.L.sa_hip_index_get_text(c.empty._h, p(c.out)), EINVAL, "sa_hip_index_get_text: no index"),
    ("get_sa_range/no index", lambda c: c.L.sa_hip_index_get_sa_range(c.empty._h, 0, 1, p(c.out)), EINVAL, "sa_hip_index_get_sa_range: no index"),
    ("deep_keys/no index", lambda c: c.L.sa_hip_index_deep_keys(c.empty._h, 2), EINVAL, "sa_hip_index_deep_keys: no index"),
    ("both/widen_device: no index before NULL output", lambda c: c.L.sa_hip_index_widen_device(c.empty._h, None), EINVAL, "sa_hip_index_widen_device: no index"),
    ("both/query_batch_device: no index before NULL argument", lambda c: c.L.sa_hip_query_batch_device(c.empty._h, None, None, 1, None), EINVAL, "sa_hip_query_batch_device: no index"),
    ("both/query_rows: long pattern before no index", lambda c: c.L.sa_hip_index_query_rows(c.empty._h, c.long, LONG, 1, p(c.out), C.byref(c.u32), None), EINVAL, "sa_hip_index_query_rows: pattern longer than 47 KB"),
    # ---- capacity exceeded
    ("build/capacity", lambda c: c.L.sa_hip_index_build(c.built._h, p(c.big), N + 1, 0), EINVAL, "sa_hip_index_build: n exceeds the index capacity"),
    ("build_device/capacity", lambda c: c.L.sa_hip_index_build_device(c.built._h, c.d, N + 1, 0), EINVAL, "sa_hip_index_build_device: n exceeds the index capacity"),
    ("build_device64/capacity", lambda c: c.L.sa_hip_index_build_device64(c.built._h, c.d, N + 1, 0, c.d), EINVAL, "sa_hip_index_build_device64: n exceeds the index capacity"),
    ("load/capacity", lambda c: c.L.sa_hip_index_load(c.built._h, p(c.big), p(c.out), N + 1, 0), EINVAL, "sa_hip_index_load: n exceeds the index capacity"),
    ("load_device/capacity", lambda c: c.L.sa_hip_index_load_device(c.built._h, c.d, c.d, N + 1, 0), EINVAL, "sa_hip_index_load: n exceeds the index capacity"),
    ("replica_reserve/capacity", lambda c: c.L.sa_hip_index_replica_reserve(c.built._h, C.byref(c.lay_big), C.byref(c.bufs)), EINVAL, "sa_hip_index_replica_reserve: n exceeds the index capacity"),
    # ---- NULL device pointers
    ("widen_device/null output", lambda c: c.L.sa_hip_index_widen_device(c.built._h, None), EINVAL, "sa_hip_index_widen_device: NULL output"),
    ("query_batch_device/null patterns", lambda c: c.L.sa_hip_query_batch_device(c.built._h, None, c.d, 1, c.d), EINVAL, "sa_hip_query_batch_device: NULL argument"),
    ("query_batch_device/null offsets", lambda c: c.L.sa_hip_query_batch_device(c.built._h, c.d, None, 1, c.d), EINVAL, "sa_hip_query_batch_device: NULL argument"),
    ("query_batch_device/null output", lambda c: c.L.sa_hip_query_batch_device(c.built._h, c.d, c.d, 1, None), EINVAL, "sa_hip_query_batch_device: NULL argument"),
    ("query_batch_device_fixed/null patterns", lambda c: c.L.sa_hip_query_batch_device_fixed(c.built._h, None, 1, 1, c.d), EINVAL, "sa_hip_query_batch_device_fixed: NULL argument"),
    ("query_batch_device_fixed/null output", lambda c: c.L.sa_hip_query_batch_device_fixed(c.built._h, c.d, 1, 1, None), EINVAL, "sa_hip_query_batch_device_fixed: NULL argument"),
    ("build_device/null text", lambda c: c.L.sa_hip_index_build_device(c.empty._h, None, 4, 0), EINVAL, "sa_hip_index_build_device: NULL argument"),
    ("build_device64/null output", lambda c: c.L.sa_hip_index_build_device64(c.empty._h, c.d, 4, 0, None), EINVAL, "sa_hip_index_build_device64: NULL argument"),
    ("load_device/null sa", lambda c: c.L.sa_hip_index_load_device(c.empty._h, c.d, None, 4, 0), EINVAL, "sa_hip_index_load_device: NULL argument"),
    # ---- replicas
    ("replica_commit/nothing reserved", lambda c: c.L.sa_hip_index_replica_commit(c.built._h), EINVAL, "sa_hip_index_replica_commit: nothing reserved"),
    ("replica_reserve/bad key width", lambda c: c.L.sa_hip_index_replica_reserve(c.empty._h, C.byref(c.lay_width), C.byref(c.bufs)), EINVAL, "sa_hip_index_replica_reserve: bad key width"),
    ("replica_reserve/inconsistent layout", lambda c: c.L.sa_hip_index_replica_reserve(c.empty._h, C.byref(c.lay_dir), C.byref(c.bufs)), EINVAL, "sa_hip_index_replica_reserve: inconsistent layout"),
    # ---- the pinned block's bound
    ("query_hits/long pattern", lambda c: c.L.sa_hip_index_query_hits(c.built._h, c.long, LONG, 4, C.byref(c.pair), p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_query_hits: pattern longer than 47 KB"),
    ("query_rows/long pattern", lambda c: c.L.sa_hip_index_query_rows(c.built._h, c.long, LONG, 1, p(c.out), C.byref(c.u32), None), EINVAL, "sa_hip_index_query_rows: pattern longer than 47 KB"),
]


@pytest.mark.parametrize("name,call,code,text", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(ctx, name, call, code, text):
    with pytest.raises(ctx.capi.SaHipError) as e:
        ctx.capi.check(call(ctx))
    assert e.value.code == code
    assert ctx.L.sa_hip_last_error().decode() == text


def test_refusals_left_the_index_alone(ctx):
    assert ctx.built.verify() == 0 and np.array_equal(ctx.built.sa_u32(), ctx.sa)
    assert ctx.L.sa_hip_query_batch_device(ctx.built._h, None, None, 0, None) == 0   # Q == 0 before the arguments


def test_one_pattern_at_the_block_edges(ctx):
    """query_hits and query_rows with patterns of 0, 1, 48 959 and 48 960 bytes cut from the text."""
    idx, text, sa = ctx.built, ctx.text, ctx.sa
    pats = [b"", bytes(text[7:8]), bytes(text[100:100 + LONG - 2]), bytes(text[16000:16000 + LONG - 1]), bytes(text[N - (LONG - 1):])]
    exp = ctx.oracle.query_batch(text, sa, MAXU, pats)
    cnt = cases.range_hits(exp)
    assert cnt[0] == N and cnt[1] > MAX_HITS and (cnt[2:] >= 1).all()
    for k in (1, 5, ctx.starts.size, 1000):
        _, model = cases.rows_reference(sa, ctx.starts, exp, k)
        for i, pat in enumerate(pats):
            (first, second), hits = idx.query_hits(pat)
            assert (first, second) == (exp["first"][i], exp["second"][i]), (len(pat), k)
            assert np.array_equal(hits, sa[first:first + min(int(cnt[i]), MAX_HITS)]), len(pat)
            (_, _), few = idx.query_hits(pat, 3)
            assert np.array_equal(few, hits[:3])
            rows, rng = idx.query_rows(pat, k)
            assert rng == (exp["first"][i], exp["second"][i]) and np.array_equal(rows, model[i].astype(np.uint64)), (len(pat), k)


def small_batch(text, q, total, seed):
    """q patterns cut from the text whose lengths add up to `total`"""
    rng = np.random.default_rng(seed)
    lens = np.full(q, total // q, dtype=np.int64)
    lens[-1] += total - int(lens.sum())
    at = rng.integers(0, text.size - int(lens.max()), q)
    return [bytes(text[a:a + n]) for a, n in zip(at.tolist(), lens.tolist())]


@pytest.mark.parametrize("q,total", [(SMALL_Q - 1, 1341), (SMALL_Q, 1344), (SMALL_Q + 1, 1347), (SMALL_Q, SMALL_BYTES), (SMALL_Q, SMALL_BYTES + 1),
                                     (1, SMALL_BYTES), (1, SMALL_BYTES + 1)])
def test_query_batch_at_the_small_batch_edges(ctx, q, total):
    pats = small_batch(ctx.text, q, total, q + total)
    assert len(pats) == q and sum(len(x) for x in pats) == total
    got = ctx.built.query_batch(pats)
    assert np.array_equal(got, ctx.oracle.query_batch(ctx.text, ctx.sa, MAXU, pats))
    assert (cases.range_hits(got) >= 1).all()


def test_every_build_entry_point(ctx):
    """build, build_device from the handle's own text pointer and from another buffer, build_device64 and its widened copy."""
    torch = ctx.torch
    text, sa = ctx.text, ctx.sa
    other = torch.from_numpy(text).to("cuda:0")
    wide = torch.full((N,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with ctx.capi.DeviceIndex(N, 0) as idx:
        idx.build(text)
        assert np.array_equal(idx.sa_u32(), sa) and np.array_equal(idx.text(), text)
        idx.build_device(idx.text_dev, N)                  # the text already in place: no copy
        assert np.array_equal(idx.sa_u32(), sa) and idx.verify() == 0
        idx.build(text[::-1].copy())
        assert not np.array_equal(idx.sa_u32(), sa)
        idx.build_device(other.data_ptr(), N)
        assert np.array_equal(idx.sa_u32(), sa) and np.array_equal(idx.text(), text)
        idx.build(text[::-1].copy())
        idx.build_device64(other.data_ptr(), N, wide.data_ptr())
        idx.sync()
        assert np.array_equal(idx.sa_u32(), sa) and np.array_equal(wide.cpu().numpy(), sa.astype(np.int64))
        wide.fill_(-1)
        torch.cuda.synchronize()
        idx.widen_device(wide.data_ptr())
        idx.sync()
        assert np.array_equal(wide.cpu().numpy(), sa.astype(np.int64)) and np.array_equal(idx.sa_i64(), sa.astype(np.int64))
        assert np.array_equal(idx.sa_range(N - 5, 5), sa[N - 5:])
        half = N // 2                                      # a shorter text into the same handle
        idx.build_device(other.data_ptr(), half)
        assert np.array_equal(idx.sa_u32(), ctx.oracle.sais(text[:half]).astype(np.uint32))


def test_create_and_destroy_handles(ctx):
    """8 handles in a row, each using every buffer a handle owns: rows, deep keys, an LCP and a BWT call."""
    text = ctx.text[:8192]
    pats = [bytes(text[i:i + 6]) for i in range(0, 600, 3)]
    for _ in range(8):
        with ctx.capi.DeviceIndex(text.size, 0) as idx:
            idx.build(text)
            idx.set_rows(ctx.starts[:8])
            idx.deep_keys(2)
            idx.query_hits(pats[0])
            idx.query_rows(pats[1], 4)
            idx.query_batch(pats)
            idx.query_batch(pats * 3)
            idx.query_rows_batch(pats, 4)
            idx.sa_i64()
            idx.lcp()
            idx.bwt()
            idx.query_stats()
            idx.build_stats()
