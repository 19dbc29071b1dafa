"""CPU: what the byte-index handle (sa_hip_index_*, sa_hip_query_*) refuses, and in which words.  One row per (entry point,
condition): the return code and the exact text of sa_hip_last_error.  Runs on the opt-in host path (SA_HIP_ALLOW_HOST=1, no HIP
device), over a 64-byte text.  Which refusal wins when two apply is part of the interface and differs between entry points: the
rows marked "both" pin that order.  The texts are those of csrc/sa_capi.hip and csrc/capi_dropins.hpp."""
import ctypes as C

import numpy as np
import pytest

EINVAL, EHIP = -1, -3
HOST = "the host path (no HIP device) has no device buffers"
N = 64
LONG = 48961   # one byte more than the pinned block of the per-call paths holds


class Ctx:
    """built: a handle with an index over TEXT; rows: the same with a row table {0, 32}; empty: a handle without an index"""

    def __init__(self, capi):
        self.capi, self.L = capi, capi.lib()
        self.text = (np.arange(N, dtype=np.uint8) % 4 + 97)
        self.sa = np.zeros(N + 1, np.uint32)
        self.built, self.rows, self.empty = (capi.DeviceIndex(N, 0) for _ in range(3))
        self.built.build(self.text)
        self.rows.build(self.text)
        self.rows.set_rows([0, 32])
        self.out = np.zeros(4 * N + 64, np.uint64)         # room for every output below
        self.off = np.array([0, 1], np.uint64)
        self.long = np.full(LONG, 97, np.uint8)
        self.pair, self.u32, self.u64 = capi.PairU32(), C.c_uint32(0), C.c_uint64(0)
        self.lay, self.bufs = capi.ReplicaLayout(), capi.ReplicaBuffers()
        self.bad_lay = capi.ReplicaLayout()
        self.bad_lay.key_bytes = 3

    def close(self):
        for h in (self.built, self.rows, self.empty):
            h.close()


@pytest.fixture(scope="module")
def ctx(capi):
    import os
    if capi.lib().sa_hip_device_count() >= 1:
        pytest.skip("a HIP device is present: the host path is never taken")
    old = os.environ.get("SA_HIP_ALLOW_HOST")
    os.environ["SA_HIP_ALLOW_HOST"] = "1"
    c = Ctx(capi)
    yield c
    c.close()
    if old is None:
        del os.environ["SA_HIP_ALLOW_HOST"]
    else:
        os.environ["SA_HIP_ALLOW_HOST"] = old


def p(a):
    return a.ctypes.data


def rg(c, first, second):
    r = c.capi.PairU32()
    r.first, r.second = first, second
    return r


# (id, call(c) -> return code, expected code, expected text)
ROWS = [
    # ---- NULL handle
    ("build/null", lambda c: c.L.sa_hip_index_build(None, p(c.text), N, 0), EINVAL, "sa_hip_index_build: NULL argument"),
    ("build_device/null", lambda c: c.L.sa_hip_index_build_device(None, p(c.text), N, 0), EINVAL, "sa_hip_index_build_device: NULL argument"),
    ("build_device64/null", lambda c: c.L.sa_hip_index_build_device64(None, p(c.text), N, 0, p(c.out)), EINVAL, "sa_hip_index_build_device64: NULL argument"),
    ("load/null", lambda c: c.L.sa_hip_index_load(None, p(c.text), p(c.sa), N, 0), EINVAL, "sa_hip_index_load: NULL argument"),
    ("load_device/null", lambda c: c.L.sa_hip_index_load_device(None, p(c.text), p(c.sa), N, 0), EINVAL, "sa_hip_index_load_device: NULL argument"),
    ("replica_layout/null", lambda c: c.L.sa_hip_index_replica_layout(None, C.byref(c.lay)), EINVAL, "sa_hip_index_replica_layout: NULL argument"),
    ("replica_buffers/null", lambda c: c.L.sa_hip_index_replica_buffers(None, C.byref(c.bufs)), EINVAL, "sa_hip_index_replica_buffers: NULL argument"),
    ("replica_reserve/null", lambda c: c.L.sa_hip_index_replica_reserve(None, C.byref(c.lay), C.byref(c.bufs)), EINVAL, "sa_hip_index_replica_reserve: NULL argument"),
    ("replica_commit/null", lambda c: c.L.sa_hip_index_replica_commit(None), EINVAL, "sa_hip_index_replica_commit: NULL index"),
    ("deep_keys/null", lambda c: c.L.sa_hip_index_deep_keys(None, 1), EINVAL, "sa_hip_index_deep_keys: invalid arguments"),
    ("sync/null", lambda c: c.L.sa_hip_index_sync(None), EINVAL, "sa_hip_index_sync: NULL index"),
    ("verify/null", lambda c: c.L.sa_hip_index_verify(None, C.byref(c.u64)), EINVAL, "sa_hip_index_verify: NULL argument"),
    ("get_sa_u32/null", lambda c: c.L.sa_hip_index_get_sa_u32(None, p(c.out)), EINVAL, "sa_hip_index_get_sa_u32: NULL index"),
    ("get_sa_i64/null", lambda c: c.L.sa_hip_index_get_sa_i64(None, p(c.out)), EINVAL, "sa_hip_index_get_sa_i64: NULL index"),
    ("widen_device/null", lambda c: c.L.sa_hip_index_widen_device(None, p(c.out)), EINVAL, "sa_hip_index_widen_device: NULL index"),
    ("get_sa_range/null", lambda c: c.L.sa_hip_index_get_sa_range(None, 0, 0, p(c.out)), EINVAL, "sa_hip_index_get_sa_range: NULL index"),
    ("get_freq/null", lambda c: c.L.sa_hip_index_get_freq(None, p(c.out)), EINVAL, "sa_hip_index_get_freq: NULL argument"),
    ("get_text/null", lambda c: c.L.sa_hip_index_get_text(None, p(c.out)), EINVAL, "sa_hip_index_get_text: NULL index"),
    ("query_batch/null", lambda c: c.L.sa_hip_query_batch(None, p(c.text), p(c.off), 1, p(c.out)), EINVAL, "sa_hip_query_batch: NULL index"),
    ("query_batch_device/null", lambda c: c.L.sa_hip_query_batch_device(None, p(c.text), p(c.off), 1, p(c.out)), EINVAL, "sa_hip_query_batch_device: NULL index"),
    ("query_batch_device_fixed/null", lambda c: c.L.sa_hip_query_batch_device_fixed(None, p(c.text), 1, 1, p(c.out)), EINVAL, "sa_hip_query_batch_device_fixed: NULL index"),
    ("query_hits/null", lambda c: c.L.sa_hip_index_query_hits(None, b"a", 1, 4, C.byref(c.pair), p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_query_hits: NULL index"),
    ("build_stats/null", lambda c: c.L.sa_hip_index_build_stats(None, C.byref(c.capi.BuildStats())), EINVAL, "sa_hip_index_build_stats: NULL argument"),
    ("query_stats/null", lambda c: c.L.sa_hip_index_query_stats(None, C.byref(c.capi.QueryStats())), EINVAL, "sa_hip_index_query_stats: NULL argument"),
    ("set_rows/null", lambda c: c.L.sa_hip_index_set_rows(None, None, 0), EINVAL, "sa_hip_index_set_rows: NULL argument"),
    ("query_rows/null", lambda c: c.L.sa_hip_index_query_rows(None, b"a", 1, 1, p(c.out), C.byref(c.u32), None), EINVAL, "sa_hip_index_query_rows: NULL argument"),
    ("query_rows_batch/null", lambda c: c.L.sa_hip_index_query_rows_batch(None, p(c.text), p(c.off), 1, 1, p(c.out), p(c.out), None), EINVAL, "sa_hip_index_query_rows_batch: NULL argument"),
    ("query_rows_batch/null, Q == 0", lambda c: c.L.sa_hip_index_query_rows_batch(None, None, None, 0, 0, None, None, None), EINVAL, "sa_hip_index_query_rows_batch: NULL argument"),
    ("rows_for_range/null", lambda c: c.L.sa_hip_index_rows_for_range(None, rg(c, 0, 0), 1, p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_rows_for_range: NULL argument"),
    ("plcp_device/null", lambda c: c.L.sa_hip_index_plcp_device(None, p(c.out), None), EINVAL, "sa_hip_index_plcp_device: NULL index"),
    ("lcp_device/null", lambda c: c.L.sa_hip_index_lcp_device(None, p(c.out), None), EINVAL, "sa_hip_index_lcp_device: NULL index"),
    ("bwt_device/null", lambda c: c.L.sa_hip_index_bwt_device(None, p(c.out), 0, None, C.byref(C.c_int64()), None), EINVAL, "sa_hip_index_bwt_device: NULL index"),
    # ---- no index yet
    ("verify/no index", lambda c: c.L.sa_hip_index_verify(c.empty._h, C.byref(c.u64)), EINVAL, "sa_hip_index_verify: no index"),
    ("get_sa_u32/no index", lambda c: c.L.sa_hip_index_get_sa_u32(c.empty._h, p(c.out)), EINVAL, "sa_hip_index_get_sa_u32: no index"),
    ("get_sa_i64/no index", lambda c: c.L.sa_hip_index_get_sa_i64(c.empty._h, p(c.out)), EINVAL, "sa_hip_index_get_sa_i64: no index"),
    ("get_text/no index", lambda c: c.L.sa_hip_index_get_text(c.empty._h, p(c.out)), EINVAL, "sa_hip_index_get_text: no index"),
    ("get_sa_range/no index", lambda c: c.L.sa_hip_index_get_sa_range(c.empty._h, 0, 0, p(c.out)), EINVAL, "sa_hip_index_get_sa_range: no index"),
    ("query_batch/no index", lambda c: c.L.sa_hip_query_batch(c.empty._h, p(c.text), p(c.off), 1, p(c.out)), EINVAL, "sa_hip_query_batch: no index"),
    ("query_hits/no index", lambda c: c.L.sa_hip_index_query_hits(c.empty._h, b"a", 1, 4, C.byref(c.pair), p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_query_hits: no index"),
    ("query_rows/no index, k == 0", lambda c: c.L.sa_hip_index_query_rows(c.empty._h, b"a", 1, 0, None, C.byref(c.u32), None), EINVAL, "sa_hip_index_query_hits: no index"),
    ("query_rows_batch/no index", lambda c: c.L.sa_hip_index_query_rows_batch(c.empty._h, p(c.text), p(c.off), 1, 1, p(c.out), p(c.out), None), EINVAL, "sa_hip_index_query_rows_batch: no index"),
    ("rows_for_range/no index", lambda c: c.L.sa_hip_index_rows_for_range(c.empty._h, rg(c, 0, 0), 1, p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_rows_for_range: no index"),
    # ---- device forms on the host path
    ("build_device/host", lambda c: c.L.sa_hip_index_build_device(c.built._h, p(c.text), N, 0), EHIP, "sa_hip_index_build_device: " + HOST),
    ("build_device64/host", lambda c: c.L.sa_hip_index_build_device64(c.built._h, p(c.text), N, 0, p(c.out)), EHIP, "sa_hip_index_build_device64: " + HOST),
    ("load_device/host", lambda c: c.L.sa_hip_index_load_device(c.built._h, p(c.text), p(c.sa), N, 0), EHIP, "sa_hip_index_load_device: " + HOST),
    ("replica_layout/host", lambda c: c.L.sa_hip_index_replica_layout(c.built._h, C.byref(c.lay)), EHIP, "sa_hip_index_replica_layout: " + HOST),
    ("replica_buffers/host", lambda c: c.L.sa_hip_index_replica_buffers(c.built._h, C.byref(c.bufs)), EHIP, "sa_hip_index_replica_buffers: " + HOST),
    ("replica_reserve/host", lambda c: c.L.sa_hip_index_replica_reserve(c.built._h, C.byref(c.lay), C.byref(c.bufs)), EHIP, "sa_hip_index_replica_reserve: " + HOST),
    ("replica_commit/host", lambda c: c.L.sa_hip_index_replica_commit(c.built._h), EHIP, "sa_hip_index_replica_commit: " + HOST),
    ("widen_device/host", lambda c: c.L.sa_hip_index_widen_device(c.built._h, p(c.out)), EHIP, "sa_hip_index_widen_device: " + HOST),
    ("query_batch_device/host", lambda c: c.L.sa_hip_query_batch_device(c.built._h, p(c.text), p(c.off), 1, p(c.out)), EHIP, "sa_hip_query_batch_device: " + HOST),
    ("query_batch_device_fixed/host", lambda c: c.L.sa_hip_query_batch_device_fixed(c.built._h, p(c.text), 1, 1, p(c.out)), EHIP, "sa_hip_query_batch_device_fixed: " + HOST),
    ("plcp_device/host", lambda c: c.L.sa_hip_index_plcp_device(c.built._h, p(c.out), None), EINVAL, "sa_hip_index_plcp_device: " + HOST),
    ("lcp_device/host", lambda c: c.L.sa_hip_index_lcp_device(c.built._h, p(c.out), None), EINVAL, "sa_hip_index_lcp_device: " + HOST),
    ("bwt_device/host", lambda c: c.L.sa_hip_index_bwt_device(c.built._h, p(c.out), 0, None, C.byref(C.c_int64()), None), EINVAL, "sa_hip_index_bwt_device: " + HOST),
    # ---- NULL inputs and outputs with n > 0
    ("build/null text", lambda c: c.L.sa_hip_index_build(c.built._h, None, N, 0), EINVAL, "sa_hip_index_build: NULL argument"),
    ("load/null sa", lambda c: c.L.sa_hip_index_load(c.built._h, p(c.text), None, N, 0), EINVAL, "sa_hip_index_load: NULL argument"),
    ("verify/null output", lambda c: c.L.sa_hip_index_verify(c.built._h, None), EINVAL, "sa_hip_index_verify: NULL argument"),
    ("get_sa_u32/null output", lambda c: c.L.sa_hip_index_get_sa_u32(c.built._h, None), EINVAL, "sa_hip_index_get_sa_u32: NULL output"),
    ("get_sa_i64/null output", lambda c: c.L.sa_hip_index_get_sa_i64(c.built._h, None), EINVAL, "sa_hip_index_get_sa_i64: NULL output"),
    ("get_text/null output", lambda c: c.L.sa_hip_index_get_text(c.built._h, None), EINVAL, "sa_hip_index_get_text: NULL output"),
    ("get_sa_range/null output", lambda c: c.L.sa_hip_index_get_sa_range(c.built._h, 0, 1, None), EINVAL, "sa_hip_index_get_sa_range: NULL output"),
    ("get_freq/null output", lambda c: c.L.sa_hip_index_get_freq(c.built._h, None), EINVAL, "sa_hip_index_get_freq: NULL argument"),
    ("build_stats/null output", lambda c: c.L.sa_hip_index_build_stats(c.built._h, None), EINVAL, "sa_hip_index_build_stats: NULL argument"),
    ("query_stats/null output", lambda c: c.L.sa_hip_index_query_stats(c.built._h, None), EINVAL, "sa_hip_index_query_stats: NULL argument"),
    ("query_batch/null offsets", lambda c: c.L.sa_hip_query_batch(c.built._h, p(c.text), None, 1, p(c.out)), EINVAL, "sa_hip_query_batch: NULL argument"),
    ("query_batch/null output", lambda c: c.L.sa_hip_query_batch(c.built._h, p(c.text), p(c.off), 1, None), EINVAL, "sa_hip_query_batch: NULL argument"),
    ("query_batch/null patterns", lambda c: c.L.sa_hip_query_batch(c.built._h, None, p(c.off), 1, p(c.out)), EINVAL, "sa_hip_query_batch: NULL patterns"),
    ("query_hits/null range", lambda c: c.L.sa_hip_index_query_hits(c.built._h, b"a", 1, 4, None, p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_query_hits: NULL argument"),
    ("query_hits/null hits", lambda c: c.L.sa_hip_index_query_hits(c.built._h, b"a", 1, 4, C.byref(c.pair), None, C.byref(c.u32)), EINVAL, "sa_hip_index_query_hits: NULL argument"),
    ("query_hits/null pattern", lambda c: c.L.sa_hip_index_query_hits(c.built._h, None, 1, 4, C.byref(c.pair), p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_query_hits: NULL argument"),
    ("query_rows/null rows", lambda c: c.L.sa_hip_index_query_rows(c.rows._h, b"a", 1, 1, None, C.byref(c.u32), None), EINVAL, "sa_hip_index_query_rows: NULL argument"),
    ("query_rows/null count", lambda c: c.L.sa_hip_index_query_rows(c.rows._h, b"a", 1, 1, p(c.out), None, None), EINVAL, "sa_hip_index_query_rows: NULL argument"),
    ("query_rows_batch/null rows", lambda c: c.L.sa_hip_index_query_rows_batch(c.rows._h, p(c.text), p(c.off), 1, 1, None, p(c.out), None), EINVAL, "sa_hip_index_query_rows_batch: NULL argument"),
    ("query_rows_batch/null counts", lambda c: c.L.sa_hip_index_query_rows_batch(c.rows._h, p(c.text), p(c.off), 1, 1, p(c.out), None, None), EINVAL, "sa_hip_index_query_rows_batch: NULL argument"),
    ("query_rows_batch/null patterns", lambda c: c.L.sa_hip_index_query_rows_batch(c.rows._h, None, p(c.off), 1, 1, p(c.out), p(c.out), None), EINVAL, "sa_hip_index_query_rows_batch: NULL patterns"),
    ("rows_for_range/null rows", lambda c: c.L.sa_hip_index_rows_for_range(c.rows._h, rg(c, 0, 0), 1, None, C.byref(c.u32)), EINVAL, "sa_hip_index_rows_for_range: NULL argument"),
    ("set_rows/null table", lambda c: c.L.sa_hip_index_set_rows(c.built._h, None, 2), EINVAL, "sa_hip_index_set_rows: NULL argument"),
    # ---- sizes and ranges
    ("build/capacity", lambda c: c.L.sa_hip_index_build(c.built._h, p(c.long), N + 1, 0), EINVAL, "sa_hip_index_build: n exceeds the index capacity"),
    ("load/capacity", lambda c: c.L.sa_hip_index_load(c.built._h, p(c.long), p(c.sa), N + 1, 0), EINVAL, "sa_hip_index_load: n exceeds the index capacity"),
    ("load/entries", lambda c: c.L.sa_hip_index_load(c.empty._h, p(c.text), p(np.full(N, N, np.uint32)), N, 0), EINVAL, "sa_hip_index_load: suffix array holds entries >= n"),
    ("get_sa_range/first beyond", lambda c: c.L.sa_hip_index_get_sa_range(c.built._h, N + 1, 0, p(c.out)), EINVAL, "sa_hip_index_get_sa_range: out of range"),
    ("get_sa_range/count beyond", lambda c: c.L.sa_hip_index_get_sa_range(c.built._h, 1, N, p(c.out)), EINVAL, "sa_hip_index_get_sa_range: out of range"),
    ("rows_for_range/second beyond", lambda c: c.L.sa_hip_index_rows_for_range(c.rows._h, rg(c, 0, N), 1, p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_rows_for_range: range outside the suffix array"),
    ("rows_for_range/first > second", lambda c: c.L.sa_hip_index_rows_for_range(c.rows._h, rg(c, 5, 3), 1, p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_rows_for_range: range outside the suffix array"),
    ("query_hits/long pattern", lambda c: c.L.sa_hip_index_query_hits(c.built._h, c.long.tobytes(), LONG, 4, C.byref(c.pair), p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_query_hits: pattern longer than 47 KB"),
    ("query_rows/long pattern", lambda c: c.L.sa_hip_index_query_rows(c.rows._h, c.long.tobytes(), LONG, 1, p(c.out), C.byref(c.u32), None), EINVAL, "sa_hip_index_query_hits: pattern longer than 47 KB"),   # (the host path searches through query_hits)
    ("deep_keys/mode 3", lambda c: c.L.sa_hip_index_deep_keys(c.built._h, 3), EINVAL, "sa_hip_index_deep_keys: invalid arguments"),
    ("deep_keys/mode -1", lambda c: c.L.sa_hip_index_deep_keys(c.built._h, -1), EINVAL, "sa_hip_index_deep_keys: invalid arguments"),
    # ---- rows
    ("query_rows/no row table", lambda c: c.L.sa_hip_index_query_rows(c.built._h, b"a", 1, 1, p(c.out), C.byref(c.u32), None), EINVAL, "sa_hip_index_query_rows: no row table (sa_hip_index_set_rows)"),
    ("query_rows_batch/no row table", lambda c: c.L.sa_hip_index_query_rows_batch(c.built._h, p(c.text), p(c.off), 1, 1, p(c.out), p(c.out), None), EINVAL, "sa_hip_index_query_rows_batch: no row table (sa_hip_index_set_rows)"),
    ("rows_for_range/no row table", lambda c: c.L.sa_hip_index_rows_for_range(c.built._h, rg(c, 0, 0), 1, p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_rows_for_range: no row table (sa_hip_index_set_rows)"),
    ("set_rows/first not 0", lambda c: c.L.sa_hip_index_set_rows(c.built._h, p(np.array([1, 2], np.uint64)), 2), EINVAL, "sa_hip_index_set_rows: the first row must start at offset 0"),
    ("set_rows/descending", lambda c: c.L.sa_hip_index_set_rows(c.built._h, p(np.array([0, 5, 3], np.uint64)), 3), EINVAL, "sa_hip_index_set_rows: offsets must ascend"),
    # ---- both: two faults at once, the one that wins
    ("both/query_batch: no index before NULL offsets", lambda c: c.L.sa_hip_query_batch(c.empty._h, p(c.text), None, 1, None), EINVAL, "sa_hip_query_batch: no index"),
    ("both/widen_device: host before no index before NULL output", lambda c: c.L.sa_hip_index_widen_device(c.empty._h, None), EHIP, "sa_hip_index_widen_device: " + HOST),
    ("both/get_sa_u32: no index before NULL output", lambda c: c.L.sa_hip_index_get_sa_u32(c.empty._h, None), EINVAL, "sa_hip_index_get_sa_u32: no index"),
    ("both/get_text: no index before NULL output", lambda c: c.L.sa_hip_index_get_text(c.empty._h, None), EINVAL, "sa_hip_index_get_text: no index"),
    ("both/get_sa_range: no index before range before NULL output", lambda c: c.L.sa_hip_index_get_sa_range(c.empty._h, 99, 1, None), EINVAL, "sa_hip_index_get_sa_range: no index"),
    ("both/get_sa_range: range before NULL output", lambda c: c.L.sa_hip_index_get_sa_range(c.built._h, 99, 1, None), EINVAL, "sa_hip_index_get_sa_range: out of range"),
    ("both/query_rows_batch: NULL argument before no index", lambda c: c.L.sa_hip_index_query_rows_batch(c.empty._h, p(c.text), None, 1, 1, p(c.out), p(c.out), None), EINVAL, "sa_hip_index_query_rows_batch: NULL argument"),
    ("both/query_rows_batch: no index before NULL patterns before row table", lambda c: c.L.sa_hip_index_query_rows_batch(c.empty._h, None, p(c.off), 1, 1, p(c.out), p(c.out), None), EINVAL, "sa_hip_index_query_rows_batch: no index"),
    ("both/query_rows_batch: NULL patterns before row table", lambda c: c.L.sa_hip_index_query_rows_batch(c.built._h, None, p(c.off), 1, 1, p(c.out), p(c.out), None), EINVAL, "sa_hip_index_query_rows_batch: NULL patterns"),
    ("both/query_rows: row table before no index", lambda c: c.L.sa_hip_index_query_rows(c.empty._h, b"a", 1, 1, p(c.out), C.byref(c.u32), None), EINVAL, "sa_hip_index_query_rows: no row table (sa_hip_index_set_rows)"),
    ("both/query_rows: row table before long pattern", lambda c: c.L.sa_hip_index_query_rows(c.built._h, c.long.tobytes(), LONG, 1, p(c.out), C.byref(c.u32), None), EINVAL, "sa_hip_index_query_rows: no row table (sa_hip_index_set_rows)"),
    ("both/query_hits: long pattern before no index", lambda c: c.L.sa_hip_index_query_hits(c.empty._h, c.long.tobytes(), LONG, 4, C.byref(c.pair), p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_query_hits: pattern longer than 47 KB"),
    ("both/query_hits: NULL argument before long pattern", lambda c: c.L.sa_hip_index_query_hits(c.built._h, c.long.tobytes(), LONG, 4, None, p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_query_hits: NULL argument"),
    ("both/rows_for_range: no index before range before row table", lambda c: c.L.sa_hip_index_rows_for_range(c.empty._h, rg(c, 0, N), 1, p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_rows_for_range: no index"),
    ("both/rows_for_range: range before row table", lambda c: c.L.sa_hip_index_rows_for_range(c.built._h, rg(c, 0, N), 1, p(c.out), C.byref(c.u32)), EINVAL, "sa_hip_index_rows_for_range: range outside the suffix array"),
    ("both/build_device: NULL argument before host", lambda c: c.L.sa_hip_index_build_device(c.built._h, None, 5, 0), EINVAL, "sa_hip_index_build_device: NULL argument"),
    ("both/build_device: host before capacity", lambda c: c.L.sa_hip_index_build_device(c.built._h, p(c.long), N + 1, 0), EHIP, "sa_hip_index_build_device: " + HOST),
    ("both/load_device: host before capacity", lambda c: c.L.sa_hip_index_load_device(c.built._h, p(c.long), p(c.sa), N + 1, 0), EHIP, "sa_hip_index_load_device: " + HOST),
    ("both/replica_layout: host before no index", lambda c: c.L.sa_hip_index_replica_layout(c.empty._h, C.byref(c.lay)), EHIP, "sa_hip_index_replica_layout: " + HOST),
    ("both/replica_reserve: host before bad key width", lambda c: c.L.sa_hip_index_replica_reserve(c.built._h, C.byref(c.bad_lay), C.byref(c.bufs)), EHIP, "sa_hip_index_replica_reserve: " + HOST),
    ("both/replica_commit: host before nothing reserved", lambda c: c.L.sa_hip_index_replica_commit(c.empty._h), EHIP, "sa_hip_index_replica_commit: " + HOST),
    ("both/query_batch_device: host before no index before NULL argument", lambda c: c.L.sa_hip_query_batch_device(c.empty._h, None, None, 1, None), EHIP, "sa_hip_query_batch_device: " + HOST),
    ("both/query_batch_device_fixed: host before no index", lambda c: c.L.sa_hip_query_batch_device_fixed(c.empty._h, None, 1, 1, None), EHIP, "sa_hip_query_batch_device_fixed: " + HOST),
    ("both/set_rows: first row before order", lambda c: c.L.sa_hip_index_set_rows(c.built._h, p(np.array([1, 0], np.uint64)), 2), EINVAL, "sa_hip_index_set_rows: the first row must start at offset 0"),
    ("both/deep_keys: arguments before the host path's 0", lambda c: c.L.sa_hip_index_deep_keys(c.empty._h, 3), EINVAL, "sa_hip_index_deep_keys: invalid arguments"),
]


@pytest.mark.parametrize("name,call,code,text", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(ctx, name, call, code, text):
    with pytest.raises(ctx.capi.SaHipError) as e:
        ctx.capi.check(call(ctx))
    assert e.value.code == code
    assert ctx.L.sa_hip_last_error().decode() == text
    assert str(e.value).endswith(": " + text)


def test_what_is_not_refused(ctx):
    """The other side of the precedence rows: what returns 0 before a refusal could apply, and the handles still work."""
    c, L = ctx, ctx.L
    assert L.sa_hip_index_deep_keys(c.empty._h, 2) == 0            # the host path answers before "no index"
    assert L.sa_hip_index_deep_keys(c.built._h, 0) == 0 and L.sa_hip_index_sync(c.empty._h) == 0
    assert L.sa_hip_query_batch(c.built._h, None, None, 0, None) == 0                                # Q == 0 before the arguments
    assert L.sa_hip_query_batch(c.empty._h, None, None, 0, None) == EINVAL                           # ... but after the index
    assert L.sa_hip_index_query_rows_batch(c.empty._h, None, None, 0, 1, None, None, None) == 0      # Q == 0 before the lock
    assert L.sa_hip_index_get_sa_range(c.built._h, N, 0, None) == 0                                  # an empty range at the end
    assert L.sa_hip_index_rows_for_range(c.built._h, rg(c, 7, 6), 0, None, C.byref(c.u32)) == 0      # a miss, k == 0: no table needed
    assert L.sa_hip_index_rows_for_range(c.rows._h, rg(c, 0xFFFFFFFF, 0xFFFFFFFF), 1, p(c.out), C.byref(c.u32)) == 0 and c.u32.value == 0
    pat = c.long[:LONG - 1].tobytes()                              # 48 960 bytes: the longest pattern the per-call paths take
    assert L.sa_hip_index_query_hits(c.built._h, pat, LONG - 1, 4, C.byref(c.pair), p(c.out), C.byref(c.u32)) == 0 and c.u32.value == 0
    assert L.sa_hip_index_query_rows(c.rows._h, pat, LONG - 1, 1, p(c.out), C.byref(c.u32), None) == 0 and c.u32.value == 0
    assert c.built.verify() == 0 and c.rows.verify() == 0
    rows, rng = c.rows.query_rows(bytes(c.text[30:34]), 4)
    assert sorted(rows.tolist()) == [0, 1] and rng[0] <= rng[1]
