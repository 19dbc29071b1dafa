"""GPU: the persistent form of the local pass of the three-pass narrow sort (radix_split.hpp: local_persist_kernel -- as many
workgroups as are resident, each ordering a run of sub-buckets with the next one's records loaded while the current one is
stored) against the form with one workgroup per sub-bucket (SA_HIP_LOCAL_PERSIST=0): the same suffix array and int64 copy bit
for bit, verified on the device, and the same query ranges (they go through the directory the local pass writes) -- on
uniform text at several sizes, many levels with sub-buckets of 0 and 1 records, texts whose staging rows of tied slots
overflow, the large form, 2048 bins, truncated builds, the flags work folded in or not, and tiny grids (SA_HIP_LOCAL_GRID) on
which one workgroup walks thousands of sub-buckets."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu


def _build(gpu, t, L, persist, env, monkeypatch, api="host"):
    import torch
    monkeypatch.setenv("SA_HIP_LOCAL_PERSIST", "1" if persist else "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        with gpu.DeviceIndex(t.size, 0) as idx:
            sa64 = None
            if api == "host":
                idx.build(t, L)
            else:
                idx.build(t, L)   # uploads the text; the device entry points build again from it
                torch.cuda.synchronize()
                if api == "device64":
                    out = torch.full((t.size,), -7, dtype=torch.int64, device="cuda:0")
                    torch.cuda.synchronize()
                    idx.build_device64(idx.text_dev, t.size, out.data_ptr(), L)
                    idx.sync()
                    sa64 = out.cpu().numpy()
                else:
                    idx.build_device(idx.text_dev, t.size, L)
                    idx.sync()
            st = idx.build_stats()
            assert st["split_plan"] > 0 or "SA_HIP_INITIAL_CHARS" in env, (env, st)   # (k0 = 4: the plan may decline)
            assert idx.verify() == 0, (env, st)
            pats = cases.query_patterns(t, 2000, np.random.default_rng(9), maxlen=24)
            return idx.sa_u32().copy(), sa64, idx.query_batch(pats).copy(), st
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def _same(gpu, t, L, env, monkeypatch, api="host"):
    a = _build(gpu, t, L, False, env, monkeypatch, api)
    b = _build(gpu, t, L, True, env, monkeypatch, api)
    assert np.array_equal(a[0], b[0]), (env, L, api)
    if api == "device64":
        assert np.array_equal(a[1], b[1]) and np.array_equal(b[1], b[0].astype(np.int64)), (env, L, api)
    assert np.array_equal(a[2], b[2]), (env, L, api)
    return b


def test_persistent_local_pass_matches_one_workgroup_per_sub_bucket(gpu, oracle, monkeypatch):
    from suffixarray_amd import synth
    monkeypatch.setenv("SA_HIP_SPLIT", "1")
    d1 = synth.d1_uniform27(6_000_000)
    small = synth.d1_uniform27(4_500_001)
    # uniform text at three sizes (the first against the oracle as well)
    sa, _, _, _ = _same(gpu, small, 0, {}, monkeypatch)
    assert np.array_equal(sa, oracle.sais(small).astype(np.uint32))
    _same(gpu, d1, 0, {}, monkeypatch)
    _same(gpu, synth.d1_uniform27(12_000_000), 0, {}, monkeypatch)
    # many levels: small bounds on a sub-bucket give sub-buckets of 0 and 1 records
    levels = set()
    for cap in ("300", "2048"):
        for flags in ("1", "0"):
            st = _same(gpu, d1, 0, {"SA_HIP_SPLIT_CAP": cap, "SA_HIP_SPLIT_FLAGS": flags}, monkeypatch)[3]
            levels.add(st["split_plan"])
    assert len(levels) >= 2, levels
    # nearly every slot tied: the staging rows overflow (k0 = 4), or nearly (k0 = 5); the large form takes these
    for k0 in ("4", "5"):
        _same(gpu, d1, 0, {"SA_HIP_INITIAL_CHARS": k0}, monkeypatch)
    # the large form, 2048 bins, the flags pass on its own
    _same(gpu, d1, 0, {"SA_HIP_LOCAL_BIG": "1"}, monkeypatch)
    _same(gpu, d1, 0, {"SA_HIP_LOCAL_BINS": "11"}, monkeypatch)
    _same(gpu, d1, 0, {"SA_HIP_SPLIT_FLAGS": "0"}, monkeypatch)
    _same(gpu, d1, 0, {"SA_HIP_SPLIT_FLAGS": "1"}, monkeypatch)
    # a truncated build whose ties must stay in text order (k0 = L)
    sa, _, _, _ = _same(gpu, synth.d1_uniform27(5_000_000), 8, {"SA_HIP_SPLIT_CAP": "500"}, monkeypatch)
    _same(gpu, d1, 8, {"SA_HIP_INITIAL_CHARS": "8"}, monkeypatch)
    # the device entry points, with and without the int64 copy out of the local pass
    _same(gpu, small, 0, {}, monkeypatch, api="device")
    _same(gpu, small, 0, {}, monkeypatch, api="device64")


@pytest.mark.parametrize("grid", [1, 3, 7])
def test_persistent_local_pass_on_tiny_grids(gpu, monkeypatch, grid):
    """One workgroup walks thousands of sub-buckets (empty ones, single records, full ones) across bucket boundaries."""
    from suffixarray_amd import synth
    monkeypatch.setenv("SA_HIP_SPLIT", "1")
    d1 = synth.d1_uniform27(6_000_000)
    g = {"SA_HIP_LOCAL_GRID": str(grid)}
    _same(gpu, d1, 0, g, monkeypatch, api="device64")
    _same(gpu, d1, 0, dict(g, SA_HIP_SPLIT_CAP="300"), monkeypatch)
    _same(gpu, d1, 0, dict(g, SA_HIP_SPLIT_CAP="2048", SA_HIP_SPLIT_FLAGS="0"), monkeypatch)
    _same(gpu, d1, 0, dict(g, SA_HIP_LOCAL_BIG="1"), monkeypatch)
    _same(gpu, d1, 0, dict(g, SA_HIP_INITIAL_CHARS="4"), monkeypatch)
