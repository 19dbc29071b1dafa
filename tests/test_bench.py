"""bench.py's contract: --steps sets the timed steps, the line carries ms_per_step, a plain run leaves the gates and the
secondary measurements to --full, and --dump-outputs writes what the timed path returned (checked against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from suffixarray_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP_LIMIT = 64_000_000


def _dumped(path):
    files = sorted(f for f in os.listdir(path) if f.endswith(".npy"))
    assert sum(os.path.getsize(os.path.join(path, f)) for f in files) <= DUMP_LIMIT
    out = {f[:-4]: np.load(os.path.join(path, f)) for f in files}
    assert all(a.dtype == np.float64 for a in out.values())
    return out


def test_dump_outputs_samples_large_outputs_within_the_budget(tmp_path):
    import torch
    import bench
    rng = np.random.default_rng(3)
    sa = rng.permutation(3_000_000).astype(np.int64)
    ranges = rng.integers(0, 1 << 32, (2_500_000, 2), dtype=np.uint64).astype(np.uint32)
    ranges[::7] = 0xFFFFFFFF
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch, sa64=torch.from_numpy(sa), ranges=ranges)
    a, b = _dumped(tmp_path / "a"), _dumped(tmp_path / "b")
    assert sorted(a) == ["query_ranges", "query_sample_index", "sa64_sample", "sa64_sample_pos"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k   # fixed, seeded samples
    pos = a["sa64_sample_pos"].astype(np.int64)
    assert pos.size > 800_000 and np.all(np.diff(pos) > 0)
    assert np.array_equal(a["sa64_sample"], sa[pos].astype(np.float64))
    sel = a["query_sample_index"].astype(np.int64)
    assert np.array_equal(a["query_ranges"], ranges[sel].astype(np.float64))
    # small outputs whole; row ids beyond a query's count as -1
    q, k = 1000, 4
    ids = rng.integers(0, 1 << 40, (q, k), dtype=np.uint64)
    cnt = rng.integers(0, k + 1, q).astype(np.uint32)
    bench.dump_outputs(str(tmp_path / "c"), torch, sa64=torch.from_numpy(sa[:5000]), ranges=ranges[:q], row_ids=ids, row_counts=cnt)
    c = _dumped(tmp_path / "c")
    assert sorted(c) == ["query_ranges", "row_counts", "row_ids", "sa64_sample", "sa64_sample_pos"]
    assert np.array_equal(c["sa64_sample"], sa[:5000].astype(np.float64)) and np.array_equal(c["query_ranges"], ranges[:q].astype(np.float64))
    live = np.arange(k)[None, :] < cnt[:, None]
    assert np.array_equal(c["row_counts"], cnt.astype(np.float64))
    assert np.array_equal(c["row_ids"][live], ids[live].astype(np.float64)) and np.all(c["row_ids"][~live] == -1)


@pytest.mark.gpu
def test_plain_and_full_runs_time_the_steps_and_dump_the_same_outputs(gpu, oracle, tmp_path):
    n, q, m, steps = 20_000_000, 300_000, 16, 3
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)

    def run(out, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--chars", str(n),
               "--queries", str(q), "--dump-outputs", str(out), *extra]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    plain = run(tmp_path / "plain")
    assert plain["metric"] == "sa_build_chars_per_s" and plain["unit"] == "chars/s" and plain["higher_is_better"] is True
    assert plain["steps"] == steps and plain["ms_per_step"] > 0 and plain["value"] > 0 and plain["dtype"]
    assert not {"gate", "query_populations", "cpu_baseline", "secondary"} & set(plain)
    full = run(tmp_path / "full", "--full", "--no-cpu-baseline", "--no-secondary")
    assert full["steps"] == steps and full["gate"]["ok"] and full["gate"]["verify_violations"] == 0
    assert "hits_only" in full["query_populations"]
    a, b = _dumped(tmp_path / "plain"), _dumped(tmp_path / "full")
    assert sorted(a) == sorted(b) == ["query_ranges", "sa64_sample", "sa64_sample_pos"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k   # same arguments, same inputs, same outputs
    # ... and what they hold is what the oracle computes
    text = synth.d1_uniform27(n)
    sa = oracle.sais(text)
    pos = a["sa64_sample_pos"].astype(np.int64)
    assert np.array_equal(a["sa64_sample"], sa[pos].astype(np.float64))
    fb, fo = synth.query_batch(text, q, m, seed=0)
    exp = oracle.query_batch(text, sa.astype(np.uint32), 0xFFFFFFFF, (fb, fo))
    assert np.array_equal(a["query_ranges"], np.stack([exp["first"], exp["second"]], axis=1).astype(np.float64))
