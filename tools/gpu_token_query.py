"""Token-index search on the device: one JSON line with, for n Zipf tokens over a 50 257-word vocabulary (the recipe of
tests/test_gpu_int.py: zipf_tokens), the four plans of the search side by side --

  default    key array + first-symbol directory        no_keys    directory only (bounds by text comparison)
  no_dir     key array only                            text_only  neither

  * prepare_ms of every plan (sa_hip_token_info: alphabet pass, range check, directory, key gather; HIP events)
  * two batches of Q n-grams of length 1..8: "hits" sampled from the text, "changed" the same with one symbol replaced --
    HIP-event time of the search launch (sa_hip_token_info.kernel_ms) after a warm-up, median and minimum over the
    repetitions, the plans taking turns inside every repetition
  * gates: the four plans answer identically, and a sample of the answers equals a count of the text's windows on the host

    python tools/gpu_token_query.py [--n N] [--q Q] [--reps R] [--out FILE]
"""
import json
import os
import sys

os.environ.setdefault("SA_HIP_DIAG", "1")   # the plan switches are read only with this set

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (first: one HIP runtime per process)

from suffixarray_amd import _capi  # noqa: E402
from test_gpu_int import zipf_tokens  # noqa: E402

VOCAB = 50257
PLANS = {
    "default": {},
    "no_keys": {"SA_HIP_TOKEN_KEYS": "0"},
    "no_dir": {"SA_HIP_TOKEN_DIR": "0"},
    "text_only": {"SA_HIP_TOKEN_KEYS": "0", "SA_HIP_TOKEN_DIR": "0"},
}


def arg(name, default):
    return int(float(sys.argv[sys.argv.index(name) + 1])) if name in sys.argv else default


def make_batches(t, q, seed=11):
    """(packed int32, uint64 offsets) of q n-grams of length 1..8 cut from the text, and the same with one symbol replaced"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 9, q)
    pos = rng.integers(0, t.size - 8, q)
    off = np.zeros(q + 1, np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    start = off[:-1].astype(np.int64)
    within = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(start, lens)
    hits = t[np.repeat(pos, lens) + within].astype(np.int32)
    changed = hits.copy()
    at = start + rng.integers(0, lens)
    changed[at] = (changed[at] + rng.integers(1, VOCAB, q)) % VOCAB
    return {"hits": (hits, off), "changed": (changed, off)}


def window_count(t, p):
    idx = np.flatnonzero(t[:t.size - len(p) + 1] == p[0])
    for j in range(1, len(p)):
        idx = idx[t[idx + j] == p[j]]
    return idx.size


def main():
    n, q, reps = arg("--n", 100_000_000), arg("--q", 1_000_000), arg("--reps", 20)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    t = zipf_tokens(n, VOCAB, seed=1)
    t_d = torch.from_numpy(t).to("cuda:0")
    sa_d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = _capi.libsais_int_device(t_d.data_ptr(), sa_d.data_ptr(), n, VOCAB)
    res = {"tool": "gpu_token_query", "n": n, "vocab": VOCAB, "q": q, "reps": reps, "ngram_lengths": "1..8",
           "build_device_ms": round(st["total_ms"], 3), "plans": {}}
    handles = {}
    for plan, env in PLANS.items():
        for k in ("SA_HIP_TOKEN_KEYS", "SA_HIP_TOKEN_DIR"):
            os.environ.pop(k, None)
        os.environ.update(env)
        handles[plan] = _capi.TokenIndex.load_device(t_d.data_ptr(), sa_d.data_ptr(), n)
        info = handles[plan].info()
        res["plans"][plan] = {"prepare_ms": round(info["prepare_ms"], 3), "dir_entries": info["dir_entries"], "key_bytes": info["key_bytes"]}
    del sa_d
    batches = make_batches(t, q)
    ok = True
    for bname, (buf, off) in batches.items():
        p_d, o_d = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off.view(np.int64)).to("cuda:0")
        outs = {plan: torch.zeros((q, 2), dtype=torch.int32, device="cuda:0") for plan in PLANS}
        torch.cuda.synchronize()
        ms = {plan: [] for plan in PLANS}
        for rep in range(reps + 2):                       # two warm-up rounds, then the plans take turns
            for plan, h in handles.items():
                h.query_batch_device(p_d.data_ptr(), o_d.data_ptr(), q, outs[plan].data_ptr())
                k_ms = h.info()["kernel_ms"]              # waits for the launch
                if rep >= 2:
                    ms[plan].append(k_ms)
        got = {plan: o.cpu().numpy().view(np.uint32) for plan, o in outs.items()}
        same = all(np.array_equal(got["default"], g) for g in got.values())
        sample = np.random.default_rng(5).integers(0, q, 24)
        counted = all(int(got["default"][i, 1]) == window_count(t, buf[int(off[i]):int(off[i + 1])]) for i in sample)
        ok = ok and same and counted
        for plan in PLANS:
            v = np.array(ms[plan])
            res["plans"][plan][bname] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4),
                                         "max_ms": round(float(v.max()), 4), "mqueries_per_s": round(q / float(np.median(v)) / 1e3, 1)}
        res[bname + "_found"] = int((got["default"][:, 1] > 0).sum())
        res[bname + "_plans_equal"] = bool(same)
        res[bname + "_sample_equals_window_count"] = bool(counted)
    for h in handles.values():
        h.close()
    res["gate_ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
