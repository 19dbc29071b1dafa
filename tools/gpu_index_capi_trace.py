"""The launches of the byte-index handle's C ABI, for comparing two builds of the library (profiles/index_capi_trace.txt).

    SA_HIP_LIB=<lib> rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d <dir> -- python3 tools/gpu_index_capi_trace.py run
    python3 tools/gpu_index_capi_trace.py compare <dir of the parent> <dir of the branch>

run: at the size of tests/test_gpu_index_capi.py (65 536 bytes over 4 symbols) a build, one query_hits, one query_rows, a batch of
448, a batch of 449, a clustered batch (SA_HIP_QCLUSTER_MIN=4096, Q = 8192), a query_rows_batch (plain copies) and a replica
reserve / commit.  compare: the ordered names and grids of the library's kernels must be equal; the copies and memsets -- the trace's copy records and
the runtime's own copy and fill kernels -- are compared as a multiset, and every position where the full lists differ is printed."""
import collections
import csv
import glob
import os
import sys

os.environ.setdefault("SA_HIP_DIAG", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import numpy as np
    import torch
    from suffixarray_amd import _capi
    n = 65536
    text = np.random.default_rng(5).integers(97, 101, n).astype(np.uint8)
    cut = lambda q, m, seed: [bytes(text[a:a + m]) for a in np.random.default_rng(seed).integers(0, n - m, q).tolist()]
    with _capi.DeviceIndex(n, 0) as idx, _capi.DeviceIndex(n, 0) as rep:
        idx.build(text)
        idx.set_rows(np.arange(0, n, 1000, dtype=np.uint64))
        idx.query_hits(bytes(text[500:512]))
        idx.query_rows(bytes(text[900:906]), 4)
        idx.query_batch(cut(448, 3, 1))
        idx.query_batch(cut(449, 3, 2))
        os.environ["SA_HIP_QCLUSTER_MIN"] = "4096"
        idx.query_batch(cut(8192, 12, 3))
        del os.environ["SA_HIP_QCLUSTER_MIN"]
        idx.query_rows_batch(cut(5000, 6, 4), 4)
        lay = idx.replica_layout()
        src, dst = idx.replica_buffers(), rep.replica_reserve(lay)
        class Raw:   # a device buffer of the library as torch sees it
            def __init__(self, ptr, nbytes):
                self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}
        for (s, nb), (d, _) in zip(src.items(), dst.items()):
            if nb:
                torch.as_tensor(Raw(d, nb), device="cuda:0").copy_(torch.as_tensor(Raw(s, nb), device="cuda:0"))
        torch.cuda.synchronize()
        rep.replica_commit()
        assert np.array_equal(rep.query_batch(cut(16, 5, 5)), idx.query_batch(cut(16, 5, 5)))
    print("ok")


def rows_of(d, pattern):
    out = []
    for f in sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True)):
        out += list(csv.DictReader(open(f)))
    return sorted(out, key=lambda r: int(r.get("Start_Timestamp", 0)))


def launches(d):
    def grid(r):
        return tuple(int(r[k]) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z") if k in r) or (r.get("Grid_Size"),)
    kernels = [(r["Kernel_Name"], grid(r)) for r in rows_of(d, "*kernel_trace.csv")]
    copies = [(r.get("Direction", "?"), r.get("Bytes", r.get("Size", "?"))) for r in rows_of(d, "*memory_copy_trace.csv")]
    return kernels, copies


def compare(a, b):
    (ka, ca), (kb, cb) = launches(a), launches(b)
    runtime = lambda k: k[0].startswith("__amd_rocclr_")          # the runtime's own copy and fill kernels: copies of pageable memory, memsets
    la, lb = [k for k in ka if not runtime(k)], [k for k in kb if not runtime(k)]
    ra, rb = [k for k in ka if runtime(k)], [k for k in kb if runtime(k)]
    print("kernels of the library: parent %d, branch %d launches, %d distinct names" % (len(la), len(lb), len({k for k, _ in la})))
    same = la == lb
    print("ordered (kernel name, grid) lists of the library's kernels:", "EQUAL" if same else "DIFFERENT")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            print("  first difference at launch %d:\n    parent %s %s\n    branch %s %s" % (i, x[0][:100], x[1], y[0][:100], y[1]))
            break
    ma, mb = collections.Counter(ca + ra), collections.Counter(cb + rb)
    print("copies and memsets (%d + %d runtime kernels on the parent, %d + %d on the branch) as a multiset:" % (len(ca), len(ra), len(cb), len(rb)),
          "EQUAL" if ma == mb else "DIFFERENT")
    for key in sorted(set(ma) | set(mb), key=str):
        if ma[key] != mb[key]:
            print("  %s: parent %d, branch %d" % (key, ma[key], mb[key]))
    moved = [i for i, (x, y) in enumerate(zip(ka, kb)) if x != y]
    print("positions in the full ordered list where the two differ:", moved or "none")
    for i in moved:
        print("  %3d  parent %-40s %-14s branch %-40s %s" % (i, ka[i][0][:40], ka[i][1], kb[i][0][:40], kb[i][1]))
    for name, cnt in sorted(collections.Counter(k for k, _ in ka).items(), key=lambda t: -t[1]):
        print("  %5d  %s" % (cnt, name[:150]))
    return 0 if same and ma == mb else 1


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["compare"] and len(sys.argv) == 4:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
