"""GPU: record retrieval (hits -> distinct rows) in every form it runs in, against the plain row model of cases.py.

csrc/rows_device.hpp answers a range by one lane (batch Q >= 4096, <= 4 hits), one wave (batch, k <= 64: a 256-slot table, at most
4096 hits, then the range is handed on), one workgroup (k <= 1536: 4096 slots; k <= 4096: 16384 slots) or, for one query, the fused
search + rows kernel; csrc/records.hpp answers k > 4096 and SA_HIP_HOST_ROWS=1 on the host.  Texts with planted markers
(cases.rows_main_case / rows_small_case) put hit counts, distinct-row counts and the k-th new row on every threshold of those forms;
every result -- counts, the ordered row ids, the slots past each count (pre-filled with a sentinel) and the ranges -- is compared
with cases.rows_reference.  The last test checks that every (form x boundary) cell below was filled."""
import ctypes as C

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

SENT = np.uint64(0xDEADBEEFDEADBEEF)
MAXU = 0xFFFFFFFF
# csrc/rows_device.hpp and csrc/sa_capi.hip, restated: launch_rows' predicates and grid caps
ROWS_K_MAX, K_SMALL, WAVE_K_MAX, LANE_MAX, LANE_MIN_BATCH, WAVE_MAX_HITS = 4096, 1536, 64, 4, 4096, 4096
RING_MIN_BYTES = 32 << 20
WG_GRID_SMALL, WG_GRID_LARGE = 2048, 512

COVER = set()   # (form, cell) filled by the sweep; checked by test_rows_coverage_matrix


class RowCase:
    """One text, built once: the device index, its verified suffix array, the pool of distinct patterns with their ranges
    (checked against the oracle) and the model's rows of every pool pattern under the current row table."""

    def __init__(self, gpu, oracle, made, label):
        text, starts, pats, claim = made
        self.label, self.gpu, self.text = label, gpu, text
        self.names = list(pats)
        self.pool = [pats[m] for m in self.names]
        self.plen = np.array([len(p) for p in self.pool], dtype=np.uint64)
        self.idx = gpu.DeviceIndex(text.size, 0)
        self.idx.build(text)
        assert self.idx.verify() == 0, label
        self.sa = self.idx.sa_u32()
        self.ranges = self.idx.query_batch(self.pool)
        assert np.array_equal(self.ranges, oracle.query_batch(text, self.sa, MAXU, self.pool)), label
        self.hits = cases.range_hits(self.ranges)
        assert [int(h) for h in self.hits] == [claim[m][0] for m in self.names], label
        self.starts0 = starts
        self.set_table(starts, "rows%d" % starts.size)

    def set_table(self, starts, table_label):
        self.starts, self.table = starts, table_label
        self.idx.set_rows(starts)
        _, self.full, self.fh = cases.rows_reference(self.sa, starts, self.ranges, starts.size, with_first_hits=True)
        self.nrows = np.array([r.size for r in self.full], dtype=np.int64)
        self._exp = {}

    def expected(self, k_in):
        """(counts, row ids [P, max(k_in, 1)] with the sentinel past every count) of the pool"""
        if k_in not in self._exp:
            cnt = np.minimum(self.nrows, min(k_in, self.starts.size))
            E = np.full((len(self.pool), max(k_in, 1)), SENT, dtype=np.uint64)
            for i, r in enumerate(self.full):
                E[i, :cnt[i]] = r[:cnt[i]]
            self._exp = {k_in: (cnt, E)}
        return self._exp[k_in]

    def packed(self, sel):
        off = np.zeros(sel.size + 1, dtype=np.uint64)
        off[1:] = np.cumsum(self.plen[sel])
        buf = np.frombuffer(b"".join(self.pool[i] for i in sel.tolist()) or b"\0", dtype=np.uint8)
        return buf, off

    def close(self):
        self.idx.close()


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _delenv(monkeypatch, env):
    for k in env:
        monkeypatch.delenv(k, raising=False)


def _hit_cell(case, i):
    h = int(case.hits[i])
    if h == 0:
        f, s = int(case.ranges[i]["first"]), int(case.ranges[i]["second"])
        return "h0_end" if f == MAXU else ("h0_wrap" if f == 0 else "h0_mid")
    if h in (1, 2, 3, 4, 5, 6, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097):
        return "h%d" % h
    return "h20000+" if h >= 20_000 else None


def _cells(case, i, k_in, k, chunk):
    """the boundary cells one range fills at (k_in, clamped k) in a form that walks `chunk` hits at a time"""
    out = {_hit_cell(case, i), "k1e9" if k_in == 10 ** 9 else "k%d" % k_in, case.table}
    if k_in > case.starts.size:
        out.add("k>rows")
    d = int(case.nrows[i])
    if case.hits[i] > 1 and d == 1:
        out.add("one_row")
    if d:
        out.add({0: "d=k", 1: "d=k+1"}.get(d - k, "d<k" if d < k else ("d>=k+256" if d >= k + 256 else None)))
    if chunk and d >= k:
        at = int(case.fh[i][k - 1])                                        # hit index of the k-th new row
        if int(np.searchsorted(case.fh[i], (at // chunk + 1) * chunk)) == k - 1 + chunk:
            out.add("table_max")                                           # the table holds k - 1 + chunk rows
        if 0 < at % chunk < chunk - 1:
            out.add("mid_chunk")
    out.discard(None)
    return out


def record(case, sel, k_in, env, single=False, sector=2):
    """Fill COVER with the (form, cell) pairs of one call: launch_rows' predicates restated over the model's hit counts."""
    Q = 1 if single else int(np.asarray(sel).size)
    k = min(k_in, case.starts.size)
    if k == 0:
        COVER.add(("none", "k0"))
        return
    u, mult = np.unique(np.asarray(sel), return_counts=True)
    host = k > ROWS_K_MAX or env.get("SA_HIP_HOST_ROWS") == "1"
    lanes = not single and Q >= LANE_MIN_BATCH and env.get("SA_HIP_ROWS_LANES") != "0"
    waves = lanes and k <= WAVE_K_MAX and env.get("SA_HIP_ROWS_WAVES") != "0"
    wg = "wg_small" if k <= K_SMALL else "wg_large"
    ring = not host and not single and Q * k * 4 >= RING_MIN_BYTES and env.get("SA_HIP_ROWS_RING") != "0"
    load = {}
    for i, m in zip(u.tolist(), mult.tolist()):
        h = int(case.hits[i])
        if host:
            forms = ["host"]
        elif single:
            forms = ["fused" if sector == 2 and k <= K_SMALL else "unfused"]
        elif lanes and h <= LANE_MAX:
            forms = ["lane"]
        elif waves:
            forms = ["wave"]
            if h > WAVE_MAX_HITS and int(np.searchsorted(case.fh[i], WAVE_MAX_HITS)) < k:
                forms += ["handoff", wg]
        else:
            forms = [wg]
        for f in forms:
            load[f] = load.get(f, 0) + m
            chunk = {"wave": 64, "handoff": 0, "lane": 0, "host": 0}.get(f, 256)
            cells = _cells(case, i, k_in, k, chunk)
            if not single:
                cells |= {"sentinel"} | ({"Q%d" % Q} if Q in (4095, 4096) else set())
                if ring:
                    cells |= {"ring"} | ({"ring_clamped"} if k_in != k else set())
                if Q >= 140_001:
                    cells.add("Q140001")
            if env.get("zero_len"):
                cells.add("zero_len")
            COVER.update((f, c) for c in cells)
    groups = int(env.get("SA_HIP_ROWS_WAVE_GROUPS", 8))
    if load.get("wave", 0) > 4 * min((Q + 3) // 4, 256 * groups):
        COVER.add(("wave", "reuse" if groups == 8 else "reuse_groups%d" % groups))
    if load.get("wg_small", 0) > min(Q, WG_GRID_SMALL):
        COVER.add(("wg_small", "reuse"))
    if load.get("wg_large", 0) > min(Q, WG_GRID_LARGE):
        COVER.add(("wg_large", "reuse"))


def run_batch(case, sel, k, monkeypatch, env=None):
    """query_rows_batch_raw over pool[sel] at k, into arrays pre-filled with a sentinel, against the model"""
    env = dict(env or {})
    sel = np.ascontiguousarray(sel, dtype=np.int64)
    Q = sel.size
    out = (np.full((Q, max(k, 1)), SENT, dtype=np.uint64), np.full(Q, 7, dtype=np.uint32),
           np.zeros(Q, dtype=case.ranges.dtype))
    _setenv(monkeypatch, {n: v for n, v in env.items() if n.startswith("SA_HIP")})
    try:
        (rows, cnt), rg = case.idx.query_rows_batch_raw(case.packed(sel), k, out=out)
    finally:
        _delenv(monkeypatch, [n for n in env if n.startswith("SA_HIP")])
    what = (case.label, case.table, "Q=%d" % Q, "k=%d" % k, env)
    assert np.array_equal(rg, case.ranges[sel]), what
    ecnt, E = case.expected(k)
    bad = np.flatnonzero(cnt != ecnt[sel])
    assert not bad.size, (what, [(case.names[sel[q]], int(cnt[q]), int(ecnt[sel[q]])) for q in bad[:5]])
    assert int(cnt.max(initial=0)) <= min(k, case.starts.size), what
    bad = np.flatnonzero((rows != E[sel]).any(axis=1))
    if bad.size:
        q = int(bad[0])
        c = int(ecnt[sel[q]])
        pytest.fail("%r: %d queries differ; first %s: got %s... expected %s... (slots past the count hold the sentinel: %s)" % (
            what, bad.size, case.names[sel[q]], rows[q, :min(c, 12)].tolist(), E[sel[q], :min(c, 12)].tolist(),
            bool(np.all(rows[q, c:] == SENT))))
    record(case, sel, k, env)
    return rows, cnt, rg


def c_query_rows(case, i, k, batch=False):
    """one query through the C entry point with a buffer of min(k, num_rows) ids + 8 sentinel slots (k = 10^9 must not size
    anything): sa_hip_index_query_rows, or sa_hip_index_query_rows_batch with Q = 1 -> (ids, range)"""
    lib, gpu = case.idx._lib, case.gpu
    cap = max(min(k, case.starts.size), 1)
    ids = np.full(cap + 8, SENT, dtype=np.uint64)
    p = case.pool[i]
    if batch:
        off = np.array([0, len(p)], dtype=np.uint64)
        cnt = np.zeros(1, np.uint32)
        rg = np.zeros(1, case.ranges.dtype)
        buf = np.frombuffer(p or b"\0", np.uint8)
        gpu.check(lib.sa_hip_index_query_rows_batch(case.idx._h, buf.ctypes.data, off.ctypes.data, 1, k, ids.ctypes.data,
                                                    cnt.ctypes.data, rg.ctypes.data))
        n, r = int(cnt[0]), (int(rg[0]["first"]), int(rg[0]["second"]))
    else:
        n32, pr = C.c_uint32(0), gpu.PairU32()
        gpu.check(lib.sa_hip_index_query_rows(case.idx._h, p, len(p), k, ids.ctypes.data, C.byref(n32), C.byref(pr)))
        n, r = n32.value, (pr.first, pr.second)
    assert np.all(ids[n:] == SENT), (case.label, case.names[i], k, n)
    return ids[:n], r


def run_single(case, ks, monkeypatch, env=None, sector=2, batch1=False):
    """every pool pattern as ONE query (the fused kernel, or the search + rows launches) at every k of ks, against the model"""
    env = dict(env or {})
    _setenv(monkeypatch, {n: v for n, v in env.items() if n.startswith("SA_HIP")})
    try:
        for k in ks:
            for i in range(len(case.pool)):
                got, rg = c_query_rows(case, i, k, batch=batch1)
                assert rg == (int(case.ranges[i]["first"]), int(case.ranges[i]["second"])), (case.label, case.names[i], k)
                exp = case.full[i][:min(k, case.starts.size)]
                assert np.array_equal(got, exp), (case.label, case.table, case.names[i], k, env, got[:12], exp[:12])
            if batch1:
                record(case, np.arange(len(case.pool)), k, {**env, "SA_HIP_ROWS_LANES": "0"})
            else:
                record(case, np.arange(len(case.pool)), k, env, single=True, sector=sector)
    finally:
        _delenv(monkeypatch, [n for n in env if n.startswith("SA_HIP")])


def check_rows_for_range(case, ks):
    """sa_hip_index_rows_for_range (host code) on the ranges the batch returned"""
    lib, gpu = case.idx._lib, case.gpu
    for k in ks:
        cap = max(min(k, case.starts.size), 1)
        for i in range(len(case.pool)):
            ids = np.full(cap + 8, SENT, dtype=np.uint64)
            n = C.c_uint32(0)
            pr = gpu.PairU32(int(case.ranges[i]["first"]), int(case.ranges[i]["second"]))
            gpu.check(lib.sa_hip_index_rows_for_range(case.idx._h, pr, k, ids.ctypes.data, C.byref(n)))
            assert np.array_equal(ids[:n.value], case.full[i][:min(k, case.starts.size)]), (case.label, case.names[i], k)
            assert np.all(ids[n.value:] == SENT)
    COVER.add(("host", "rows_for_range"))


def tiled(case, Q, seed):
    """Q queries drawn from the pool: every pattern at least once, the rest at random (neighbouring queries share rows, so a
    wave or workgroup that walks several ranges must clear its table in between)"""
    rng = np.random.default_rng(seed)
    P = len(case.pool)
    sel = np.concatenate([np.arange(P), rng.integers(0, P, max(Q - P, 0))])[:Q]
    rng.shuffle(sel)
    return sel


K_POOL = (0, 1, 2, 4, 5, 63, 64, 65, 256, 1536, 1537, 4096, 4097)


@pytest.fixture(scope="module")
def main(gpu, oracle):
    c = RowCase(gpu, oracle, cases.rows_main_case(), "main")
    yield c
    c.close()


def test_main_pool_every_k(main, monkeypatch):
    """The pool once per batch (Q < 4096: the workgroup forms, k > 4096: the host), every k of the sweep, and k = 10^9 as a
    batch of one; rows_for_range on the returned ranges."""
    sel = np.arange(len(main.pool))
    for k in K_POOL:
        run_batch(main, sel, k, monkeypatch)
    run_single(main, (10 ** 9,), monkeypatch, batch1=True)
    check_rows_for_range(main, (1, 64, 5000))


def test_main_batches_4095_4096(main, monkeypatch):
    """Q = 4095 (every range through the workgroup forms) and 4096 (lanes, waves for k <= 64, handoffs, workgroups)"""
    for Q in (4095, 4096):
        sel = tiled(main, Q, Q)
        for k in (1, 2, 4, 5, 63, 64, 65, 256, 1536, 1537, 4096):
            run_batch(main, sel, k, monkeypatch)


def test_main_switches(main, monkeypatch):
    """the same batch with the wave form off, the lanes off, the ring off, on the host, and with one wave workgroup per CU"""
    sel = tiled(main, 4096, 1)
    for env in ({"SA_HIP_ROWS_WAVES": "0"}, {"SA_HIP_ROWS_LANES": "0"}, {"SA_HIP_ROWS_RING": "0"}, {"SA_HIP_HOST_ROWS": "1"}):
        for k in (1, 5, 64, 65, 1537, 4096):
            run_batch(main, sel, k, monkeypatch, env)
    for k in (2, 13, 64):
        run_batch(main, sel, k, monkeypatch, {"SA_HIP_ROWS_WAVE_GROUPS": "1"})


def test_main_ring_batches(main, monkeypatch):
    """Batches whose Q x k ids reach the pinned ring: k <= 64 at Q = 140 001 (lanes, waves walking several ranges each,
    handoffs; pieces that end inside the batch), k = 4096 at Q = 2049 (the large table, several queries per workgroup), the
    same without the ring"""
    sel = tiled(main, 140_001, 2)
    for k in (60, 64):
        run_batch(main, sel, k, monkeypatch)
    run_batch(main, sel, 64, monkeypatch, {"SA_HIP_ROWS_WAVE_GROUPS": "1"})
    run_batch(main, sel, 64, monkeypatch, {"SA_HIP_ROWS_RING": "0"})
    sel = tiled(main, 2049, 3)
    run_batch(main, sel, 4096, monkeypatch)
    run_batch(main, sel, 4096, monkeypatch, {"SA_HIP_ROWS_RING": "0"})


def test_main_single_queries(main, gpu, oracle, monkeypatch):
    """ONE query: the fused search + rows kernel (k <= 1536), the search + rows launches (k > 1536; SA_HIP_SECTOR_SEARCH=1 for
    every k), the host (k > 4096)"""
    run_single(main, (0, 1, 2, 64, 65, 1536, 1537, 4096, 4097, 10 ** 9), monkeypatch)
    monkeypatch.setenv("SA_HIP_SECTOR_SEARCH", "1")   # read when the index is created
    try:
        other = RowCase(gpu, oracle, cases.rows_main_case(), "main_sector1")
    finally:
        monkeypatch.delenv("SA_HIP_SECTOR_SEARCH")
    try:
        run_single(other, (1, 64, 1536), monkeypatch, sector=1)
    finally:
        other.close()


def test_main_zero_length_rows(main, monkeypatch):
    """the same text under a row table with zero-length rows (the last row of several at one offset holds the hit)"""
    main.set_table(cases.zero_length_rows(main.starts), "rows_zero_len")
    try:
        env = {"zero_len": "1"}
        run_batch(main, np.arange(len(main.pool)), 1536, monkeypatch, env)
        sel = tiled(main, 4096, 4)
        for k in (1, 5, 64, 1536, 4096):
            run_batch(main, sel, k, monkeypatch, env)
        run_single(main, (1, 64, 4096), monkeypatch, env)
    finally:
        main.set_table(main.starts0, "rows70001")


@pytest.mark.parametrize("num_rows", (1, 255, 256, 257, 512, 513))
def test_small_row_tables(gpu, oracle, num_rows, monkeypatch):
    """Row tables of 1 .. 513 rows: the coarse table is off up to 256 rows and its last block is short or full above; k past
    the rows is clamped"""
    case = RowCase(gpu, oracle, cases.rows_small_case(num_rows), "rows%d" % num_rows)
    try:
        sel = np.arange(len(case.pool))
        for k in (0, 1, 2, 4, 5, 64, 65, 256, 257, 600, 4096, 4097):
            run_batch(case, sel, k, monkeypatch)
        run_batch(case, sel, 600, monkeypatch, {"SA_HIP_HOST_ROWS": "1"})
        big = tiled(case, 4096, num_rows)
        for k in (1, 5, 64, 65, 600):
            run_batch(case, big, k, monkeypatch)
        run_single(case, (1, 64, 300, 4096, 10 ** 9), monkeypatch)
        if num_rows in (257, 513):
            case.set_table(cases.zero_length_rows(case.starts), "rows_zero_len")
            for k in (1, 64, 600):
                run_batch(case, big, k, monkeypatch, {"zero_len": "1"})
            run_single(case, (1, 600), monkeypatch, {"zero_len": "1"})
    finally:
        case.close()


def test_ring_with_k_clamped_to_the_rows(gpu, oracle, monkeypatch):
    """k = 4000 / 4096 asked of a 3000-row table with Q = 2800: the device walks with k = 3000 and the ring widens into the
    caller's rows of k_in ids each (csrc/sa_capi.hip: the piece callback's output stride)"""
    case = RowCase(gpu, oracle, cases.rows_small_case(3000), "rows3000")
    try:
        sel = tiled(case, 2800, 5)
        for k in (4000, 4096):
            run_batch(case, sel, k, monkeypatch)
        run_batch(case, sel, 4000, monkeypatch, {"SA_HIP_ROWS_RING": "0"})
        assert ("wg_large", "ring_clamped") in COVER
    finally:
        case.close()


def test_query_records_batch_slices(gpu):
    """SuffixArray(documents=...).query_records_batch at k = 4096 over ~9000 live patterns (empty strings and mixed case among
    them): slices of ROWS_BUDGET / k = 4096 patterns, the last one shorter (no lanes); against query_records per pattern and a
    lower-case scan of the documents -- equal sets up to k matching rows, a k-row subset beyond"""
    from suffixarray_amd import SuffixArray
    from suffixarray_amd.suffix_array import ROWS_BUDGET
    rng = np.random.default_rng(21)
    vocab = ["alpha", "Beta", "gamma", "DELTA", "milk", "Store", "fox", "lazy", "quick", "brown", "zeta", "eta", "omega", "x"]
    docs = [" ".join(vocab[j] for j in rng.integers(0, len(vocab), rng.integers(1, 7))) + " #%d" % i for i in range(6000)]
    low = [d.lower() for d in docs]
    pool = sorted(set(vocab + [v.upper() for v in vocab] + ["e", "A", " ", "#1", "#59", "#5999 ", "qqzz", "ALPHA beta", "a #"]
                      + [docs[i][2:8] for i in rng.integers(0, len(docs), 120)] + [docs[i].swapcase() for i in rng.integers(0, len(docs), 40)]))
    live = 9003
    k = 4096
    pats = [pool[i] for i in rng.integers(0, len(pool), live)]
    for j in rng.integers(0, live, 300):
        pats.insert(int(j), "")
    s = SuffixArray(documents=docs, max_suffix_length=64)
    try:
        per = ROWS_BUDGET // k
        assert per == 4096 and live > 2 * per and 0 < live % per < LANE_MIN_BATCH
        got = s.query_records_batch(pats, k=k)
        assert len(got) == len(pats)
        one = {p: s.query_records(p, k=k) for p in pool}
        for p in pool:
            exp = {d for d, l in zip(docs, low) if p.lower() in l}
            g = one[p]
            assert len(g) == len(set(g)) == min(k, len(exp)) and set(g) <= exp, p
            if len(exp) <= k:
                assert set(g) == exp, p
        assert any(len(one[p]) == k for p in pool) and any(0 < len(one[p]) < k for p in pool)
        for p, r in zip(pats, got):
            assert r == ([] if p == "" else one[p]), p
        COVER.add(("class", "slices"))
    finally:
        s.close()


# (form, cell) pairs the sweep above must fill; forms as launch_rows picks them (record() above), cells as _cells names them
_H = ["h0_end", "h0_mid", "h0_wrap", "h1", "h2", "h3", "h4", "h5", "h6", "h63", "h64", "h65", "h255", "h256", "h257", "h4095",
      "h4096", "h4097", "h20000+"]
_D = ["d<k", "d=k", "d=k+1", "d>=k+256", "one_row"]
_TABLES = ["rows1", "rows255", "rows256", "rows257", "rows512", "rows513", "rows70001", "zero_len"]
REQUIRED = {
    "lane": _H[:7] + ["d<k", "d=k", "d=k+1", "one_row", "k1", "k2", "k4", "k5", "k64", "k65", "k1536", "k4096", "Q4096", "ring",
                      "Q140001", "sentinel", "rows70001", "zero_len"],
    "wave": _H[7:] + _D + ["k1", "k2", "k4", "k5", "k63", "k64", "table_max", "mid_chunk", "reuse", "reuse_groups1", "ring",
                           "Q4096", "Q140001", "sentinel", "zero_len"],
    "handoff": ["h4097", "h20000+", "one_row", "d<k", "d>=k+256", "k2", "k5", "k64", "ring", "Q4096"],
    "wg_small": _H + _D + ["k1", "k2", "k4", "k5", "k63", "k64", "k65", "k256", "k1536", "table_max", "mid_chunk", "reuse",
                           "Q4095", "Q4096", "k>rows", "sentinel"] + _TABLES,
    "wg_large": _H + _D + ["k1537", "k4000", "k4096", "table_max", "reuse", "ring", "ring_clamped", "k>rows", "Q4095", "Q4096",
                           "sentinel", "zero_len"],
    "fused": _H + _D + ["k1", "k64", "k1536", "k>rows", "table_max", "mid_chunk"] + _TABLES,
    "unfused": ["h0_end", "h0_mid", "h0_wrap", "h1", "h5", "h4097", "h20000+", "d<k", "d=k", "d=k+1", "d>=k+256", "one_row",
                "k1", "k64", "k1536", "k1537", "k4096", "table_max", "zero_len"],
    "host": ["h0_end", "h0_mid", "h0_wrap", "h1", "h20000+", "d<k", "d=k", "one_row", "k1", "k4097", "k1e9", "k>rows",
             "sentinel", "rows_for_range"],
    "none": ["k0"],
    "class": ["slices"],
}


def test_rows_coverage_matrix():
    """After the sweep: every (form x boundary) cell was filled -- a change of launch_rows' predicates, of a threshold or of a
    generator cannot quietly empty one."""
    assert COVER, "run the whole module: the matrix is filled by the sweep"
    for f in sorted(REQUIRED):
        print("%-9s %s" % (f, " ".join(sorted(c for g, c in COVER if g == f))))
    missing = [(f, c) for f, cells in REQUIRED.items() for c in cells if (f, c) not in COVER]
    assert not missing, missing
