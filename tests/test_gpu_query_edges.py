"""query_one (csrc/sa_query.hpp) asked where its stages hand over: every pattern of the sets of tests/query_cases.py -- a bound on
every slot that starts or ends a run, the misses between adjacent keys, the patterns beyond the key of every slot of every key
group -- against the oracle, per case and form on a fresh DeviceIndex (the switches are read at init), under
SA_HIP_SECTOR_SEARCH 2, 1 and 0 and with the deep keys dropped (deep_keys(0)), built on the way by a large batch, and prepared.
tests/test_query_cases_cpu.py shows from the model's traces which edge each case reaches; here nothing is thinned.  The first
differing pattern is reported with the model's trace: bucket, window walk, the stage each bound was found in.

The second half sends the batch sizes no other test sends: the line at which a batch builds the deep keys (32768), one full
tile of the clustered order and a tile of one query (threshold lowered to 4096), the default threshold of the clustered order
and the second trip of query_kernel's grid-stride loop (2^20), clustered, in the plain order and over narrow keys, with offsets
and in the fixed-length form; and the degenerate orders of the clustering passes.  The output buffer is pre-filled with a pair no
answer can be, so an entry nobody wrote shows."""
import time

import numpy as np
import pytest

import query_cases as qc

pytestmark = pytest.mark.gpu

UNWRITTEN = (0xFFFFFFFE, 0)
_memo = {}


def _cached(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _open(gpu, monkeypatch, t, sa, env, adopted, L, sector):
    for k in qc.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SA_HIP_SECTOR_SEARCH", str(sector))
    idx = gpu.DeviceIndex(t.size, 0)
    if adopted:
        idx.load(t, sa, L)
    else:
        idx.build(t, L)
    return idx


class Batch:
    """patterns on the device (uploaded once, asked many times) with the expected ranges"""

    def __init__(self, buf, off, first, second):
        import torch
        self.buf, self.off, self.q = buf, off, int(off.size - 1)
        self.first, self.second = np.asarray(first, np.uint32), np.asarray(second, np.uint32)
        self.d_pat = torch.from_numpy(np.concatenate([buf, np.zeros(64, np.uint8)])).to("cuda:0")
        self.d_off = torch.from_numpy(off.view(np.int64)).to("cuda:0")
        self.d_out = torch.empty(2 * max(self.q, 1), dtype=torch.int32, device="cuda:0")

    def pattern(self, i):
        return bytes(self.buf[int(self.off[i]):int(self.off[i + 1])])

    def ask(self, idx, fixed=0):
        import torch
        self.d_out[0::2] = -2          # 0xFFFFFFFE
        self.d_out[1::2] = 0
        torch.cuda.synchronize()
        if fixed:
            idx.query_batch_device_fixed(self.d_pat.data_ptr(), fixed, self.q, self.d_out.data_ptr())
        else:
            idx.query_batch_device(self.d_pat.data_ptr(), self.d_off.data_ptr(), self.q, self.d_out.data_ptr())
        idx.sync()
        return self.d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)[:self.q]

    def check(self, idx, what, errors, model=None, fixed=0):
        got = self.ask(idx, fixed)
        bad = np.flatnonzero((got[:, 0] != self.first) | (got[:, 1] != self.second))
        if bad.size:
            i = int(bad[0])
            p = self.pattern(i)
            g = (int(got[i, 0]), int(got[i, 1]))
            msg = "%s: pattern %d %r: device %s, oracle (%d, %d); %d of %d differ" % (what, i, p[:48], "never written" if g == UNWRITTEN else g,
                                                                                   int(self.first[i]), int(self.second[i]), bad.size, self.q)
            if model is not None:
                ix, mode = model()
                msg += "\n    model: " + qc.describe(qc.query_model(ix, p, mode)[2])
            errors.append(msg)
        return got


def _case_batches(oracle, case, t, sa, L):
    """one Batch per pattern set of the case at truncation depth L; the expected ranges from the oracle, those of every_bound
    read off the sorted array (checked against the oracle without a GPU)"""
    k0 = qc.effective_k0(case, L)
    shape = qc.Index(t, sa, L, k0, case.dbits, case.key_bytes, case.partial, False)
    out = []
    for name, pats, short in qc.pattern_sets(case, shape, cpu=False):
        buf, off = qc.as_packed(pats)
        if short is None:
            exp = oracle.query_batch(t, sa, L if L else 0xFFFFFFFF, (buf, off))
            short = (exp["first"], exp["second"])
        out.append((name, Batch(buf, off, short[0], short[1])))
    return out


def _forms(case, L):
    """(tag, extra switches, adopted, key bytes, deep-key states); every form runs under the three modes, at every L of the case.
    Wide-key forms run the three deep-key states on one handle in turn; narrow keys have none."""
    states = ("off", "auto", "prepared")
    if case.key_bytes == 4:
        return [("built", {}, False, 4, ("auto",)), ("narrow_k=0", {"SA_HIP_NARROW_K": "0"}, False, 8, states), ("adopted", {}, True, 8, states)]
    if case.partial:      # the plan exists only as a build
        return [("built", {}, False, 8, states)]
    return [("built", {}, False, 8, states), ("adopted", {}, True, 8, states)]


MODES = (2, 1, 0)


@pytest.mark.parametrize("cid", [c.id for c in qc.CASES])
def test_every_bound_of_the_case(gpu, oracle, monkeypatch, cid):
    """verify(), then every pattern of the case against the oracle: per form, window width and deep-key state"""
    case = qc.CASE_BY_ID[cid]
    errors, t0, asked = [], time.time(), 0
    for L in case.Ls:
        t, sa = qc.text_and_array(oracle, case, case.n, L)
        k0 = qc.effective_k0(case, L)
        batches = _case_batches(oracle, case, t, sa, L)
        for tag, extra, adopted, kb, states in _forms(case, L):
            for mode in MODES:
                who = "%s/%s/L%d/mode%d" % (cid, tag, L, mode)
                idx = _open(gpu, monkeypatch, t, sa, dict(case.env, **extra), adopted, L, mode)
                try:
                    bad = idx.verify()
                    if bad:
                        errors.append("%s: verify() = %d" % (who, bad))
                    lay = idx.replica_layout()
                    got_shape = (int(lay.initial_chars), int(lay.dir_bits), int(lay.key_bytes))
                    assert got_shape == (k0, case.dbits, kb), "%s: the index has (k0, dbits, key bytes) = %s, the case says %s" % (who, got_shape, (k0, case.dbits, kb))
                    if case.partial:
                        import query_struct_cases as qs
                        st = idx.build_stats()
                        assert qs.partial_applies(int(lay.bits_per_symbol), k0, L, st["narrow48"]), (who, st)
                    for state in states:
                        if state == "off":
                            assert idx.deep_keys(0) is False
                        elif state == "prepared":
                            assert idx.prepare_deep_keys() is (kb == 8)
                        else:
                            assert idx.deep_keys(1) is False, who          # nothing built yet: large batches build them on their way
                        deep = state == "prepared"

                        def model(deep=deep):
                            return qc.Index(t, sa, L, k0, case.dbits, kb, case.partial, deep and kb == 8), mode
                        for name, b in batches:
                            b.check(idx, "%s/%s/%s" % (who, state, name), errors, model)
                            asked += b.q
                        if state == "auto":
                            # the sets of at least K2_AUTO_BATCH patterns built the deep keys on their way (wide keys), no smaller one did
                            want = kb == 8 and case.n >= 2 and any(b.q >= qc.K2_AUTO_BATCH for _, b in batches)
                            assert idx.deep_keys(1) is want, (who, want, [b.q for _, b in batches])
                finally:
                    idx.close()
    print("%s: %d patterns asked in %.1f s" % (cid, asked, time.time() - t0))
    assert not errors, "%d mismatches:\n%s" % (len(errors), "\n".join(errors[:20]))


# ---- batch sizes -----------------------------------------------------------------------------------------------------------------

def _base(oracle, cid, limit):
    """distinct patterns of a case (every set but the millions of every_bound rows of a narrow case), the oracle's answer to each"""
    case = qc.CASE_BY_ID[cid]
    t, sa = qc.text_and_array(oracle, case, case.n, 0)

    def make():
        shape = qc.Index(t, sa, 0, case.k0, case.dbits, case.key_bytes, case.partial, False)
        pats = set()
        for name, p, _ in qc.pattern_sets(case, shape, cpu=True):
            pats |= set(qc.as_list(p))
        pats = sorted(pats)
        rng = np.random.default_rng(3)
        pats = [b""] + [pats[i] for i in rng.permutation(len(pats))[:limit] if pats[i]]
        return pats, oracle.query_batch(t, sa, 0xFFFFFFFF, pats)
    return (case, t, sa) + _cached(("base", cid, limit), make)


def _repeat(pats, exp, pick):
    """the batch pats[pick[0]], pats[pick[1]], ...: expected ranges by index, the oracle answered each distinct pattern once"""
    buf, off = qc.as_packed(pats)
    off = off.astype(np.int64)
    ln = (off[1:] - off[:-1])[pick]
    new = np.zeros(pick.size + 1, np.int64)
    np.cumsum(ln, out=new[1:])
    src = np.repeat(off[:-1][pick] - new[:-1], ln) + np.arange(int(new[-1]))
    return Batch(np.ascontiguousarray(buf[src]), new.astype(np.uint64), exp["first"][pick], exp["second"][pick])


def _sizes(oracle, cid, sizes, limit=20000, seed=1):
    case, t, sa, pats, exp = _base(oracle, cid, limit)
    rng = np.random.default_rng(seed)
    return case, t, sa, [(q, _repeat(pats, exp, rng.integers(0, len(pats), q))) for q in sizes]


def test_batch_of_32768_builds_the_deep_keys(gpu, oracle, monkeypatch):
    """K2_AUTO_BATCH: 32767 patterns leave a handle in the automatic state without the deep keys, 32768 build them (wide keys);
    over narrow keys neither does"""
    errors = []
    for cid, after in (("words_wide", True), ("markov_narrow", False)):
        case, t, sa, batches = _sizes(oracle, cid, (32767, 32768))
        idx = _open(gpu, monkeypatch, t, sa, case.env, False, 0, 2)
        try:
            assert idx.deep_keys(1) is False
            batches[0][1].check(idx, cid + "/32767", errors)
            assert idx.deep_keys(1) is False, cid
            batches[1][1].check(idx, cid + "/32768", errors)
            assert idx.deep_keys(1) is after, cid
            batches[0][1].check(idx, cid + "/32767 again", errors)
        finally:
            idx.close()
    assert not errors, "\n".join(errors)


def test_clustered_order_at_the_lowered_threshold(gpu, oracle, monkeypatch):
    """SA_HIP_QCLUSTER_MIN=4096: one full tile, a full tile and a tile of one query, two tiles less one query"""
    errors = []
    case, t, sa, batches = _sizes(oracle, "words_wide", (4096, 4097, 8191, 4095))
    idx = _open(gpu, monkeypatch, t, sa, case.env, False, 0, 2)
    try:
        monkeypatch.setenv("SA_HIP_QCLUSTER_MIN", "4096")
        for q, b in batches:      # (4095: below QC_TILE, the plain order)
            b.check(idx, "words_wide/qcluster_min=4096/%d" % q, errors)
        assert idx.prepare_deep_keys()
        for q, b in batches:
            b.check(idx, "words_wide/qcluster_min=4096/prepared/%d" % q, errors)
    finally:
        idx.close()
    assert not errors, "\n".join(errors)


BIG_Q = ((1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 4097)


@pytest.mark.parametrize("form", ["clustered", "qcluster=0", "narrow"])
def test_batches_around_two_to_the_twenty(gpu, oracle, monkeypatch, form):
    """no threshold switch: the clustered order from 2^20 patterns on and the second trip of query_kernel's grid-stride loop
    (4096 blocks of 256 threads) -- clustered, in the plain order (SA_HIP_QCLUSTER=0), and over narrow keys"""
    errors = []
    cid = "markov_narrow" if form == "narrow" else "words_wide"
    case, t, sa, batches = _sizes(oracle, cid, BIG_Q)
    idx = _open(gpu, monkeypatch, t, sa, case.env, False, 0, 2)
    try:
        assert int(idx.replica_layout().key_bytes) == case.key_bytes
        if form == "qcluster=0":
            monkeypatch.setenv("SA_HIP_QCLUSTER", "0")
        for q, b in batches:
            b.check(idx, "%s/%s/%d" % (cid, form, q), errors)
    finally:
        idx.close()
    assert not errors, "\n".join(errors)


def test_fixed_length_form_beyond_two_to_the_twenty(gpu, oracle, monkeypatch):
    """query_batch_device_fixed at Q = 2^20 + 1, m = 8 and m = 3, equal to the form with offsets and to the oracle"""
    errors = []
    case = qc.CASE_BY_ID["words_wide"]
    t, sa = qc.text_and_array(oracle, case, case.n, 0)
    rng = np.random.default_rng(9)
    idx = _open(gpu, monkeypatch, t, sa, case.env, False, 0, 2)
    try:
        for m in (8, 3):
            rows = np.stack([t[p:p + m] for p in rng.integers(0, t.size - m, 4000)])
            rows[1::4] = rng.integers(97, 123, rows[1::4].shape, dtype=np.uint8)
            rows = np.unique(rows, axis=0)
            pats = [bytes(r) for r in rows]
            exp = oracle.query_batch(t, sa, 0xFFFFFFFF, pats)
            b = _repeat(pats, exp, rng.integers(0, len(pats), (1 << 20) + 1))
            fixed = b.check(idx, "words_wide/fixed m=%d" % m, errors, fixed=m)
            plain = b.check(idx, "words_wide/offsets m=%d" % m, errors)
            assert np.array_equal(fixed, plain), m
    finally:
        idx.close()
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("cid", ["equal_wide", "words_wide", "sized_wide"])
def test_degenerate_orders_of_the_clustering_passes(gpu, oracle, monkeypatch, cid):
    """Q = 8192 with the threshold lowered to 4096, at b = 1, 5 and 8: every pattern the same one (one bin takes a whole tile, rank
    4095), every pattern empty, patterns of one and two symbols only (fewer than 22 key bits), a batch already sorted and one
    sorted in reverse"""
    errors = []
    case, t, sa, pats, exp = _base(oracle, cid, 20000)
    order = np.array(sorted(range(len(pats)), key=lambda i: pats[i]))
    short = np.array([i for i in range(len(pats)) if 1 <= len(pats[i]) <= 2])
    some = next(i for i in range(len(pats)) if len(pats[i]) >= 3 and exp["first"][i] != qc.NONE)      # a hit of three bytes and more: a key other than 0
    assert pats[some] and pats[some] != pats[pats.index(b"")]
    empty = pats.index(b"")
    Q = 8192
    rng = np.random.default_rng(4)
    runs = [("identical", np.full(Q, some)), ("empty", np.full(Q, empty)), ("short", short[rng.integers(0, short.size, Q)]),
            ("sorted", np.sort(rng.integers(0, order.size, Q))), ("reverse", np.sort(rng.integers(0, order.size, Q))[::-1].copy())]
    idx = _open(gpu, monkeypatch, t, sa, case.env, False, 0, 2)
    try:
        monkeypatch.setenv("SA_HIP_QCLUSTER_MIN", "4096")
        assert {1, 5, 8} >= {int(idx.replica_layout().bits_per_symbol)}
        for name, pick in runs:
            pick = order[pick] if name in ("sorted", "reverse") else pick
            _repeat(pats, exp, np.asarray(pick, np.int64)).check(idx, "%s/%s" % (cid, name), errors)
    finally:
        idx.close()
    assert not errors, "\n".join(errors)
