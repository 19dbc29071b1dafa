"""The claims of tests/query_cases.py, checked without a GPU: the constants the model restates are the sources'; the model's
ranges equal the oracle's for every pattern it traces, under every mode; every edge a case claims is reached by one of its
patterns, measured from the traces (the edge-by-case matrix is printed); every deliberate mistake changes the range of a pattern
of the case that claims its edge.  The device test (tests/test_gpu_query_edges.py) asks the same sets, unthinned."""
import copy
import os
import re
import time

import numpy as np
import pytest

import query_cases as qc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "suffixarray_amd", "csrc")
MATRIX = {}      # (claim, item) -> {column: reached}
_state = {}         # case -> seconds
_kept = {}          # (case, L, deep) -> (Index, sets, expected): what the mistake tests need again


def test_restated_constants_are_the_sources():
    for fname, rx, value in qc.SOURCE_CONSTANTS:
        src = open(os.path.join(CSRC, fname)).read()
        m = re.findall(rx, src)
        assert len(m) == 1 and m[0] == value, (fname, rx, m)
    assert (qc.SKEY_STRIDE, qc.QC_DIGIT_BITS, qc.QC_TILE, qc.K2_AUTO_BATCH, qc.CLUSTER_MIN, qc.GRID_CAP) == (64, 11, 4096, 32768, 1 << 20, 4096)
    assert [qc.window_slots(kb, m) for kb in (8, 4) for m in (2, 1)] == [4, 8, 8, 16]
    assert [qc.k2n_of(b) for b in (1, 4, 5, 7, 8)] == [16, 16, 12, 9, 8]


def _combos(case, L):
    """(mode, deep keys) the model runs a case under: both window widths with the deep keys (wide) at every L; without them, and
    the plain bisection, at L = 0"""
    if case.key_bytes == 4:
        return [(2, False), (1, False), (0, False)]
    out = [(2, True), (1, True)]
    if case.claims == ("samples_last",):      # (the samples exist only with the deep keys)
        return out + [(0, True)]
    if case.partial:                            # (2^22 slots: the plan differs from words_wide's only where the deep keys are used)
        return out + [(0, True)]
    if L == 0:
        out += [(2, False), (1, False), (0, True), (0, False)]
    return out


def _expected(oracle, t, sa, L, sets):
    """the oracle's ranges of every set; the ranges every_bound read off the sorted array are checked against them (on every
    pattern the CPU test keeps: a thinned set is the sample)"""
    out = []
    for name, pats, short in sets:
        exp = oracle.query_batch(t, sa, L if L else 0xFFFFFFFF, qc.as_packed(pats))
        if short is not None:
            assert np.array_equal(exp["first"], short[0]) and np.array_equal(exp["second"], short[1]), "every_bound's read-off ranges differ from the oracle: " + name
        out.append(exp)
    return out


@pytest.mark.parametrize("cid", [c.id for c in qc.CASES])
def test_model_equals_oracle_and_claims_are_met(oracle, cid):
    case = qc.CASE_BY_ID[cid]
    t0 = time.time()
    errors, missing, pool = [], [], {}
    for L in case.Ls:
        t, sa = qc.text_and_array(oracle, case, case.n_cpu, L)
        k0 = qc.effective_k0(case, L)
        ixs = {deep: qc.Index(t, sa, L, k0, case.dbits, case.key_bytes, case.partial, deep) for deep in {d for _, d in _combos(case, L)}}
        sets = qc.pattern_sets(case, ixs[min(ixs)], cpu=True)
        exps = _expected(oracle, t, sa, L, sets)
        lists = [qc.as_list(p) for _, p, _ in sets]
        for deep, ix in ixs.items():
            if any((cid, L, deep) == (m[0], m[1], m[3]) for m in qc.MISTAKES.values()):
                _kept[(cid, L, deep)] = (ix, sets, exps)
        hits_beyond_L = 0
        for mode, deep in _combos(case, L):
            ix, traces = ixs[deep], []
            for (name, _, _), pats, exp in zip(sets, lists, exps):
                ef, es = exp["first"].tolist(), exp["second"].tolist()
                for i, p in enumerate(pats):
                    f, s, tr = qc.query_model(ix, p, mode)
                    traces.append(tr)
                    if (f, s) != (ef[i], es[i]) and len(errors) < 10:
                        errors.append("L %d mode %d deep %s %s %r: model (%d, %d), oracle (%d, %d); %s" % (L, mode, deep, name, p[:40], f, s, ef[i], es[i], qc.describe(tr)))
                    if L and len(p) > L and ef[i] != qc.NONE:
                        hits_beyond_L += 1
            pool.setdefault((mode, deep), []).extend(traces)
        if case.key_bytes == 4:      # UNREACHABLE["t_hi1_not_widened"]: the bisection with h_strict (mode 0, and every span) answers the same without it
            for (name, _, _), pats, exp in zip(sets, lists, exps):
                ef, es = exp["first"].tolist(), exp["second"].tolist()
                for i, p in enumerate(pats):
                    f, s, _tr = qc.query_model(ixs[False], p, 0, mistake="t_hi1_not_widened")
                    assert (f, s) == (ef[i], es[i]), (name, p)
        if L and "truncated" in case.claims:
            MATRIX.setdefault(("truncated", "L = %d: patterns longer than L are hits" % L), {})[case.id] = hits_beyond_L > 0
            if not hits_beyond_L:
                missing.append("%s: truncated L = %d" % (case.id, L))
    for (mode, deep), traces in sorted(pool.items()):
        if mode == 0:
            continue
        W = qc.window_slots(case.key_bytes, mode)
        col = "%s m%d%s" % (case.id, mode, "+deep" if deep else "")
        for claim in case.claims:
            name, _, only = claim.partition(":")
            items = qc.CLAIMS[name](traces, W, deep)
            assert not only or set(only.split("|")) <= set(items) or not items, (claim, sorted(items))
            for item, reached in items.items():
                if only and item not in only.split("|"):
                    continue
                MATRIX.setdefault((name, item), {})[col] = reached
                if not reached and (name, item) not in qc.ANY_COLUMN:
                    missing.append("%s: %s / %s" % (col, name, item))
    _state[cid] = time.time() - t0
    print("%s: %.1f s" % (cid, _state[cid]))
    assert not errors, "\n".join(errors)
    assert not missing, "claims no pattern reaches:\n" + "\n".join(missing)


def test_query_trace_over_given_arrays(oracle):
    """query_trace -- the model over K, dir, K2 and S handed in one by one, as read back from a device -- answers and traces as
    query_model does over its own Index"""
    case = qc.CASE_BY_ID["far2_wide"]
    t, sa = qc.text_and_array(oracle, case, case.n_cpu, 0)
    ix = qc.Index(t, sa, 0, case.k0, case.dbits, case.key_bytes, case.partial, True)
    pats = [p for _, ps, _ in qc.pattern_sets(case, ix, cpu=True) for p in qc.as_list(ps)]
    exp = oracle.query_batch(t, sa, 0xFFFFFFFF, pats)
    for mode in (2, 1, 0):
        for i, p in enumerate(pats):
            got = qc.query_trace(t, sa, ix.code, ix.b, ix.k0, ix.dbits, ix.key_bytes, ix.lo_shift, 0, mode, ix.K, ix.dir, p, K2=ix.K2, S=ix.S, k2n=ix.k2n)
            assert got[:2] == (int(exp["first"][i]), int(exp["second"][i])) and got == qc.query_model(ix, p, mode), (mode, p)


def test_edge_by_case_matrix():
    """prints which edge was reached by which case, window width and deep-key state, for the cases that ran before it in this
    process (every claim is asserted in the case's own test; run alone, this one has nothing to print)"""
    for (claim, item) in sorted(MATRIX):
        cols = MATRIX[(claim, item)]
        print("%-14s %-52s %s" % (claim, item, "  ".join("%s%s" % ("" if v else "MISSING ", c) for c, v in sorted(cols.items()))))
    for key, cols in MATRIX.items():
        assert all(cols.values()) or (key in qc.ANY_COLUMN and any(cols.values())), (key, cols)


@pytest.mark.parametrize("name", sorted(qc.MISTAKES))
def test_every_mistake_is_caught(oracle, name):
    cid, L, modes, deep, _ = qc.MISTAKES[name]
    case = qc.CASE_BY_ID[cid]
    if (cid, L, deep) in _kept:
        good, sets, exps = _kept[(cid, L, deep)]
    else:
        t, sa = qc.text_and_array(oracle, case, case.n_cpu, L)
        good = qc.Index(t, sa, L, qc.effective_k0(case, L), case.dbits, case.key_bytes, case.partial, deep)
        sets = qc.pattern_sets(case, good, cpu=True)
        exps = _expected(oracle, good.t, good.sa, L, sets)
    ix = good
    if name == "k2_group_by_stored_key":
        ix = copy.copy(good)
        ix.K2, ix.tied = qc.k2_keys(good.t, good.sa, good.code_arr, good.b, good.k0, good.k2n, L, stored=good.K)
    for mode in modes:
        caught = None
        for (sname, pats, _), exp in zip(sets, exps):
            ef, es = exp["first"].tolist(), exp["second"].tolist()
            for i, p in enumerate(qc.as_list(pats)):
                f, s, _tr = qc.query_model(ix, p, mode, mistake=name)
                if (f, s) != (ef[i], es[i]):
                    caught = (sname, p, (f, s), (ef[i], es[i]))
                    break
            if caught:
                break
        assert caught, "mistake %s (%s) changes no range of %s under mode %d" % (name, qc.MISTAKES[name][4], cid, mode)
        print("%s, mode %d: first caught by %s %r: (%d, %d) for (%d, %d)" % ((name, mode, caught[0], caught[1][:24]) + caught[2] + caught[3]))


def test_what_the_sets_cannot_show(oracle):
    """the mistakes that cannot change a range are named with their reason, not dropped silently -- and the model with each of
    them still answers every pattern of the window case as the oracle does"""
    assert not set(qc.UNREACHABLE) & set(qc.MISTAKES)
    case = qc.CASE_BY_ID["sized_wide"]
    t, sa = qc.text_and_array(oracle, case, case.n_cpu, 0)
    ix = qc.Index(t, sa, 0, case.k0, case.dbits, case.key_bytes, case.partial, True)
    sets = qc.pattern_sets(case, ix, cpu=True)
    exps = _expected(oracle, t, sa, 0, sets)
    ix12 = qc.Index(t, qc.text_and_array(oracle, case, case.n_cpu, 12)[1], 12, case.k0, case.dbits, case.key_bytes, case.partial, True, k2_mistake="k2_not_cut_at_L")
    sets12 = qc.pattern_sets(case, ix12, cpu=True)
    for (sname, pats, _), exp in zip(sets12, _expected(oracle, t, ix12.sa, 12, sets12)):
        ef, es = exp["first"].tolist(), exp["second"].tolist()
        for i, p in enumerate(qc.as_list(pats)):
            f, s, _tr = qc.query_model(ix12, p, 2, mistake="k2_not_cut_at_L")
            assert (f, s) == (ef[i], es[i]), ("k2_not_cut_at_L", sname, p)
    for name in ("sample_hi_plus_1", "sample_lo_minus_1", "estimate_not_clamped"):
        for (sname, pats, _), exp in zip(sets, exps):
            ef, es = exp["first"].tolist(), exp["second"].tolist()
            for i, p in enumerate(qc.as_list(pats)):
                f, s, _tr = qc.query_model(ix, p, 2, mistake=name)
                assert (f, s) == (ef[i], es[i]), (name, sname, p)
