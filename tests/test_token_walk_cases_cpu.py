"""The case module of the token-walk tests without a GPU: its constants against the headers, its layout-derived expectations
against the existing CPU models (token_next_cases over the model suffix array, token_top_cases' top-k and sample models), its step
model against the run-length encoding of every layout, and the assertions that the case lists stand on the edges they name."""
import os
import re

import numpy as np
import pytest

import token_next_cases as nc
import token_top_cases as tt
import token_walk_cases as wc
from test_int_cpu import model_sa

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "suffixarray_amd", "csrc")
FILL = -7
UFILL = FILL & 0xFFFFFFFF


@pytest.mark.parametrize("fname,pattern,value", wc.HEADER_CONSTANTS)
def test_constants_are_the_headers(fname, pattern, value):
    with open(os.path.join(CSRC, fname)) as f:
        found = re.findall(pattern, f.read())
    assert found and all(x == value for x in found), (fname, pattern, found)
    assert (wc.WAVE, wc.NEXT_WAVES, wc.WAVE_GRID_MAX, wc.NEXT_JUMP_MIN, wc.NEXT_JUMP_STEPS) == (64, 4, 4096, 256, 6)
    assert (wc.NEXT_LANE_MAX, wc.DOC_UNROLL, wc.TOP_MAX, nc.LANE_MAX, tt.WINDOW) == (4, 4, 64, wc.NEXT_LANE_MAX, wc.WAVE)


def test_every_loop_over_rows_is_known():
    """the `row += waves` loops of the token kernels are the ones test_gpu_token_launch_cap.py serves: a new one fails here"""
    found = {}
    for fname in sorted(os.listdir(CSRC)):
        if fname.startswith("token_") and fname.endswith(".hpp"):
            with open(os.path.join(CSRC, fname)) as f:
                found[fname] = len(re.findall(r"\+= waves\)", f.read()))
    assert {k: v for k, v in found.items() if v} == wc.ROW_LOOPS, found


def test_layouts_are_what_they_say():
    names = [l.name for l in wc.WINDOW + wc.JUMP] + [l.name for l in wc.CAP_LAYOUTS if l.name != "ones_200"]
    assert len(set(names)) == len(names)
    for lay in wc.ALL_LAYOUTS.values():
        sym = [s for s, _ in lay.runs]
        assert sym == sorted(set(sym)) and all(0 <= s < wc.A for s in sym) and all(r >= 1 for _, r in lay.runs), lay.name
    for b in range(1, 130):
        assert wc.lengths_of(wc.ALL_LAYOUTS["two_%d" % b]) == [b, 130 - b] and wc.ALL_LAYOUTS["two_%d_ended" % b].ended
    assert wc.lengths_of(wc.MIXED)[:6] == [1, 63, 1, 64, 1, 65] and len(wc.ONES.runs) == 200
    for lead in wc.JUMP_LEADS:
        for trail in wc.JUMP_TRAILS:
            for rest in wc.JUMP_RESTS:
                lay = wc.ALL_LAYOUTS["jump_%d_%d_%d" % (lead, rest, trail)]
                m = wc.mid_run(lay)
                e = [e for e in wc.steps_of(lay)[2] if e.run == m][0]              # its first all-equal window
                assert sum(wc.lengths_of(lay)[:m]) == lead and sum(wc.lengths_of(lay)[m + 1:]) == trail, lay.name
                assert e.rest == rest + trail and e.jumped == (rest + trail > wc.NEXT_JUMP_MIN), (lay.name, e)


@pytest.mark.parametrize("length", [1, 2])
def test_expectations_are_the_existing_models(length):
    """every layout small enough: span, entries, capped rows, top-k under budgets and draws against token_next_cases /
    token_top_cases over the model suffix array"""
    ctx = wc.context(length)
    caps = {l.name: [c for x, c in wc.CAPS if x is l] for l in wc.CAP_LAYOUTS}
    budgets = {l.name: [b for x, b in wc.BUDGET if x is l] for l in wc.BUDGET_LAYOUTS}
    done = 0
    for lay in wc.ALL_LAYOUTS.values():
        if wc.total_of(lay) > wc.SMALL_MAX:
            continue
        t = wc.text(lay, length)
        sa = model_sa(t).astype(np.int32)
        span = wc.span_expected(t, ctx)
        want = nc.spans_a([int(v) for v in t], [int(v) for v in sa], [ctx], 0, 0, 1)[0].tolist()
        assert list(span) == want and span[3] == int(lay.ended), (lay.name, span, want)
        ent = wc.entries_of(t, ctx)
        model = nc.entries_a(t, sa, span)
        assert ent[0].tolist() == model[0].tolist() == [s for s, _ in lay.runs], lay.name
        assert ent[1].tolist() == model[1].tolist() == wc.lengths_of(lay), lay.name
        for cap in caps.get(lay.name, [64]):
            s, c, h = wc.next_expected(ent, cap, FILL, UFILL)
            ms, mc, mh = nc.capped([model], cap, FILL, UFILL)
            assert s.tolist() == ms[0].tolist() and c.tolist() == mc[0].tolist() and list(h) == mh[0].tolist(), (lay.name, cap)
        for budget in [0] + budgets.get(lay.name, [1, wc.total_of(lay) - 1]):
            walked = wc.entries_of(t, ctx, budget)
            mw = tt.walked_entries(t, sa, span, budget)
            assert walked[0].tolist() == mw[0].tolist() and walked[1].tolist() == mw[1].tolist(), (lay.name, budget)
            for k in wc.TOP_KS:
                s, c, h = wc.top_expected(ent, walked, k, FILL, UFILL)
                top = tt.top_of(mw, k)
                assert list(zip(s[:h[0]].tolist(), c[:h[0]].tolist())) == top and (s[h[0]:] == FILL).all() and (c[h[0]:] == UFILL).all()
                assert h == (len(top), len(mw[0]), sum(n for _, n in top), span[1] - span[3]), (lay.name, budget, k)
        ranks = wc.boundary_ranks(lay)
        s_of = np.repeat([s for s, _ in lay.runs], wc.lengths_of(lay))
        for r, d in zip(ranks, wc.draws_at(ranks, wc.total_of(lay))):
            assert 0 <= d < 2 ** 64 and tt.sample_of(t, sa, span, d) == (int(s_of[r]), span[0] + span[3] + r), (lay.name, r)
        done += 1
    assert done > 300


def test_large_expectations_are_the_layout():
    """the layouts beyond the CPU models: np.unique over the text gives the layout back, at both lengths, and so does a budget"""
    for lay in wc.JUMP_MID[::5] + wc.JUMP_LARGE:
        for length in (1, 2):
            t = wc.text(lay, length)
            ent = wc.entries_of(t, wc.context(length))
            assert ent[0].tolist() == [s for s, _ in lay.runs] and ent[1].tolist() == wc.lengths_of(lay), (lay.name, length)
            assert wc.span_expected(t, wc.context(length)) == (wc.total_of(lay), wc.total_of(lay) + lay.ended, length, int(lay.ended))
            cut = wc.entries_of(t, wc.context(length), wc.total_of(lay) - 10)
            assert int(cut[1].sum()) == wc.total_of(lay) - 10 and cut[1][0] == wc.lengths_of(lay)[0], (lay.name, length)


def test_step_model_reproduces_every_layout():
    """window steps alone, with the jump step, with the gallop in front of it, and cut to every budget of the BUDGET list"""
    for lay in wc.ALL_LAYOUTS.values():
        s = np.repeat(np.array([v for v, _ in lay.runs], np.int64), wc.lengths_of(lay))
        for jump, gallop in ((False, False), (True, False), (True, True)):
            runs, windows, events = wc.walk(s, jump, gallop)
            assert runs == list(lay.runs), (lay.name, jump, gallop)
            assert jump or not any(e.jumped for e in events)
    for lay, budget in wc.BUDGET:
        s = np.repeat(np.array([v for v, _ in lay.runs], np.int64), wc.lengths_of(lay))[:budget]
        sym, cnt = np.unique(s, return_counts=True)
        assert wc.steps_of(lay, True, budget)[0] == list(zip(sym.tolist(), cnt.tolist())), (lay.name, budget)


def test_case_lists_stand_on_their_edges():
    wc.coverage()
    d = lambda lens, gallop=False: wc.depth_of(wc.layout("x", lens), 1, gallop)
    # the pinned lengths are the smallest that reach their depth (scanned from 64^3 - 64 for the three-step ones)
    assert d((5, wc.THREE_TRAIL, 9)) == 3 and all(d((5, m, 9)) == 2 for m in range(wc.CUBE - 64, wc.THREE_TRAIL, 7)) and d((5, wc.THREE_TRAIL - 1, 9)) == 2
    assert d((5, wc.THREE_ALONE)) == 3 and d((5, wc.THREE_ALONE - 1)) == 2
    assert d((5, wc.TOP_TWO, 9), True) == 2 and d((5, wc.TOP_TWO - 1, 9), True) == 1
    assert d((5, wc.TOP_THREE, 9), True) == 3 and d((5, wc.TOP_THREE - 1, 9), True) == 2
    assert {d((5, wc.CUBE + j, 9)) for j in (-1, 0, 1)} == {2}


def test_coverage_fails_when_a_case_leaves_its_edge():
    """a JUMP middle run of rest 257 swapped for one of rest 256, and the three-step length swapped for 64^3 - 1"""
    swapped = [wc.ALL_LAYOUTS["jump_64_256_0"] if l.name == "jump_64_257_0" else l for l in wc.JUMP]
    with pytest.raises(AssertionError):
        wc.coverage(jump=swapped)
    swapped = [wc.ALL_LAYOUTS["cube_m1"] if l.name == "three_trail" else l for l in wc.JUMP]
    with pytest.raises(AssertionError):
        wc.coverage(jump=swapped)
    with pytest.raises(AssertionError):
        wc.coverage(window=[l for l in wc.WINDOW if l.name != "two_77_ended"])
    with pytest.raises(AssertionError):
        wc.coverage(caps=[(l, c) for l, c in wc.CAPS if c != len(l.runs)])
