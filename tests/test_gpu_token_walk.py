"""The walks of the token index on the device at their window, jump and budget edges (token_walk_cases.py): every layout at
length 1 (the key array's low field) and at length 2 (T[SA[r] + length]), the span from spans_batch, then next symbols under the
caps and plans, the top k under the budgets, draws one rank before, at and behind every run boundary, and the same layouts as a
shard set of one shard (tq_next_merge_kernel over one list, the one-shard path of tq_shard_top_kernel) and of three shards that
each hold a slice of every run (the merge, the merge walk and its refills).  Expected values are the layout's own; all fields are
compared, cells beyond `written` keep the fill, and the bytes are the same under every plan."""
import numpy as np
import pytest

import token_next_cases as nc
import token_walk_cases as wc

pytestmark = pytest.mark.gpu

FILL = -7
UFILL = FILL & 0xFFFFFFFF
UFILL64 = FILL & 0xFFFFFFFFFFFFFFFF
NEXT_PLANS = ("default", "lanes", "no_jump", "no_keys", "text_only")
TOP_PLANS = ("default", "no_jump", "text_only")
LARGE_PLANS = ("default", "no_jump")
CAPS_OF = {l.name: [c for x, c in wc.CAPS if x is l] for l in wc.CAP_LAYOUTS}
BUDGETS_OF = {l.name: [b for x, b in wc.BUDGET if x is l] for l in wc.BUDGET_LAYOUTS}


def _caps(lay):
    return CAPS_OF.get(lay.name, [1, 2, 64])


def _ks(lay):
    return wc.TOP_KS if lay.name in CAPS_OF else (1, 8)


def _budgets(lay):
    """0 (none), and the BUDGET list's where the layout has some; else one rank, and all but one"""
    return [0] + BUDGETS_OF.get(lay.name, [1, wc.total_of(lay) - 1])


class _Want:
    """the expectations of one layout at one length, from the text alone"""

    def __init__(self, lay, length):
        self.lay, self.length, self.ctx = lay, length, wc.context(length)
        self.t = wc.text(lay, length)
        self.span = wc.span_expected(self.t, self.ctx)
        self.entries = wc.entries_of(self.t, self.ctx)
        self.total = int(self.entries[1].sum())
        assert self.entries[1].tolist() == wc.lengths_of(lay) and self.span[3] == int(lay.ended)
        self._walked = {0: self.entries}

    def walked(self, budget):
        if budget not in self._walked:
            self._walked[budget] = wc.entries_of(self.t, self.ctx, budget)
        return self._walked[budget]


def _handles(gpu, monkeypatch, t, plans):
    """one build (the first plan); the other plans adopt its device text and suffix array, so the plan switches, which a handle
    reads when it is made, are all served by one sort"""
    nc.set_plan(monkeypatch, plans[0])
    out = {plans[0]: gpu.TokenIndex.build(t)}
    for plan in plans[1:]:
        nc.set_plan(monkeypatch, plan)
        out[plan] = gpu.TokenIndex.load_device(out[plans[0]].text_dev, out[plans[0]].sa_dev, t.size)
    nc.set_plan(monkeypatch, "default")
    return out


def _check_index(ti, w, plan, seen, next_plan, top_plan):
    where = (w.lay.name, w.length, plan)
    spans = ti.spans_batch([w.ctx], 0)
    assert spans.view(np.uint32).tolist() == list(w.span), (where, spans)
    blob = []
    if next_plan:
        for cap in _caps(w.lay):
            sym, cnt, head = wc.next_expected(w.entries, cap, FILL, UFILL)
            for got in (ti.next_batch([w.ctx], cap=cap, mode=0, fill=FILL), ti.next_of_spans(spans, cap=cap, fill=FILL)):
                assert got["heads"].view(np.uint32).tolist() == list(head), (where, cap, got["heads"], head)
                assert np.array_equal(got["symbols"][0], sym) and np.array_equal(got["counts"][0], cnt), (where, cap)
                assert got["spans"].view(np.uint32).tolist() == list(w.span), (where, cap)
                blob += [got[f].tobytes() for f in ("symbols", "counts", "heads")]
        info = ti.next_info()
        assert info["lane_spans"] + info["wave_spans"] == 1 and info["lane_spans"] == int(plan == "lanes" and w.span[1] <= wc.NEXT_LANE_MAX), (where, info)
        assert seen.setdefault(("next", w.lay.name, w.length), blob) == blob, (where, "differs from the first plan")
    if top_plan:
        blob = []
        for budget in _budgets(w.lay):
            for k in _ks(w.lay):
                sym, cnt, head = wc.top_expected(w.entries, w.walked(budget), k, FILL, UFILL)
                got = ti.top_batch([w.ctx], k=k, mode=0, budget=budget, fill=FILL)
                assert got["heads"].view(np.uint32).tolist() == list(head), (where, k, budget, got["heads"], head)
                assert np.array_equal(got["symbols"][0], sym) and np.array_equal(got["counts"][0], cnt), (where, k, budget, got["symbols"][0][:4], sym[:4])
                blob += [got[f].tobytes() for f in ("symbols", "counts", "heads")]
        assert seen.setdefault(("top", w.lay.name, w.length), blob) == blob, (where, "differs from the first plan")
        ranks = wc.boundary_ranks(w.lay)
        draws = np.array(wc.draws_at(ranks, w.total), np.uint64).reshape(1, -1)
        got = ti.sample_batch([w.ctx], draws, mode=0)
        s_of = np.repeat(w.entries[0], w.entries[1])
        assert got["symbols"][0].tolist() == s_of[ranks].tolist(), where
        assert got["ranks"][0].tolist() == [w.span[0] + w.span[3] + r for r in ranks], where


def _run_layouts(gpu, monkeypatch, layouts, length, next_plans, top_plans):
    seen = {}
    plans = list(dict.fromkeys(next_plans + top_plans))
    for lay in layouts:
        w = _Want(lay, length)
        handles = _handles(gpu, monkeypatch, w.t, plans)
        try:
            for plan in plans:
                _check_index(handles[plan], w, plan, seen, plan in next_plans, plan in top_plans)
        finally:
            for h in handles.values():
                h.close()


def _parts(layouts, n):
    return [layouts[j::n] for j in range(n)]


SMALL_GROUPS = ([("window%d" % j, p) for j, p in enumerate(_parts(wc.WINDOW, 4))] + [("caps", list(wc.CAP_LAYOUTS))] +
                [("jump%d" % j, p) for j, p in enumerate(_parts(wc.JUMP_SMALL, 2))] + [("mid%d" % j, p) for j, p in enumerate(_parts(wc.JUMP_MID, 2))])


@pytest.mark.parametrize("length", [1, 2])
@pytest.mark.parametrize("group", [g for g, _ in SMALL_GROUPS])
def test_small_layouts_under_every_plan(gpu, monkeypatch, group, length):
    _run_layouts(gpu, monkeypatch, dict(SMALL_GROUPS)[group], length, NEXT_PLANS, TOP_PLANS)


@pytest.mark.parametrize("length", [1, 2])
@pytest.mark.parametrize("name", [l.name for l in wc.JUMP_LARGE])
def test_large_layout(gpu, monkeypatch, name, length):
    """one index build; the jump step against window steps alone"""
    _run_layouts(gpu, monkeypatch, [wc.ALL_LAYOUTS[name]], length, LARGE_PLANS, LARGE_PLANS)


# ---- the same layouts as shard sets -------------------------------------------------------------------------------------------

def shard_slices(lay, S=3):
    """S layouts that each hold a slice of every run: a run of up to 600 ranks is dealt rank by rank (a run of one rank goes to
    shard j % S alone), a longer one leaves 130 and 70 ranks to the shards behind the one that keeps the rest and still jumps"""
    parts = [[] for _ in range(S)]
    for j, (s, r) in enumerate(lay.runs):
        if r > 600:
            share = [r - 200, 130, 70]
        else:
            share = [r // S + (1 if (x - j) % S < r % S else 0) for x in range(S)]
        assert sum(share) == r
        for x in range(S):
            if share[x]:
                parts[x].append((s, share[x]))
    return [wc.Layout("%s/%d" % (lay.name, x), tuple(p), lay.ended and bool(p)) for x, p in enumerate(parts)]


def _check_set(ts, w, where, shards):
    for cap in _caps(w.lay):
        sym, cnt, head = wc.next_expected(w.entries, cap, FILL, UFILL64, np.uint64)
        got = ts.next_batch([w.ctx], cap=cap, mode=0, fill=FILL)
        assert got["heads"].tolist() == [(head[0], w.length, head[1], head[2])], (where, cap, got["heads"], head)
        assert np.array_equal(got["symbols"][0], sym) and np.array_equal(got["counts"][0], cnt), (where, cap)
    for budget in _budgets(w.lay):
        for k in _ks(w.lay):
            sym, cnt, head = wc.top_expected(w.entries, w.walked(budget), k, FILL, UFILL64, np.uint64)
            got = ts.top_batch([w.ctx], k=k, mode=0, budget=budget, fill=FILL)
            assert got["heads"].tolist() == [(head[0], head[1], w.length, shards, head[2], head[3])], (where, k, budget, got["heads"], head)
            assert np.array_equal(got["symbols"][0], sym) and np.array_equal(got["counts"][0], cnt), (where, k, budget)


def _run_sets(gpu, monkeypatch, layouts, length, plans):
    for lay in layouts:
        w = _Want(lay, length)
        slices = shard_slices(lay)
        assert [sum(c) for c in zip(*[[dict(p.runs).get(s, 0) for s, _ in lay.runs] for p in slices])] == wc.lengths_of(lay)
        m = wc.mid_run(lay)
        if lay.runs[m][1] > 600:                                   # the long run: shard 0 keeps all but 200 ranks of it
            assert wc.lengths_of(slices[0])[[s for s, _ in slices[0].runs].index(lay.runs[m][0])] == lay.runs[m][1] - 200
        for plan in plans:
            nc.set_plan(monkeypatch, plan)
            with gpu.TokenShards.build([w.t]) as ts:
                _check_set(ts, w, (lay.name, length, plan, 1), 1)
            with gpu.TokenShards.build([wc.text(p, length) for p in slices]) as ts:
                _check_set(ts, w, (lay.name, length, plan, 3), sum(1 for p in slices if p.runs))


@pytest.mark.parametrize("length", [1, 2])
@pytest.mark.parametrize("group", [g for g, _ in SMALL_GROUPS])
def test_small_layouts_as_shard_sets(gpu, monkeypatch, group, length):
    _run_sets(gpu, monkeypatch, dict(SMALL_GROUPS)[group], length, ("default", "no_jump"))


@pytest.mark.parametrize("length", [1, 2])
@pytest.mark.parametrize("name", [l.name for l in wc.JUMP_LARGE])
def test_large_layout_as_shard_sets(gpu, monkeypatch, name, length):
    _run_sets(gpu, monkeypatch, [wc.ALL_LAYOUTS[name]], length, ("default",))
