"""Layouts, expectations and the step model of the token-walk tests (test_token_walk_cases_cpu.py, test_gpu_token_walk.py).

Every kernel of the token index and of the shard sets that walks a span does so one wave per row in windows of 64 ranks, with the
window step, the jump step (tq_jump_run) and -- in the top walk -- the gallop (tq_gallop_run) of csrc/token_next.hpp and
csrc/token_top.hpp.  The cases here put run boundaries, caps, budgets and run lengths on the edges of exactly that machinery.

  layout        Layout(name, runs, ended): runs is ((symbol, run length), ...) with ascending symbols; the text is [A, s_j] * r_j
                for every run and, with `ended`, one more A (token_next_cases.planted_text() is built this way).  The span of [A]
                walks the layout at length 1 (the key array's low field).  text(layout, 2) puts [A, B] in front instead: the same
                layout at length 2, the T[SA[r] + length] path of tq_next_symbol.
  expectations  from the layout and from numpy over the text alone (occurrences(): the positions where the context stands, then
                np.unique of what follows) -- never from the step model.  next_expected(): symbols, counts and (written, covered,
                total) under a cap; top_expected(): the top k by (count descending, symbol ascending) and (written, distinct,
                covered, total) under a budget, a run cut by the budget counting with what lies inside it.
  step model    walk(): a transcription of the window step, tq_jump_run and tq_gallop_run over the step function s(r).  It is
                used for ONE thing: the case lists assert with it that they reach the branch they are named for (coverage()).
                It also has to reproduce the run-length encoding of every layout, which test_token_walk_cases_cpu.py asserts.
"""
from collections import namedtuple

import numpy as np

import token_next_cases as nc

HEADER_CONSTANTS = [
    ("common.hpp", r"constexpr int WAVE = (\d+);", "64"),
    ("token_next.hpp", r"constexpr int NEXT_WAVES = (\d+);", "4"),
    ("token_next.hpp", r"constexpr u32 WAVE_GRID_MAX = (256u \* 16u);", "256u * 16u"),
    ("token_next.hpp", r"constexpr u32 NEXT_JUMP_MIN = (\d+);", "256"),
    ("token_next.hpp", r"constexpr int NEXT_JUMP_STEPS = (\d+);", "6"),
    ("token_next.hpp", r"constexpr u32 NEXT_LANE_MAX = (\d+);", "4"),
    ("token_next.hpp", r"if \(jump && hi - lo - 1 (>) NEXT_JUMP_MIN\)", ">"),
    ("token_top.hpp", r"if \(jump && end - lo - 1 (>) NEXT_JUMP_MIN\)", ">"),
    ("token_top.hpp", r"tq_jump_run\(x, lane, cur, length, lo \+ \(u32\)\((WAVE \* WAVE)\), hi\)", "WAVE * WAVE"),
    ("token_docs.hpp", r"constexpr int DOC_UNROLL = (\d+);", "4"),
    ("token_top.hpp", r"constexpr u32 TOP_MAX = (\d+);", "64"),
]
WAVE = 64
NEXT_WAVES = 4
WAVE_GRID_MAX = 256 * 16
NEXT_JUMP_MIN = 256
NEXT_JUMP_STEPS = 6
NEXT_LANE_MAX = 4
DOC_UNROLL = 4
TOP_MAX = 64

# the `for (row = ...; row < rows; row += waves)` loops per header: each is run beyond the cap by test_gpu_token_launch_cap.py
# (token_top.hpp and token_shard_top.hpp by test_gpu_token_top.py and test_gpu_token_shard_top.py)
ROW_LOOPS = {"token_next.hpp": 1, "token_top.hpp": 1, "token_docs.hpp": 1, "token_all.hpp": 1, "token_match.hpp": 1, "token_score.hpp": 1,
             "token_shards.hpp": 1, "token_shard_docs.hpp": 2, "token_shard_all.hpp": 3, "token_shard_score.hpp": 1, "token_shard_top.hpp": 1}
CAP_ROWS = NEXT_WAVES * WAVE_GRID_MAX          # rows that one trip of every wave serves

A = nc.PLANT_A                                 # the context symbol; every run symbol is below it
B = A + 1                                      # the second context symbol of the length-2 texts
CUBE = WAVE ** 3

Layout = namedtuple("Layout", "name runs ended")


def layout(name, lengths, ended=False):
    """runs of these lengths (zeros dropped) with the symbols 2, 5, 8, ..."""
    runs = tuple((3 * j + 2, int(r)) for j, r in enumerate(r for r in lengths if r))
    return Layout(name, runs, bool(ended))


def lengths_of(lay):
    return [r for _, r in lay.runs]


def total_of(lay):
    return sum(lengths_of(lay))


def text(lay, length=1):
    """the int32 text whose context ([A] or [A, B]) has the layout behind it"""
    head = [A] if length == 1 else [A, B]
    parts = [np.tile(np.array(head + [s], np.int32), r) for s, r in lay.runs]
    return np.concatenate(parts + ([np.array(head, np.int32)] if lay.ended else []) + [np.zeros(0, np.int32)])


def context(length=1):
    return [A] if length == 1 else [A, B]


def occurrences(t, ctx):
    """the text positions where ctx stands, by brute force"""
    t = np.asarray(t, np.int64)
    idx = np.arange(max(t.size - len(ctx) + 1, 0), dtype=np.int64)
    for j, v in enumerate(ctx):
        idx = idx[t[idx + j] == v]
    return idx


def span_expected(t, ctx):
    """(first, count, length, ended) of ctx in t.  Every symbol of a layout is below A < B, A stands only where the context
    starts and B only behind A, so the suffixes below the span are those that start with a run symbol."""
    t = np.asarray(t, np.int64)
    occ = occurrences(t, ctx)
    assert occ.size == int((t == A).sum())
    return int((t < A).sum()), int(occ.size), len(ctx), int(occ.size > 0 and int(occ[-1]) + len(ctx) == t.size)


def entries_of(t, ctx, budget=0):
    """(symbols, counts) behind the occurrences of ctx: np.unique over the text.  budget: only the first `budget` ranks of the span
    behind the ended suffix -- the ranks of a span are ordered by next symbol, so those are the `budget` smallest next symbols."""
    t = np.asarray(t, np.int64)
    occ = occurrences(t, ctx) + len(ctx)
    nxt = np.sort(t[occ[occ < t.size]])
    if budget:
        nxt = nxt[:budget]
    sym, cnt = np.unique(nxt, return_counts=True)
    return sym.astype(np.int64), cnt.astype(np.int64)


def next_expected(entries, cap, fill_sym, fill_cnt, count_dtype=np.uint32):
    """one row of next_batch under `cap`: symbols[cap], counts[cap] (cells beyond written keep the fills), (written, covered,
    total, 0); a shard set's counts are uint64"""
    sym, cnt = entries
    w = min(len(sym), cap)
    s = np.full(cap, fill_sym, np.int32)
    c = np.full(cap, fill_cnt, count_dtype)
    s[:w], c[:w] = sym[:w], cnt[:w]
    return s, c, (w, int(cnt[:w].sum()), int(cnt.sum()), 0)


def top_expected(entries, walked, k, fill_sym, fill_cnt, count_dtype=np.uint32):
    """one row of top_batch: `walked` are the entries within the budget, `entries` those of the whole span -> symbols[k],
    counts[k], (written, distinct, covered, total)"""
    sym, cnt = walked
    order = sorted(zip(sym.tolist(), cnt.tolist()), key=lambda p: (-p[1], p[0]))[:k]
    s = np.full(k, fill_sym, np.int32)
    c = np.full(k, fill_cnt, count_dtype)
    for j, (v, n) in enumerate(order):
        s[j], c[j] = v, n
    return s, c, (len(order), len(sym), sum(n for _, n in order), int(entries[1].sum()))


def draws_at(ranks, total):
    """the draw floor((r + 1/2) * 2^64 / total) of every rank r (relative to the span's first rank with a next symbol): it lands
    on r, as (r + 1/2) * 2^64 / total - 1 < draw means draw * total / 2^64 > r + 1/2 - total / 2^64 >= r"""
    return [(((2 * int(r) + 1) << 63) // total) for r in ranks]


def boundary_ranks(lay):
    """the ranks one before, at and after every run boundary, and the two ends"""
    total, out, j = total_of(lay), {0}, 0
    out.add(total - 1)
    for r in lengths_of(lay)[:-1]:
        j += r
        out |= {j - 1, j, j + 1}
    return sorted(r for r in out if 0 <= r < total)


# ---- the step model ----------------------------------------------------------------------------------------------------------

def _samples(s, cur, lo, hi, stride):
    q = lo + (np.arange(WAVE, dtype=np.int64) + 1) * stride
    eq = (q < hi) & (s[np.minimum(q, s.size - 1)] == cur)
    return WAVE if eq.all() else int(np.argmin(eq))                # the samples still equal


def jump_run(s, cur, lo, hi):
    """tq_jump_run -> (the last rank known to hold cur, steps taken)"""
    steps = 0
    while steps < NEXT_JUMP_STEPS and hi - lo - 1 > WAVE:
        stride = (hi - lo - 1 + WAVE - 1) // WAVE
        lead = _samples(s, cur, lo, hi, stride)
        cut = lo + (lead + 1) * stride
        if lead < WAVE and cut < hi:
            hi = cut
        lo += lead * stride
        steps += 1
    return lo, steps


def gallop_run(s, cur, lo, hi):
    """tq_gallop_run -> (rank, steps of the jump behind it, whether all 64 samples were equal)"""
    lead = _samples(s, cur, lo, hi, WAVE)
    if lead == WAVE:
        lo, steps = jump_run(s, cur, lo + WAVE * WAVE, hi)
        return lo, steps, True
    return lo + lead * WAVE, 0, False


Event = namedtuple("Event", "run rest jumped steps all_equal")    # one all-equal window: the run it lies in, the ranks behind it


def walk(s, jump=True, gallop=False):
    """the walk of one wave over the step function s (ranks behind the ended suffix; the top walk with gallop=True, cut to a
    budget by the caller) -> (runs [(symbol, count)], windows [(first rank, head lanes)], events [Event])"""
    s = np.asarray(s, np.int64)
    end, a, run_start, cur, have = int(s.size), 0, 0, 0, False
    runs, windows, events = [], [], []
    while a < end:
        nact = min(end - a, WAVE)
        seg = s[a:a + nact]
        head = np.empty(nact, bool)
        head[0] = (not have) or seg[0] != cur
        head[1:] = seg[1:] != seg[:-1]
        hl = np.flatnonzero(head)
        if hl.size == 0:
            lo, steps, alleq = a + nact - 1, 0, False
            rest = end - lo - 1
            jumped = bool(jump and rest > NEXT_JUMP_MIN)
            if jumped:
                lo, steps, alleq = gallop_run(s, cur, lo, end) if gallop else jump_run(s, cur, lo, end) + (False,)
            events.append(Event(len(runs) - 1, rest, jumped, steps, alleq))
            assert lo + 1 > a
            a = lo + 1
            continue
        if have:
            runs[-1][1] = a + int(hl[0]) - run_start
        for i, nx in zip(hl[:-1].tolist(), hl[1:].tolist()):
            runs.append([int(seg[i]), nx - i])
        last = int(hl[-1])
        runs.append([int(seg[last]), None])
        cur, run_start, have = int(seg[last]), a + last, True
        windows.append((a, tuple(hl.tolist())))
        a += nact
    if have:
        runs[-1][1] = end - run_start
    return [tuple(r) for r in runs], windows, events


def steps_of(lay, gallop=False, budget=0):
    """walk() over a layout -> (runs, windows, events)"""
    s = np.repeat(np.array([v for v, _ in lay.runs], np.int64), lengths_of(lay))
    return walk(s[:budget] if budget else s, True, gallop)


def depth_of(lay, run, gallop=False):
    """jump steps of the deepest jump inside run `run` (0: window steps only, or the gallop alone)"""
    return max([e.steps for e in steps_of(lay, gallop)[2] if e.run == run] + [0])


# ---- the case lists ----------------------------------------------------------------------------------------------------------

def _mid_for(lead, own_rest):
    """the length of a run behind `lead` ranks whose first all-equal window has own_rest of its ranks behind it: the head falls
    into window lead // 64, the next window is the first that is all the run"""
    lo = (lead // WAVE + 2) * WAVE - 1
    return own_rest + lo + 1 - lead


WINDOW = ([layout("two_%d" % b, (b, 130 - b)) for b in range(1, 130)] +
          [layout("two_%d_ended" % b, (b, 130 - b), True) for b in range(1, 130)] +
          [layout("lane63_lane0", (63, 1, 70)), layout("lane63_lane0_ended", (63, 1, 70), True),
           layout("lane63_lane0_second", (127, 1, 70)), layout("ones_200", (1,) * 200), layout("ones_200_ended", (1,) * 200, True)])

ONES = layout("ones_200", (1,) * 200)
MIXED = layout("mixed", tuple(v for j in range(40) for v in (1, 63 + j % 5)))      # 1, 63, 1, 64, 1, 65, 1, 66, 1, 67, 1, 63, ...
CAP_LAYOUTS = (ONES, MIXED)


def caps_of(lay):
    d = len(lay.runs)
    return sorted({1, 63, 64, 65, 127, 128, 129, d - 1, d, d + 1})


CAPS = [(lay, cap) for lay in CAP_LAYOUTS for cap in caps_of(lay)]
TOP_KS = (1, 63, 64)

JUMP_LEADS = (0, 1, 63, 64, 65)
JUMP_TRAILS = (0, 1, 64, 300)
JUMP_RESTS = (255, 256, 257, 258)              # ranks of the middle run behind its first all-equal window
THREE_TRAIL = CUBE + 4337                      # the smallest middle run (behind 5 ranks, in front of 9) with three jump steps
THREE_ALONE = CUBE + 8314                      # ... with nothing behind it
TOP_TWO = 8371                                 # the smallest middle run (5, ., 9) with two jump steps behind the gallop
TOP_THREE = CUBE + 8433                        # ... with three

JUMP_SMALL = [layout("jump_%d_%d_%d" % (lead, rest, trail), (lead, _mid_for(lead, rest), trail))
              for lead in JUMP_LEADS for trail in JUMP_TRAILS for rest in JUMP_RESTS]
JUMP_MID = [layout("mid_%d_%d_%d" % (lead, mid, trail), (lead, mid, trail))
            for mid in (4095, 4096, 4097, 4159, 4160, 4161, 4162) for lead, trail in ((5, 9), (64, 0), (0, 300))]
JUMP_MID += [layout("mid_%d_%d_%d" % (lead, mid, trail), (lead, mid, trail))
             for lead, mid, trail in [(5, _mid_for(5, r), 9) for r in (4095, 4096, 4097)] + [(5, 5000, 9), (5, TOP_TWO - 1, 9), (5, TOP_TWO, 9), (5, TOP_TWO, 0)]]
JUMP_LARGE = [layout("cube_m1", (5, CUBE - 1, 9)), layout("cube", (5, CUBE, 9)), layout("cube_p1", (5, CUBE + 1, 9)),
              layout("three_trail", (5, THREE_TRAIL, 9), True), layout("three_alone", (5, THREE_ALONE)),
              layout("top_three", (5, TOP_THREE, 9))]
JUMP = JUMP_SMALL + JUMP_MID + JUMP_LARGE


def mid_run(lay):
    """the index of the longest run"""
    return int(np.argmax(lengths_of(lay)))


def budgets_of(lay):
    """budgets one rank before, at and after every run boundary, and strictly inside the longest run: behind its first window,
    around the gallop's reach, in its middle and just in front of its end"""
    total, j = total_of(lay), 0
    out = {1, total - 1, total, total + 1}
    for r in lengths_of(lay):
        j += r
        out |= {j - 1, j, j + 1}
    m = mid_run(lay)
    first, r = sum(lengths_of(lay)[:m]), lengths_of(lay)[m]
    inside = {first + 65, first + 129, first + 321, first + 322, first + 385, first + r // 2, first + r - 64, first + r - 2,
              first + WAVE * WAVE + 63, first + WAVE * WAVE + 130, first + WAVE * WAVE + 400}
    return sorted(b for b in out | {b for b in inside if first < b < first + r} if b >= 1)


BUDGET_LAYOUTS = ([l for l in JUMP_SMALL if l.name in ("jump_1_257_300", "jump_65_258_64", "jump_0_257_0")] +
                  [l for l in JUMP_MID if l.name in ("mid_5_4161_9", "mid_0_4097_300")] +
                  [l for l in JUMP_LARGE if l.name in ("three_trail", "top_three")])
BUDGET = [(lay, b) for lay in BUDGET_LAYOUTS for b in budgets_of(lay)]

ALL_LAYOUTS = {l.name: l for l in WINDOW + list(CAP_LAYOUTS) + JUMP}
SMALL_MAX = 3000                               # ranks of a layout that the CPU models of token_next_cases still take


# ---- what the lists have to reach ----------------------------------------------------------------------------------------------

def coverage(window=WINDOW, caps=CAPS, jump=JUMP, budget=BUDGET):
    """asserts, from the step model and the layouts, that every list stands on the edges it is named for"""
    # WINDOW: a boundary in every lane of the first and the second window, without and with the ended suffix in front; a head in
    # lane 63 followed by one in lane 0; a window of 64 heads
    seen = {False: set(), True: set()}
    pair, full = False, False
    for lay in window:
        _, windows, _ = steps_of(lay)
        for w, (a, hl) in enumerate(windows):
            for h in hl:
                if a + h and len(lay.runs) == 2:               # the one boundary of a two-run layout: the only head of its window
                    seen[lay.ended].add((a // WAVE, h))
            if hl[-1] == WAVE - 1 and w + 1 < len(windows) and windows[w + 1][1][0] == 0 and windows[w + 1][0] == a + WAVE:
                pair = True
            full |= len(hl) == WAVE
    want = {(w, h) for w in (0, 1) for h in range(WAVE)} - {(0, 0)}
    assert want <= seen[False] and want <= seen[True], (sorted(want - seen[False]), sorted(want - seen[True]))
    assert pair and full
    # CAPS: the entry behind the last written one (the `over` ballot) inside a window of 64 heads, in its lane 0 and in its lane
    # 63; a cap at, one below and one above the number of runs
    over = set()
    for lay, cap in caps:
        _, windows, _ = steps_of(lay)
        heads = [(a, h, len(hl)) for a, hl in windows for h in hl]
        d = len(lay.runs)
        over.add("none" if cap >= d else ("lane0" if heads[cap][1] == 0 else "lane63" if heads[cap][1] == WAVE - 1 else "inside") +
                 ("_full" if heads[cap][2] == WAVE else ""))
        assert len(heads) == d
    assert {"none", "lane0_full", "lane63_full", "inside_full", "inside"} <= over, over
    for lay in {l for l, _ in caps}:
        d = len(lay.runs)
        assert {d - 1, d, d + 1} <= {c for l, c in caps if l is lay}
    # JUMP: the threshold from both sides for every leading run, with nothing and with one rank behind the run; every depth 0..3
    # of the next walk with and without a trailing run, the third from its first length; the gallop's two branches and the depths
    # 0..3 behind it; a stride that does not divide the rest
    edge = {}
    depth_next, depth_top, gallops, ragged, first3 = set(), set(), set(), False, set()
    for lay in jump:
        m = mid_run(lay)
        lens = lengths_of(lay)
        lead, trail = sum(lens[:m]), sum(lens[m + 1:])
        runs, _, events = steps_of(lay)
        assert [c for _, c in runs] == lens
        mine = [e for e in events if e.run == m]
        if mine:
            e = mine[0]
            assert e.jumped == (e.rest > NEXT_JUMP_MIN)
            edge.setdefault((lead, trail), set()).add((e.rest, e.jumped))
            deepest = max(x.steps for x in mine)
            depth_next.add((deepest, trail > 0))
            if deepest == 3:                                       # on the edge: one rank less takes two steps
                lens[m] -= 1
                first3.add((trail > 0, depth_of(layout("x", lens), mid_run(layout("x", lens))) == 2))
            ragged |= e.jumped and e.rest % WAVE != 0
        top = [e for e in steps_of(lay, gallop=True)[2] if e.run == m and e.jumped]
        for e in top:
            gallops.add(e.all_equal)
            if e.all_equal:
                depth_top.add((e.steps, trail > 0))
    for lead in JUMP_LEADS:
        for trail in (0, 1):
            assert {(NEXT_JUMP_MIN, False), (NEXT_JUMP_MIN + 1, True)} <= edge.get((lead, trail), set()), (lead, trail, edge.get((lead, trail)))
    assert {(d, t) for d in range(4) for t in (False, True)} <= depth_next, sorted(depth_next)
    assert {(False, True), (True, True)} <= first3, sorted(first3)
    assert gallops == {False, True} and {(d, True) for d in range(4)} <= depth_top and ragged, (gallops, sorted(depth_top), ragged)
    # BUDGET: one before, at and after every run boundary of its layouts, and ends strictly inside the run the jump step skips
    for lay in {l for l, _ in budget}:
        mine = {b for l, b in budget if l is lay}
        lens = lengths_of(lay)
        edges = np.cumsum(lens).tolist()
        assert {b for j in edges for b in (j - 1, j, j + 1) if b >= 1} <= mine, lay.name
        m = mid_run(lay)
        first = sum(lens[:m])
        assert any(e.run == m and e.jumped for e in steps_of(lay, gallop=True)[2]), lay.name
        assert sum(first + WAVE < b < first + lens[m] - 1 for b in mine) >= 3, lay.name
