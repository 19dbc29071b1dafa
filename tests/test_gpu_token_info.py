"""The host plumbing around the token kernels (launch stopwatches, staging buffers, the copy of written rows), on one token index
with documents and one 3-shard set over 400 random tokens of 4 symbols, in batches of 5 and of 300 contexts: the *_info calls
resolve once and keep their figures, a launch of one kind moves only that kind's figures, q follows the last launch, the staging
buffers regrow and are shared by the host forms, and the cells of a row beyond `written` keep the caller's fill.  Every answer is
compared with the CPU models of token_cases, token_next_cases, token_doc_cases, token_all_cases and token_shard_cases."""
import numpy as np
import pytest

import token_all_cases as ac
import token_cases as tc
import token_doc_cases as dc
import token_next_cases as nc
import token_shard_cases as sc

pytestmark = pytest.mark.gpu

N, CAP, FILL = 400, 4, dc.FILL
UFILL = FILL & 0xFFFFFFFF
SIZES = (5, 300)
CUTS = ((0, 150), (100, 300), (250, N))                            # the shards: overlapping pieces of the text


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _batches(tl):
    """5: no occurrence, one, about a hundred, every suffix, some.  300: windows of 1 .. 6 symbols, every 7th behind a symbol
    that does not occur"""
    return {5: [[9], tl[200:208], [1], [], [2, 3]], 300: [([9] if p % 7 == 3 else []) + tl[p:p + 1 + p % 6] for p in range(300)]}


class Case:
    """the text, its tables, the models of both batches, and the two handles"""

    def __init__(self, gpu):
        self.t = np.random.default_rng(77).integers(0, 4, N).astype(np.int32)
        self.sa = dc.model_sa(self.t).astype(np.int32)
        self.starts = dc.with_empties(N)                           # 9 entries, the documents 2, 5 and 6 hold tokens
        self.da, _ = dc.model_da_pv(self.sa, self.starts)
        self.rk, self.cl = ac.model_rk(self.da), ac.closed(self.starts, N)
        self.shards = [self.t[a:b] for a, b in CUTS]
        self.sas = [dc.model_sa(s).astype(np.int32) for s in self.shards]
        tl, sl = self.t.tolist(), self.sa.tolist()
        self.m = {}
        for q, ctx in _batches(tl).items():
            first, count = tc.model_a(self.t, self.sa, ctx)
            spans = nc.spans_a(tl, sl, ctx, 0, 0, 1)
            length, totals, sspans, sentries = sc.combine(self.shards, self.sas, ctx, 0, 0, 1)
            per = [tc.model_a(s, a, ctx) for s, a in zip(self.shards, self.sas)]
            self.m[q] = {"ctx": ctx, "first": first, "count": count, "spans": spans, "fc": [(int(s[0]), int(s[1])) for s in spans],
                         "entries": [nc.entries_a(self.t, self.sa, s) for s in spans], "length": length, "totals": totals,
                         "sspans": sspans, "sentries": sentries, "sfirst": np.array([f for f, _ in per]),
                         "scount": np.array([c for _, c in per])}
        self.ti = gpu.TokenIndex.build(self.t)
        self.ti.set_documents(self.starts)
        self.ti.prepare_doc_ranks()
        self.st = gpu.TokenShards.build(self.shards)

    def close(self):
        self.ti.close()
        self.st.close()

    # ---- what the host forms must answer ----
    def check_ranges(self, got, q):
        assert np.array_equal(got["first"], self.m[q]["first"]) and np.array_equal(got["second"], self.m[q]["count"]), q

    def check_spans(self, got, q):
        assert np.array_equal(got.view(np.uint32).reshape(-1, 4), self.m[q]["spans"]), q

    def check_next(self, got, q, cap=CAP):
        sym, cnt, heads = nc.capped(self.m[q]["entries"], cap, FILL, UFILL)
        self.check_spans(got["spans"], q)
        assert np.array_equal(got["heads"].view(np.uint32).reshape(-1, 4), heads), q
        assert np.array_equal(got["symbols"], sym) and np.array_equal(got["counts"], cnt), q           # the fill beyond written too
        return heads[:, 0]

    def check_rows(self, got, q, want, width):
        docs, offs, heads = want
        self.check_spans(got["spans"], q)
        assert np.array_equal(got["heads"].view(np.uint32).reshape(-1, width), heads), q
        assert np.array_equal(got["docs"], docs) and np.array_equal(got["offsets"], offs), q
        return heads[:, 0]

    def check_locate(self, got, q, cap=CAP):
        return self.check_rows(got, q, dc.locate_rows(self.sa, self.da, self.starts, self.m[q]["fc"], cap), 2)

    def check_docs(self, got, q, cap=CAP):
        return self.check_rows(got, q, dc.docs_rows(dc.docs_full(self.sa, self.da, self.starts, self.m[q]["fc"], 0), cap), 4)

    def check_set_ranges(self, got, q):
        totals, per = got
        m = self.m[q]
        assert np.array_equal(per["first"], m["sfirst"]) and np.array_equal(per["second"], m["scount"]), q
        assert totals.tolist() == m["scount"].astype(np.int64).sum(axis=0).tolist(), q

    def check_set_spans(self, got, q):
        m = self.m[q]
        assert got["length"].tolist() == m["length"] and got["totals"].tolist() == m["totals"], q
        assert np.array_equal(got["spans"].view(np.uint32).reshape(m["sspans"].shape), m["sspans"]), q

    def check_set_next(self, got, q, cap=CAP):
        m = self.m[q]
        sym, cnt, heads = sc.capped(sc.span_length(m["sspans"]), m["sentries"], sc.next_total(m["sspans"]), cap, FILL)
        assert np.array_equal(got["spans"].view(np.uint32).reshape(m["sspans"].shape), m["sspans"]), q
        assert [tuple(int(v) for v in h) for h in got["heads"].tolist()] == heads, q
        assert np.array_equal(got["symbols"], sym) and np.array_equal(got["counts"], cnt), q
        return np.array([h[0] for h in heads])


@pytest.fixture(scope="module")
def case(gpu):
    c = Case(gpu)
    yield c
    c.close()


class Kinds:
    """One device-form launch per kind of stopwatch, on buffers sized for the larger batch: name -> (launch(q), the info call that
    reports it, the keys of that info the kind owns, the key of its q).  A kind owns its q, its times, and what its *_info call
    reads back or derives for it: next the lane / wave split, docs the examined ranks, the set's next the chunk."""

    def __init__(self, case):
        import torch
        ti, st = case.ti, case.st
        self.infos = {"info": ti.info, "next_info": ti.next_info, "docs_info": ti.docs_info, "doc_ranks_info": ti.doc_ranks_info,
                      "set_info": st.info}
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda:0")
        a, b, h = i32(3 * 300, 4), i32(3 * 300, 4), i32(300, 8)
        c, h64 = torch.zeros((300, CAP), dtype=torch.int64, device="cuda:0"), torch.zeros((300, 3), dtype=torch.int64, device="cuda:0")
        self.inp, self.keep = {}, (a, b, h, c, h64)
        for q in SIZES:
            buf, off = tc.pack(case.m[q]["ctx"])
            self.inp[q] = {"pat": _dev(buf), "off": _dev(off.view(np.int64)), "spans": _dev(case.m[q]["spans"].view(np.int32)),
                           "sspans": _dev(case.m[q]["sspans"].view(np.int32)), "docs": _dev(np.tile(np.array([2, 5, 6, 0], np.int32), (q, 1))),
                           "goff": np.arange(q + 1, dtype=np.uint64)}
        p = lambda q, k: self.inp[q][k].data_ptr()
        A, B, H, C64, H64 = a.data_ptr(), b.data_ptr(), h.data_ptr(), c.data_ptr(), h64.data_ptr()
        self.kinds = {
            "ranges": (lambda q: ti.query_batch_device(p(q, "pat"), p(q, "off"), q, A), "info", {"q", "kernel_ms"}, "q"),
            "spans": (lambda q: ti.spans_batch_device(p(q, "pat"), p(q, "off"), q, 0, 0, 1, A), "next_info", {"q", "spans_ms"}, "q"),
            "next": (lambda q: ti.next_batch_device(p(q, "spans"), q, CAP, A, B, H), "next_info",
                     {"q", "next_ms", "lane_spans", "wave_spans"}, "q"),
            "locate": (lambda q: ti.locate_batch_device(p(q, "spans"), q, CAP, A, B, H), "docs_info", {"locate_q", "locate_ms"}, "locate_q"),
            "docs": (lambda q: ti.docs_batch_device(p(q, "spans"), q, CAP, 0, A, B, H), "docs_info", {"docs_q", "docs_ms", "examined"}, "docs_q"),
            "doc_counts": (lambda q: ti.doc_counts_batch_device(p(q, "spans"), q, CAP, p(q, "docs"), None, 0, A), "doc_ranks_info",
                           {"counts_q", "counts_ms"}, "counts_q"),
            "all": (lambda q: ti.all_batch_device(p(q, "spans"), q, self.inp[q]["goff"], CAP, 0, A, B, H), "doc_ranks_info",
                    {"all_q", "all_ms"}, "all_q"),
            "set_ranges": (lambda q: st.query_batch_device(p(q, "pat"), p(q, "off"), q, C64), "set_info", {"q", "ranges_ms"}, "q"),
            "set_spans": (lambda q: st.spans_batch_device(p(q, "pat"), p(q, "off"), q, 0, 0, 1, H, C64, A), "set_info", {"q", "spans_ms"}, "q"),
            "set_next": (lambda q: st.next_batch_device(p(q, "sspans"), q, CAP, B, C64, H64), "set_info",
                         {"q", "chunk", "next_ms", "merge_ms"}, "q"),
        }
        self.sync = lambda: (ti.sync(), st.sync())

    def launch(self, name, q):
        self.kinds[name][0](q)
        self.sync()

    def snapshot(self):
        return {name: call() for name, call in self.infos.items()}

    def times(self, name, snap):
        _, info, own, _ = self.kinds[name]
        return [snap[info][k] for k in sorted(own) if k.endswith("_ms")]


@pytest.fixture(scope="module")
def kinds(case):
    import torch
    k = Kinds(case)
    torch.cuda.synchronize()
    return k


def test_info_resolves_once_and_a_launch_moves_only_its_own_figures(kinds):
    for name in kinds.kinds:
        kinds.launch(name, 5)
    before = kinds.snapshot()
    assert kinds.snapshot() == before                                                                 # resolved: nothing moves
    for name, (_, info, own, qkey) in kinds.kinds.items():
        assert before[info][qkey] == 5 and all(ms > 0 for ms in kinds.times(name, before)), (name, before[info])
    for name, (_, info, own, qkey) in kinds.kinds.items():
        kinds.launch(name, 300)
        now = kinds.snapshot()
        moved = [(i, k) for i in now for k in now[i] if now[i][k] != before[i][k]]
        assert all(i == info and k in own for i, k in moved), (name, moved)
        assert now[info][qkey] == 300 and all(ms > 0 for ms in kinds.times(name, now)), (name, now[info])
        assert kinds.snapshot() == now, name
        before = now


def test_q_follows_the_last_launch(kinds):
    for name, (_, info, _, qkey) in kinds.kinds.items():
        kinds.launch(name, 300)
        kinds.launch(name, 5)
        assert kinds.infos[info]()[qkey] == 5, name
    kinds.launch("spans", 300)                                                                        # next_info: whichever came last
    kinds.launch("next", 5)
    got = kinds.infos["next_info"]()
    assert got["q"] == 5 and got["lane_spans"] + got["wave_spans"] == 5, got
    kinds.launch("spans", 300)
    got = kinds.infos["next_info"]()
    assert got["q"] == 300 and got["lane_spans"] + got["wave_spans"] == 5, got                        # ... the split stays the next launch's


def test_staging_regrows_and_is_shared_by_the_host_forms(gpu, case):
    ctx = {q: case.m[q]["ctx"] for q in SIZES}
    with gpu.TokenIndex.build(case.t) as ti:                                                          # fresh: nothing staged yet
        ti.set_documents(case.starts)
        case.check_ranges(ti.query_batch(ctx[5]), 5)
        case.check_spans(ti.spans_batch(ctx[300]), 300)
        case.check_ranges(ti.query_batch(ctx[300]), 300)
        case.check_next(ti.next_batch(ctx[5], cap=CAP, fill=FILL), 5)
        case.check_locate(ti.locate_batch(ctx[300], cap=CAP, fill=FILL), 300)
        case.check_docs(ti.docs_batch(ctx[5], cap=CAP, fill=FILL), 5)
    with gpu.TokenShards.build(case.shards) as st:
        case.check_set_ranges(st.query_batch(ctx[5]), 5)
        case.check_set_spans(st.spans_batch(ctx[300]), 300)
        case.check_set_ranges(st.query_batch(ctx[300]), 300)
        case.check_set_next(st.next_batch(ctx[5], cap=CAP, fill=FILL), 5)
        case.check_set_next(st.next_batch(ctx[300], cap=CAP, fill=FILL), 300)
        case.check_set_spans(st.spans_batch(ctx[5]), 5)


def _row_kinds(written, cap):
    w = np.asarray(written)
    return {"none": bool((w == 0).any()), "some": bool(((w > 0) & (w < cap)).any()), "full": bool((w == cap).any())}


def test_cells_beyond_written_keep_the_fill(case):
    """cap = 4 throughout.  The text has 4 symbols and 3 documents that hold tokens, so a row of next symbols or of hits can fill
    4 cells, a row of documents at most 3: docs_batch and all_batch run at cap = 3 as well, where a row can be full."""
    ti, st = case.ti, case.st
    ctx = case.m[5]["ctx"]
    all3 = {"none": True, "some": True, "full": True}
    assert _row_kinds(case.check_next(ti.next_batch(ctx, cap=CAP, fill=FILL), 5), CAP) == all3
    assert _row_kinds(case.check_locate(ti.locate_batch(ctx, cap=CAP, fill=FILL), 5), CAP) == all3
    assert _row_kinds(case.check_set_next(st.next_batch(ctx, cap=CAP, fill=FILL), 5), CAP) == all3
    assert _row_kinds(case.check_docs(ti.docs_batch(ctx, cap=CAP, fill=FILL), 5), CAP) == {"none": True, "some": True, "full": False}
    assert _row_kinds(case.check_docs(ti.docs_batch(ctx, cap=3, fill=FILL), 5, 3), 3) == all3
    groups = [[0], [1], [2], [1, 2], [4, 3]]                                                          # indexes into ctx
    goff = np.cumsum([0] + [len(g) for g in groups]).astype(np.uint64)
    flat = [ctx[i] for g in groups for i in g]
    sgroups = [[case.m[5]["fc"][i] for i in g] for g in groups]
    full = [ac.all_a(ac.all_walk(case.sa, case.da, case.cl, N, g), ac.group_first(N, g), 0) for g in sgroups]
    for cap, kinds_of_row in ((CAP, {"none": True, "some": True, "full": False}), (3, all3)):
        docs, offs, heads = ac.all_rows(full, cap)
        got = ti.all_batch(flat, goff, cap=cap, fill=FILL)
        assert np.array_equal(got["heads"].view(np.uint32).reshape(-1, 8), heads), cap
        assert np.array_equal(got["docs"], docs) and np.array_equal(got["offsets"], offs), cap
        assert _row_kinds(heads[:, 0], cap) == kinds_of_row, cap
    # doc_counts_batch: the caller's rows of 0, 2 and cap document ids; foreign ids and ids of empty documents among them
    ids = np.tile(np.array([2, 6, -1, 5], np.int32), (5, 1))
    written = np.array([0, 2, CAP, 2, CAP + 3], np.uint32)                                            # (beyond cap: clamped)
    got = ti.doc_counts_batch(ctx, ids, written, fill=FILL)
    want = ac.counts_rows(case.rk, case.cl, N, case.m[5]["fc"], ids, written)
    case.check_spans(got["spans"], 5)
    assert np.array_equal(got["counts"], want) and (want[0] == UFILL).all() and (want[1, 2:] == UFILL).all() and (want[2:] != UFILL).any()
