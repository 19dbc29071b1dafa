"""Matching statistics on the device against the two CPU models of token_match_cases.py: every text and batch under the four
plans (key array and directory on or off) for every max_length and min_length, byte-identical across plans; every match against
what spans_batch answers in mode 0 for it, and one symbol more; cap and min_length around a document's planted matches; the device
chain against the host form; positions before the first document; what match_info follows; the Python class."""
import numpy as np
import pytest

import token_match_cases as mc

pytestmark = pytest.mark.gpu

FILL = -7                                                         # cells a launch must not write keep it
U32 = FILL & 0xFFFFFFFF
CAP = 8


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


_HEADS = {}                                                       # (text, batch, max_length, min_length) -> (heads_a, heads_b)
_SEEN = {}                                                        # (text, batch, max_length, min_length) -> the bytes of the first plan


def _heads(name, batch, M, mlen):
    key = (name, batch, M, mlen)
    if key not in _HEADS:
        e = mc.expected(name)
        lengths = e["spans"][batch, M][:, 2]
        _HEADS[key] = (mc.heads_a(lengths, e["batches"][batch], mlen), mc.heads_b(lengths, e["batches"][batch], mlen))
    return _HEADS[key]


def _check(got, spans, ha, cap, where):
    """a host-form answer against the spans and heads of the models"""
    sp = got["spans"].view(np.uint32).reshape(-1, 4)
    bad = np.flatnonzero((sp != spans).any(axis=1))
    assert bad.size == 0, (where, bad[:5], sp[bad[:5]].tolist(), spans[bad[:5]].tolist())
    pos, outs, hd = mc.rows([f for f, _ in ha], [h for _, h in ha], spans, cap, FILL)
    assert np.array_equal(got["heads"].view(np.uint32).reshape(-1, 4), hd), (where, got["heads"][:5], hd[:5])
    if cap:
        assert np.array_equal(got["positions"], pos), (where, "positions")
        assert np.array_equal(got["out_spans"].view(np.uint32).reshape(len(ha), cap, 4), outs), (where, "out_spans")


@pytest.mark.parametrize("plan", list(mc.PLANS))
def test_every_text_and_batch_under_every_plan(gpu, monkeypatch, plan):
    mc.set_plan(monkeypatch, plan)
    for name in mc.TEXTS:
        e, b = mc.expected(name), mc.expected_b(name)
        with gpu.TokenIndex.build(e["t"]) as ti:
            for batch, docs in e["batches"].items():
                packed = mc.pack(docs)
                for M in mc.MAX_LENGTHS:
                    spans = e["spans"][batch, M]
                    for mlen in mc.MIN_LENGTHS:
                        where = (plan, name, batch, M, mlen)
                        ha, hb = _heads(name, batch, M, mlen)
                        got = ti.match_docs_batch(packed, min_length=mlen, max_length=M, cap=CAP, fill=FILL)
                        _check(got, spans, ha, CAP, where)                                          # model A: exactly
                        g = got["spans"]                                                            # model B: counts, lengths, heads
                        mine = np.stack([g["count"], g["length"], g["ended"]], axis=1).astype(np.int64)
                        assert np.array_equal(mine, b[batch, M]), where
                        assert [(int(h["maximal"]), int(h["longest"]), int(h["covered"])) for h in got["heads"]] == [h for _, h in hb], where
                        w = got["heads"]["written"]
                        assert [got["positions"][d, :w[d]].tolist() for d in range(len(docs))] == [[p for p, _ in f][:CAP] for f, _ in hb], where
                        blob = b"".join(got[k].tobytes() for k in ("spans", "positions", "out_spans", "heads"))
                        assert _SEEN.setdefault((name, batch, M, mlen), blob) == blob, (where, "differs from the first plan")
                    assert np.array_equal(ti.match_batch(packed, max_length=M), got["spans"]), (plan, name, batch, M)


@pytest.mark.parametrize("name", ["n2", "all_equal", "rand_k2", "zero_and_max", "planted"])
def test_every_match_is_the_mode0_span_of_its_prefix(gpu, monkeypatch, name):
    mc.set_plan(monkeypatch, "default")
    e = mc.expected(name)
    n = len(e["t"])
    with gpu.TokenIndex.build(e["t"]) as ti:
        for batch in ("windows", "tails", "odd_tokens", "doc_sizes", "total257"):
            docs = e["batches"][batch]
            flat = [(doc, j) for doc in docs for j in range(len(doc))]
            for M in mc.MAX_LENGTHS:
                sp = ti.match_batch(docs, max_length=M)
                assert sp.size == len(flat)
                same = ti.spans_batch([doc[j:j + int(L)] for (doc, j), L in zip(flat, sp["length"])], mode=0)
                assert np.array_equal(same, sp), (name, batch, M)
                if M == 0:                                          # one symbol more, where the document has one, occurs nowhere
                    more = [doc[j:j + int(L) + 1] for (doc, j), L in zip(flat, sp["length"]) if j + int(L) < len(doc)]
                    assert len(more) > 0 and (ti.spans_batch(more, mode=0)["count"] == 0).all(), (name, batch)
                else:
                    assert (sp["length"] <= min(M, n)).all()


def _planted_doc(tl, lengths, rng):
    """windows of the text of the given lengths, every one closed by NONE: one maximal match per window, of exactly its length
    (a window of a text over 1000 random symbols is not continued by NONE, and what lies inside a window ends where it ends)"""
    doc = []
    for m in lengths:
        p = int(rng.integers(0, len(tl) - m))
        doc += tl[p:p + m] + [mc.NONE]
    return doc


def test_cap_and_min_length_at_the_planted_lengths(gpu, monkeypatch):
    mc.set_plan(monkeypatch, "default")
    e = mc.expected("rand_k1000")
    tl, sl = [int(v) for v in e["t"]], [int(v) for v in e["sa"]]
    rng = np.random.default_rng(41)
    planted = (5, 9, 9, 17, 33, 9, 70)
    docs = [_planted_doc(tl, planted, rng), [mc.NONE] * 4, _planted_doc(tl, planted[::-1], rng), []]
    spans = mc.spans_a(tl, sl, docs, 0)
    with gpu.TokenIndex.build(e["t"]) as ti:
        for mlen in (1, 4, 5, 6, 8, 9, 10, 16, 17, 18, 32, 33, 34, 69, 70, 71):
            ha = mc.heads_a(spans[:, 2], docs, mlen)
            assert ha == mc.heads_b(spans[:, 2], docs, mlen)
            m = sum(L >= mlen for L in planted)                     # the planted windows of at least mlen, and nothing else
            assert [h[0] for _, h in ha] == [m, 0, m, 0], (mlen, ha)
            assert [h[2] for _, h in ha] == [sum(L for L in planted if L >= mlen), 0, sum(L for L in planted if L >= mlen), 0]
            for cap in sorted({max(m - 1, 0), m, m + 1, 0, 1}):
                got = ti.match_docs_batch(docs, min_length=mlen, cap=cap, fill=FILL)
                _check(got, spans, ha, cap, (mlen, cap))
                assert got["heads"]["written"].tolist() == [min(m, cap), 0, min(m, cap), 0] and got["heads"]["longest"].tolist() == [70, 0, 70, 0]
                if cap:                                             # the guard pattern beyond written
                    for d, w in enumerate(got["heads"]["written"]):
                        assert (got["positions"][d, w:] == U32).all() and (got["out_spans"].view(np.uint32).reshape(4, cap, 4)[d, w:] == U32).all(), (mlen, cap, d)


def test_the_device_chain_and_positions_before_the_first_document(gpu, monkeypatch):
    import torch
    mc.set_plan(monkeypatch, "default")
    e = mc.expected("zero_and_max")
    kept = []
    with gpu.TokenIndex.build(e["t"]) as ti:
        assert ti.match_batch([]).size == 0 and ti.match_docs_batch([], cap=3)["positions"].shape == (0, 3)          # Q == 0
        empty = ti.match_docs_batch([[], []], cap=3, fill=FILL)                                                    # no position at all
        assert empty["spans"].size == 0 and not empty["heads"].view(np.uint32).any() and (empty["positions"] == U32).all()
        for batch, front, M, mlen, cap in (("carried", 0, 0, 8, 4), ("doc_sizes", 5, 7, 2, 8), ("q4", 0, 0, 1, 2), ("total257", 3, 3, 3, 0),
                                           ("empty_docs", 2, 0, 1, 3), ("whole", 0, 0, 8, 64)):
            docs = e["batches"][batch]
            buf, off = mc.pack(docs, front)
            q, total = len(docs), int(off[-1])
            host = ti.match_docs_batch((buf, off), min_length=mlen, max_length=M, cap=cap, fill=FILL)
            assert host["spans"].size == total and not host["spans"][:front].view(np.uint32).any(), (batch, "positions before offsets[0]")
            assert np.array_equal(host["spans"][front:].view(np.uint32).reshape(-1, 4), e["spans"][batch, M]), batch
            ha = _heads("zero_and_max", batch, M, mlen)[0]
            assert np.array_equal(host["heads"].view(np.uint32).reshape(-1, 4), mc.rows([f for f, _ in ha], [h for _, h in ha], e["spans"][batch, M], cap, FILL)[2])
            # the device chain: match -> docs with no host trip, and a second launch pair before the one sync
            pd, od = _dev(buf), _dev(off.view(np.int64))
            outs = []
            for rep in range(2):
                outs.append((torch.full((total, 4), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((q, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((q, max(cap, 1), 4), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((q, 4), FILL, dtype=torch.int32, device="cuda:0")))
            torch.cuda.synchronize()
            for sp_d, ps_d, os_d, hd_d in outs:
                ti.match_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, sp_d.data_ptr())
                ti.match_docs_batch_device(sp_d.data_ptr(), od.data_ptr(), q, mlen, cap, ps_d.data_ptr() if cap else None,
                                           os_d.data_ptr() if cap else None, hd_d.data_ptr())
            ti.sync()
            for sp_d, ps_d, os_d, hd_d in outs:
                assert sp_d.cpu().numpy().tobytes() == host["spans"].tobytes(), batch
                assert hd_d.cpu().numpy().tobytes() == host["heads"].tobytes(), batch
                if cap:
                    assert ps_d.cpu().numpy().tobytes() == host["positions"].tobytes(), batch
                    assert os_d.cpu().numpy().tobytes() == host["out_spans"].tobytes(), batch
                else:                                               # cap == 0 touches neither array
                    assert (ps_d.cpu().numpy() == FILL).all() and (os_d.cpu().numpy() == FILL).all(), batch
            info = ti.match_info()
            assert info["q"] == q and info["positions"] == total and info["match_ms"] > 0 and info["docs_ms"] > 0, info
            kept.append((pd, od, outs))


def test_match_info_follows_the_match_launches_alone(gpu, monkeypatch):
    mc.set_plan(monkeypatch, "default")
    e = mc.expected("rand_k2")
    with gpu.TokenIndex.build(e["t"]) as ti:
        assert ti.match_info() == {"q": 0, "positions": 0, "match_ms": 0.0, "docs_ms": 0.0}
        ti.match_batch(e["batches"]["q5"])
        a = ti.match_info()
        assert a["q"] == 5 and a["positions"] == sum(len(d) for d in e["batches"]["q5"]) and a["match_ms"] > 0 and a["docs_ms"] == 0.0, a
        ti.spans_batch([[0, 1], [1]], mode=1)                       # launches of another kind move neither
        ti.next_batch([[0, 1], [1], [0]], cap=2)
        ti.query_batch([[0], [1], [1, 1], [0, 0]])
        assert ti.match_info() == a and ti.next_info()["q"] == 3
        ti.match_docs_batch(e["batches"]["q3"], min_length=2, cap=0)
        b = ti.match_info()
        assert b["q"] == 3 and b["positions"] == sum(len(d) for d in e["batches"]["q3"]) and b["docs_ms"] > 0, b
        ti.match_batch([[], []])                                    # no position: no launch, nothing moves
        assert ti.match_info() == b


def test_python_class(gpu, monkeypatch):
    import suffixarray_amd
    mc.set_plan(monkeypatch, "default")
    with suffixarray_amd.TokenIndex([1, 0, 2, 0, 2, 0], k=3) as ti:                                      # "banana"
        (length, count, first), = ti.matching_statistics([[0, 2, 0, 2, 7, 1, 0]])
        assert length.tolist() == [4, 3, 2, 1, 0, 2, 1] and count.tolist() == [1, 1, 2, 2, 6, 1, 3] and first.tolist() == [2, 5, 1, 4, 0, 3, 0]
        assert ti.matching_statistics([[0, 2, 0, 2], []], max_length=2)[0][0].tolist() == [2, 2, 2, 1]
        assert ti.matching_statistics([[0, 2, 0, 2], []], max_length=2)[1][0].size == 0 and ti.matching_statistics([]) == []
        assert ti.matched_spans([[0, 2, 0, 2, 7, 1, 0], [7], []], 1) == [([(0, 4, 1, 2), (5, 2, 1, 3)], True), ([], True), ([], True)]
        assert ti.matched_spans([[0, 2, 0, 2, 7, 1, 0]], 1, cap=1) == [([(0, 4, 1, 2)], False)]
        assert ti.matched_spans([[0, 2, 0, 2, 7, 1, 0]], 3) == [([(0, 4, 1, 2)], True)]
        assert ti.matched_spans([[0, 2, 0, 2, 7, 1, 0]], 1, max_length=2)[0][0] == [(0, 2, 2, 1), (1, 2, 2, 4), (2, 2, 2, 1), (5, 2, 1, 3)]
        c = ti.coverage([[0, 2, 0, 2, 7, 1, 0], [7, 7], []], 3)
        assert c["covered"].tolist() == [4, 0, 0] and c["longest"].tolist() == [4, 0, 0] and c["maximal"].tolist() == [1, 0, 0]
        assert ti.coverage([[0, 2, 0, 2, 7, 1, 0]], 1)["covered"].tolist() == [6]
    e, b = mc.expected("planted"), mc.expected_b("planted")
    with suffixarray_amd.TokenIndex(e["t"]) as ti:
        for batch, M, mlen in (("doc_sizes", 0, 8), ("carried", 0, 2), ("windows", 7, 1)):
            docs = e["batches"][batch]
            hb = mc.heads_b(e["spans"][batch, M][:, 2], docs, mlen)
            ms = ti.matching_statistics(docs, max_length=M or None)
            assert np.array_equal(np.concatenate([m[0] for m in ms]), b[batch, M][:, 1]) and np.array_equal(np.concatenate([m[1] for m in ms]), b[batch, M][:, 0])
            assert np.array_equal(np.concatenate([m[2] for m in ms]), e["spans"][batch, M][:, 0])
            cov = ti.coverage(docs, mlen, max_length=M or None)
            assert [(int(x), int(y), int(z)) for x, y, z in zip(cov["maximal"], cov["longest"], cov["covered"])] == [h for _, h in hb]
            for (got, complete), (found, h) in zip(ti.matched_spans(docs, mlen, max_length=M or None, cap=3), hb):
                assert complete == (h[0] <= 3)
                assert got == [(p, *(int(v) for v in e["spans"][batch, M][j][[2, 1, 0]])) for p, j in found[:3]]
