"""Matching statistics over shard sets on the device against the two CPU models of token_shard_match_cases.py: every set and batch
under the four plans (key array and directory on or off), byte-identical across plans; every per-shard span against what the
shard's own handle answers, and one symbol more; a set of one shard against the single index; cap and min_length around a document's
planted matches with a guard pattern; the device chain against the host form and into the next tokens; positions before the first
document; what match_info follows; the Python class."""
import numpy as np
import pytest

import token_match_cases as mc
import token_shard_match_cases as smc

pytestmark = pytest.mark.gpu

FILL = -7                                                         # cells a launch must not write keep it
U32 = FILL & 0xFFFFFFFF
CAP = 8


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


_HEADS = {}                                                       # (set, batch, max_length, min_length) -> heads_a
_SEEN = {}                                                        # (set, batch, max_length, ...) -> the bytes of the first plan


def _heads(name, batch, M, mlen):
    key = (name, batch, M, mlen)
    if key not in _HEADS:
        e = smc.expected(name)
        _HEADS[key] = mc.heads_a(e["merged"][batch, M][:, 0], e["batches"][batch], mlen)
    return _HEADS[key]


def _check_docs(got, merged, ha, cap, where):
    """a host-form answer of the docs step against the merged rows and heads of model A, byte for byte"""
    want = smc.merged_bytes(merged)
    assert got["merged"].tobytes() == want.tobytes(), (where, np.flatnonzero(got["merged"] != want)[:5])
    pos, outs, hd = smc.rows([f for f, _ in ha], [h for _, h in ha], merged, cap, FILL)
    assert np.array_equal(got["heads"].view(np.uint32).reshape(-1, 4), hd), (where, got["heads"][:5], hd[:5])
    if cap:
        assert np.array_equal(got["positions"], pos), (where, "positions")
        assert np.array_equal(got["out_matches"].view(np.uint32).reshape(len(ha), cap, 4), outs), (where, "out_matches")


@pytest.mark.parametrize("plan", list(smc.PLANS))
def test_every_set_and_batch_under_every_plan(gpu, monkeypatch, plan):
    smc.set_plan(monkeypatch, plan)
    for name in smc.SETS:
        e, b = smc.expected(name), smc.expected_b(name)
        with gpu.TokenShards.build(e["shards"]) as st:
            for batch, docs in e["batches"].items():
                packed = mc.pack(docs)
                for k, M in enumerate(smc.MAX_LENGTHS):
                    merged, per = e["merged"][batch, M], e["per"][batch, M]
                    got_m, got_p = st.match_batch(packed, max_length=M)
                    assert got_m.tobytes() == smc.merged_bytes(merged).tobytes(), (plan, name, batch, M)              # model A: exactly
                    assert got_p.shape == per.shape[:2] and np.array_equal(np.ascontiguousarray(got_p).view(np.uint32).reshape(per.shape), per), (plan, name, batch, M)
                    length, held, count, _ = b[batch, M]                                                             # model B
                    assert np.array_equal(got_m["length"], length) and np.array_equal(got_m["shards"], held) and np.array_equal(got_m["count"], count)
                    blob = got_m.tobytes() + got_p.tobytes()
                    for mlen in (smc.MIN_LENGTHS if M == 0 else smc.MIN_LENGTHS[k % 3:k % 3 + 1]):
                        where = (plan, name, batch, M, mlen)
                        got = st.match_docs_batch(packed, min_length=mlen, max_length=M, cap=CAP, fill=FILL)
                        _check_docs(got, merged, _heads(name, batch, M, mlen), CAP, where)
                        hb = mc.heads_b(length, docs, mlen)
                        assert [(int(h["maximal"]), int(h["longest"]), int(h["covered"])) for h in got["heads"]] == [h for _, h in hb], where
                        blob += b"".join(got[x].tobytes() for x in ("positions", "out_matches", "heads"))
                    assert _SEEN.setdefault((name, batch, M), blob) == blob, (plan, name, batch, M, "differs from the first plan")


@pytest.mark.parametrize("name", ["rand_k2/3", "zero_and_max/2", "planted/3", "small_beside_long", "planted3", "mod_deal", "tiny64"])
def test_per_shard_spans_are_the_shards_own_answers(gpu, monkeypatch, name):
    smc.set_plan(monkeypatch, "default")
    e = smc.expected(name)
    S = len(e["shards"])
    with gpu.TokenShards.build(e["shards"]) as st:
        shards = [st.shard(s) for s in range(S)]
        pick = [b for b in e["batches"] if b not in ("whole", "all_empty")][:6]
        longer = 0
        for batch in pick:
            docs = e["batches"][batch]
            flat = [(doc, j) for doc in docs for j in range(len(doc))]
            for M in (0, 3) if S > 8 else smc.MAX_LENGTHS:
                merged, per = st.match_batch(docs, max_length=M)
                assert merged.size == len(flat) and per.shape == (S, len(flat))
                pref = [doc[j:j + int(L)] for (doc, j), L in zip(flat, merged["length"])]
                own = np.zeros(len(flat), np.uint32)
                for s, sh in enumerate(shards):
                    assert np.array_equal(sh.spans_batch(pref, mode=0), per[s]), (name, batch, M, s)
                    own = np.maximum(own, sh.match_batch(docs, max_length=M)["length"])
                assert np.array_equal(own, merged["length"]), (name, batch, M)
                assert np.array_equal(merged["count"], per["count"].astype(np.uint64).sum(axis=0)), (name, batch, M)
                assert np.array_equal(merged["shards"], (per["count"] > 0).sum(axis=0)), (name, batch, M)
                if M == 0:                                          # one symbol more, where the document has one, occurs in no shard
                    more = [doc[j:j + int(L) + 1] for (doc, j), L in zip(flat, merged["length"]) if j + int(L) < len(doc)]
                    assert (st.query_batch(more, per_shard=False)[0] == 0).all(), (name, batch)
                    longer += len(more)
                else:
                    assert (merged["length"] <= M).all()
        assert longer > 0, name


@pytest.mark.parametrize("text", ["rand_k2", "zero_and_max", "planted", "n1"])
def test_one_shard_answers_as_the_single_index(gpu, monkeypatch, text):
    smc.set_plan(monkeypatch, "default")
    e = mc.expected(text)
    with gpu.TokenIndex.build(e["t"]) as ti, gpu.TokenShards.build([e["t"]]) as st:
        for batch, docs in e["batches"].items():
            if batch == "whole":
                docs = [d[-mc.BODY_CAP:] for d in docs]
            for M, mlen, cap in ((0, 1, CAP), (0, 8, 2), (3, 2, CAP), (7, 1, 0)):
                one = ti.match_docs_batch(docs, min_length=mlen, max_length=M, cap=cap, fill=FILL)
                got = st.match_docs_batch(docs, min_length=mlen, max_length=M, cap=cap, fill=FILL)
                merged, per = st.match_batch(docs, max_length=M)
                where = (text, batch, M, mlen, cap)
                assert per[0].tobytes() == one["spans"].tobytes() == ti.match_batch(docs, max_length=M).tobytes(), where
                assert merged.tobytes() == got["merged"].tobytes(), where
                assert np.array_equal(merged["length"], one["spans"]["length"]) and np.array_equal(merged["count"], one["spans"]["count"]), where
                assert got["heads"].tobytes() == one["heads"].tobytes() and got["positions"].tobytes() == one["positions"].tobytes(), where
                w = got["heads"]["written"]
                for d in range(len(docs)):
                    assert np.array_equal(got["out_matches"][d, :w[d]]["length"], one["out_spans"][d, :w[d]]["length"]), where
                    assert np.array_equal(got["out_matches"][d, :w[d]]["count"], one["out_spans"][d, :w[d]]["count"]), where


def _planted_doc(tls, lengths, rng):
    """windows of the shards' texts of the given lengths, shard after shard, every one closed by NONE: one maximal match per window,
    of exactly its length (a window of a text over 1000 random symbols is not continued by NONE or elsewhere)"""
    doc = []
    for k, m in enumerate(lengths):
        tl = tls[k % len(tls)]
        p = int(rng.integers(0, len(tl) - m))
        doc += tl[p:p + m] + [mc.NONE]
    return doc


def test_cap_and_min_length_at_the_planted_lengths(gpu, monkeypatch):
    smc.set_plan(monkeypatch, "default")
    e = smc.expected("rand_k1000/3")
    tls = [[int(v) for v in t] for t in e["shards"]]
    rng = np.random.default_rng(41)
    planted = (5, 9, 9, 17, 33, 9, 70)
    docs = [_planted_doc(tls, planted, rng), [mc.NONE] * 4, _planted_doc(tls, planted[::-1], rng), []]
    merged, _ = smc.model_a(e["shards"], e["sas"], docs, 0)
    with gpu.TokenShards.build(e["shards"]) as st:
        for mlen in (1, 4, 5, 6, 8, 9, 10, 16, 17, 18, 32, 33, 34, 69, 70, 71):
            ha = mc.heads_a(merged[:, 0], docs, mlen)
            assert ha == mc.heads_b(merged[:, 0].astype(np.int64), docs, mlen)
            m = sum(L >= mlen for L in planted)                     # the planted windows of at least mlen, and nothing else
            assert [h[0] for _, h in ha] == [m, 0, m, 0], (mlen, ha)
            assert [h[2] for _, h in ha] == [sum(L for L in planted if L >= mlen), 0, sum(L for L in planted if L >= mlen), 0]
            for cap in sorted({max(m - 1, 0), m, m + 1, 0, 1}):
                got = st.match_docs_batch(docs, min_length=mlen, cap=cap, fill=FILL)
                _check_docs(got, merged, ha, cap, (mlen, cap))
                assert got["heads"]["written"].tolist() == [min(m, cap), 0, min(m, cap), 0] and got["heads"]["longest"].tolist() == [70, 0, 70, 0]
                if cap:                                             # the guard pattern beyond written
                    for d, w in enumerate(got["heads"]["written"]):
                        assert (got["positions"][d, w:] == U32).all() and (got["out_matches"].view(np.uint32).reshape(4, cap, 4)[d, w:] == U32).all(), (mlen, cap, d)


def test_the_device_chain_and_positions_before_the_first_document(gpu, monkeypatch):
    import torch
    smc.set_plan(monkeypatch, "default")
    name = "zero_and_max/2"
    e = smc.expected(name)
    S = len(e["shards"])
    kept = []
    with gpu.TokenShards.build(e["shards"]) as st:
        assert st.match_batch([])[0].size == 0 and st.match_batch([])[1].shape == (S, 0)                               # Q == 0
        assert st.match_docs_batch([], cap=3)["positions"].shape == (0, 3)
        empty = st.match_docs_batch([[], []], cap=3, fill=FILL)                                                     # no position at all
        assert empty["merged"].size == 0 and not empty["heads"].view(np.uint32).any() and (empty["positions"] == U32).all()
        for batch, front, M, mlen, cap in (("carried", 0, 0, 8, 4), ("doc_sizes", 5, 7, 2, 8), ("q4", 0, 0, 1, 2), ("total257", 3, 3, 3, 0),
                                           ("empty_docs", 2, 0, 1, 3), ("whole", 0, 0, 8, 64)):
            docs = e["batches"][batch]
            buf, off = mc.pack(docs, front)
            q, total = len(docs), int(off[-1])
            host = st.match_docs_batch((buf, off), min_length=mlen, max_length=M, cap=cap, fill=FILL)
            hm, hp = st.match_batch((buf, off), max_length=M)
            assert hm.tobytes() == host["merged"].tobytes() and hm.size == total and hp.shape == (S, total)
            assert not hm[:front].view(np.uint32).any() and not hp[:, :front].view(np.uint32).any(), (batch, "positions before offsets[0]")
            assert hm[front:].tobytes() == smc.merged_bytes(e["merged"][batch, M]).tobytes(), batch
            assert np.array_equal(np.ascontiguousarray(hp[:, front:]).view(np.uint32).reshape(S, total - front, 4), e["per"][batch, M]), batch
            ha = _heads(name, batch, M, mlen)
            assert np.array_equal(host["heads"].view(np.uint32).reshape(-1, 4), smc.rows([f for f, _ in ha], [h for _, h in ha], e["merged"][batch, M], cap, FILL)[2])
            # the device chain: match -> docs with no host trip, and a second launch pair before the one sync
            pd, od = _dev(buf), _dev(off.view(np.int64))
            outs = []
            for rep in range(2):
                outs.append((torch.full((total, 4), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((S, total, 4), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((q, max(cap, 1)), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((q, max(cap, 1), 4), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((q, 4), FILL, dtype=torch.int32, device="cuda:0")))
            torch.cuda.synchronize()
            for mg_d, pr_d, ps_d, os_d, hd_d in outs:
                st.match_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, mg_d.data_ptr(), pr_d.data_ptr())
                st.match_docs_batch_device(mg_d.data_ptr(), od.data_ptr(), q, mlen, cap, ps_d.data_ptr() if cap else None,
                                           os_d.data_ptr() if cap else None, hd_d.data_ptr())
            st.sync()
            for mg_d, pr_d, ps_d, os_d, hd_d in outs:
                assert mg_d.cpu().numpy().tobytes() == host["merged"].tobytes(), batch
                assert pr_d.cpu().numpy().tobytes() == hp.tobytes(), batch
                assert hd_d.cpu().numpy().tobytes() == host["heads"].tobytes(), batch
                if cap:
                    assert ps_d.cpu().numpy().tobytes() == host["positions"].tobytes(), batch
                    assert os_d.cpu().numpy().tobytes() == host["out_matches"].tobytes(), batch
                else:                                               # cap == 0 touches neither array
                    assert (ps_d.cpu().numpy() == FILL).all() and (os_d.cpu().numpy() == FILL).all(), batch
            info = st.match_info()
            assert info["q"] == q and info["positions"] == total and info["match_ms"] > 0 and info["docs_ms"] > 0, info
            kept.append((pd, od, outs))


def test_the_per_shard_spans_chain_into_the_next_tokens(gpu, monkeypatch):
    """the per-shard spans have the layout of the set's span output with Q = total: handed to next_batch_device they give what
    follows the longest match at every position -- next_batch in mode 0 on the matched prefixes"""
    import torch
    smc.set_plan(monkeypatch, "default")
    e = smc.expected("planted3")
    docs = e["batches"]["planted"]
    S, cap = len(e["shards"]), 4
    buf, off = mc.pack(docs)
    q, total = len(docs), int(off[-1])
    with gpu.TokenShards.build(e["shards"]) as st:
        merged, per = st.match_batch((buf, off))
        flat = [(doc, j) for doc in docs for j in range(len(doc))]
        want = st.next_batch([doc[j:j + int(L)] for (doc, j), L in zip(flat, merged["length"])], cap=cap, mode=0, fill=FILL)
        assert want["spans"].tobytes() == per.tobytes()
        pd, od = _dev(buf), _dev(off.view(np.int64))
        mg_d = torch.zeros((total, 4), dtype=torch.int32, device="cuda:0")
        pr_d = torch.zeros((S, total, 4), dtype=torch.int32, device="cuda:0")
        sy_d = torch.full((total, cap), FILL, dtype=torch.int32, device="cuda:0")
        ct_d = torch.full((total, cap), FILL, dtype=torch.int64, device="cuda:0")
        hd_d = torch.zeros((total, 3), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        st.match_batch_device(pd.data_ptr(), od.data_ptr(), q, total, 0, mg_d.data_ptr(), pr_d.data_ptr())
        st.next_batch_device(pr_d.data_ptr(), total, cap, sy_d.data_ptr(), ct_d.data_ptr(), hd_d.data_ptr())          # no host trip in between
        st.sync()
        assert sy_d.cpu().numpy().tobytes() == want["symbols"].tobytes() and ct_d.cpu().numpy().tobytes() == want["counts"].tobytes()
        assert hd_d.cpu().numpy().tobytes() == want["heads"].tobytes()
        assert np.array_equal(want["heads"]["length"], merged["length"])
        assert (want["heads"]["written"] > 0).sum() > total // 2


def test_match_info_follows_the_match_launches_alone(gpu, monkeypatch):
    smc.set_plan(monkeypatch, "default")
    e = smc.expected("rand_k2/3")
    with gpu.TokenShards.build(e["shards"]) as st:
        assert st.match_info() == {"q": 0, "positions": 0, "match_ms": 0.0, "docs_ms": 0.0}
        st.match_batch(e["batches"]["q5"])
        a = st.match_info()
        assert a["q"] == 5 and a["positions"] == sum(len(d) for d in e["batches"]["q5"]) and a["match_ms"] > 0 and a["docs_ms"] == 0.0, a
        before = st.info()
        st.spans_batch([[0, 1], [1]], mode=1)                       # launches of another kind move neither
        st.next_batch([[0, 1], [1], [0]], cap=2)
        st.query_batch([[0], [1], [1, 1], [0, 0]])
        assert st.match_info() == a and st.info()["q"] == 4 and before["q"] == 0
        st.match_docs_batch(e["batches"]["q3"], min_length=2, cap=0)
        b = st.match_info()
        assert b["q"] == 3 and b["positions"] == sum(len(d) for d in e["batches"]["q3"]) and b["docs_ms"] > 0, b
        st.match_batch([[], []])                                    # no position: no launch, nothing moves
        assert st.match_info() == b and st.info()["q"] == 4


def test_python_class(gpu, monkeypatch):
    import suffixarray_amd
    smc.set_plan(monkeypatch, "default")
    # "banana" (b = 1, a = 0, n = 2) and "nana" + 9 as two shards; the query document is "anan?ba" (? = 7 occurs nowhere)
    with suffixarray_amd.ShardedTokenIndex([[1, 0, 2, 0, 2, 0], [2, 0, 2, 0, 9]]) as sti:
        (length, count, shards), = sti.matching_statistics([[0, 2, 0, 2, 7, 1, 0]])
        assert length.dtype == np.uint32 and count.dtype == np.uint64 and shards.dtype == np.uint32
        assert length.tolist() == [4, 3, 2, 1, 0, 2, 1] and count.tolist() == [1, 2, 3, 4, 11, 1, 5] and shards.tolist() == [1, 2, 2, 2, 2, 1, 2]
        assert sti.matching_statistics([[0, 2, 0, 2], []], max_length=2)[0][0].tolist() == [2, 2, 2, 1]
        assert sti.matching_statistics([[0, 2, 0, 2], []], max_length=2)[1][0].size == 0 and sti.matching_statistics([]) == []
        assert sti.matched_spans([[0, 2, 0, 2, 7, 1, 0], [7], []], 1) == [([(0, 4, 1, 1), (5, 2, 1, 1)], True), ([], True), ([], True)]
        assert sti.matched_spans([[0, 2, 0, 2, 7, 1, 0]], 1, cap=1) == [([(0, 4, 1, 1)], False)]
        assert sti.matched_spans([[0, 2, 0, 2, 7, 1, 0]], 3) == [([(0, 4, 1, 1)], True)]
        assert sti.matched_spans([[0, 2, 0, 2, 7, 1, 0]], 1, max_length=2)[0][0] == [(0, 2, 3, 2), (1, 2, 4, 2), (2, 2, 3, 2), (5, 2, 1, 1)]
        c = sti.coverage([[0, 2, 0, 2, 7, 1, 0], [7, 7], []], 3)
        assert c["covered"].tolist() == [4, 0, 0] and c["longest"].tolist() == [4, 0, 0] and c["maximal"].tolist() == [1, 0, 0]
        assert sti.coverage([[0, 2, 0, 2, 7, 1, 0]], 1)["covered"].tolist() == [6]
    e, b = smc.expected("planted/3"), smc.expected_b("planted/3")
    with suffixarray_amd.ShardedTokenIndex(e["shards"]) as sti:
        for batch, M, mlen in (("doc_sizes", 0, 8), ("carried", 0, 2), ("windows", 7, 1)):
            docs = e["batches"][batch]
            length, held, count, _ = b[batch, M]
            hb = mc.heads_b(length, docs, mlen)
            ms = sti.matching_statistics(docs, max_length=M or None)
            assert np.array_equal(np.concatenate([m[0] for m in ms]), length) and np.array_equal(np.concatenate([m[1] for m in ms]), count)
            assert np.array_equal(np.concatenate([m[2] for m in ms]), held)
            cov = sti.coverage(docs, mlen, max_length=M or None)
            assert [(int(x), int(y), int(z)) for x, y, z in zip(cov["maximal"], cov["longest"], cov["covered"])] == [h for _, h in hb]
            for (got, complete), (found, h) in zip(sti.matched_spans(docs, mlen, max_length=M or None, cap=3), hb):
                assert complete == (h[0] <= 3)
                assert got == [(p, int(length[j]), int(count[j]), int(held[j])) for p, j in found[:3]]
