"""Infinity-gram scores over shard sets on the device against the two CPU models of token_shard_score_cases.py: every set and batch
under the four plans (key array and directory on or off) for every max_length, with and without the merged matching statistics,
byte-identical between the two ways and across plans; every per-shard span against what the shard's own handle answers in mode 0 for
the context with the token, and length and context_count against the set's own spans_batch in mode 1; a set of one shard against the
single index; the device chain match -> score -> docs against the host form and into the next tokens and the located hits of the
set; positions before the first document; the heads against a NumPy reduction; what score_info follows; the Python class; a set of
empty shards."""
import numpy as np
import pytest

import token_score_cases as sc
import token_shard_score_cases as ssc

pytestmark = pytest.mark.gpu

FILL = -7                                                         # cells a launch must not write keep it


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _chain(st, capi, buf, off, q, total, M):
    """match -> score (with the merged records) -> docs, and score without them, on device buffers, one sync behind all launches.
    -> (scores with, per-shard with, scores without, per-shard without, heads)"""
    import torch
    S = st.shards
    pd, od = _dev(buf), _dev(off.view(np.int64))
    rows = max(total, 1)
    mg = torch.full((rows, 4), FILL, dtype=torch.int32, device="cuda:0")
    mp = torch.full((S, rows, 4), FILL, dtype=torch.int32, device="cuda:0")
    s1, s2 = (torch.full((rows, 6), FILL, dtype=torch.int32, device="cuda:0") for _ in range(2))
    p1, p2 = (torch.full((S, rows, 4), FILL, dtype=torch.int32, device="cuda:0") for _ in range(2))
    hd = torch.full((q, 6), FILL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st.match_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, mg.data_ptr(), mp.data_ptr())
    st.score_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, mg.data_ptr(), s1.data_ptr(), p1.data_ptr())
    st.score_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, None, s2.data_ptr(), p2.data_ptr())
    st.score_docs_batch_device(s1.data_ptr(), od.data_ptr(), q, hd.data_ptr())
    st.sync()
    cut = lambda s: s.cpu().numpy()[:total].view(capi.SHARDS_SCORE_DTYPE).reshape(-1)
    per = lambda p: np.ascontiguousarray(p.cpu().numpy()[:, :total]).view(capi.SPAN_DTYPE).reshape(S, total)
    return cut(s1), per(p1), cut(s2), per(p2), hd.cpu().numpy().view(capi.SCORE_HEAD_DTYPE).reshape(-1)


def _heads_rows(h):
    return np.stack([h[k].astype(np.uint64) for k in ("scored", "seen", "certain", "longest", "length_sum")], axis=1)


def _words(per):
    return np.ascontiguousarray(per).view(np.uint32).reshape(per.shape + (4,))


_SEEN = {}                                                        # (set, batch, max_length) -> the bytes of the first plan


@pytest.mark.parametrize("plan", list(ssc.PLANS))
def test_every_set_and_batch_under_every_plan_both_ways(gpu, monkeypatch, plan):
    ssc.set_plan(monkeypatch, plan)
    for name in ssc.SETS:
        e, b = ssc.expected(name), ssc.expected_b(name)
        with gpu.TokenShards.build(e["shards"]) as st:
            for batch, docs in e["batches"].items():
                buf, off = ssc.pack(docs)
                q, total = len(docs), int(off[-1])
                for M in ssc.MAX_LENGTHS:
                    where = (plan, name, batch, M)
                    want, want_per = e["scores"][batch, M], e["per"][batch, M]
                    s1, p1, s2, p2, hd = _chain(st, gpu, buf, off, q, total, M)
                    assert s1.tobytes() == s2.tobytes() and p1.tobytes() == p2.tobytes(), (where, "with and without the matching statistics")
                    bad = np.flatnonzero(s1 != ssc.score_bytes(want))
                    assert bad.size == 0, (where, bad[:5], s1[bad[:5]].tolist(), want[bad[:5]].tolist())                  # model A: exactly
                    assert np.array_equal(_words(p1), want_per), (where, np.argwhere(_words(p1) != want_per)[:5].tolist())
                    length, held, cc, tc, per_tc = b[batch, M]                                                           # model B
                    assert np.array_equal(s1["length"], length) and np.array_equal(s1["shards"], held), where
                    assert np.array_equal(s1["context_count"], cc) and np.array_equal(s1["token_count"], tc) and np.array_equal(p1["count"], per_tc), where
                    assert np.array_equal(_heads_rows(hd), ssc.heads_of(want, docs)), (where, hd[:5])
                    host = st.score_batch((buf, off), max_length=M)
                    assert host["scores"].tobytes() == s1.tobytes() and host["per_shard"].tobytes() == p1.tobytes(), (where, "host form")
                    assert host["heads"].tobytes() == hd.tobytes(), (where, "host form")
                    blob = s1.tobytes() + p1.tobytes() + hd.tobytes()
                    assert _SEEN.setdefault((name, batch, M), blob) == blob, (where, "differs from the first plan")


@pytest.mark.parametrize("name", ["rand_k2/3", "zero_and_max/2", "planted/3", "small_beside_long", "planted3", "mod_deal", "tiny64"] + list(ssc.HAND))
def test_every_record_against_the_existing_entry_points(gpu, monkeypatch, name):
    ssc.set_plan(monkeypatch, "default")
    e = ssc.expected(name)
    S = len(e["shards"])
    with gpu.TokenShards.build(e["shards"]) as st:
        shards = [st.shard(s) for s in range(S)]
        pick = [b for b in e["batches"] if b not in ("whole", "all_empty")][:6]
        for batch in pick:
            docs = e["batches"][batch]
            flat = [(doc, k) for doc in docs for k in range(len(doc))]
            for M in (0, 3) if S > 8 else ssc.MAX_LENGTHS:
                where = (name, batch, M)
                r = st.score_batch(docs, max_length=M, heads=False)
                s, per = r["scores"], r["per_shard"]
                assert s.size == len(flat) and per.shape == (S, len(flat))
                # the context: the longest suffix of what the cap and the document's start leave that some shard holds with a token behind it
                ctx = st.spans_batch([doc[k - min(k, M or k):k] for doc, k in flat], mode=1, need_next=True)
                assert np.array_equal(ctx["length"], s["length"]) and np.array_equal(ctx["totals"], s["context_count"]), where
                # the context with the token: every shard's own answer in mode 0, also where it does not hold it
                gram = [doc[k - int(L):k + 1] for (doc, k), L in zip(flat, s["length"])]
                for i, sh in enumerate(shards):
                    assert np.array_equal(sh.spans_batch(gram, mode=0), per[i]), (where, i)
                assert np.array_equal(s["token_count"], per["count"].astype(np.uint64).sum(axis=0)), where
                assert np.array_equal(s["shards"], (per["count"] > 0).sum(axis=0)), where
                assert np.array_equal(st.query_batch(gram, per_shard=False)[0], s["token_count"]), where


@pytest.mark.parametrize("text", ["rand_k2", "zero_and_max", "planted", "n1"])
def test_one_shard_answers_as_the_single_index(gpu, monkeypatch, text):
    ssc.set_plan(monkeypatch, "default")
    e = ssc.expected(text + "/1")
    (t,) = e["shards"]
    with gpu.TokenIndex.build(t) as ti, gpu.TokenShards.build([t]) as st:
        for batch, docs in e["batches"].items():
            for M in (0, 3, 7):
                one = ti.score_batch(docs, max_length=M)
                got = st.score_batch(docs, max_length=M)
                where = (text, batch, M)
                for mine, theirs in (("length", "length"), ("context_count", "context_count"), ("token_count", "token_count")):
                    assert np.array_equal(got["scores"][mine], one["scores"][theirs]), (where, mine)
                assert np.array_equal(got["per_shard"][0]["first"], one["scores"]["first"]), where
                assert np.array_equal(got["per_shard"][0]["count"], one["scores"]["token_count"]), where
                assert got["heads"].tobytes() == one["heads"].tobytes(), where


def test_the_device_chain_positions_before_the_first_document_and_score_info(gpu, monkeypatch):
    import torch
    ssc.set_plan(monkeypatch, "default")
    name = "zero_and_max/2"
    e = ssc.expected(name)
    S = len(e["shards"])
    kept = []
    with gpu.TokenShards.build(e["shards"]) as st:
        assert st.score_info() == {"q": 0, "positions": 0, "match_ms": 0.0, "score_ms": 0.0, "docs_ms": 0.0}
        r = st.score_batch([])                                                                                      # Q == 0
        assert r["scores"].size == 0 and r["heads"].size == 0 and r["per_shard"].shape == (S, 0)
        empty = st.score_batch([[], []])                                                                            # no position at all
        assert empty["scores"].size == 0 and empty["heads"].size == 2 and not _heads_rows(empty["heads"]).any()
        assert st.score_info()["positions"] == 0 and st.score_info()["q"] == 2                                      # the docs launch alone ran
        st.match_batch(e["batches"]["q5"])                                                                          # the match launches alone
        a = st.score_info()
        assert a["positions"] == 0 and a["q"] == 2 and a["match_ms"] > 0 and a["score_ms"] == 0.0, a                # ... do not move positions
        for batch, front, M in (("carried", 0, 0), ("doc_sizes", 5, 7), ("q4", 0, 0), ("total257", 3, 3), ("empty_docs", 2, 0), ("whole", 1, 2)):
            docs = e["batches"][batch]
            buf, off = ssc.pack(docs, front)
            q, total = len(docs), int(off[-1])
            host = st.score_batch((buf, off), max_length=M)
            hs, hp = host["scores"], host["per_shard"]
            assert hs.size == total and hp.shape == (S, total)
            assert not hs[:front].view(np.uint32).any() and not _words(hp[:, :front]).any(), (batch, "positions before offsets[0]")
            assert hs[front:].tobytes() == ssc.score_bytes(e["scores"][batch, M]).tobytes(), batch
            assert np.array_equal(_words(hp[:, front:]), e["per"][batch, M]), batch
            assert np.array_equal(_heads_rows(host["heads"]), ssc.heads_of(e["scores"][batch, M], docs)), batch
            only = st.score_batch((buf, off), max_length=M, scores=False, per_shard=False)                          # one output alone
            assert only["scores"] is None and only["per_shard"] is None and only["heads"].tobytes() == host["heads"].tobytes()
            only = st.score_batch((buf, off), max_length=M, heads=False, per_shard=False)
            assert only["heads"] is None and only["scores"].tobytes() == hs.tobytes()
            only = st.score_batch((buf, off), max_length=M, heads=False, scores=False)
            assert only["scores"] is None and only["per_shard"].tobytes() == hp.tobytes()
            # the device chain: match -> score -> docs with no host trip, and a second chain (without the records) before the one sync
            pd, od = _dev(buf), _dev(off.view(np.int64))
            outs = []
            for rep in range(2):
                outs.append((torch.full((total, 4), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((S, total, 4), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((total, 6), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((S, total, 4), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((q, 6), FILL, dtype=torch.int32, device="cuda:0")))
            torch.cuda.synchronize()
            for rep, (mg_d, mp_d, sc_d, pr_d, hd_d) in enumerate(outs):
                st.match_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, mg_d.data_ptr(), mp_d.data_ptr())
                st.score_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, mg_d.data_ptr() if rep == 0 else None, sc_d.data_ptr(), pr_d.data_ptr())
                st.score_docs_batch_device(sc_d.data_ptr(), od.data_ptr(), q, hd_d.data_ptr())
            st.sync()
            for mg_d, mp_d, sc_d, pr_d, hd_d in outs:
                assert sc_d.cpu().numpy().tobytes() == hs.tobytes(), batch
                assert pr_d.cpu().numpy().tobytes() == hp.tobytes(), batch
                assert hd_d.cpu().numpy().tobytes() == host["heads"].tobytes(), batch
            info = st.score_info()
            assert info["q"] == q and info["positions"] == total and info["match_ms"] > 0 and info["score_ms"] > 0 and info["docs_ms"] > 0, info
            kept.append((pd, od, outs))
        before = st.score_info()
        st.spans_batch([[0, 1], [1]], mode=1)                       # launches of another kind move none of its own
        st.next_batch([[0, 1], [1], [0]], cap=2)
        st.query_batch([[0], [1], [1, 1], [0, 0]])
        assert st.score_info() == before


def test_the_per_shard_spans_chain_into_the_next_tokens_and_the_located_hits(gpu, monkeypatch):
    """the per-shard spans have the layout of the set's span output with Q = total: handed to next_batch_device they give what
    follows the scored (L + 1)-gram, handed to locate_batch_device where it stands -- next_batch and locate_batch in mode 0 on it"""
    import torch
    ssc.set_plan(monkeypatch, "default")
    e = ssc.expected("planted3")
    docs = e["batches"]["planted"]
    S, cap = len(e["shards"]), 4
    buf, off = ssc.pack(docs)
    q, total = len(docs), int(off[-1])
    with gpu.TokenShards.build(e["shards"]) as st:
        st.set_documents([np.arange(0, len(t), 50) for t in e["shards"]])
        r = st.score_batch((buf, off), heads=False)
        flat = [(doc, k) for doc in docs for k in range(len(doc))]
        gram = [doc[k - int(L):k + 1] for (doc, k), L in zip(flat, r["scores"]["length"])]
        want = st.next_batch(gram, cap=cap, mode=0, fill=FILL)
        assert want["spans"].tobytes() == r["per_shard"].tobytes()
        where = st.locate_batch(gram, cap=cap, fill=FILL)
        assert where["spans"].tobytes() == r["per_shard"].tobytes()
        pd, od = _dev(buf), _dev(off.view(np.int64))
        mg_d = torch.zeros((total, 4), dtype=torch.int32, device="cuda:0")
        mp_d = torch.zeros((S, total, 4), dtype=torch.int32, device="cuda:0")
        sc_d = torch.zeros((total, 6), dtype=torch.int32, device="cuda:0")
        pr_d = torch.zeros((S, total, 4), dtype=torch.int32, device="cuda:0")
        sy_d = torch.full((total, cap), FILL, dtype=torch.int32, device="cuda:0")
        ct_d = torch.full((total, cap), FILL, dtype=torch.int64, device="cuda:0")
        hd_d = torch.zeros((total, 3), dtype=torch.int64, device="cuda:0")
        ld_d = torch.full((total, cap), FILL, dtype=torch.int64, device="cuda:0")
        lo_d = torch.full((total, cap), FILL, dtype=torch.int32, device="cuda:0")
        lh_d = torch.zeros((total, 2), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        st.match_batch_device(pd.data_ptr(), od.data_ptr(), q, total, 0, mg_d.data_ptr(), mp_d.data_ptr())
        st.score_batch_device(pd.data_ptr(), od.data_ptr(), q, total, 0, mg_d.data_ptr(), sc_d.data_ptr(), pr_d.data_ptr())
        st.next_batch_device(pr_d.data_ptr(), total, cap, sy_d.data_ptr(), ct_d.data_ptr(), hd_d.data_ptr())          # no host trip in between
        st.locate_batch_device(pr_d.data_ptr(), total, cap, ld_d.data_ptr(), lo_d.data_ptr(), lh_d.data_ptr())
        st.sync()
        assert sc_d.cpu().numpy().tobytes() == r["scores"].tobytes()
        assert sy_d.cpu().numpy().tobytes() == want["symbols"].tobytes() and ct_d.cpu().numpy().tobytes() == want["counts"].tobytes()
        assert hd_d.cpu().numpy().tobytes() == want["heads"].tobytes()
        assert ld_d.cpu().numpy().tobytes() == where["docs"].tobytes() and lo_d.cpu().numpy().tobytes() == where["offsets"].tobytes()
        assert lh_d.cpu().numpy().tobytes() == where["heads"].tobytes()
        assert np.array_equal(where["heads"]["count"], r["scores"]["token_count"])
        assert np.array_equal(want["heads"]["length"], r["scores"]["length"] + 1)
        assert (where["heads"]["written"] > 0).sum() > total // 2


def test_a_set_of_empty_shards(gpu, monkeypatch):
    ssc.set_plan(monkeypatch, "default")
    e = ssc.expected("n0/3")
    with gpu.TokenShards.build(e["shards"]) as st:
        docs = e["batches"]["doc_sizes"]
        r = st.score_batch(docs, max_length=0)
        assert r["scores"].size == sum(len(d) for d in docs) and not r["scores"].view(np.uint32).any() and not _words(r["per_shard"]).any()
        h = _heads_rows(r["heads"])
        assert h[:, 0].tolist() == [len(d) for d in docs] and not h[:, 1].any() and np.array_equal(h[:, 2], h[:, 0]) and not h[:, 3:].any()


def test_python_class(gpu, monkeypatch):
    import suffixarray_amd
    ssc.set_plan(monkeypatch, "default")
    with suffixarray_amd.ShardedTokenIndex([[7, 8, 9, 1, 2, 3], [1, 2, 3, 4]]) as sti:
        (length, cc, tc), = sti.infgram([[5, 1, 2, 3, 4, 6]])
        assert length.tolist() == [0, 0, 1, 2, 3, 0] and cc.tolist() == [10, 10, 2, 2, 1, 10] and tc.tolist() == [0, 2, 2, 2, 1, 0]
        assert length.dtype == np.uint32 and cc.dtype == tc.dtype == np.uint64
        p, p2, p3 = sti.infgram_probs([[5, 1, 2, 3, 4, 6], [], [1, 2]])
        assert p.dtype == np.float64 and p.tolist() == [0.0, 0.2, 1.0, 1.0, 1.0, 0.0] and p2.size == 0 and p3.tolist() == [0.2, 1.0]
        assert sti.infgram([[5, 1, 2, 3, 4, 6]], max_length=2)[0][0].tolist() == [0, 0, 1, 2, 2, 0]
        assert sti.infgram([]) == [] and sti.infgram_probs([]) == []
        s = sti.infgram_summary([[5, 1, 2, 3, 4, 6], [], [1, 2]])
        assert {k: v.tolist() for k, v in s.items()} == {"scored": [6, 0, 2], "seen": [4, 0, 2], "certain": [3, 0, 1], "longest": [3, 0, 1],
                                                        "length_sum": [6, 0, 1]}
        assert s["length_sum"].dtype == np.uint64
    for name, batch, M in (("planted/3", "doc_sizes", 0), ("rand_k2/3", "q5", 7), ("tail_of_two", "hand", 0), ("equal_shards", "hand", 3)):
        e, b = ssc.expected(name), ssc.expected_b(name)
        docs = e["batches"][batch]
        length, held, cc, tc, _ = b[batch, M]
        with suffixarray_amd.ShardedTokenIndex(e["shards"]) as sti:
            got = sti.infgram(docs, max_length=M or None)
            assert [len(g[0]) for g in got] == [len(d) for d in docs]
            for k, want in enumerate((length, cc, tc)):
                assert np.array_equal(np.concatenate([g[k] for g in got]), want), (name, k)
            pr = np.concatenate(sti.infgram_probs(docs, max_length=M or None))
            assert np.array_equal(pr, tc / cc) and (pr >= 0).all() and (pr <= 1).all(), name
            s = sti.infgram_summary(docs, max_length=M or None)
            assert np.array_equal(np.stack([s[k].astype(np.uint64) for k in ("scored", "seen", "certain", "longest", "length_sum")], axis=1),
                                  ssc.heads_of(e["scores"][batch, M], docs)), name
