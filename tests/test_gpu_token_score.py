"""Infinity-gram scores on the device against the two CPU models of token_score_cases.py: every case under the four plans (key
array and directory on or off) for every max_length, with and without the matching statistics, byte-identical between the two ways
and across plans; every record against what spans_batch answers in mode 1 for its context and in mode 0 for the context with the
token, and against next_batch where that lists every next token; the device chain match -> score -> docs against the host form;
positions before the first document; the heads against a NumPy reduction; what score_info follows; the Python class."""
import numpy as np
import pytest

import token_score_cases as sc

pytestmark = pytest.mark.gpu

FILL = -7                                                         # cells a launch must not write keep it


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _by_text():
    """the cases grouped by corpus: one index serves all of them"""
    groups = {}
    for name in sc.names():
        groups.setdefault(sc.case(name)[0].tobytes(), []).append(name)
    return list(groups.values())


def _chain(ti, capi, buf, off, q, total, M):
    """match -> score (with the matches) -> docs, and score without them, on device buffers, one sync behind all four launches.
    -> (scores with, scores without, heads) as structured arrays"""
    import torch
    pd, od = _dev(buf), _dev(off.view(np.int64))
    ms = torch.full((max(total, 1), 4), FILL, dtype=torch.int32, device="cuda:0")
    s1 = torch.full((max(total, 1), 4), FILL, dtype=torch.int32, device="cuda:0")
    s2 = torch.full((max(total, 1), 4), FILL, dtype=torch.int32, device="cuda:0")
    hd = torch.full((q, 6), FILL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ti.match_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, ms.data_ptr())
    ti.score_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, ms.data_ptr(), s1.data_ptr())
    ti.score_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, None, s2.data_ptr())
    ti.score_docs_batch_device(s1.data_ptr(), od.data_ptr(), q, hd.data_ptr())
    ti.sync()
    return (s1.cpu().numpy()[:total].view(capi.SCORE_DTYPE).reshape(-1), s2.cpu().numpy()[:total].view(capi.SCORE_DTYPE).reshape(-1),
            hd.cpu().numpy().view(capi.SCORE_HEAD_DTYPE).reshape(-1))


def _heads_rows(h):
    return np.stack([h[k].astype(np.uint64) for k in ("scored", "seen", "certain", "longest", "length_sum")], axis=1)


_SEEN = {}                                                        # (case, max_length) -> the bytes of the first plan


@pytest.mark.parametrize("plan", list(sc.PLANS))
def test_every_case_under_every_plan_both_ways(gpu, monkeypatch, plan):
    sc.set_plan(monkeypatch, plan)
    for group in _by_text():
        with gpu.TokenIndex.build(sc.case(group[0])[0]) as ti:
            for name in group:
                e, b = sc.expected(name), sc.expected_b(name)
                docs = e["docs"]
                buf, off = sc.pack(docs)
                q, total = len(docs), int(off[-1])
                for M in sc.MAX_LENGTHS:
                    where = (plan, name, M)
                    want = e["scores"][M]
                    s1, s2, hd = _chain(ti, gpu, buf, off, q, total, M)
                    assert s1.tobytes() == s2.tobytes(), (where, "with and without the matching statistics")
                    got = s1.view(np.uint32).reshape(-1, 4)
                    bad = np.flatnonzero((got != want).any(axis=1))
                    assert bad.size == 0, (where, bad[:5], got[bad[:5]].tolist(), want[bad[:5]].tolist())                 # model A: exactly
                    assert np.array_equal(got[:, :3].astype(np.int64), b[M]), where                                       # model B: the counts
                    assert np.array_equal(_heads_rows(hd), sc.heads_of(want, docs)), (where, hd[:5])
                    host = ti.score_batch((buf, off), max_length=M)
                    assert host["scores"].tobytes() == s1.tobytes() and host["heads"].tobytes() == hd.tobytes(), (where, "host form")
                    blob = s1.tobytes() + hd.tobytes()
                    assert _SEEN.setdefault((name, M), blob) == blob, (where, "differs from the first plan")


@pytest.mark.parametrize("name", ["equal20", "unique_tail", "tail_twice", "never_followed", "n2/windows", "all_equal/tails", "rand_k2/total257",
                                  "zero_and_max/odd_tokens", "planted/doc_sizes", "rand_k1000/q5"])
def test_every_record_against_the_existing_entry_points(gpu, monkeypatch, name):
    sc.set_plan(monkeypatch, "default")
    e = sc.expected(name)
    docs = e["docs"]
    flat = [(doc, k) for doc in docs for k in range(len(doc))]
    complete = 0
    with gpu.TokenIndex.build(e["t"]) as ti:
        for M in sc.MAX_LENGTHS:
            where = (name, M)
            s = ti.score_batch(docs, max_length=M, heads=False)["scores"]
            assert s.size == len(flat)
            # the context: the longest suffix of what the cap and the document's start leave that has a next token
            ctx = ti.spans_batch([doc[k - min(k, M or k):k] for doc, k in flat], mode=1, need_next=True)
            assert np.array_equal(ctx["length"], s["length"]), where
            assert np.array_equal(ctx["count"] - ctx["ended"], s["context_count"]), where
            # the context with the token: its range, also where it does not occur
            gram = ti.spans_batch([doc[k - int(L):k + 1] for (doc, k), L in zip(flat, s["length"])], mode=0)
            assert np.array_equal(gram["first"], s["first"]) and np.array_equal(gram["count"], s["token_count"]), where
            # the next tokens of the context: where all of them are listed, the token stands there with its count, or not at all
            nx = ti.next_batch([doc[k - int(L):k] for (doc, k), L in zip(flat, s["length"])], cap=64, mode=0)
            h = nx["heads"]
            assert np.array_equal(h["total"], s["context_count"]), where
            for i in np.flatnonzero(h["covered"] == h["total"]):
                doc, k = flat[i]
                w = int(h["written"][i])
                at = np.flatnonzero(nx["symbols"][i, :w] == doc[k])
                assert at.size == (1 if s["token_count"][i] else 0), (where, i)
                assert at.size == 0 or nx["counts"][i, at[0]] == s["token_count"][i], (where, i)
                complete += 1
    assert complete > 0, name


def test_the_device_chain_positions_before_the_first_document_and_score_info(gpu, monkeypatch):
    import torch
    sc.set_plan(monkeypatch, "default")
    kept = []
    with gpu.TokenIndex.build(sc.case("zero_and_max/carried")[0]) as ti:
        assert ti.score_info() == {"q": 0, "positions": 0, "match_ms": 0.0, "score_ms": 0.0, "docs_ms": 0.0}
        r = ti.score_batch([])                                                                                      # Q == 0
        assert r["scores"].size == 0 and r["heads"].size == 0
        empty = ti.score_batch([[], []])                                                                            # no position at all
        assert empty["scores"].size == 0 and empty["heads"].size == 2 and not _heads_rows(empty["heads"]).any()
        assert ti.score_info()["positions"] == 0 and ti.score_info()["q"] == 2                                      # the docs launch alone ran
        for batch, front, M in (("carried", 0, 0), ("doc_sizes", 5, 7), ("q4", 0, 0), ("total257", 3, 3), ("empty_docs", 2, 0), ("whole", 1, 2)):
            name = "zero_and_max/" + batch
            e = sc.expected(name)
            docs = e["docs"]
            buf, off = sc.pack(docs, front)
            q, total = len(docs), int(off[-1])
            host = ti.score_batch((buf, off), max_length=M)
            assert host["scores"].size == total and not host["scores"][:front].view(np.uint32).any(), (batch, "positions before offsets[0]")
            assert np.array_equal(host["scores"][front:].view(np.uint32).reshape(-1, 4), e["scores"][M]), batch
            assert np.array_equal(_heads_rows(host["heads"]), sc.heads_of(e["scores"][M], docs)), batch
            only = ti.score_batch((buf, off), max_length=M, scores=False)                                           # one output alone
            assert only["scores"] is None and only["heads"].tobytes() == host["heads"].tobytes()
            only = ti.score_batch((buf, off), max_length=M, heads=False)
            assert only["heads"] is None and only["scores"].tobytes() == host["scores"].tobytes()
            # the device chain: match -> score -> docs with no host trip, and a second chain before the one sync
            pd, od = _dev(buf), _dev(off.view(np.int64))
            outs = []
            for rep in range(2):
                outs.append((torch.full((total, 4), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((total, 4), FILL, dtype=torch.int32, device="cuda:0"),
                             torch.full((q, 6), FILL, dtype=torch.int32, device="cuda:0")))
            torch.cuda.synchronize()
            for rep, (ms_d, sc_d, hd_d) in enumerate(outs):
                ti.match_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, ms_d.data_ptr())
                ti.score_batch_device(pd.data_ptr(), od.data_ptr(), q, total, M, ms_d.data_ptr() if rep == 0 else None, sc_d.data_ptr())
                ti.score_docs_batch_device(sc_d.data_ptr(), od.data_ptr(), q, hd_d.data_ptr())
            ti.sync()
            for ms_d, sc_d, hd_d in outs:
                assert sc_d.cpu().numpy().tobytes() == host["scores"].tobytes(), batch
                assert hd_d.cpu().numpy().tobytes() == host["heads"].tobytes(), batch
            info = ti.score_info()
            assert info["q"] == q and info["positions"] == total and info["match_ms"] > 0 and info["score_ms"] > 0 and info["docs_ms"] > 0, info
            kept.append((pd, od, outs))
        before = ti.score_info()
        ti.spans_batch([[0, 1], [1]], mode=1)                       # launches of another kind move neither of its own two
        ti.next_batch([[0, 1], [1], [0]], cap=2)
        ti.query_batch([[0], [1], [1, 1], [0, 0]])
        assert ti.score_info() == before


def test_python_class(gpu, monkeypatch):
    import suffixarray_amd
    sc.set_plan(monkeypatch, "default")
    with suffixarray_amd.TokenIndex([7, 8, 9, 1, 2, 3]) as ti:
        (length, cc, tc), = ti.infgram([[5, 1, 2, 3, 4]])
        assert length.tolist() == [0, 0, 1, 2, 0] and cc.tolist() == [6, 6, 1, 1, 6] and tc.tolist() == [0, 1, 1, 1, 0]
        assert length.dtype == cc.dtype == tc.dtype == np.uint32
        p, p2, p3 = ti.infgram_probs([[5, 1, 2, 3, 4], [], [1, 2]])
        assert p.dtype == np.float64 and p.tolist() == [0.0, 1 / 6, 1.0, 1.0, 0.0] and p2.size == 0 and p3.tolist() == [1 / 6, 1.0]
        assert ti.infgram([[5, 1, 2, 3, 4]], max_length=1)[0][0].tolist() == [0, 0, 1, 1, 0]
        assert ti.infgram([]) == [] and ti.infgram_probs([]) == []
        s = ti.infgram_summary([[5, 1, 2, 3, 4], [], [1, 2]])
        assert {k: v.tolist() for k, v in s.items()} == {"scored": [5, 0, 2], "seen": [3, 0, 2], "certain": [2, 0, 1], "longest": [2, 0, 1],
                                                        "length_sum": [3, 0, 1]}
        assert s["length_sum"].dtype == np.uint64
    for name, M in (("planted/doc_sizes", 0), ("rand_k2/q5", 7), ("unique_tail", 0), ("equal20", 3)):
        e, b = sc.expected(name), sc.expected_b(name)
        with suffixarray_amd.TokenIndex(e["t"]) as ti:
            got = ti.infgram(e["docs"], max_length=M or None)
            assert [len(g[0]) for g in got] == [len(d) for d in e["docs"]]
            for k in range(3):
                assert np.array_equal(np.concatenate([g[k] for g in got]), b[M][:, k]), (name, k)
            pr = np.concatenate(ti.infgram_probs(e["docs"], max_length=M or None))
            assert np.array_equal(pr, b[M][:, 2] / b[M][:, 1]) and (pr >= 0).all() and (pr <= 1).all(), name
            s = ti.infgram_summary(e["docs"], max_length=M or None)
            assert np.array_equal(np.stack([s[k].astype(np.uint64) for k in ("scored", "seen", "certain", "longest", "length_sum")], axis=1),
                                  sc.heads_of(e["scores"][M], e["docs"])), name
