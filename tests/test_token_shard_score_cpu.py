"""Infinity-gram scores over shard sets without a GPU: the four entry points are declared, exported and bound and the class methods
exist; the two new structs match the C compiler's view of the header; every argument error is answered with -1 before the set or a
device is touched, and a missing device is -3; the two CPU models that test_gpu_token_shard_score.py measures the device against
(token_shard_score_cases.py) agree on every set and batch, with and without the matching statistics; a set of one shard answers as
token_score_cases' own model; model A's trace shows the fallbacks the hand sets were written for; the invariants hold; a context
across a cut is none; and a hand-worked example pins what the words of the contract mean."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_score_cases as sc
import token_shard_match_cases as smc
import token_shard_score_cases as ssc
from test_int_cpu import model_sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_shards_score_batch_device", "sa_hip_token_shards_score_docs_batch_device", "sa_hip_token_shards_score_batch",
       "sa_hip_token_shards_score_info"]


def test_shard_score_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    for name in ("score_batch", "score_batch_device", "score_docs_batch_device", "score_info"):
        assert callable(getattr(capi.TokenShards, name)), name
    from suffixarray_amd import token_shards
    for name in ("infgram", "infgram_probs", "infgram_summary"):
        assert callable(getattr(token_shards.ShardedTokenIndex, name)), name
    assert capi.SHARDS_SCORE_DTYPE.itemsize == C.sizeof(capi.TokenShardsScore) == 24 and C.alignment(capi.TokenShardsScore) == 8
    assert capi.SHARDS_SCORE_DTYPE.names == tuple(f for f, _ in capi.TokenShardsScore._fields_)
    assert [capi.SHARDS_SCORE_DTYPE.fields[f][1] for f in capi.SHARDS_SCORE_DTYPE.names] == [getattr(capi.TokenShardsScore, f).offset for f in capi.SHARDS_SCORE_DTYPE.names]
    assert ssc.score_bytes(np.zeros((1, 4), np.uint64)).dtype == capi.SHARDS_SCORE_DTYPE


@pytest.mark.parametrize("struct, cls, fields, offsets, size", [
    ("sa_hip_token_shards_score", "TokenShardsScore", ["length", "shards", "context_count", "token_count"], [0, 4, 8, 16], 24),
    ("sa_hip_token_shards_score_stats", "TokenShardsScoreStats", ["q", "positions", "match_ms", "score_ms", "docs_ms"], [0, 8, 16, 24, 32], 40),
])
def test_shard_score_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields, offsets, size):
    S = getattr(capi, cls)
    assert [f for f, _ in S._fields_] == fields and C.sizeof(S) == size and [getattr(S, f).offset for f in fields] == offsets
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sa_hip.h"\nint main(void) { printf("%zu %zu'
                   + "".join(" %zu" for _ in fields) + '\\n", sizeof(' + struct + "), _Alignof(" + struct + ")"
                   + "".join(", offsetof(%s, %s)" % (struct, f) for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [size, 8] + offsets, got
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
    assert [f for f in re.findall(r"^\s*\w+\s+(\w+);", body, re.M)] == fields


def test_the_pinned_stats_structs_did_not_grow(capi):
    assert C.sizeof(capi.TokenShardsMatchStats) == 32 and C.sizeof(capi.TokenScoreInfo) == 40 and C.sizeof(capi.TokenShardsStats) == 56
    assert C.sizeof(capi.TokenScoreHead) == 24 and C.sizeof(capi.TokenShardsMatch) == 16


def test_shard_score_argument_errors_before_any_device_call(capi):
    """every refusal comes before the set is touched: the set of these calls is an address that holds nothing"""
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    huge = np.array([0, 2, 1 << 31], np.uint64)                    # total >= 2^31: refused before a symbol is read
    scores, per, heads = np.zeros(4, capi.SHARDS_SCORE_DTYPE), np.zeros(8, capi.SPAN_DTYPE), np.zeros(2, capi.SCORE_HEAD_DTYPE)
    p, o, s, pr, hd = (a.ctypes.data for a in (pat, off, scores, per, heads))
    D = 1 << 20                                                    # "device pointers": never touched
    # NULL set
    assert lib.sa_hip_token_shards_score_batch(None, p, o, 2, 0, s, pr, hd) == -1
    assert b"sa_hip_token_shards_score_batch" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_score_batch_device(None, D, D, 2, 4, 0, D, D, D) == -1
    assert lib.sa_hip_token_shards_score_batch_device(None, D, D, 2, 4, 0, None, D, D) == -1
    assert lib.sa_hip_token_shards_score_docs_batch_device(None, D, D, 2, D) == -1
    assert lib.sa_hip_token_shards_score_info(None, C.byref(capi.TokenShardsScoreStats())) == -1
    assert lib.sa_hip_token_shards_score_info(h, None) == -1
    # total >= 2^31
    for total in (1 << 31, (1 << 31) + 5, 1 << 40, (1 << 64) - 1):
        assert lib.sa_hip_token_shards_score_batch_device(h, D, D, 2, total, 0, D, D, D) == -1, total
        assert lib.sa_hip_token_shards_score_batch_device(h, D, D, 2, total, 0, None, D, D) == -1, total
    assert b"2^31" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_score_batch(h, p, huge.ctypes.data, 2, 0, s, pr, hd) == -1
    assert b"2^31" in lib.sa_hip_last_error()
    # NULL arguments (merged of the device form may be NULL, two of the three outputs of the host form: not among them)
    for args in ((None, D, D, D), (D, None, D, D), (D, D, None, D), (D, D, D, None)):
        assert lib.sa_hip_token_shards_score_batch_device(h, args[0], args[1], 2, 4, 0, D, args[2], args[3]) == -1, args
        assert lib.sa_hip_token_shards_score_batch_device(h, args[0], args[1], 2, 4, 0, None, args[2], args[3]) == -1, args
    assert lib.sa_hip_token_shards_score_docs_batch_device(h, D, None, 2, D) == -1
    assert lib.sa_hip_token_shards_score_docs_batch_device(h, D, D, 2, None) == -1
    assert lib.sa_hip_token_shards_score_batch(h, p, None, 2, 0, s, pr, hd) == -1
    assert lib.sa_hip_token_shards_score_batch(h, None, o, 2, 0, s, pr, hd) == -1                               # symbols without a buffer
    assert lib.sa_hip_token_shards_score_batch(h, p, o, 2, 0, None, None, None) == -1                           # all three outputs
    assert b"NULL" in lib.sa_hip_last_error()
    # descending offsets
    for a, b, c in ((s, pr, hd), (s, None, None), (None, pr, None), (None, None, hd)):
        assert lib.sa_hip_token_shards_score_batch(h, p, down.ctypes.data, 2, 0, a, b, c) == -1
        assert b"descend" in lib.sa_hip_last_error()
    # Q == 0 with good arguments: a no-op that touches nothing
    assert lib.sa_hip_token_shards_score_batch(h, None, None, 0, 0, None, None, None) == 0
    assert lib.sa_hip_token_shards_score_batch_device(h, None, None, 0, 0, 0, None, None, None) == 0
    assert lib.sa_hip_token_shards_score_docs_batch_device(h, None, None, 0, None) == 0


def test_shard_score_no_device_is_minus_three(capi):
    """no set without a device, so no answer from anywhere else: the class raises -3 before a score can be asked"""
    lib = capi.lib()
    if lib.sa_hip_device_count() >= 1:
        h = C.c_void_p(0x1234)
        t = np.array([3, 1, 2, 1], np.int32)
        assert lib.sa_hip_token_index_build(C.byref(h), t.ctypes.data, 4, 4, 1 << 20) == -3 and not h.value
        return
    import suffixarray_amd
    for call in (lambda sti: sti.infgram([[5, 1]]), lambda sti: sti.infgram_probs([[5, 1]]), lambda sti: sti.infgram_summary([[5, 1]])):
        with pytest.raises(capi.SaHipError) as e:
            call(suffixarray_amd.ShardedTokenIndex([[5, 1, 5, 1, 5], [1, 5]]))
        assert e.value.code == -3
    with pytest.raises(capi.SaHipError) as e:
        capi.TokenShards.build([[1, 2, 3], [2]]).score_batch([[1]])
    assert e.value.code == -3


@pytest.mark.parametrize("name", ssc.SETS)
def test_shard_score_models_agree(name):
    """model A == model B for every max_length on every batch of the set, model A without the matching statistics == with them, and
    the invariants of the contract"""
    e, b = ssc.expected(name), ssc.expected_b(name)
    S, sizes = len(e["shards"]), [len(t) for t in e["shards"]]
    n, max_n = sum(sizes), max(sizes)
    for (batch, M), a in e["scores"].items():
        where = (name, batch, M)
        per, docs = e["per"][batch, M], e["batches"][batch]
        length, held, cc, tc, per_tc = b[batch, M]
        mine = a.astype(np.int64)
        bad = np.flatnonzero((mine[:, 0] != length) | (mine[:, 1] != held) | (mine[:, 2] != cc) | (mine[:, 3] != tc))
        assert bad.size == 0, (where, bad[:5], mine[bad[:5]].tolist(), length[bad[:5]], held[bad[:5]], cc[bad[:5]], tc[bad[:5]])
        assert per.shape == (S, a.shape[0], 4) and np.array_equal(per[:, :, 1].astype(np.int64), per_tc), where
        a2, per2, _ = ssc.score_a(e["shards"], e["sas"], docs, M, None)                # way 2
        assert np.array_equal(a2, a) and np.array_equal(per2, per), where
        # the invariants
        offs = np.concatenate([np.arange(len(d)) for d in docs]) if a.shape[0] else np.zeros(0, np.int64)
        assert (mine[:, 3] <= mine[:, 2]).all() and (mine[:, 1] <= S).all(), where
        assert ((mine[:, 2] >= 1) if n else (mine == 0)).all(), where
        assert (mine[:, 0] <= np.minimum(offs, min(M or max_n, max_n))).all(), where
        assert (mine[mine[:, 0] == 0, 2] == n).all(), where
        assert np.array_equal(mine[:, 1], (per[:, :, 1] > 0).sum(axis=0)) and np.array_equal(mine[:, 3], per[:, :, 1].astype(np.int64).sum(axis=0)), where
        for s in range(S):                                                              # every shard that is not empty says L + 1
            assert (per[s, :, 2] == (mine[:, 0] + 1 if sizes[s] else 0)).all() and (sizes[s] or not per[s].any()), (where, s)
        for j, ended, shift in e["trace"][batch, M]:
            assert 1 <= ended <= S and 1 <= shift, (where, j)


@pytest.mark.parametrize("text", list(smc.CUTS))
def test_one_shard_is_the_single_index_model(text):
    e = ssc.expected(text + "/1")
    (t,), (sa,) = e["shards"], e["sas"]
    tl, sl = [int(v) for v in t], [int(v) for v in sa]
    for (batch, M), a in e["scores"].items():
        one, _ = sc.score_a(tl, sl, e["batches"][batch], M, e["ms"][batch, M])
        where = (text, batch, M)
        assert np.array_equal(a[:, 0], one[:, 0]) and np.array_equal(a[:, 2], one[:, 1]) and np.array_equal(a[:, 3], one[:, 2]), where
        assert np.array_equal(a[:, 1], one[:, 2] > 0), where
        per = e["per"][batch, M][0]
        assert np.array_equal(per[:, 0], one[:, 3]) and np.array_equal(per[:, 1], one[:, 2]), where
        assert np.array_equal(ssc.heads_of(a, e["batches"][batch]), sc.heads_of(one, e["batches"][batch])), where


def _trace(name, M=0):
    e = ssc.expected(name)
    return e, e["scores"]["hand", M].astype(np.int64), e["per"]["hand", M], {j: (ended, shift) for j, ended, shift in e["trace"]["hand", M]}


def _starts(docs):
    return np.concatenate([[0], np.cumsum([len(d) for d in docs])]).tolist()


def test_the_fallbacks_the_hand_sets_were_written_for():
    """on model A's trace: a fallback where two shards ended the context, one that moves the start by one, one by three or more"""
    # the tail (A, B, C) ends shards 0 and 1 and stands nowhere else
    e, a, per, tr = _trace("tail_of_two")
    n = sum(len(t) for t in e["shards"])
    base = _starts(e["batches"]["hand"])
    j = base[1] + 3                                                 # document (A, B, C, A): the token behind the tail
    assert e["ms"]["hand", 0][base[1]] == 3                         # fact 1 finds the tail ...
    assert [int((t[-3:] == [ssc.A, ssc.B, ssc.C]).all()) for t in e["shards"]] == [1, 1, 0]
    assert tr[j] == (2, 3) and a[j].tolist() == [0, 2, n, 2]        # ... held by two shards, both as their tail: down to L = 0 (two A)
    assert base[1] + 2 not in tr and a[base[1] + 2].tolist() == [2, 2, 2, 2]            # (A, B) is no tail: a C follows it in both
    assert tr[base[3] + 2] == (2, 2) and tr[base[4] + 1] == (2, 1)  # (B, C) and (C): only the two tails
    assert max(ended for ended, _ in tr.values()) == 2 and {1, 2, 3} <= {shift for _, shift in tr.values()}
    k = base[2] + 13                                                # behind ten tokens of shard 0's body and the tail: one shard holds that
    assert tr[k] == (1, 13) and a[k, 0] == 0
    # ending shard 0, in the interior of shard 1: count 2, one of them ended, an effective count of 1 and no fallback
    e, a, per, tr = _trace("tail_and_interior")
    base = _starts(e["batches"]["hand"])
    j = base[1] + 3
    body = len(e["shards"][0]) - 3                                  # shard 0: every body suffix and the tail itself sort before (A, B, C, x)
    assert j not in tr and a[j].tolist() == [3, 1, 1, 1] and per[:, j].tolist() == [[body + 1, 0, 4, 0], [per[1, j, 0], 1, 4, 0]]
    # the last shard's tail behind a copied window of 20 tokens: the start moves over all 23
    e, a, per, tr = _trace("tail_behind_window")
    assert tr[23] == (1, 23) and a[23, 0] == 0 and a[22].tolist()[0] == 22 and a[22].tolist()[2:] == [1, 1]
    assert min(shift for _, shift in tr.values()) >= 1 and max(shift for _, shift in tr.values()) >= 3
    # all-equal shards of 20, 12 and 20 tokens scored with 30 of them: at position 20 the context 7^20 is two whole shards
    e, a, per, tr = _trace("equal_shards")
    assert a[:20, 0].tolist() == list(range(20)) and a[19].tolist() == [19, 2, 2, 2]
    assert [tr.get(j) for j in range(19, 23)] == [None, (2, 1), (2, 1), (2, 1)] and a[20:30].tolist() == [[19, 2, 2, 2]] * 10
    assert a[12].tolist() == [12, 2, 16, 16]                        # the shard of 12 holds 7^12 once, as its tail: nothing behind it
    # everywhere: a list that holds all three kinds
    every = [x for name in ssc.HAND for M in ssc.MAX_LENGTHS for x in ssc.expected(name)["trace"]["hand", M]]
    assert any(ended >= 2 for _, ended, _ in every) and any(shift == 1 for _, _, shift in every) and any(shift >= 3 for _, _, shift in every)


def test_the_numerator_over_a_set_by_hand():
    e, a, per, tr = _trace("followed")
    base = _starts(e["batches"]["hand"])
    # (1, 2) stands twice in shards 0 and 1 and once in shard 2, always with a token behind it; 5 follows it in shard 1 only
    assert a[base[0] + 2].tolist() == [2, 1, 5, 2] and per[:, base[0] + 2, 1].tolist() == [0, 2, 0]
    # ... and 9 nowhere: a token count of 0 behind a context of two symbols
    assert a[base[1] + 2].tolist() == [2, 0, 5, 0] and not per[:, base[1] + 2, 1].any() and (per[:, base[1] + 2, 2] == 3).all()
    # the lower bounds where the shard does not hold the (L + 1)-gram are the shard's own
    for s, t in enumerate(e["shards"]):
        tl, sl = [int(v) for v in t], [int(v) for v in model_sa(t)]
        assert per[s, base[1] + 2, 0] == sc._span(tl, sl, [1, 2, 9])[0]
        assert per[s, base[0] + 2].tolist() == list(sc._span(tl, sl, [1, 2, 5])[:2]) + [3, 0]
    # shards of 0, 1 and 2 tokens beside a long one: the empty shard answers zeros, the shard (3) holds 3 only as its tail
    e, a, per, tr = _trace("tiny_beside_long")
    assert not per[0].any() and a[1, 0] == 1 and per[:, 1, 1].tolist()[:3] == [0, 0, 1] and per[:, 1, 2].tolist() == [0, 2, 2, 2]
    in_body = sum(int(v == 3) for v in e["shards"][3][:-1])         # (the body's own last token is a 3 as well: its tail)
    assert a[1].tolist() == [1, 1, 1 + in_body, 1]


def test_a_context_across_a_cut_is_none():
    """the unsharded index of the concatenation answers a longer context than the set, here and on the cut window"""
    e, a, per, tr = _trace("cut_context")
    docs = e["batches"]["hand"]
    whole = ssc.unsharded("cut_context")
    tl, sl = [int(v) for v in whole], [int(v) for v in model_sa(whole)]
    one, _ = sc.score_a(tl, sl, docs, 0, sc.mc.spans_a(tl, sl, docs, 0)[:, 2])
    assert one[4].tolist()[:3] == [4, 1, 1] and a[4].tolist() == [2, 1, 1, 1]           # (A, B, C, D) | (C, D)
    assert one[2].tolist()[:3] == [2, 1, 1] and a[2, 0] == 0                            # C behind (A, B): the set has nothing behind its tail
    assert (one[:, 0] >= a[:, 0]).all() and (one[:, 0] > a[:, 0]).sum() >= 5
    e = ssc.expected("cut_window")
    (doc,) = e["batches"]["window"]
    whole = ssc.unsharded("cut_window")
    tl, sl = [int(v) for v in whole], [int(v) for v in model_sa(whole)]
    one, _ = sc.score_a(tl, sl, [doc], 0, sc.mc.spans_a(tl, sl, [doc], 0)[:, 2])
    a = e["scores"]["window", 0].astype(np.int64)
    at = 3 + smc.CUT_LEN - 1                                         # the last token of the window: 129 tokens of it in front
    assert one[at, 0] == smc.CUT_LEN - 1 and a[at, 0] == smc.CUT_LEN - smc.CUT_AT - 1
    # the first token behind the cut: what stands in front of it is shard 0's tail, of which only a few tokens stand elsewhere
    assert a[3 + smc.CUT_AT, 0] < 4 and one[3 + smc.CUT_AT, 0] == smc.CUT_AT
    assert (3 + smc.CUT_AT, 1, smc.CUT_AT - int(a[3 + smc.CUT_AT, 0])) in e["trace"]["window", 0]


def test_shard_score_hand_worked():
    """shards 7 8 9 1 2 3 and 1 2 3 4, text 5 1 2 3 4 6.  5 and 6 occur nowhere.  1 after "5": the empty context, ten tokens, two of
    them a 1.  2 after "1" and 3 after "1 2": once in each shard.  4 after "1 2 3": shard 0 holds that as its tail with nothing behind
    it, shard 1 once with a 4.  6 after "1 2 3 4": that is shard 1 itself and nothing follows it; so are "2 3 4", "3 4" and "4"."""
    shards = [np.array([7, 8, 9, 1, 2, 3], np.int32), np.array([1, 2, 3, 4], np.int32)]
    sas = [model_sa(t).astype(np.int32) for t in shards]
    assert [sa.tolist() for sa in sas] == [[3, 4, 5, 0, 1, 2], [0, 1, 2, 3]]
    docs = [[5, 1, 2, 3, 4, 6]]
    ms = smc.model_a(shards, sas, docs, 0)[0][:, 0].astype(np.int64)
    assert ms.tolist() == [0, 4, 3, 2, 1, 0]
    a, per, trace = ssc.score_a(shards, sas, docs, 0, ms)
    assert a.tolist() == [[0, 0, 10, 0], [0, 2, 10, 2], [1, 2, 2, 2], [2, 2, 2, 2], [3, 1, 1, 1], [0, 0, 10, 0]]
    assert trace == [(5, 1, 4)]                                     # fact 1 finds "1 2 3 4"; the fallback goes down to nothing
    assert per[:, 4].tolist() == [[1, 0, 4, 0], [0, 1, 4, 1]]       # "1 2 3 4": behind shard 0's "1 2 3"; shard 1 itself
    assert per[:, 1].tolist() == [[0, 1, 1, 0], [0, 1, 1, 0]] and per[:, 0].tolist() == [[3, 0, 1, 0], [4, 0, 1, 0]]
    a2, per2, _ = ssc.score_a(shards, sas, docs, 0, None)
    assert np.array_equal(a2, a) and np.array_equal(per2, per)
    b = ssc.model_b(shards, {"x": docs}, (0, 2))
    assert [b["x", 0][k].tolist() for k in range(4)] == [a[:, k].tolist() for k in range(4)] and b["x", 0][4].tolist() == per[:, :, 1].tolist()
    assert ssc.heads_of(a, docs).tolist() == [[6, 4, 3, 3, 6]]      # seen: 1, 2, 3, 4; certain: the 2, the 3 and the 4
    # max_length 2: the 4 is scored behind "2 3", which shard 0 holds only as its tail
    a1 = ssc.score_a(shards, sas, docs, 2, smc.model_a(shards, sas, docs, 2)[0][:, 0])[0]
    assert a1.tolist() == [[0, 0, 10, 0], [0, 2, 10, 2], [1, 2, 2, 2], [2, 2, 2, 2], [2, 1, 1, 1], [0, 0, 10, 0]]
    assert [b["x", 2][k].tolist() for k in range(4)] == [a1[:, k].tolist() for k in range(4)]
    assert ssc.score_bytes(a).tobytes()[24 * 4:24 * 5] == np.array([3, 1], np.uint32).tobytes() + np.array([1, 1], np.uint64).tobytes()
