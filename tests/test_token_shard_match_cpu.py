"""Matching statistics over shard sets without a GPU: the five entry points are declared, exported and bound and the class methods
exist; the two new structs match the C compiler's view of the header; every argument error is answered with -1 before the set or a
device is touched; the two CPU models that test_gpu_token_shard_match.py measures the device against (token_shard_match_cases.py)
agree on the whole case list; end(j) never decreases; a set of one shard answers as token_match_cases' own model; and the planted
sets, the cut window among them, are worked by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_match_cases as mc
import token_shard_match_cases as smc
from test_int_cpu import model_sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sa_hip_token_shards_match_batch_device", "sa_hip_token_shards_match_docs_batch_device", "sa_hip_token_shards_match_batch",
       "sa_hip_token_shards_match_docs_batch", "sa_hip_token_shards_match_info"]


def test_shard_match_symbols_declared_exported_bound(capi):
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    for name in ("match_batch", "match_batch_device", "match_docs_batch", "match_docs_batch_device", "match_info"):
        assert callable(getattr(capi.TokenShards, name)), name
    from suffixarray_amd import token_shards
    for name in ("matching_statistics", "matched_spans", "coverage"):
        assert callable(getattr(token_shards.ShardedTokenIndex, name)), name
    assert capi.SHARDS_MATCH_DTYPE.itemsize == C.sizeof(capi.TokenShardsMatch) == 16
    assert capi.SHARDS_MATCH_DTYPE.names == tuple(f for f, _ in capi.TokenShardsMatch._fields_)
    assert [capi.SHARDS_MATCH_DTYPE.fields[f][1] for f in capi.SHARDS_MATCH_DTYPE.names] == [getattr(capi.TokenShardsMatch, f).offset for f in capi.SHARDS_MATCH_DTYPE.names]


@pytest.mark.parametrize("struct, cls, fields", [
    ("sa_hip_token_shards_match", "TokenShardsMatch", ["length", "shards", "count"]),
    ("sa_hip_token_shards_match_stats", "TokenShardsMatchStats", ["q", "positions", "match_ms", "docs_ms"]),
])
def test_shard_match_struct_layouts_match_the_compiler(capi, tmp_path, struct, cls, fields):
    S = getattr(capi, cls)
    assert [f for f, _ in S._fields_] == fields
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sa_hip.h"\nint main(void) { printf("%zu'
                   + "".join(" %zu" for _ in fields) + '\\n", sizeof(' + struct + ")"
                   + "".join(", offsetof(%s, %s)" % (struct, f) for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields], got
    header = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
    assert [f for f in re.findall(r"^\s*\w+\s+(\w+);", body, re.M)] == fields


def test_shard_match_argument_errors_before_any_device_call(capi):
    """every refusal comes before the set is touched: the set of these calls is an address that holds nothing"""
    lib = capi.lib()
    h = 0x1234
    pat = np.array([3, 1, 2, 1], np.int32)
    off = np.array([0, 2, 4], np.uint64)
    down = np.array([0, 3, 2], np.uint64)
    huge = np.array([0, 2, 1 << 31], np.uint64)                    # total >= 2^31: refused before a symbol is read
    merged, outs, per = np.zeros(4, capi.SHARDS_MATCH_DTYPE), np.zeros(8, capi.SHARDS_MATCH_DTYPE), np.zeros(8, capi.SPAN_DTYPE)
    pos, heads = np.zeros(8, np.uint32), np.zeros(2, capi.MATCH_HEAD_DTYPE)
    p, o, m, ps, os_, hd, pr = (a.ctypes.data for a in (pat, off, merged, pos, outs, heads, per))
    D = 1 << 20                                                    # "device pointers": never touched
    # NULL set
    assert lib.sa_hip_token_shards_match_batch(None, p, o, 2, 0, m, pr) == -1
    assert b"sa_hip_token_shards_match_batch" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_match_batch_device(None, D, D, 2, 4, 0, D, D) == -1
    assert lib.sa_hip_token_shards_match_docs_batch_device(None, D, D, 2, 1, 4, D, D, D) == -1
    assert lib.sa_hip_token_shards_match_docs_batch(None, p, o, 2, 0, 1, 4, m, ps, os_, hd) == -1
    assert lib.sa_hip_token_shards_match_info(None, C.byref(capi.TokenShardsMatchStats())) == -1
    assert lib.sa_hip_token_shards_match_info(h, None) == -1
    # min_length == 0
    assert lib.sa_hip_token_shards_match_docs_batch_device(h, D, D, 2, 0, 4, D, D, D) == -1
    assert b"min_length" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_match_docs_batch(h, p, o, 2, 0, 0, 4, m, ps, os_, hd) == -1
    assert lib.sa_hip_token_shards_match_docs_batch(h, p, o, 0, 0, 0, 4, m, ps, os_, hd) == -1                  # also with Q == 0
    # total >= 2^31
    for total in (1 << 31, (1 << 31) + 5, 1 << 40, (1 << 64) - 1):
        assert lib.sa_hip_token_shards_match_batch_device(h, D, D, 2, total, 0, D, D) == -1, total
    assert b"2^31" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_match_batch(h, p, huge.ctypes.data, 2, 0, m, pr) == -1
    assert b"2^31" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_match_docs_batch(h, p, huge.ctypes.data, 2, 0, 1, 4, m, ps, os_, hd) == -1
    # Q * cap >= 2^31
    for q, cap in ((1 << 31, 1), (1 << 20, 1 << 11), (1, 0xFFFFFFFF), (3, 0x80000000 // 3 + 1)):
        assert lib.sa_hip_token_shards_match_docs_batch_device(h, D, D, q, 1, cap, D, D, D) == -1, (q, cap)
        assert lib.sa_hip_token_shards_match_docs_batch(h, p, o, q, 0, 1, cap, m, ps, os_, hd) == -1, (q, cap)
    assert b"2^31" in lib.sa_hip_last_error()
    # NULL arguments (per_shard of match_batch and merged of match_docs_batch may be NULL, positions and out_matches with cap == 0:
    # not among them; per_shard_dev is required)
    assert lib.sa_hip_token_shards_match_batch(h, p, None, 2, 0, m, pr) == -1
    assert lib.sa_hip_token_shards_match_batch(h, p, o, 2, 0, None, pr) == -1
    assert lib.sa_hip_token_shards_match_batch(h, None, o, 2, 0, m, pr) == -1                                   # symbols without a buffer
    for args in ((None, D, D, D), (D, None, D, D), (D, D, None, D), (D, D, D, None)):
        assert lib.sa_hip_token_shards_match_batch_device(h, args[0], args[1], 2, 4, 0, args[2], args[3]) == -1, args
    for args in ((None, D, D, D), (D, None, D, D), (D, D, None, D), (D, D, D, None)):
        assert lib.sa_hip_token_shards_match_docs_batch_device(h, D, args[0], 2, 1, 4, *args[1:]) == -1, args
    assert lib.sa_hip_token_shards_match_docs_batch_device(h, D, D, 2, 1, 0, None, None, None) == -1            # heads, also with cap == 0
    for args in ((None, os_, hd), (ps, None, hd), (ps, os_, None)):
        assert lib.sa_hip_token_shards_match_docs_batch(h, p, o, 2, 0, 1, 4, m, *args) == -1, args
    assert lib.sa_hip_token_shards_match_docs_batch(h, p, None, 2, 0, 1, 4, m, ps, os_, hd) == -1
    assert lib.sa_hip_token_shards_match_docs_batch(h, None, o, 2, 0, 1, 4, m, ps, os_, hd) == -1
    assert lib.sa_hip_token_shards_match_docs_batch(h, p, o, 2, 0, 1, 0, None, None, None, None) == -1
    # descending offsets
    assert lib.sa_hip_token_shards_match_batch(h, p, down.ctypes.data, 2, 0, m, pr) == -1
    assert b"descend" in lib.sa_hip_last_error()
    assert lib.sa_hip_token_shards_match_docs_batch(h, p, down.ctypes.data, 2, 0, 1, 4, m, ps, os_, hd) == -1
    assert b"descend" in lib.sa_hip_last_error()
    # Q == 0 with good arguments: a no-op that touches nothing
    assert lib.sa_hip_token_shards_match_batch(h, None, None, 0, 0, None, None) == 0
    assert lib.sa_hip_token_shards_match_batch_device(h, None, None, 0, 0, 0, None, None) == 0
    assert lib.sa_hip_token_shards_match_docs_batch_device(h, None, None, 0, 1, 4, None, None, None) == 0
    assert lib.sa_hip_token_shards_match_docs_batch(h, None, None, 0, 7, 1, 4, None, None, None, None) == 0


@pytest.mark.parametrize("name", smc.SETS)
def test_shard_match_models_agree(name):
    e, b = smc.expected(name), smc.expected_b(name)
    shards = e["shards"]
    S, sizes = len(shards), [len(t) for t in shards]
    hits = 0
    for (batch, M), merged in e["merged"].items():
        where = (name, batch, M)
        per, dl = e["per"][batch, M], e["batches"][batch]
        length, held, count, per_count = b[batch, M]
        assert per.shape == (S, merged.shape[0], 4)
        mine = merged.astype(np.int64)
        bad = np.flatnonzero((mine[:, 0] != length) | (mine[:, 1] != held) | (mine[:, 2] != count))
        assert bad.size == 0, (where, bad[:5], mine[bad[:5]].tolist(), length[bad[:5]], held[bad[:5]], count[bad[:5]])
        assert np.array_equal(per[:, :, 1].astype(np.int64), per_count), where
        # every shard that is not empty says the merged length; an empty one says zeros
        for s in range(S):
            assert (per[s, :, 2] == (merged[:, 0] if sizes[s] else 0)).all() and (sizes[s] or not per[s].any()), (where, s)
        # end(j) never decreases, never passes its document's end, and the length respects the caps
        base = np.concatenate([[0], np.cumsum([len(d) for d in dl])]).astype(np.int64)
        doc_end = np.repeat(base[1:], np.diff(base))
        end = np.arange(mine.shape[0], dtype=np.int64) + mine[:, 0]
        assert (np.diff(end) >= 0).all() and (end <= doc_end).all(), where
        assert (mine[:, 0] <= min(M or max(sizes), max(sizes))).all(), where
        for mlen in smc.MIN_LENGTHS:
            ha, hb = mc.heads_a(mine[:, 0], dl, mlen), mc.heads_b(length, dl, mlen)
            assert ha == hb, (where, mlen, [(x, y) for x, y in zip(ha, hb) if x != y][:2])
        hits += int((mine[:, 0] > 0).sum())
    assert hits > 0 or max(sizes) == 0, name


@pytest.mark.parametrize("text", list(smc.CUTS))
def test_one_shard_is_the_single_index_model(text):
    e, single = smc.expected(text + "/1"), mc.expected(text)
    assert list(e["batches"]) == list(single["batches"])
    for key, sp in single["spans"].items():
        if e["batches"][key[0]] != single["batches"][key[0]]:       # "whole" is cut to its tail here
            assert key[0] == "whole"
            continue
        merged, per = e["merged"][key], e["per"][key]
        assert np.array_equal(per[0], sp), key
        assert np.array_equal(merged[:, 0], sp[:, 2]) and np.array_equal(merged[:, 2], sp[:, 1]) and np.array_equal(merged[:, 1], sp[:, 1] > 0), key


def test_the_cut_window_by_hand():
    """the corpus holds the window of 130 tokens once, cut after 50 of them: the set answers the halves, an unsharded index the whole"""
    e = smc.expected("cut_window")
    (doc,) = e["batches"]["window"]
    merged, per = e["merged"]["window", 0], e["per"]["window", 0]
    n0, n1 = (len(t) for t in e["shards"])
    assert len(doc) == 3 + smc.CUT_LEN + 2 and smc.CUT_LEN - smc.CUT_AT == 80
    assert merged[3].tolist() == [50, 1, 1] and merged[3 + 50].tolist() == [80, 1, 1]
    assert merged[3 + 49].tolist()[0] == 1 and merged[3 + 129].tolist()[0] == 1 and merged[0].tolist() == [0, 2, n0 + n1]
    assert per[0, 3, 1:].tolist() == [1, 50, 1] and per[1, 3, 1:].tolist() == [0, 50, 0]              # the first half only ends shard 0
    assert per[0, 3 + 50, 1:].tolist() == [0, 80, 0] and per[1, 3 + 50, 1:].tolist() == [1, 80, 0]    # the second half begins shard 1
    assert int(model_sa(e["shards"][1]).tolist().index(0)) == int(per[1, 3 + 50, 0])
    heads = mc.heads_a(merged[:, 0], [doc], 8)
    assert heads == [([(3, 3), (53, 53)], (2, 80, 130))]                                              # two maximal matches cover the window
    whole = smc.unsharded("cut_window")
    sp = mc.spans_a(whole.tolist(), model_sa(whole).tolist(), [doc], 0)
    assert sp[3].tolist()[1:] == [1, 130, 0] and mc.heads_a(sp[:, 2], [doc], 8) == [([(3, 3)], (1, 130, 130))]
    assert int(merged[:, 0].max()) == 80 and int(sp[:, 2].max()) == 130


def test_the_planted_set_by_hand():
    e = smc.expected("planted3")
    docs = e["batches"]["planted"]
    merged, per = e["merged"]["planted", 0], e["per"]["planted", 0]
    base = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).tolist()
    W = smc.W
    first, last = base[0] + 1, base[0] + 1 + W + 1
    assert merged[first].tolist() == [W, 1, 1] and per[:, first, 1].tolist() == [1, 0, 0]             # only the first shard
    assert merged[last].tolist() == [W, 1, 1] and per[:, last, 1].tolist() == [0, 0, 1]               # only the last shard
    assert merged[base[1]].tolist() == [W, 2, 3] and per[:, base[1], 1].tolist() == [1, 2, 0]         # two shards at the same length
    assert merged[base[2]].tolist() == [W, 1, 1] and per[:, base[2]].tolist()[1][1:] == [1, W, 1]      # it only ends shard 1's text
    assert per[:, base[2], 3].tolist() == [0, 1, 0] and per[0, base[2], 1] == 0 and per[0, base[2], 2] == W
    assert merged[base[3]].tolist() == [W, 1, 1]
    a = base[4]                                                                                        # W_LAST[5:] then W_FIRST[:5]: two matches
    assert merged[a].tolist() == [W - 5, 1, 1] and merged[a + W - 5].tolist() == [5, 1, 1]
    assert mc.heads_a(merged[:, 0], docs, 5)[4] == ([(0, a), (W - 5, a + W - 5)], (2, W - 5, W))
    # model rows: what a launch with cap 1 leaves of document 4
    h = mc.heads_a(merged[:, 0], docs, 5)
    pos, outs, hd = smc.rows([f for f, _ in h], [x for _, x in h], merged, 1, -7)
    assert pos[4].tolist() == [0] and outs[4].tolist() == [[W - 5, 1, 1, 0]] and hd[4].tolist() == [1, 2, W - 5, W]
    # the small shards beside the long one: a prefix longer than a shard is clamped there, the empty shard answers zeros
    s = smc.expected("small_beside_long")
    m, p = s["merged"]["clamp", 0], s["per"]["clamp", 0]
    assert m[0].tolist() == [7, 1, 1] and not p[0].any() and p[:, 0, 2].tolist() == [0, 7, 7, 7] and p[1:3, 0, 1].tolist() == [0, 0]
    assert m[2].tolist() == [5, 1, 1] and p[:, 2, 2].tolist() == [0, 5, 5, 5]                          # longer than the shard of one token that holds its head
    two = sum(len(d) for d in s["batches"]["clamp"][:1])
    assert m[two].tolist()[:2] == [2, 2] and p[:, two, 3].tolist() == [0, 0, 1, 0]                     # the shard of 2 tokens holds it whole
