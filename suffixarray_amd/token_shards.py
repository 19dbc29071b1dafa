"""`ShardedTokenIndex` -- the queries of `TokenIndex` over a corpus held as S <= 64 shards on one device.

    sti = ShardedTokenIndex([tokens_a, tokens_b, tokens_c])   # one suffix array per shard, each at most 2^31 - 1 tokens
    sti.count([[464, 2068], [11]])                 # occurrences over all shards: uint64[Q]
    sti.positions([464, 2068], limit=10)           # (shard, position) pairs
    sti.next_token_counts([464, 2068])             # {token: count} of what follows the n-gram anywhere
    sti.next_tokens(contexts, cap=64, longest_suffix=True)    # backing off to the longest suffix that ANY shard holds

The corpus is cut by the caller, at document boundaries: an n-gram never spans two shards, so its count is the sum of the shards'
counts.  On top of include/sa_hip.h section 6c (suffixarray_amd._capi.TokenShards).  No CPU fallback.
"""
import numpy as np

from . import _capi


class ShardedTokenIndex:
    def __init__(self, shards, k=None, device=0):
        """shards: a list of 1 to 64 int sequences or arrays with symbols in [0, k) (k defaults to each shard's max + 1)."""
        shards = list(shards)
        if not 1 <= len(shards) <= _capi.SHARDS_MAX:
            raise ValueError("a shard set holds 1 to %d shards" % _capi.SHARDS_MAX)
        self._set = _capi.TokenShards.build(shards, k, device)
        self.shards = self._set.shards
        self._sizes = np.array([self._set.shard(s).info()["n"] for s in range(self.shards)], dtype=np.uint64)
        self.n = int(self._sizes.sum())

    def shard_sizes(self):
        """tokens of every shard: uint64[S]"""
        return self._sizes.copy()

    def ranges(self, ngrams):
        """-> (first, count), uint32[S, Q] each: in shard s, n-gram i occurs at the positions SA_s[first .. first + count)"""
        _, per = self._set.query_batch(ngrams)
        return per["first"].copy(), per["second"].copy()

    def count(self, ngrams):
        """occurrences of every n-gram over all shards: uint64[Q]"""
        return self._set.query_batch(ngrams, per_shard=False)[0].copy()

    def positions(self, ngram, limit=None):
        """-> (shard, position): where one n-gram occurs (at most `limit` places), shard-major, suffix order inside a shard"""
        first, count = self.ranges([list(ngram)])
        left = None if limit is None else int(limit)
        sh, pos = [], []
        for s in range(self.shards):
            c = int(count[s, 0]) if left is None else min(int(count[s, 0]), left)
            if c:
                pos.append(self._set.shard(s).sa_range(int(first[s, 0]), c))
                sh.append(np.full(c, s, dtype=np.int32))
                left = None if left is None else left - c
        if not pos:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        return np.concatenate(sh), np.concatenate(pos)

    def longest_suffix(self, contexts, max_length=None, need_next=True):
        """-> (length uint32[Q], total uint64[Q], spans[S, Q]): the longest suffix of context i (at most max_length symbols) that
        occurs in some shard -- with need_next, that occurs with a symbol behind it -- its occurrences over all shards, and its span
        (first, count, length, ended) in every shard."""
        r = self._set.spans_batch(contexts, mode=1, max_length=max_length or 0, need_next=need_next)
        return r["length"].copy(), r["totals"].copy(), r["spans"].copy()

    def next_tokens(self, ngrams, cap=64, longest_suffix=False, max_length=None):
        """As TokenIndex.next_tokens over all shards: symbols int32[Q, cap] (ascending), counts uint64[Q, cap], written, total
        (uint64), length, complete."""
        r = self._set.next_batch(ngrams, cap=cap, mode=1 if longest_suffix else 0, max_length=max_length or 0, need_next=True)
        h = r["heads"]
        return {"symbols": r["symbols"], "counts": r["counts"], "written": h["written"].copy(), "total": h["total"].copy(),
                "length": h["length"].copy(), "complete": h["covered"] == h["total"]}

    def next_token_counts(self, ngram, cap=64, longest_suffix=False, max_length=None):
        """{token: count} of what follows one n-gram in any shard (the cap smallest tokens when there are more)"""
        r = self.next_tokens([list(ngram)], cap=cap, longest_suffix=longest_suffix, max_length=max_length)
        w = int(r["written"][0])
        return {int(s): int(c) for s, c in zip(r["symbols"][0, :w], r["counts"][0, :w])}

    def info(self):
        return self._set.info()

    def close(self):
        self._set.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
