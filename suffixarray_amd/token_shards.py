"""`ShardedTokenIndex` -- the queries of `TokenIndex` over a corpus held as S <= 64 shards on one device.

    sti = ShardedTokenIndex([tokens_a, tokens_b, tokens_c])   # one suffix array per shard, each at most 2^31 - 1 tokens
    sti.count([[464, 2068], [11]])                 # occurrences over all shards: uint64[Q]
    sti.positions([464, 2068], limit=10)           # (shard, position) pairs
    sti.next_token_counts([464, 2068])             # {token: count} of what follows the n-gram anywhere
    sti.next_tokens(contexts, cap=64, longest_suffix=True)    # backing off to the longest suffix that ANY shard holds
    sti.top_next_tokens(contexts, k=8)             # the k most frequent next tokens over all shards, exact uint64 counts
    sti.sample_next(contexts, samples=4, seed=0)   # next tokens drawn with the probability they have over the whole corpus
    sti.matching_statistics([doc])                 # per position: the longest match in any shard, its count, the shards that hold it
    sti.matched_spans([doc], min_length=8)         # the maximal verbatim spans of a text; sti.coverage([doc], 8): how much they cover
    sti.infgram([doc])                             # per position: the longest context any shard holds, its count, the token's count
    sti.infgram_probs([doc])                       # token_count / context_count; sti.infgram_summary([doc]): per-document sums
    sti = ShardedTokenIndex([tokens_a, tokens_b], doc_starts=[starts_a, starts_b])     # documents: one table per shard
    sti.locate([464, 2068], limit=10)              # (document uint64, offset int32): ids count through the shards in order
    sti.documents([[464, 2068]], cap=16)           # the distinct documents that hold an n-gram, over all shards
    sti.document_counts([[464, 2068], [11]])       # (document frequency uint64[Q], exact flags)
    sti.term_counts([[464, 2068]], [0, 7, 2 ** 33])              # occurrences per document (global ids): uint32[Q, len(docs)]
    sti.documents_with_all([[[464, 2068], [11]]], cap=16)        # AND: documents of the corpus holding every n-gram of a group
    sti.count_documents_with_all([[[464, 2068], [11]]])          # (matched uint64[G], exact flags)

The corpus is cut by the caller, at document boundaries: an n-gram never spans two shards, so its count is the sum of the shards'
counts.  On top of include/sa_hip.h sections 6c, 6g, 6h, 6j and 6l (suffixarray_amd._capi.TokenShards).  No CPU fallback.
"""
import numpy as np

from . import _capi


class ShardedTokenIndex:
    def __init__(self, shards, k=None, device=0, doc_starts=None):
        """shards: a list of 1 to 64 int sequences or arrays with symbols in [0, k) (k defaults to each shard's max + 1).
        doc_starts: one table per shard of the first position of every document inside it (see set_documents)."""
        shards = list(shards)
        if not 1 <= len(shards) <= _capi.SHARDS_MAX:
            raise ValueError("a shard set holds 1 to %d shards" % _capi.SHARDS_MAX)
        self._set = _capi.TokenShards.build(shards, k, device)
        self.shards = self._set.shards
        self._sizes = np.array([self._set.shard(s).info()["n"] for s in range(self.shards)], dtype=np.uint64)
        self.n = int(self._sizes.sum())
        if doc_starts is not None:
            try:
                self.set_documents(doc_starts)
            except Exception:
                self._set.close()
                raise

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

    def top_next_tokens(self, ngrams, k=8, longest_suffix=False, max_length=None, budget=None):
        """As TokenIndex.top_next_tokens over all shards: the k (1 .. 64) most frequent tokens behind every n-gram, their counts
        summed over the shards.  -> dict of arrays: symbols int32[Q, k] and counts uint64[Q, k], by count descending, ties by token
        ascending, of which the first written[i] = min(k, distinct[i]) are valid in row i; distinct[i] = the distinct next tokens,
        covered[i] = the sum of the written counts and total[i] = occurrences that have a next token (uint64 both), length[i] =
        matched symbols, shards[i] = the shards that hold a continuation; spans as in _capi.TokenShards.spans_batch, [S, Q].
        budget: only the first `budget` occurrences in the order of a single index over the whole corpus are walked (the tokens
        with the smallest ids); exact[i] = every occurrence was walked, so row i is the true top-k.  longest_suffix: as in
        next_tokens."""
        r = self._set.top_batch(ngrams, k=k, mode=1 if longest_suffix else 0, max_length=max_length or 0, need_next=True, budget=budget or 0)
        h = r["heads"]
        return {"symbols": r["symbols"], "counts": r["counts"], "written": h["written"].copy(), "distinct": h["distinct"].copy(),
                "covered": h["covered"].copy(), "total": h["total"].copy(), "length": h["length"].copy(), "shards": h["shards"].copy(),
                "exact": h["total"] <= np.uint64(budget or 2 ** 64 - 1), "spans": r["spans"]}

    def sample_next(self, ngrams, draws=None, samples=1, seed=None, longest_suffix=True, max_length=None):
        """As TokenIndex.sample_next over all shards: next tokens drawn with the probability they have over the whole corpus,
        int32[Q, samples], -1 where nothing follows.  draws: uint64[Q, samples] (or [Q]), draw d picks the occurrence
        floor(d * total / 2^64) of the context's total, the occurrences numbered shard by shard and in suffix order inside a shard
        -- the same draws give the same tokens; without them they come from np.random.default_rng(seed).  longest_suffix: a
        context backs off to its longest suffix (at most max_length symbols) that has a next token in some shard."""
        q = len(ngrams[1]) - 1 if isinstance(ngrams, tuple) else len(ngrams)
        if draws is None:
            draws = np.random.default_rng(seed).integers(0, 2 ** 64, size=(q, int(samples)), dtype=np.uint64)
        return self._set.sample_batch(ngrams, draws, mode=1 if longest_suffix else 0, max_length=max_length or 0, need_next=True,
                                      shards=False, ranks=False)["symbols"]

    def matching_statistics(self, docs, max_length=None):
        """Which parts of query texts stand verbatim in some shard.  docs: a list of int sequences.  -> one (length, count, shards)
        per document, arrays over its positions: length[i] (uint32) = the longest prefix of doc[i:] (at most max_length symbols)
        that a shard holds, count[i] (uint64) its occurrences over all shards, shards[i] (uint32) the shards that hold it.  A match
        never spans two shards."""
        buf, off, q = self._set._contexts(docs)
        m, _ = self._set.match_batch((buf, off), max_length=max_length or 0, per_shard=False)
        cut = [(int(off[d]), int(off[d + 1])) for d in range(q)]
        return [(m["length"][a:b].copy(), m["count"][a:b].copy(), m["shards"][a:b].copy()) for a, b in cut]

    def matched_spans(self, docs, min_length, max_length=None, cap=64):
        """The maximal verbatim spans of every document: the matches of at least min_length symbols that no other position's match
        contains, in position order.  -> one (spans, complete) per document: spans = a list of (position, length, count, shards),
        at most cap of them; complete = these are all."""
        r = self._set.match_docs_batch(docs, min_length=min_length, max_length=max_length or 0, cap=max(int(cap), 1))
        out = []
        for d, h in enumerate(r["heads"]):
            w = min(int(h["written"]), int(cap))
            o = r["out_matches"][d, :w]
            out.append(([(int(p), int(l), int(c), int(k)) for p, l, c, k in zip(r["positions"][d, :w], o["length"], o["count"], o["shards"])],
                        int(h["maximal"]) <= int(cap)))
        return out

    def coverage(self, docs, min_length, max_length=None):
        """-> dict of uint32[Q] arrays: covered = the tokens of every document that lie inside a match of at least min_length
        symbols, longest = its longest match (whatever min_length is), maximal = the number of its maximal spans."""
        h = self._set.match_docs_batch(docs, min_length=min_length, max_length=max_length or 0, cap=0)["heads"]
        return {"covered": h["covered"].copy(), "longest": h["longest"].copy(), "maximal": h["maximal"].copy()}

    def infgram(self, docs, max_length=None):
        """The infinity-gram score of query texts over all shards.  docs: a list of int sequences.  -> one (length, context_count,
        token_count) per document, arrays over its positions: length[i] (uint32) = the longest doc[i - L : i] (at most max_length
        symbols) that some shard holds with a token behind it, context_count[i] (uint64) how often over all shards (length 0: the
        tokens of the corpus), token_count[i] (uint64) how often followed by doc[i].  A context never spans two shards."""
        buf, off, q = self._set._contexts(docs)
        s = self._set.score_batch((buf, off), max_length=max_length or 0, per_shard=False, heads=False)["scores"]
        cut = [(int(off[d]), int(off[d + 1])) for d in range(q)]
        return [(s["length"][a:b].copy(), s["context_count"][a:b].copy(), s["token_count"][a:b].copy()) for a, b in cut]

    def infgram_probs(self, docs, max_length=None):
        """-> one float64 array per document: token_count / context_count of every position (computed on the host; 0 for a token
        the context was never followed by, and for every token when the corpus is empty)"""
        out = []
        for _, cc, tc in self.infgram(docs, max_length=max_length):
            p = np.zeros(cc.size, np.float64)
            np.divide(tc, cc, out=p, where=cc > 0)
            out.append(p)
        return out

    def infgram_summary(self, docs, max_length=None):
        """-> dict of per-document arrays as TokenIndex.infgram_summary gives them: scored, seen (token_count > 0), certain
        (token_count == context_count), longest, length_sum (uint64)."""
        h = self._set.score_batch(docs, max_length=max_length or 0, scores=False, per_shard=False)["heads"]
        return {k: h[k].copy() for k in ("scored", "seen", "certain", "longest", "length_sum")}

    def set_documents(self, doc_starts):
        """doc_starts: per shard, the first position inside the shard of every document (starts[0] == 0, non-decreasing, <= the
        shard's length; equal neighbours are empty documents).  The documents of the corpus are numbered through the shards in order:
        document d of shard s is document_bases()[s] + d.  None removes the documents."""
        self._set.set_documents(None if doc_starts is None else list(doc_starts))

    def document_bases(self):
        """uint64[S + 1]: the global id of the first document of every shard; the last entry is the number of documents"""
        return self._set.doc_bases()

    def locate(self, ngram, limit=16):
        """-> (document uint64, offset int32): where one n-gram occurs (at most `limit` places), in the order of positions():
        shard-major, suffix order inside a shard"""
        r = self._set.locate_batch([list(ngram)], cap=max(int(limit), 1))
        w = min(int(r["heads"]["written"][0]), int(limit))
        return r["docs"][0, :w].copy(), r["offsets"][0, :w].copy()

    def documents(self, ngrams, cap=16, budget=None, longest_suffix=False, max_length=None):
        """As TokenIndex.documents over all shards: docs uint64[Q, cap] (global ids: the shards' lists one after another, each in
        order of first appearance by rank), offsets int32[Q, cap], written, examined, distinct, count (uint64) and exact = the walk
        saw the whole span, so `distinct` is the document frequency.  budget: the ranks examined, taken from the front of the
        shards' spans in shard order (None: all)."""
        r = self._set.docs_batch(ngrams, cap=cap, budget=budget or 0, mode=1 if longest_suffix else 0, max_length=max_length or 0)
        h = r["heads"]
        return {"docs": r["docs"], "offsets": r["offsets"], "written": h["written"].copy(), "examined": h["examined"].copy(),
                "distinct": h["distinct"].copy(), "count": h["count"].copy(), "exact": h["examined"] == h["count"]}

    def document_counts(self, ngrams, budget=None):
        """-> (document frequency uint64[Q], exact bool[Q]): in how many documents of the corpus every n-gram occurs; with a budget,
        among its first `budget` hits, and exact says whether those were all"""
        h = self._set.docs_batch(ngrams, cap=0, budget=budget or 0)["heads"]
        return h["distinct"].copy(), h["examined"] == h["count"]

    def prepare_document_ranks(self):
        """Build every shard's rank-by-document array (4 bytes per token) and the set's table of them, which term_counts and
        documents_with_all need; they call this on first use.  set_documents drops the arrays."""
        self._set.prepare_doc_ranks(True)

    def term_counts(self, ngrams, docs):
        """-> uint32[len(ngrams), len(docs)]: how often n-gram i occurs in document docs[j] (global ids, as document_bases()
        numbers them); an id at or beyond the number of documents counts 0."""
        ids = [int(d) for d in np.asarray(docs, dtype=object).reshape(-1)]
        if any(d < 0 or d >= 2 ** 64 for d in ids):
            raise ValueError("docs: document ids are uint64")
        ids = np.array(ids, dtype=np.uint64)
        buf, off = self._set._packed(ngrams)
        q = max(off.size - 1, 0)
        if q == 0 or ids.size == 0:
            return np.zeros((q, ids.size), np.uint32)
        self.prepare_document_ranks()
        rows = np.ascontiguousarray(np.broadcast_to(ids, (q, ids.size)))
        return self._set.doc_counts_batch((buf, off), rows)["counts"]

    def documents_with_all(self, groups, cap=16, budget=None, longest_suffix=False, max_length=None):
        """As TokenIndex.documents_with_all over all shards.  -> one dict per group: documents (uint64 global ids) and offsets (int32),
        at most cap entries: the shards' matches one after another, each in the rank order of the group's rarest n-gram over the
        whole corpus, with the offset of that n-gram's smallest-rank occurrence in the document; matched (a Python int: documents
        matched among the first `budget` occurrences of that n-gram, taken in shard order), exact (these were all its occurrences,
        so matched is the number of documents that hold all n-grams), driver (the index of that n-gram inside the group)."""
        from .token_index import TokenIndex
        flat, goff = TokenIndex._grouped(groups)
        if not len(groups):
            return []
        self.prepare_document_ranks()
        r = self._set.all_batch(flat, goff, cap=cap, budget=budget or 0, mode=1 if longest_suffix else 0, max_length=max_length or 0,
                                need_next=False)
        out = []
        for i, h in enumerate(r["heads"]):
            w = int(h["written"])
            out.append({"documents": r["docs"][i, :w].copy(), "offsets": r["offsets"][i, :w].copy(), "matched": int(h["matched"]),
                        "exact": bool(h["examined"] == h["count"]), "driver": int(h["driver"])})
        return out

    def count_documents_with_all(self, groups, budget=None):
        """-> (matched uint64[G], exact bool[G]): in how many documents of the corpus all n-grams of every group occur"""
        from .token_index import TokenIndex
        flat, goff = TokenIndex._grouped(groups)
        if not len(groups):
            return np.zeros(0, np.uint64), np.zeros(0, np.bool_)
        self.prepare_document_ranks()
        h = self._set.all_batch(flat, goff, cap=0, budget=budget or 0)["heads"]
        return h["matched"].copy(), h["examined"] == h["count"]

    def info(self):
        return self._set.info()

    def close(self):
        self._set.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
