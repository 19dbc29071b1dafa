"""`TokenIndex` -- n-gram counts, ranges and positions over a token corpus (int32 ids) on the device.

    ti = TokenIndex(tokens)                # upload, suffix array (sa_hip_libsais_int's build), search structures
    ti.count([[464, 2068], [11]])          # occurrences of every n-gram: uint32[Q]
    ti.positions([464, 2068], limit=10)    # where: text positions in suffix order
    ti.next_token_counts([464, 2068])      # {token: count} of what follows the n-gram
    ti.next_tokens(contexts, cap=64, longest_suffix=True)   # the same per context, backing off to its longest suffix that occurs
    ti.top_next_tokens(contexts, k=8)      # the k most frequent next tokens per context, by count descending
    ti.sample_next(contexts, samples=4, seed=0)             # next tokens drawn with the corpus's probability: int32[Q, samples]
    ti = TokenIndex(tokens, doc_starts=starts)              # ... with documents: document d is tokens[starts[d] : starts[d + 1]]
    ti.locate([464, 2068], limit=10)       # where, as (document, offset inside it)
    ti.document_counts([[464, 2068], [11]])   # in how many documents every n-gram occurs
    ti.documents(ngrams, cap=16)           # which documents, in order of first appearance by rank
    ti.term_counts(ngrams, docs)           # how often every n-gram occurs in every one of these documents: uint32[Q, len(docs)]
    ti.documents_with_all([[[464, 2068], [11]]], cap=16)    # per group of n-grams: the documents that hold all of them
    ti.documents_with_cnf([[[[464, 2068], [7]], [[11]]]], exclude=[[[13]]])   # (A or B) and C, but not D: the documents
    ti.matching_statistics([text])         # per position of a query text: the longest prefix of what follows that the corpus holds
    ti.matched_spans([text], min_length=8)    # its maximal verbatim spans as (position, length, count, first)
    ti.coverage([text], min_length=8)      # how many of its tokens lie inside such a span, the longest one, how many there are
    ti.infgram([text])                     # per position: the longest context the corpus holds, its count, its count with the token
    ti.infgram_probs([text])               # the infinity-gram probability of every token: token_count / context_count
    ti.infgram_summary([text])             # per text: tokens scored, seen, certain, the longest context and the sum of the lengths

On top of the handle API of include/sa_hip.h section 6 (suffixarray_amd._capi.TokenIndex).  No CPU fallback.
"""
import numpy as np

from . import _capi


class TokenIndex:
    def __init__(self, tokens, k=None, device=0, doc_starts=None):
        """tokens: int sequence or array with symbols in [0, k) (k defaults to max + 1), at most 2^31 - 1 of them.
        doc_starts: see set_documents."""
        self._idx = _capi.TokenIndex.build(tokens, k, device)
        self.n = int(self._idx.info()["n"])
        if doc_starts is not None:
            try:
                self.set_documents(doc_starts)
            except Exception:
                self.close()
                raise

    def set_documents(self, starts):
        """Document d is tokens[starts[d] : starts[d + 1]] (the last one runs to the end): starts[0] == 0, non-decreasing, <= n.
        Equal neighbours are empty documents.  An occurrence belongs to the document of its first token; separate documents with
        a token of their own to keep n-grams from running over a boundary.  A second call replaces the table, None removes it."""
        self._idx.set_documents(starts)

    def locate(self, ngram, limit):
        """-> (doc, offset), int32 arrays: the first `limit` occurrences of one n-gram in suffix order, each as its document and
        the offset inside it: tokens[starts[doc] + offset :] starts with the n-gram."""
        r = self._idx.locate_batch([list(ngram)], cap=max(int(limit), 1))
        w = min(int(r["heads"]["written"][0]), int(limit))
        return r["docs"][0, :w].copy(), r["offsets"][0, :w].copy()

    def documents(self, ngrams, cap=16, budget=None, longest_suffix=False, max_length=None):
        """Which documents hold every n-gram.  -> dict of arrays: docs int32[Q, cap] and offsets int32[Q, cap], of which the first
        written[i] are valid in row i: the distinct documents in order of first appearance by rank, each with the offset of its
        smallest-rank occurrence; distinct[i] = distinct documents among the examined[i] = min(count[i], budget) first ranks;
        exact[i] = every occurrence was examined, so distinct[i] is the document frequency.  longest_suffix: as in next_tokens,
        without the demand for a next token."""
        r = self._idx.docs_batch(ngrams, cap=cap, budget=budget or 0, mode=1 if longest_suffix else 0, max_length=max_length or 0,
                                 need_next=False)
        h = r["heads"]
        return {"docs": r["docs"], "offsets": r["offsets"], "written": h["written"].copy(), "distinct": h["distinct"].copy(),
                "examined": h["examined"].copy(), "count": h["count"].copy(), "exact": h["examined"] == h["count"]}

    def document_counts(self, ngrams, budget=None):
        """-> (distinct uint32[Q], exact bool[Q]): in how many documents every n-gram occurs (counted over its first `budget`
        occurrences in suffix order when given; exact says that these were all)"""
        h = self._idx.docs_batch(ngrams, cap=0, budget=budget or 0)["heads"]
        return h["distinct"].copy(), h["examined"] == h["count"]

    def prepare_document_ranks(self):
        """Build the rank-by-document array (4 bytes per token) that term_counts and documents_with_all need; they call this on
        first use.  set_documents drops it."""
        self._idx.prepare_doc_ranks(True)

    def term_counts(self, ngrams, docs):
        """-> uint32[len(ngrams), len(docs)]: how often n-gram i occurs in document docs[j] (its term frequency there); a document
        id outside the table counts 0."""
        docs = np.ascontiguousarray(docs, dtype=np.int64).reshape(-1)
        if docs.size and (docs.min() < -2 ** 31 or docs.max() > 2 ** 31 - 1):
            raise ValueError("docs: document ids are int32")
        buf, off = self._idx._packed(ngrams)
        q = max(off.size - 1, 0)
        if q == 0 or docs.size == 0:
            return np.zeros((q, docs.size), np.uint32)
        self.prepare_document_ranks()
        rows = np.broadcast_to(docs.astype(np.int32), (q, docs.size))
        return self._idx.doc_counts_batch((buf, off), rows)["counts"]

    @staticmethod
    def _grouped(groups):
        flat, goff = [], [0]
        for g in groups:
            g = [list(x) for x in g]
            if not 1 <= len(g) <= _capi.TOKEN_ALL_MAX:
                raise ValueError("a group holds 1 .. %d n-grams" % _capi.TOKEN_ALL_MAX)
            flat += g
            goff.append(len(flat))
        return flat, np.array(goff, np.uint64)

    def documents_with_all(self, groups, cap=16, budget=None, longest_suffix=False, max_length=None):
        """Which documents hold ALL n-grams of a group (an AND query).  groups: a list of lists of n-grams, 1 .. 16 per group.
        -> one dict per group: documents and offsets (int32 arrays, at most cap entries: the matching documents in the rank order
        of the group's rarest n-gram, each with the offset of that n-gram's smallest-rank occurrence in it), matched (how many
        documents matched among the first `budget` occurrences of the rarest n-gram), exact (these were all its occurrences, so
        matched is the number of documents that hold all n-grams), driver (the index of that n-gram inside the group)."""
        flat, goff = self._grouped(groups)
        if not len(groups):
            return []
        self.prepare_document_ranks()
        r = self._idx.all_batch(flat, goff, cap=cap, budget=budget or 0, mode=1 if longest_suffix else 0, max_length=max_length or 0,
                                need_next=False)
        out = []
        for i, h in enumerate(r["heads"]):
            w = int(h["written"])
            out.append({"documents": r["docs"][i, :w].copy(), "offsets": r["offsets"][i, :w].copy(), "matched": int(h["matched"]),
                        "exact": bool(h["examined"] == h["count"]), "driver": int(h["driver"])})
        return out

    def count_documents_with_all(self, groups, budget=None):
        """-> (matched uint32[G], exact bool[G]): in how many documents all n-grams of every group occur"""
        flat, goff = self._grouped(groups)
        if not len(groups):
            return np.zeros(0, np.uint32), np.zeros(0, np.bool_)
        self.prepare_document_ranks()
        h = self._idx.all_batch(flat, goff, cap=0, budget=budget or 0)["heads"]
        return h["matched"].copy(), h["examined"] == h["count"]

    @staticmethod
    def _cnf_tables(queries, exclude):
        """-> (literals, clause offsets uint64, negated uint8, group offsets uint64) of CNF queries; exclude[i] becomes one negated
        clause behind the clauses of query i"""
        if exclude is not None and len(exclude) != len(queries):
            raise ValueError("exclude: one list of n-grams per query (an empty one or None for no exclusion)")
        flat, coff, neg, goff = [], [0], [], [0]
        for i, q in enumerate(queries):
            clauses = [([list(x) for x in c], 0) for c in q]
            if not clauses:
                raise ValueError("a query holds at least one clause")
            ex = exclude[i] if exclude is not None else None
            if ex is not None and len(ex):
                clauses.append(([list(x) for x in ex], 1))
            if len(clauses) > _capi.TOKEN_CNF_MAX_CLAUSES:
                raise ValueError("a query holds at most %d clauses, its exclusion included" % _capi.TOKEN_CNF_MAX_CLAUSES)
            if sum(len(c) for c, _ in clauses) > _capi.TOKEN_CNF_MAX_LITERALS:
                raise ValueError("a query holds at most %d n-grams" % _capi.TOKEN_CNF_MAX_LITERALS)
            for c, n in clauses:
                if not c:
                    raise ValueError("a clause holds at least one n-gram")
                flat += c
                coff.append(len(flat))
                neg.append(n)
            goff.append(len(neg))
        return flat, np.array(coff, np.uint64), np.array(neg, np.uint8), np.array(goff, np.uint64)

    def documents_with_cnf(self, queries, exclude=None, cap=16, budget=None, longest_suffix=False, max_length=None):
        """Which documents satisfy a CNF query: queries[i] is a list of clauses, a clause a list of n-grams of which the document
        holds at least one; exclude[i] (optional) is a list of n-grams none of which may occur.  At most 16 clauses (the exclusion
        counts as one) and 64 n-grams per query.  -> one dict per query: documents and offsets (int32 arrays, at most cap entries:
        the matching documents in the order of the driver clause's n-grams and then by rank, each with the offset of the occurrence
        that listed it), matched (how many documents matched among the first `budget` occurrences of the driver clause), exact
        (these were all its occurrences, so matched is the number of documents that satisfy the query), driver (the index of the
        clause with the fewest occurrences, which was walked), duplicates (documents met again under a later n-gram of the driver)."""
        flat, coff, neg, goff = self._cnf_tables(queries, exclude)
        if not len(queries):
            return []
        self.prepare_document_ranks()
        r = self._idx.cnf_batch(flat, coff, neg, goff, cap=cap, budget=budget or 0, mode=1 if longest_suffix else 0,
                                max_length=max_length or 0, need_next=False)
        out = []
        for i, h in enumerate(r["heads"]):
            w = int(h["written"])
            out.append({"documents": r["docs"][i, :w].copy(), "offsets": r["offsets"][i, :w].copy(), "matched": int(h["matched"]),
                        "exact": bool(h["examined"] == h["count"]), "driver": int(h["driver"]), "duplicates": int(h["duplicates"])})
        return out

    def count_documents_with_cnf(self, queries, exclude=None, budget=None):
        """-> (matched uint32[G], exact bool[G]): how many documents satisfy every CNF query"""
        flat, coff, neg, goff = self._cnf_tables(queries, exclude)
        if not len(queries):
            return np.zeros(0, np.uint32), np.zeros(0, np.bool_)
        self.prepare_document_ranks()
        h = self._idx.cnf_batch(flat, coff, neg, goff, cap=0, budget=budget or 0)["heads"]
        return h["matched"].copy(), h["examined"] == h["count"]

    def ranges(self, ngrams):
        """-> (first, count), uint32[Q] each: n-gram i occurs at the text positions SA[first[i] .. first[i] + count[i]);
        first[i] is the number of suffixes that sort before it, also when it does not occur.  ngrams: a list of int
        sequences, or (packed int32 array, uint64 offsets[Q + 1])."""
        r = self._idx.query_batch(ngrams)
        return r["first"].copy(), r["second"].copy()

    def count(self, ngrams):
        """occurrences of every n-gram: uint32[Q]"""
        return self.ranges(ngrams)[1]

    def positions(self, ngram, limit=None):
        """text positions of one n-gram in suffix order (at most `limit` of them): int32 array"""
        first, count = self.ranges([list(ngram)])
        c = int(count[0]) if limit is None else min(int(count[0]), int(limit))
        return self._idx.sa_range(int(first[0]), c)

    def longest_suffix(self, contexts, max_length=None, need_next=True):
        """-> (length, first, count), uint32[Q] each: the longest suffix of context i (at most max_length symbols) that occurs in
        the text -- with need_next, that occurs with a symbol behind it -- and its range.  length 0: nothing matched, {0, n}."""
        s = self._idx.spans_batch(contexts, mode=1, max_length=max_length or 0, need_next=need_next)
        return s["length"].copy(), s["first"].copy(), s["count"].copy()

    def next_tokens(self, ngrams, cap=64, longest_suffix=False, max_length=None):
        """Which tokens follow every n-gram, and how often.  -> dict of arrays: symbols int32[Q, cap] (ascending) and counts
        uint32[Q, cap], of which the first written[i] are valid in row i; total[i] = occurrences that have a next token;
        length[i] = matched symbols; complete[i] = every distinct next token fits in cap (else the cap smallest are given).
        longest_suffix: an n-gram backs off to its longest suffix (at most max_length symbols) that has a next token."""
        r = self._idx.next_batch(ngrams, cap=cap, mode=1 if longest_suffix else 0, max_length=max_length or 0, need_next=True)
        h = r["heads"]
        return {"symbols": r["symbols"], "counts": r["counts"], "written": h["written"].copy(), "total": h["total"].copy(),
                "length": r["spans"]["length"].copy(), "complete": h["covered"] == h["total"]}

    def next_token_counts(self, ngram, cap=64, longest_suffix=False, max_length=None):
        """{token: count} of what follows one n-gram (the cap smallest tokens when there are more)"""
        r = self.next_tokens([list(ngram)], cap=cap, longest_suffix=longest_suffix, max_length=max_length)
        w = int(r["written"][0])
        return {int(s): int(c) for s, c in zip(r["symbols"][0, :w], r["counts"][0, :w])}

    def top_next_tokens(self, ngrams, k=8, longest_suffix=False, max_length=None, budget=None):
        """The k (1 .. 64) most frequent tokens behind every n-gram.  -> dict of arrays: symbols int32[Q, k] and counts
        uint32[Q, k], by count descending, ties by token ascending, of which the first written[i] = min(k, distinct[i]) are valid
        in row i; distinct[i] = the distinct next tokens, covered[i] = the sum of the written counts, total[i] = occurrences that
        have a next token; spans as in _capi.TokenIndex.spans_batch.  budget: only the first `budget` occurrences in suffix order
        are walked (the tokens with the smallest ids); exact[i] = every occurrence was walked, so row i is the true top-k.
        longest_suffix: as in next_tokens."""
        r = self._idx.top_batch(ngrams, k=k, mode=1 if longest_suffix else 0, max_length=max_length or 0, need_next=True, budget=budget or 0)
        h = r["heads"]
        return {"symbols": r["symbols"], "counts": r["counts"], "written": h["written"].copy(), "distinct": h["distinct"].copy(),
                "covered": h["covered"].copy(), "total": h["total"].copy(), "exact": h["total"] <= (budget or 0xFFFFFFFF),
                "spans": r["spans"]}

    def sample_next(self, ngrams, draws=None, samples=1, seed=None, longest_suffix=True, max_length=None):
        """Next tokens drawn with the corpus's probability: int32[Q, samples], -1 where nothing follows.  draws: uint64[Q, samples]
        (or [Q]), draw d picks the occurrence floor(d * total / 2^64) of the context's total in suffix order -- the same draws
        give the same tokens; without them they come from np.random.default_rng(seed).  longest_suffix: a context backs off to
        its longest suffix (at most max_length symbols) that has a next token."""
        q = len(ngrams[1]) - 1 if isinstance(ngrams, tuple) else len(ngrams)
        if draws is None:
            draws = np.random.default_rng(seed).integers(0, 2 ** 64, size=(q, int(samples)), dtype=np.uint64)
        return self._idx.sample_batch(ngrams, draws, mode=1 if longest_suffix else 0, max_length=max_length or 0, need_next=True)["symbols"]

    def matching_statistics(self, docs, max_length=None):
        """Which parts of query texts stand verbatim in the corpus.  docs: a list of int sequences.  -> one (length, count, first)
        per document, uint32 arrays over its positions: length[i] = the longest prefix of doc[i:] (at most max_length symbols)
        that the corpus holds, count[i] its occurrences, SA[first[i] .. first[i] + count[i]) where.  length 0: {first 0, count n}."""
        buf, off, q = self._idx._contexts(docs)
        s = self._idx.match_batch((buf, off), max_length=max_length or 0)
        cut = [(int(off[d]), int(off[d + 1])) for d in range(q)]
        return [(s["length"][a:b].copy(), s["count"][a:b].copy(), s["first"][a:b].copy()) for a, b in cut]

    def matched_spans(self, docs, min_length, max_length=None, cap=64):
        """The maximal verbatim spans of every document: the matches of at least min_length symbols that no other position's match
        contains, in position order.  -> one (spans, complete) per document: spans = a list of (position, length, count, first),
        at most cap of them; complete = these are all."""
        r = self._idx.match_docs_batch(docs, min_length=min_length, max_length=max_length or 0, cap=max(int(cap), 1))
        out = []
        for d, h in enumerate(r["heads"]):
            w = min(int(h["written"]), int(cap))
            o = r["out_spans"][d, :w]
            out.append(([(int(p), int(l), int(c), int(f)) for p, l, c, f in zip(r["positions"][d, :w], o["length"], o["count"], o["first"])],
                        int(h["maximal"]) <= int(cap)))
        return out

    def coverage(self, docs, min_length, max_length=None):
        """-> dict of uint32[Q] arrays: covered = the tokens of every document that lie inside a match of at least min_length
        symbols, longest = its longest match (whatever min_length is), maximal = the number of its maximal spans."""
        h = self._idx.match_docs_batch(docs, min_length=min_length, max_length=max_length or 0, cap=0)["heads"]
        return {"covered": h["covered"].copy(), "longest": h["longest"].copy(), "maximal": h["maximal"].copy()}

    def infgram(self, docs, max_length=None):
        """The infinity-gram score of query texts.  docs: a list of int sequences.  -> one (length, context_count, token_count) per
        document, uint32 arrays over its positions: length[i] = the longest doc[i - L : i] (at most max_length symbols) that the
        corpus holds with a token behind it, context_count[i] how often (length 0: n), token_count[i] how often followed by
        doc[i]."""
        buf, off, q = self._idx._contexts(docs)
        s = self._idx.score_batch((buf, off), max_length=max_length or 0, heads=False)["scores"]
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
        """-> dict of per-document arrays: scored = its tokens, seen = those the corpus has behind their context (token_count > 0),
        certain = those that are the only token ever behind it (token_count == context_count), longest = the longest context,
        length_sum = the sum of the context lengths (uint64)."""
        h = self._idx.score_batch(docs, max_length=max_length or 0, scores=False)["heads"]
        return {k: h[k].copy() for k in ("scored", "seen", "certain", "longest", "length_sum")}

    def info(self):
        return self._idx.info()

    def close(self):
        self._idx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
