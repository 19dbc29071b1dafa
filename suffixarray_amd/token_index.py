"""`TokenIndex` -- n-gram counts, ranges and positions over a token corpus (int32 ids) on the device.

    ti = TokenIndex(tokens)                # upload, suffix array (sa_hip_libsais_int's build), search structures
    ti.count([[464, 2068], [11]])          # occurrences of every n-gram: uint32[Q]
    ti.positions([464, 2068], limit=10)    # where: text positions in suffix order

On top of the handle API of include/sa_hip.h section 6 (suffixarray_amd._capi.TokenIndex).  No CPU fallback.
"""
import numpy as np

from . import _capi


class TokenIndex:
    def __init__(self, tokens, k=None, device=0):
        """tokens: int sequence or array with symbols in [0, k) (k defaults to max + 1), at most 2^31 - 1 of them."""
        self._idx = _capi.TokenIndex.build(tokens, k, device)
        self.n = int(self._idx.info()["n"])

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

    def info(self):
        return self._idx.info()

    def close(self):
        self._idx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
