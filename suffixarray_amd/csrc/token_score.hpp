// token_score.hpp -- the infinity-gram score of query texts against the token index: for every position of a text the longest
// context before it that the corpus holds with a token behind it, how often, and how often followed by the token that stands
// there; per query document the sums a perplexity needs (sa_hip_token_index_score_*).
//
// A batch is Q query documents in the layout of token_match.hpp, a position a flat index j, s(j) the start of j's document,
// M = max_length (0: no cap).  For a context C the effective count is eff(C) = count(C) - ended(C): its occurrences that have a
// token behind them (the empty context: n).
//   L(j)           the largest L <= min(j - s(j), M, n) with eff(patterns[j - L .. j)) >= 1;
//   context_count  that eff: >= 1 whenever n >= 1;
//   token_count    the occurrences of patterns[j - L .. j], the context with the token at j appended: <= context_count;
//   first          what tq_range gives for that (L + 1)-gram, exact also when it does not occur.
// n == 0, and a position outside every document, give {0, 0, 0, 0}.
//
// Two facts carry the kernel (DESIGN.md 9s has the arguments):
//   1  with ms of token_match.hpp over the same batch and cap, end(i) = i + ms(i) is non-decreasing, and patterns[i .. j) occurs
//      iff end(i) >= j.  So the smallest start i in [max(s(j), j - M), j] whose context occurs comes from a binary search over the
//      16-byte match records, without one read of the index.
//   2  eff(C) >= 1 is monotone in the start (a context with a token behind it leaves every suffix of itself with one), and a
//      context that occurs has eff == 0 only when count == 1 and the lone suffix has ended: the context is the corpus's tail and
//      stands nowhere else.  So way 1 probes the context of fact 1 once and, in that one case, goes on as way 2 does.
//
//   tq_score_kernel       one lane per position, BLOCK threads, no LDS.  The document's start by the upper bound over offsets of
//                         tq_match_kernel.  Way 1 (ms != nullptr): fact 1, then one tq_range; where its eff is 0, way 2 over the
//                         shorter contexts.  Way 2 (ms == nullptr): the binary search over L of tq_span_kernel's mode 1 on the
//                         text in place, one tq_range per probe.  The numerator needs no further range search: inside the
//                         context's range s(r) = T[SA[r] + L] is non-decreasing with the ended suffix first (token_next.hpp), so
//                         two bounds over the ranks, comparing one symbol each (from K[r] when L <= 1), give {first, token_count}.
//   tq_score_docs_kernel  one wave per document, NEXT_WAVES per workgroup, no LDS.  The document's records in windows of 64, read
//                         coalesced (16 bytes per lane, the next window's load in flight: tq_doc_windows), summed per lane and
//                         reduced once with wave_reduce; lane 0 writes the head {scored, seen, certain, longest, length_sum}.
//
// Cost: a probe whose suffix shares k symbols with the context reads k + 1 of them, so a text copied verbatim from the corpus
// costs about m * min(m, M) * log2 n symbol reads for its m positions in way 1 (one range search per position) and log2 min(m, M)
// times that in way 2; way 1 pays for the match launch before it (the same product once more).  max_length is the caller's lever.
//
// Bounds: every loop is bounded whatever the arrays hold.  The upper bound halves [0, Q] (<= 64 steps), the search over the match
// records and the search over L halve a range below 2^31 (<= SCORE_STEPS each), tq_range is <= 32 steps of comparisons of
// <= min(L, n) symbols, the two rank bounds halve a range clamped to [0, n) (<= STEPS), every text index is tested against n.  A
// start is clamped to [j - min(M, n), j] and to the document's start, which is clamped to j: no pattern symbol outside
// [0, total) is read.  Match records are read at indices in [0, total) for their length alone.  Records that no match launch
// wrote, or an in-range array that is not the suffix array, give unspecified answers, never a spin or a read outside the buffers.
//
// Not built: log-probability sums on the device; carrying LCPs across probes (Manber-Myers); one very long document split over
// several waves.  (The same over shard sets is token_shard_score.hpp, which says what is not built there.)
#pragma once
#include "token_match.hpp"

namespace sa {
namespace tq {

constexpr int SCORE_STEPS = 32;        // bound of the searches over a start or a length (total < 2^31)

struct ScoreArgs {
    const int32_t* pat;            // [total]
    const u64* off;                // [Q + 1]
    u64 Q;
    u64 total;                     // positions answered: offsets[Q]
    u32 max_length;                // 0: no cap
    const sa_hip_token_span* ms;   // [total] as tq_match_kernel wrote them for this batch and cap; nullptr: way 2
    sa_hip_token_score* scores;    // [total]
};

// the span of the context P[0 .. L); its effective count is count - ended: the occurrences that have a token behind them
__device__ __forceinline__ sa_hip_token_span tq_score_probe(const View& x, const int32_t* __restrict__ P, u64 L) {
    const sa_hip_pair_u32 r = tq_range(x, P, L);
    sa_hip_token_span s;
    s.first = r.first; s.count = r.second;
    s.length = (u32)L;
    s.ended = tq_span_ended(x, r.first, r.second, L);
    return s;
}

// {first, count} of the context's range [a, e) narrowed by the symbol v at depth L: the ranks whose next symbol is < v (the
// ended suffix, which has none, among them) stand before, those whose next symbol is v are counted.  Both bounds in one loop.
__device__ __forceinline__ sa_hip_pair_u32 tq_score_narrow(const View& x, u32 a, u32 e, u32 L, int32_t v) {
    u32 lo1 = a, hi1 = e, lo2 = a, hi2 = e;
    for (int s = 0; s < STEPS && (lo1 < hi1 || lo2 < hi2); ++s) {
        const u32 m1 = lo1 + ((hi1 - lo1) >> 1), m2 = lo2 + ((hi2 - lo2) >> 1);
        const bool live1 = lo1 < hi1, live2 = lo2 < hi2;
        int32_t s1 = 0, s2 = 0;
        const bool ok1 = live1 && tq_next_symbol(x, m1, L, &s1);
        bool ok2 = ok1;
        if (live1 && m2 == m1) s2 = s1;                       // while both searches walk together
        else ok2 = live2 && tq_next_symbol(x, m2, L, &s2);
        if (live1) { if (!ok1 || s1 < v) lo1 = m1 + 1; else hi1 = m1; }
        if (live2) { if (!ok2 || s2 <= v) lo2 = m2 + 1; else hi2 = m2; }
    }
    sa_hip_pair_u32 res;
    res.first = lo1;
    res.second = (lo2 < lo1 ? lo1 : lo2) - lo1;   // an array that is not sorted cannot turn the range inside out
    return res;
}

// One lane per position.
__global__ __launch_bounds__(BLOCK) void tq_score_kernel(View x, ScoreArgs g) {
    const u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= g.total) return;
    sa_hip_token_score sc{0u, 0u, 0u, 0u};
    // ub = the entries of offsets[0 .. Q] that are <= j: offsets[ub - 1] is the start of j's document
    u64 lo = 0, hi = g.Q + 1;
    for (int st = 0; st < MATCH_DOC_STEPS && lo < hi; ++st) {
        const u64 m = lo + ((hi - lo) >> 1);
        if (g.off[m] <= j) lo = m + 1; else hi = m;
    }
    if (lo == 0 || lo > g.Q || x.n == 0) { g.scores[j] = sc; return; }   // outside every document, or nothing to count
    u64 start = g.off[lo - 1];
    if (start > j) start = j;                                           // (offsets that do not ascend: a bound for the loads)
    u64 Lmax = j - start;
    if (g.max_length && Lmax > g.max_length) Lmax = g.max_length;
    if (Lmax > x.n) Lmax = x.n;                                         // no more than n symbols match
    const int32_t* const E = g.pat + j;                                 // a context of L symbols is E[-L .. 0), the token E[0]

    // the longest context with an effective count >= 1 lies in [Llo, Lhi]; c is the span of Llo (L = 0: {0, n})
    u64 Llo = 0, Lhi = Lmax;
    sa_hip_token_span c{0u, x.n, 0u, 0u};
    if (g.ms && Lmax > 0) {
        // fact 1: the smallest start i in [j - Lmax, j] with end(i) >= j (i == j always qualifies)
        u64 a = j - Lmax, b = j;
        for (int st = 0; st < SCORE_STEPS && a < b; ++st) {
            const u64 i = a + ((b - a) >> 1);
            if (i + (u64)g.ms[i].length >= j) b = i; else a = i + 1;
        }
        Lhi = j - b;
        if (Lhi > 0) {
            const sa_hip_token_span p = tq_score_probe(x, E - Lhi, Lhi);
            if (p.count > p.ended) { Llo = Lhi; c = p; } else --Lhi;      // fact 2: the corpus's tail, go on over the shorter ones
        }
    }
    for (int probe = 0; probe < SCORE_STEPS && Llo < Lhi; ++probe) {
        const u64 L = Llo + (Lhi - Llo + 1) / 2;
        const sa_hip_token_span p = tq_score_probe(x, E - L, L);
        if (p.count > p.ended) { Llo = L; c = p; } else Lhi = L - 1;
    }
    // the context's range as it is walked: clamped to the array (the ended suffix, when there is one, stands first in it)
    const u32 ra = c.first < x.n ? c.first : x.n;
    const u32 re = ra + (c.count < x.n - ra ? c.count : x.n - ra);
    const sa_hip_pair_u32 t = tq_score_narrow(x, ra, re, (u32)Llo, E[0]);
    sc.length = (u32)Llo;
    sc.context_count = c.count - c.ended;
    sc.token_count = t.second;
    sc.first = t.first;
    g.scores[j] = sc;
}

struct ScoreDocsArgs {
    const sa_hip_token_score* scores;  // [offsets[Q]], by position
    const u64* off;                    // [Q + 1]
    u64 Q;
    sa_hip_token_score_head* heads;    // [Q]
};

// One wave per document.  The walk is tq_doc_windows (token_match.hpp).
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_score_docs_kernel(ScoreDocsArgs g) {
    const u32 lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    for (u64 d = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); d < g.Q; d += waves) {
        const DocSpan doc = tq_doc_span(g.off, d);
        u64 length_sum = 0;            // this lane's share, as the three below
        u32 seen = 0, certain = 0, longest = 0;
        tq_doc_windows(doc, lane, [&](u64 j) { return tq_match_rec_load(g.scores + j); }, [&](u64, bool act, const MatchRecWords& w) {
            if (act) {
                const u32 length = w[offsetof(sa_hip_token_score, length) / 4];
                const u32 cc = w[offsetof(sa_hip_token_score, context_count) / 4];
                const u32 tc = w[offsetof(sa_hip_token_score, token_count) / 4];
                length_sum += length;
                seen += tc > 0 ? 1u : 0u;
                certain += tc == cc ? 1u : 0u;
                if (length > longest) longest = length;
            }
        });
        length_sum = wave_reduce(length_sum, ScanSum{});
        seen = wave_reduce(seen, ScanSum{});
        certain = wave_reduce(certain, ScanSum{});
        longest = wave_reduce(longest, ScanMax{});
        if (lane == 0) {
            sa_hip_token_score_head h;
            const u64 scored = doc.o1 - doc.o0;
            h.scored = scored > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)scored;
            h.seen = seen;
            h.certain = certain;
            h.longest = longest;
            h.length_sum = length_sum;
            g.heads[d] = h;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// total >= 1 positions (< 2^31), every pointer on the device; asynchronous on `stream`
inline int launch_score(const Index& x, hipStream_t stream, const ScoreArgs& g) {
    const u64 grid = (g.total + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(tq_score_kernel, dim3((u32)grid), dim3(BLOCK), 0, stream, x.view(), g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// Q >= 1 documents; every pointer on the device; asynchronous on `stream`
inline int launch_score_docs(hipStream_t stream, const ScoreDocsArgs& g) {
    hipLaunchKernelGGL(tq_score_docs_kernel, dim3(wave_row_grid(g.Q)), dim3(NEXT_WAVES * WAVE), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
