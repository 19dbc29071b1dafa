// token_shard_score.hpp -- the infinity-gram score of query texts over a shard set (sa_hip_token_shards_score_*): for every position
// of a text the longest context before it that SOME shard holds with a token behind it, how often over all shards, how often
// followed by the token that stands there, and the span of that (L + 1)-gram in every shard; per query document the sums of
// token_score.hpp's head.
//
// The batch layout, M = max_length, s(j) and the flat positions are token_score.hpp's; total = offsets[Q], S shards, n_s the length
// of shard s, max_n the longest.  eff_s(C) = count_s(C) - ended_s(C), the empty context: n_s; eff(C) = the sum over s.
//   L(j)           the largest L <= min(j - s(j), M, max_n) with eff(patterns[j - L .. j)) >= 1;
//   scores[j]      {length = L(j), shards = the shards that hold patterns[j - L .. j], context_count = eff of the context,
//                  token_count = the occurrences of patterns[j - L .. j] over all shards};
//   per_shard      [s * total + j] = shard s's mode-0 span of the (L + 1)-gram patterns[j - L .. j]: {first, count, L + 1, ended}, the
//                  exact lower bound where the shard does not hold it (also where it does not hold the context), zeros from an
//                  empty shard and, in every shard, for a position outside every document.
//
// Two facts carry the kernels (DESIGN.md 9u has the arguments):
//   1  with the merged ms of token_shard_match.hpp over the same batch and cap, end(i) = i + ms(i) is non-decreasing and
//      patterns[i .. j) occurs in some shard iff end(i) >= j: the smallest start whose context occurs comes from the binary search
//      of tq_score_kernel, here over the 16-byte merged records, read for .length alone;
//   2  eff >= 1 is monotone in the start (a sum of monotone terms), and a context that occurs has eff == 0 exactly when every shard
//      that holds it holds it once and as the tail of its text.  Up to S shards can share a tail, so the test is the sum and not
//      "count == 1"; the search over the shorter contexts that follows probes with "some shard has an effective count >= 1".
//
// The chains that touch an index run one lane per (position, shard) pair, t = j * S + s, as token_shard_match.hpp has them.  The
// scratch of the set is three words per pair, each plane position-major [j * S + s]:
//   w0  eff_s of the candidate context (SCORE_OUTSIDE for a position outside every document): written by the probe, read by all S
//       lanes of the position in the narrow launch and never written there;
//   w1  eff_s of the context at the final L: written by the narrow launch, read by the total launch;
//   w2  the candidate length Lhi after the probe, the final L after the narrow launch: a lane reads and writes its own word only.
//
//   tq_shard_score_probe_kernel   the document's start by the upper bound over offsets, Lmax = min(j - s(j), M, max_n); with merged,
//                                 fact 1 gives Lhi (every lane of a position repeats the search over the cached records), without,
//                                 Lhi = Lmax.  One tq_range of patterns[j - Lhi .. j) in the lane's shard; {first, count} stay in the
//                                 pair's per_shard cell, eff_s goes to w0, Lhi to w2.
//   tq_shard_score_narrow_kernel  the sum of the position's S words of w0.  >= 1: L = Lhi and the own cell's range is the context's.
//                                 0 with Lhi > 0: the search of fact 2 over [0, Lhi - 1], every probe a loop over the shards that
//                                 stops at the first that qualifies (tq_shard_span_kernel's probe), then tq_span_exact at the L
//                                 found in the own shard.  All S lanes of a position run that search and reach the same L: the case
//                                 is rare (DESIGN.md 9s's trace), the redundancy is accepted.  Then tq_score_narrow with the token at
//                                 j inside the own context range and tq_span_ended: the own cell is overwritten with the span of the
//                                 (L + 1)-gram, eff_s at L goes to w1, L to w2.  What other shards found comes from w0 alone, never
//                                 from a per_shard cell: this launch overwrites cells while other lanes still run.
//   tq_shard_score_total_kernel   one lane per position: context_count and token_count summed as u64 in shard order (integers:
//                                 deterministic), the shards with a token_count counted, scores[j] written.
//   tq_shard_score_docs_kernel    tq_score_docs_kernel's shape over the 24-byte record: one wave per document, NEXT_WAVES per
//                                 workgroup, windows of 64 records held as three pairs of words per lane, the next window's load in
//                                 flight, one wave_reduce per field, lane 0 writes the head.
//
// merged == nullptr ("way 2") is the same three launches with every position that the capped context misses taking the search over
// L: an independent path to the same bytes.
//
// Cost: a pair costs one range search of <= min(Lhi, n_s) symbols per step and two rank bounds of one symbol per step; the fallback
// costs <= SCORE_STEPS * S range searches in each of the position's S lanes.
//
// Bounds: every loop is bounded whatever the arrays hold.  The upper bound halves [0, Q] (<= MATCH_DOC_STEPS), the search over the
// merged records and the search over L halve a range below 2^31 (<= SCORE_STEPS each), tq_range is <= STEPS steps of comparisons of
// <= min(L, n_s) symbols, the two rank bounds halve a range clamped to [0, n_s), the loops over the shards and over the scratch
// words are S <= 64, an empty shard is skipped before its view is used, every text index is tested against n_s.  A start is clamped
// to [j - min(M, max_n), j] and to the document's start, which is clamped to j, and a length read back from the scratch is clamped
// to j: pattern symbols are read in [0, total) only.  Merged records are read at indices in [0, total) for their length alone.  A
// launch of more than 2^31 - 1 workgroups is refused.  No LDS; every store is an ordinary store from C++.
//
// Not built: log-probability sums on the device; carrying LCPs across probes; one very long document split over several waves; a
// fallback search shared by the S lanes of a position.
#pragma once
#include "token_score.hpp"
#include "token_shard_match.hpp"

namespace sa {
namespace tq {

constexpr u32 SCORE_OUTSIDE = 0xFFFFFFFFu;   // w0 of a position outside every document (an effective count is < 2^31)

struct ShardScoreArgs {
    const View* tab;                          // [S]
    u32 S;
    u32 max_n;                                // the longest shard
    u32 max_length;                           // 0: no cap
    const int32_t* pat;                       // [total]
    const u64* off;                           // [Q + 1]
    u64 Q;
    u64 total;                                // positions answered: offsets[Q]
    const sa_hip_token_shards_match* merged;  // [total] as the match launches wrote them for this batch and cap; nullptr: way 2
    u32* w;                                   // [3 * total * S]: scratch of the set, the planes w0, w1, w2
    sa_hip_token_shards_score* scores;        // [total]
    sa_hip_token_span* per;                   // [S * total], shard-major
};

__global__ __launch_bounds__(BLOCK) void tq_shard_score_probe_kernel(ShardScoreArgs g) {
    const u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const Pair p = tq_pair_of(t, g.S);
    const u64 j = p.row;
    const u32 s = p.s;
    if (j >= g.total) return;
    const u64 pairs = g.total * g.S;
    u32* const w0 = g.w;
    u32* const w2 = g.w + 2 * pairs;
    const u64 cell = (u64)s * g.total + j;
    sa_hip_token_span sp{0u, 0u, 0u, 0u};
    // ub = the entries of offsets[0 .. Q] that are <= j: offsets[ub - 1] is the start of j's document
    u64 lo = 0, hi = g.Q + 1;
    for (int st = 0; st < MATCH_DOC_STEPS && lo < hi; ++st) {
        const u64 m = lo + ((hi - lo) >> 1);
        if (g.off[m] <= j) lo = m + 1; else hi = m;
    }
    if (lo == 0 || lo > g.Q) { w0[t] = SCORE_OUTSIDE; w2[t] = 0u; g.per[cell] = sp; return; }
    u64 start = g.off[lo - 1];
    if (start > j) start = j;                                             // (offsets that do not ascend: a bound for the loads)
    u64 Lmax = j - start;
    if (g.max_length && Lmax > g.max_length) Lmax = g.max_length;
    if (Lmax > g.max_n) Lmax = g.max_n;                                   // no more than max_n symbols match anywhere
    u64 Lhi = Lmax;
    if (g.merged && Lmax > 0) {
        // fact 1: the smallest start i in [j - Lmax, j] with end(i) >= j (i == j always qualifies)
        u64 a = j - Lmax, b = j;
        for (int st = 0; st < SCORE_STEPS && a < b; ++st) {
            const u64 i = a + ((b - a) >> 1);
            if (i + (u64)g.merged[i].length >= j) b = i; else a = i + 1;
        }
        Lhi = j - b;
    }
    w2[t] = (u32)Lhi;
    const View x = g.tab[s];
    if (x.n == 0) { w0[t] = 0u; g.per[cell] = sp; return; }               // an empty shard holds no context
    const sa_hip_pair_u32 r = tq_range(x, g.pat + j - Lhi, Lhi);          // (a shard shorter than Lhi: count 0)
    sp.first = r.first; sp.count = r.second;
    w0[t] = r.second - tq_span_ended(x, r.first, r.second, Lhi);
    g.per[cell] = sp;
}

__global__ __launch_bounds__(BLOCK) void tq_shard_score_narrow_kernel(ShardScoreArgs g) {
    const u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const Pair p = tq_pair_of(t, g.S);
    const u64 j = p.row;
    const u32 s = p.s;
    if (j >= g.total) return;
    const u64 pairs = g.total * g.S;
    const u32* const w0 = g.w + j * g.S;
    u32* const w1 = g.w + pairs;
    u32* const w2 = g.w + 2 * pairs;
    u64 sum = 0;
    bool outside = false;
    for (u32 k = 0; k < g.S; ++k) {
        const u32 v = w0[k];
        if (v == SCORE_OUTSIDE) outside = true; else sum += v;
    }
    const u64 cell = (u64)s * g.total + j;
    sa_hip_token_span sp{0u, 0u, 0u, 0u};
    const View x = g.tab[s];
    if (outside || x.n == 0) { w1[t] = 0u; w2[t] = 0u; g.per[cell] = sp; return; }
    u64 L = w2[t];
    if (L > j) L = j;                                                     // (Lhi never passes the batch's start: a bound for the loads)
    const int32_t* const E = g.pat + j;                                   // a context of L symbols is E[-L .. 0), the token E[0]
    sa_hip_token_span c = g.per[cell];                                    // the own shard's range of the candidate context
    if (sum == 0 && L > 0) {
        // fact 2: every shard that holds the candidate holds it as its tail alone.  The longest shorter context that some shard
        // holds with a token behind it (L = 0 qualifies: this shard is not empty)
        u64 Llo = 0, Lhi = L - 1;
        for (int probe = 0; probe < SCORE_STEPS && Llo < Lhi; ++probe) {
            const u64 mid = Llo + (Lhi - Llo + 1) / 2;
            bool ok = false;
            for (u32 k = 0; k < g.S && !ok; ++k) {
                const View y = g.tab[k];
                if (y.n == 0) continue;
                const sa_hip_pair_u32 r = tq_range(y, E - mid, mid);
                u32 eff = r.second;
                if (r.second == 1) eff -= tq_span_ended(y, r.first, 1u, mid);   // only a lone suffix can be decided by it
                ok = eff != 0;
            }
            if (ok) Llo = mid; else Lhi = mid - 1;
        }
        L = Llo;
        c = tq_span_exact(x, E - L, L);
    } else {
        c.ended = tq_span_ended(x, c.first, c.count, L);
    }
    // the context's range as it is walked: clamped to the array (the ended suffix, when there is one, stands first in it)
    const u32 ra = c.first < x.n ? c.first : x.n;
    const u32 re = ra + (c.count < x.n - ra ? c.count : x.n - ra);
    const sa_hip_pair_u32 r = tq_score_narrow(x, ra, re, (u32)L, E[0]);
    sp.first = r.first; sp.count = r.second;
    sp.length = (u32)L + 1u;
    sp.ended = tq_span_ended(x, r.first, r.second, L + 1);
    w1[t] = c.count - c.ended;                                            // (ended is 1 only where count >= 1)
    w2[t] = (u32)L;
    g.per[cell] = sp;
}

__global__ __launch_bounds__(BLOCK) void tq_shard_score_total_kernel(ShardScoreArgs g) {
    const u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= g.total) return;
    const u64 pairs = g.total * g.S;
    const u32* const w1 = g.w + pairs + j * g.S;
    const u32* const w2 = g.w + 2 * pairs + j * g.S;
    sa_hip_token_shards_score sc{0u, 0u, 0ull, 0ull};
    for (u32 s = 0; s < g.S; ++s) {
        const u32 tc = g.per[(u64)s * g.total + j].count;
        if (w2[s] > sc.length) sc.length = w2[s];                         // (every shard that is not empty says the same L)
        sc.context_count += w1[s];
        sc.token_count += tc;
        sc.shards += tc > 0 ? 1u : 0u;
    }
    g.scores[j] = sc;
}

struct ShardScoreDocsArgs {
    const sa_hip_token_shards_score* scores;  // [offsets[Q]], by position
    const u64* off;                           // [Q + 1]
    u64 Q;
    sa_hip_token_score_head* heads;           // [Q]
};

// A lane holds a record as three pairs of words, whatever its fields are.
typedef u32 ScorePairWords __attribute__((ext_vector_type(2)));

__device__ __forceinline__ ScorePairWords tq_shard_score_words(const sa_hip_token_shards_score* p, int k) {
    ScorePairWords w;
    __builtin_memcpy(&w, reinterpret_cast<const char*>(p) + 8 * k, sizeof w);
    return w;
}

// One wave per document.  Every trip of the walk advances by one window of 64 positions.
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_shard_score_docs_kernel(ShardScoreDocsArgs g) {
    static_assert(sizeof(sa_hip_token_shards_score) == 24 && offsetof(sa_hip_token_shards_score, length) == 0 &&
                  offsetof(sa_hip_token_shards_score, context_count) == 8 && offsetof(sa_hip_token_shards_score, token_count) == 16,
                  "a record is three pairs of words: {length, shards}, context_count, token_count");
    const u32 lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    for (u64 d = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); d < g.Q; d += waves) {
        const u64 o0 = g.off[d], o1r = g.off[d + 1];
        const u64 o1 = o1r > o0 ? o1r : o0;
        u64 length_sum = 0;            // this lane's share, as the three below
        u32 seen = 0, certain = 0, longest = 0;
        ScorePairWords n0 = {0u, 0u}, n1 = {0u, 0u}, n2 = {0u, 0u};
        if (o0 + lane < o1) {
            n0 = tq_shard_score_words(g.scores + o0 + lane, 0);
            n1 = tq_shard_score_words(g.scores + o0 + lane, 1);
            n2 = tq_shard_score_words(g.scores + o0 + lane, 2);
        }
        for (u64 a = o0; a < o1; a += (u64)WAVE) {
            const u64 j = a + lane;
            const ScorePairWords head = n0, cc = n1, tc = n2;
            if (j + WAVE < o1) {
                n0 = tq_shard_score_words(g.scores + j + WAVE, 0);
                n1 = tq_shard_score_words(g.scores + j + WAVE, 1);
                n2 = tq_shard_score_words(g.scores + j + WAVE, 2);
            }
            if (j < o1) {
                const u32 length = head[0];
                length_sum += length;
                seen += (tc[0] | tc[1]) != 0u ? 1u : 0u;
                certain += (tc[0] == cc[0] && tc[1] == cc[1]) ? 1u : 0u;
                if (length > longest) longest = length;
            }
        }
        length_sum = wave_reduce(length_sum, ScanSum{});
        seen = wave_reduce(seen, ScanSum{});
        certain = wave_reduce(certain, ScanSum{});
        longest = wave_reduce(longest, ScanMax{});
        if (lane == 0) {
            sa_hip_token_score_head h;
            const u64 scored = o1 - o0;
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

// total >= 1 positions (< 2^31), every pointer on the device, g.w[3 * total * S]; asynchronous on `stream`
inline int launch_shard_score(hipStream_t stream, const ShardScoreArgs& g) {
    const u32 grid = shard_pair_grid(g.total, g.S, "sa_hip_token_shards_score_batch", "too many positions for one launch");
    if (!grid) return SA_HIP_EINVAL;
    hipLaunchKernelGGL(tq_shard_score_probe_kernel, dim3(grid), dim3(BLOCK), 0, stream, g);
    hipLaunchKernelGGL(tq_shard_score_narrow_kernel, dim3(grid), dim3(BLOCK), 0, stream, g);
    hipLaunchKernelGGL(tq_shard_score_total_kernel, dim3((u32)((g.total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// Q >= 1 documents; every pointer on the device; asynchronous on `stream`
inline int launch_shard_score_docs(hipStream_t stream, const ShardScoreDocsArgs& g) {
    hipLaunchKernelGGL(tq_shard_score_docs_kernel, dim3(wave_row_grid(g.Q)), dim3(NEXT_WAVES * WAVE), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
