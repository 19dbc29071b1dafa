// token_shard_match.hpp -- matching statistics of query texts over a shard set (sa_hip_token_shards_match_*): for every position of
// a text the longest prefix of what follows that SOME shard holds, its span in every shard and the merged record.  The documents
// step is tq_match_docs_kernel of token_match.hpp, instantiated for the merged record.
//
// The batch layout, M = max_length, avail(j) and the flat positions are token_match.hpp's; total = offsets[Q], S shards, n_s the
// length of shard s.
//   ms(j)      the largest L <= min(avail(j), M) such that patterns[j .. j + L) occurs in some shard: the maximum over s of ms_s(j),
//              what shard s's own match answers.  Shards are cut at document boundaries, so no match spans a cut;
//   per_shard  [s * total + j] = shard s's mode-0 span of patterns[j .. j + ms(j)), as the set's mode-1 spans: count 0 with the exact
//              lower bound where the shard does not hold it, {first, 1, L, 1} where it only ends the shard's text, {0, n_s, 0, 0} for
//              L = 0, zeros from an empty shard and for a position outside every document;
//   merged     [j] = {length = ms(j), shards = the shards with a count > 0, count = the sum of the counts}.
//
// One lane per (position, shard) pair, t = j * S + s: the S shards of a position in neighbouring lanes, as tq_shard_range_kernel
// has them.  A query batch is often small (one document of 1000 tokens is 1000 positions), and a lane's search is a dependent chain
// of about min(m, M) * log2 n symbol reads: the pairs are what fills the device.
//
//   tq_shard_match_kernel        fact 1 of token_match.hpp in shard s: the document's end by the upper bound over offsets, len =
//                                min(avail, M, n_s), one tq_range, on a miss the two neighbours' tq_lcp.  ms_s(j) goes to the
//                                scratch word ms[j * S + s] (MATCH_OUTSIDE for a position outside every document); the range of a
//                                hit is left in the pair's own per_shard cell.  No second range search: most shards lose, and the
//                                length to search for is not known yet.
//   tq_shard_match_span_kernel   L = the maximum of the position's S scratch words, then the pair's exact span at L.  The shard whose
//                                own search hit at ms_s == L keeps that range (its own cell, which no other lane reads); every
//                                other shard searches once more.  The lengths come from the scratch and never from per_shard:
//                                this launch overwrites per_shard while other lanes of it still read, and that is why the scratch
//                                exists.
//   tq_shard_match_total_kernel  one lane per position: the counts summed as u64 in shard order (integers: deterministic), the
//                                shards with a count counted, merged[j] written.
//
// Bounds: every loop is bounded whatever the arrays hold.  The upper bound halves [0, Q] (<= MATCH_DOC_STEPS), a document's end is
// clamped to `total`, tq_range takes <= STEPS steps of <= min(m, n_s) symbols, tq_lcp reads <= min(m, n_s - p) symbols, a rank is
// tested against [0, n_s) before SA is read, an empty shard is skipped, the span kernel's loop over the scratch is S <= 64 words and
// clamps L to what is left of the batch.  No LDS.
//
// Not built: documents (locate, document_counts) over shard sets; what token_match.hpp lists.
#pragma once
#include "token_match.hpp"
#include "token_shards.hpp"

namespace sa {
namespace tq {

constexpr u32 MATCH_OUTSIDE = 0xFFFFFFFFu;   // scratch word of a position outside every document (a length is < 2^31)

struct ShardMatchArgs {
    const View* tab;                     // [S]
    u32 S;
    u32 max_length;                      // 0: no cap
    const int32_t* pat;                  // [total]
    const u64* off;                      // [Q + 1]
    u64 Q;
    u64 total;                           // positions answered: offsets[Q]
    u32* ms;                             // [total * S], position-major: scratch of the set
    sa_hip_token_span* per;              // [S * total], shard-major
    sa_hip_token_shards_match* merged;   // [total]
};

__global__ __launch_bounds__(BLOCK) void tq_shard_match_kernel(ShardMatchArgs g) {
    const u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const Pair p = tq_pair_of(t, g.S);
    const u64 j = p.row;
    const u32 s = p.s;
    if (j >= g.total) return;
    const u64 cell = (u64)s * g.total + j;
    sa_hip_token_span sp{0u, 0u, 0u, 0u};
    // ub = the entries of offsets[0 .. Q] that are <= j: offsets[ub] is the end of j's document
    u64 lo = 0, hi = g.Q + 1;
    for (int st = 0; st < MATCH_DOC_STEPS && lo < hi; ++st) {
        const u64 m = lo + ((hi - lo) >> 1);
        if (g.off[m] <= j) lo = m + 1; else hi = m;
    }
    if (lo == 0 || lo > g.Q) { g.ms[t] = MATCH_OUTSIDE; g.per[cell] = sp; return; }
    const View x = g.tab[s];
    if (x.n == 0) { g.ms[t] = 0u; g.per[cell] = sp; return; }             // an empty shard matches nothing
    u64 end = g.off[lo];
    if (end > g.total) end = g.total;
    u64 len = end > j ? end - j : 0;
    if (g.max_length && len > g.max_length) len = g.max_length;
    if (len > x.n) len = x.n;                                             // no more than n_s symbols match in this shard
    const int32_t* P = g.pat + j;
    const sa_hip_pair_u32 r = tq_range(x, P, len);
    u64 L = len;
    if (r.second == 0 && len > 0) {
        const u32 at = r.first < x.n ? r.first : x.n;
        const u64 below = at > 0 ? tq_lcp(x.T, x.n, x.sa[at - 1], P, len) : 0;
        const u64 above = at < x.n ? tq_lcp(x.T, x.n, x.sa[at], P, len) : 0;
        L = below > above ? below : above;
    } else if (len > 0) {
        sp.first = r.first; sp.count = r.second;                          // a hit: the range of P[0 .. ms_s), kept for the span kernel
    }
    g.ms[t] = (u32)L;
    g.per[cell] = sp;
}

__global__ __launch_bounds__(BLOCK) void tq_shard_match_span_kernel(ShardMatchArgs g) {
    const Pair p = tq_pair_of((u64)blockIdx.x * BLOCK + threadIdx.x, g.S);
    const u64 j = p.row;
    const u32 s = p.s;
    if (j >= g.total) return;
    const u32* const w = g.ms + j * g.S;
    u64 L = 0;
    bool outside = false;
    for (u32 k = 0; k < g.S; ++k) {
        const u32 v = w[k];
        if (v == MATCH_OUTSIDE) outside = true; else if (v > L) L = v;
    }
    const u64 cell = (u64)s * g.total + j;
    sa_hip_token_span sp{0u, 0u, 0u, 0u};
    const View x = g.tab[s];
    if (!outside && x.n != 0) {
        if (L > g.total - j) L = g.total - j;                             // (ms never passes its document: a bound for the loads)
        const sa_hip_token_span mine = g.per[cell];
        const bool own = L > 0 && w[s] == L && mine.count > 0;            // this shard's own search hit at L: its range stands
        const sa_hip_pair_u32 r = own ? sa_hip_pair_u32{mine.first, mine.count} : tq_range(x, g.pat + j, L);
        sp = tq_span_of(x, r, L);                                         // (L == 0: {0, n_s} without a search)
    }
    g.per[cell] = sp;
}

__global__ __launch_bounds__(BLOCK) void tq_shard_match_total_kernel(ShardMatchArgs g) {
    const u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= g.total) return;
    sa_hip_token_shards_match m{0u, 0u, 0ull};
    for (u32 s = 0; s < g.S; ++s) {
        const sa_hip_token_span sp = g.per[(u64)s * g.total + j];
        if (sp.length > m.length) m.length = sp.length;                   // (every shard that is not empty says the same L)
        m.count += sp.count;
        m.shards += sp.count > 0 ? 1u : 0u;
    }
    g.merged[j] = m;
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// total >= 1 positions (< 2^31), every pointer on the device, g.ms[total * S]; asynchronous on `stream`
inline int launch_shard_match(hipStream_t stream, const ShardMatchArgs& g) {
    const u32 grid = shard_pair_grid(g.total, g.S, "sa_hip_token_shards_match_batch", "too many positions for one launch");
    if (!grid) return SA_HIP_EINVAL;
    hipLaunchKernelGGL(tq_shard_match_kernel, dim3(grid), dim3(BLOCK), 0, stream, g);
    hipLaunchKernelGGL(tq_shard_match_span_kernel, dim3(grid), dim3(BLOCK), 0, stream, g);
    hipLaunchKernelGGL(tq_shard_match_total_kernel, dim3((u32)((g.total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
