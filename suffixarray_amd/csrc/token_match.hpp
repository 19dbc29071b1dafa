// token_match.hpp -- matching statistics of query texts against the token index: for every position of a text the longest
// prefix of what follows that the corpus holds, and per query document the maximal matches, the longest one and the covered
// tokens (sa_hip_token_index_match_*).
//
// A batch is Q query documents in the usual layout, document d = patterns[offsets[d] .. offsets[d + 1]); a position is a flat
// index j into patterns, avail(j) the tokens from j to the end of j's document, M = max_length (0: no cap).
//   ms(j)   the largest L <= min(avail(j), M, n) such that patterns[j .. j + L) occurs in the text;
//   match   the span {first, count, length = ms(j), ended} of that prefix: what tq_span_kernel answers in mode 0 for it.  L = 0
//           gives {0, n, 0, 0}; n == 0, and a position outside every document, give {0, 0, 0, 0};
//   end(j)  j + ms(j); it never passes the end of j's document.
//
// Three facts carry the kernels (DESIGN.md 9m has the arguments):
//   1  one search gives ms(j).  P = the capped prefix, r = tq_range(P).first, exact also for a miss.  P occurs: ms = |P|.  Else
//      every suffix that shares the most symbols with P stands next to P's place in suffix order, so ms = max(lcp(P, suffix
//      SA[r - 1]), lcp(P, suffix SA[r])), a neighbour that does not exist counting 0.  The span is one more tq_range of length ms.
//   2  end(j) is non-decreasing in j (ms(j + 1) >= ms(j) - 1 inside a document, also under the cap; a match never passes its
//      document's end).  A match of length >= 1 is maximal -- contained in no other position's match -- iff end(j) > end(j - 1):
//      the predecessor alone decides, and in flat coordinates a document's first position needs no special case.  A match that
//      contains another is longer, so "maximal among those of at least min_length" and "maximal, then of at least min_length"
//      are the same set.
//   3  the tokens of a document covered by matches of at least min_length number the sum over the qualifying j of
//      end(j) - max(j, E(j)), E(j) = the largest end of a qualifying position before j in the document (0: none).
//
//   tq_match_kernel       one lane per position, BLOCK threads.  The document's end by an upper bound over offsets (<= 64 steps),
//                         then fact 1: a range search, two neighbour LCPs (tq_lcp), and a second range search when 1 <= ms < |P|.
//   tq_match_docs_kernel  a template over the position's 16-byte record (here sa_hip_token_span; over a shard set the merged
//                         record of token_shard_match.hpp), of which it reads .length and which it copies out whole.
//                         One wave per document, NEXT_WAVES per workgroup, no LDS.  The document's positions by tq_doc_windows,
//                         spans[j] read coalesced (16 bytes per lane); the predecessor's end by
//                         lane_shift_up with prev_end carried across windows (fact 2), E by wave_scan_incl with max and a carried
//                         value (fact 3); a ballot and a popcount prefix give the output slots of the maximal matches of at least
//                         min_length.  Lanes with a slot < cap write positions[d * cap + slot] (the offset inside the document)
//                         and out_spans[d * cap + slot]; lane 0 writes the head {written, maximal, longest, covered}.  cap == 0
//                         computes the heads alone and touches neither array.
//
// Cost: a position costs about (search steps) x (symbols compared per step).  A probe whose suffix shares k symbols with P reads
// k + 1 of them, so a text copied verbatim from the corpus costs about m * min(m, M) * log2 n symbol reads for its m positions:
// max_length is the caller's lever.  The docs kernel streams 16 bytes per position once.
//
// Bounds: every loop is bounded whatever the arrays hold.  The upper bound halves [0, Q] (<= 64 steps), tq_range is <= 32 steps of
// comparisons of <= min(|P|, n) symbols, tq_lcp reads <= min(|P|, n - p) symbols, r - 1 and r are tested against [0, n) before SA
// is read, a document's end is clamped to `total` so no pattern symbol beyond it is read.  The docs kernel clamps a span's length
// to what is left of its document and advances by one window per trip.  An in-range array that is not the suffix array, or spans
// that no match launch wrote, give unspecified answers, never a spin or a read outside the buffers.
//
// Not built: carrying the LCPs of the search's two ends so that a probe's comparison starts behind them (Manber-Myers); starting
// position j + 1 from ms(j) - 1; one very long document split over several waves.  (The same over shard sets is
// token_shard_match.hpp, which says what is not built there.)
#pragma once
#include "token_next.hpp"

namespace sa {
namespace tq {

constexpr int MATCH_DOC_STEPS = 64;    // bound of the upper bound over offsets (Q + 1 < 2^64 entries)

// the equal leading symbols of suffix p and P[0 .. m): at most min(m, n - p) reads; a p outside the text shares none
__device__ __forceinline__ u64 tq_lcp(const int32_t* __restrict__ T, u32 n, u32 p, const int32_t* __restrict__ P, u64 m) {
    if (p >= n) return 0;
    const u64 avail = (u64)(n - p);
    const u64 len = m < avail ? m : avail;
    u64 j = 0;
    while (j < len && T[p + j] == P[j]) ++j;
    return j;
}

struct MatchArgs {
    const int32_t* pat;            // [total]
    const u64* off;                // [Q + 1]
    u64 Q;
    u64 total;                     // positions answered: offsets[Q]
    u32 max_length;                // 0: no cap
    sa_hip_token_span* spans;      // [total]
};

// One lane per position.
__global__ __launch_bounds__(BLOCK) void tq_match_kernel(View x, MatchArgs g) {
    const u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= g.total) return;
    sa_hip_token_span s{0u, 0u, 0u, 0u};
    // ub = the entries of offsets[0 .. Q] that are <= j: offsets[ub] is the end of j's document
    u64 lo = 0, hi = g.Q + 1;
    for (int st = 0; st < MATCH_DOC_STEPS && lo < hi; ++st) {
        const u64 m = lo + ((hi - lo) >> 1);
        if (g.off[m] <= j) lo = m + 1; else hi = m;
    }
    if (lo == 0 || lo > g.Q || x.n == 0) { g.spans[j] = s; return; }   // outside every document, or nothing to match
    u64 end = g.off[lo];
    if (end > g.total) end = g.total;                                   // (offsets[Q] == total: a bound for the loads all the same)
    u64 len = end > j ? end - j : 0;
    if (g.max_length && len > g.max_length) len = g.max_length;
    if (len > x.n) len = x.n;                                           // no more than n symbols match
    const int32_t* P = g.pat + j;
    sa_hip_pair_u32 r = tq_range(x, P, len);
    u64 L = len;
    if (r.second == 0 && len > 0) {
        const u32 at = r.first < x.n ? r.first : x.n;
        const u64 below = at > 0 ? tq_lcp(x.T, x.n, x.sa[at - 1], P, len) : 0;
        const u64 above = at < x.n ? tq_lcp(x.T, x.n, x.sa[at], P, len) : 0;
        L = below > above ? below : above;
        r = tq_range(x, P, L);                                          // (L == 0: {0, n} without a search)
    }
    s.first = r.first; s.count = r.second;
    s.length = (u32)L;
    s.ended = tq_span_ended(x, r.first, r.second, L);
    g.spans[j] = s;
}

// Rec: the 16-byte record of a position, read for its .length and copied out whole -- sa_hip_token_span here,
// sa_hip_token_shards_match over a shard set (token_shard_match.hpp).  A lane holds it as four words, whatever its fields are.
typedef u32 MatchRecWords __attribute__((ext_vector_type(4)));

template <class Rec>
__device__ __forceinline__ MatchRecWords tq_match_rec_load(const Rec* p) {
    static_assert(sizeof(Rec) == sizeof(MatchRecWords) && offsetof(Rec, length) % 4 == 0, "a record is four words");
    MatchRecWords w;
    __builtin_memcpy(&w, p, sizeof w);
    return w;
}

// One wave's walk over document [o0, o1) (o1 clamped to >= o0), here and in token_score.hpp: windows of 64, lane l at j = a + l.
// load(j) is called for j < o1 only, one trip before body(j, j < o1, record) uses it; a lane beyond o1 gets a zero record.
struct DocSpan { u64 o0, o1; };
__device__ __forceinline__ DocSpan tq_doc_span(const u64* off, u64 d) {
    const u64 o0 = off[d], o1 = off[d + 1];
    return DocSpan{o0, o1 > o0 ? o1 : o0};
}
template <class Load, class Body>
__device__ __forceinline__ void tq_doc_windows(const DocSpan& doc, u32 lane, Load load, Body body) {
    decltype(load(u64{})) nxt{};
    if (doc.o0 + lane < doc.o1) nxt = load(doc.o0 + lane);
    for (u64 a = doc.o0; a < doc.o1; a += (u64)WAVE) {
        const u64 j = a + lane;
        const auto rec = nxt;
        if (j + WAVE < doc.o1) nxt = load(j + WAVE);
        body(j, j < doc.o1, rec);
    }
}

template <class Rec>
struct MatchDocsArgs {
    const Rec* spans;                  // [offsets[Q]], by position
    const u64* off;                    // [Q + 1]
    u64 Q;
    u32 min_length;                    // >= 1
    u32 cap;                           // 0: heads only
    u32* positions;                    // [Q * cap]; never touched when cap == 0
    Rec* out_spans;                    // [Q * cap]
    sa_hip_token_match_head* heads;    // [Q]
};

// One wave per document.  Every trip of the walk advances by one window of 64 positions.
template <class Rec>
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_match_docs_kernel(MatchDocsArgs<Rec> g) {
    const u32 lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    for (u64 d = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); d < g.Q; d += waves) {
        const DocSpan doc = tq_doc_span(g.off, d);
        const u64 o0 = doc.o0, o1 = doc.o1;
        u32* const pos = g.positions + d * g.cap;
        Rec* const outs = g.out_spans + d * g.cap;
        u64 prev_end = o0;         // end(j - 1) of the window's first position: no match before the document reaches into it
        u64 E = 0;                 // the largest end of a qualifying position so far
        u64 covered = 0;           // this lane's share
        u32 longest = 0;           // this lane's share
        u32 maximal = 0;
        tq_doc_windows(doc, lane, [&](u64 j) { return tq_match_rec_load(g.spans + j); }, [&](u64 j, bool act, const MatchRecWords& sp) {
            const u32 sp_length = sp[offsetof(Rec, length) / 4];
            const u64 left = act ? o1 - j : 0;
            const u32 len = act ? (sp_length < left ? sp_length : (u32)left) : 0u;   // a match never passes its document's end
            const u64 end = act ? j + len : o1;
            u64 pe = lane_shift_up(end, 1);
            if (lane == 0) pe = prev_end;
            const bool out = len >= g.min_length && end > pe;                        // (min_length >= 1: of length >= 1)
            const bool qual = len >= g.min_length;
            const u64 incl = wave_scan_incl(qual ? end : (u64)0, ScanMax{});
            u64 before = lane_shift_up(incl, 1);
            if (lane == 0) before = 0;
            if (E > before) before = E;
            const u64 from = j > before ? j : before;
            if (qual && end > from) covered += end - from;
            if (len > longest) longest = len;
            const u64 hb = __ballot(out);
            const u32 slot = maximal + (u32)__popcll(hb & lanemask_lt());
            if (out && slot < g.cap) {
                pos[slot] = (u32)(j - o0);
                __builtin_memcpy(outs + slot, &sp, sizeof sp);
            }
            maximal += (u32)__popcll(hb);
            const u64 top = __shfl(incl, WAVE - 1);
            if (top > E) E = top;
            prev_end = __shfl(end, WAVE - 1);                                        // (inactive lanes hold o1: >= every end)
        });
        covered = wave_reduce(covered, ScanSum{});
        longest = wave_reduce(longest, ScanMax{});
        if (lane == 0) {
            sa_hip_token_match_head h;
            h.written = maximal < g.cap ? maximal : g.cap;
            h.maximal = maximal;
            h.longest = longest;
            h.covered = (u32)covered;
            g.heads[d] = h;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// total >= 1 positions (< 2^31), every pointer on the device; asynchronous on `stream`
inline int launch_match(const Index& x, hipStream_t stream, const MatchArgs& g) {
    const u64 grid = (g.total + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(tq_match_kernel, dim3((u32)grid), dim3(BLOCK), 0, stream, x.view(), g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// Q >= 1 documents, Q * cap < 2^31 (cap may be 0); every pointer on the device; asynchronous on `stream`
template <class Rec>
inline int launch_match_docs(hipStream_t stream, const MatchDocsArgs<Rec>& g) {
    hipLaunchKernelGGL(tq_match_docs_kernel<Rec>, dim3(wave_row_grid(g.Q)), dim3(NEXT_WAVES * WAVE), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
