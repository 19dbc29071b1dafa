// token_shard_all.hpp -- per-document counts and AND groups of a shard set (sa_hip_token_shards_doc_counts_* / _all_*): how often an
// n-gram occurs in a given document of the whole corpus, and which documents of it hold all n-grams of a group.
//
// The set is one corpus cut at document boundaries (token_shard_docs.hpp): a document lives in exactly one shard, its global id is
// base[s] + d, and D_s >= 1 makes the bases strictly ascending.  Every shard carries RK, the rank-by-document array of
// token_all.hpp; the set holds RankView[S] beside View[S] and base[S + 1].  Pattern p has the span spans[s * P + p] in shard s,
// c_{s,p} is its count after the clamp of tq_walk_of and C_p = the sum over s, a u64 below 2^37.
//
// A group has ONE driver for the whole set: its span with the smallest C_j, the lowest index on a tie.  examined = budget ?
// min(C_driver, budget) : C_driver ranks are taken from the front of the concatenation of the driver's ranges in shard order, so
// shard s examines e_s = clamp(budget - (c_{0,driver} + .. + c_{s-1,driver}), 0, c_{s,driver}).  Per shard the candidates and the
// matches are token_all.hpp's over those e_s ranks; two shards never share a document, so `matched` and `candidates` of the group
// are the plain sums and the list is the shards' lists one after another.
//
//   tq_shard_tf_kernel         one lane per cell (context i, j < cap), the layout of tq_tf_kernel.  The shard of a global id is
//                              found by a search of base[0 .. S], at most SHARD_STEPS halvings; then tq_seg_lower twice in RK_s.
//                              An id >= base[S] gives 0 without touching any RK.
//   tq_shard_all_plan_kernel   one wave per group.  Lane s loads shard s's clamped count of the group's m <= ALL_MAX spans, one span
//                              per trip; a wave sum (u64) gives C_j, kept by lane j.  One wave_reduce(ScanMax) over the inverted
//                              key (C_j << 4) | j gives the driver; an exclusive u64 scan of c_{s,driver} gives e_s by
//                              tq_budget_share (token_shards.hpp), as tq_shard_docs_kernel has it.  It writes
//                              {driver, e_s} per (group, shard) pair and {driver, C_driver} per group.  A launch of its own: inside
//                              every pair wave the same S * m span loads would be repeated S times per group.
//   tq_shard_all_kernel        one wave per (group, shard) pair, pair = g * S + s, NEXT_WAVES per workgroup: the walk of
//                              tq_all_kernel (tq_all_walk) over the pair's e_s ranks.  A 16-byte pair head {written, examined,
//                              matched, candidates} and the list, local ids, go to scratch of the set, shard-major [s * G + g].
//                              One atomic add per wave into a u64 counter: the ranks streamed.
//   tq_shard_all_merge_kernel  one wave per group, lane s holds pair (s, g)'s head: an exclusive u64 scan of `matched` gives every
//                              shard's first slot, wave_reduce the three sums.  Shard by shard, while the first
//                              slot is below cap, the wave copies the written entries, 64 per step, and adds base[s].  Lane 0 writes
//                              the head from the plan's {driver, C_driver}.
//
// No kernel uses LDS; the lane operations are scan.hpp's; every store is an ordinary vector store.  Bounds: nothing about the spans
// is trusted.  first and count are clamped to the shard by tq_walk_of and e_s <= c_{s,driver}, so every rank read is below n_s; DA
// holds values in [0, D_s) whatever SA holds, so starts[d] and starts[d + 1] exist; every search is at most STEPS (SHARD_STEPS)
// halvings; every trip of the walk advances by >= 1 rank; m is clamped to ALL_MAX and a pair's `written` to cap before its list is
// read; every other loop is counted (m, S, cap / 64).
#pragma once
#include "token_all.hpp"
#include "token_shard_docs.hpp"

namespace sa {
namespace tq {

constexpr int SHARD_STEPS = 7;         // halvings that empty a range of SHARDS_MAX = 64 candidates

struct ShardAllPair {                  // head of one (group, shard) pair, in scratch
    u32 written, examined, matched, candidates;
};
struct ShardAllPlan {                  // per (group, shard) pair
    u32 driver, examined;              // e_s
};
struct ShardAllGroup {                 // per group
    u32 driver, reserved;
    u64 count;                         // C_driver
};

struct ShardTfArgs {
    const View* tab;                   // [S]
    const RankView* rtab;              // [S]
    const u64* base;                   // [S + 1]
    const sa_hip_token_span* spans;    // span of (s, i) at spans[s * Q + i]
    u64 Q;
    u32 S, cap;                        // cap >= 1
    const u64* docs;                   // [Q * cap], global ids
    const unsigned char* written;      // nullptr: every row has cap entries; else a uint32 per context, `stride` bytes apart
    u64 stride;
    u32* counts;                       // [Q * cap]
};

// one lane per (context, j), j < cap; Q * cap < 2^31
__global__ __launch_bounds__(BLOCK) void tq_shard_tf_kernel(ShardTfArgs g) {
    const u64 cell = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const u64 i = cell / g.cap;
    if (i >= g.Q) return;
    const u32 j = (u32)(cell - i * g.cap);
    if (g.written && j >= *reinterpret_cast<const u32*>(g.written + i * g.stride)) return;
    const u64 id = g.docs[cell];
    u32 lo = 0, hi = g.S;                                  // lo = shards known to end at or below id
    for (int t = 0; t < SHARD_STEPS && lo < hi; ++t) {
        const u32 m = (lo + hi) >> 1;
        if (g.base[m + 1] <= id) lo = m + 1; else hi = m;
    }
    u32 count = 0;
    if (lo < g.S) {                                        // base[lo] <= id < base[lo + 1]
        const RankView d = g.rtab[lo];
        const u64 local = id - g.base[lo];
        if (local < d.D) {                                 // (the bases were summed from the D_s: it is)
            const Walk k = tq_walk_of(g.tab[lo], g.spans[(u64)lo * g.Q + i]);
            const u32 s0 = (u32)d.starts[local], s1 = (u32)d.starts[local + 1];
            const u32 at = tq_seg_lower(d.rk, s0, s1, k.a);
            count = tq_seg_lower(d.rk, at, s1, k.end) - at;
        }
    }
    g.counts[cell] = count;
}

struct ShardAllPlanArgs {
    const View* tab;                   // [S]
    const sa_hip_token_span* spans;    // span of (s, p) at spans[s * P + p]
    u64 P;
    const u32* group_offsets;          // [G + 1] of this chunk (absolute pattern indices); checked on the host
    u64 G;                             // groups of this chunk
    u32 S;
    u64 budget;                        // 0: none
    ShardAllPlan* pairs;               // [G * S], at g * S + s
    ShardAllGroup* groups;             // [G]
};

// One wave per group.
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_shard_all_plan_kernel(ShardAllPlanArgs g) {
    const u32 lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    for (u64 w = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); w < g.G; w += waves) {
        const u32 p0 = g.group_offsets[w];
        u32 m = g.group_offsets[w + 1] - p0;
        if (m > ALL_MAX) m = ALL_MAX;                      // (the host refused such a table)
        View x{};
        if (lane < g.S) x = g.tab[lane];
        u64 mine = 0;                                      // C_lane, in the lanes below m
        for (u32 j = 0; j < m; ++j) {
            u32 c = 0;
            if (lane < g.S) {
                const Walk k = tq_walk_of(x, g.spans[(u64)lane * g.P + p0 + j]);
                c = k.end - k.a;
            }
            const u64 C = wave_reduce((u64)c, ScanSum{});
            if (lane == j) mine = C;
        }
        // the driver: the smallest {C_j, j}; lanes beyond the group hold the largest key there is
        const u64 key = lane < m ? (mine << 4) | lane : ~0ull;
        const u64 best = ~wave_reduce(~key, ScanMax{});
        const u32 driver = m ? (u32)(best & 15u) : 0u;     // (m == 0: the host refused such a table)
        const u64 count = m ? best >> 4 : 0ull;
        u32 c = 0;
        if (lane < g.S && m) {
            const Walk k = tq_walk_of(x, g.spans[(u64)lane * g.P + p0 + driver]);
            c = k.end - k.a;
        }
        const u64 before = wave_scan_incl((u64)c, ScanSum{}) - c;   // the driver's ranks in the shards in front
        if (lane < g.S) g.pairs[w * g.S + lane] = ShardAllPlan{driver, tq_budget_share(g.budget, before, c)};
        if (lane == 0) g.groups[w] = ShardAllGroup{driver, 0u, count};
    }
}

struct ShardAllArgs {
    const View* tab;                   // [S]
    const RankView* rtab;              // [S]
    const sa_hip_token_span* spans;    // span of (s, p) at spans[s * P + p]
    u64 P;
    const u32* group_offsets;          // [G + 1] of this chunk
    const ShardAllPlan* pairs;         // [G * S]
    u64 G;                             // groups of this chunk
    u32 S, cap;                        // cap == 0: counts only
    int32_t* docs;                     // [S * G * cap]: the list of pair (s, g) starts at (s * G + g) * cap; local ids
    int32_t* offsets;                  // [S * G * cap]
    ShardAllPair* heads;               // [S * G], at s * G + g
    unsigned long long* streamed;      // one counter: the sum of the pairs' examined
};

// One wave per (group, shard) pair.
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_shard_all_kernel(ShardAllArgs g) {
    const u32 lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    const u64 pairs = g.G * g.S;
    unsigned long long streamed = 0;
    for (u64 w = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); w < pairs; w += waves) {
        const u64 i = w / g.S;
        const u32 s = (u32)(w - i * g.S);
        const u32 p0 = g.group_offsets[i];
        u32 m = g.group_offsets[i + 1] - p0;
        if (m > ALL_MAX) m = ALL_MAX;
        const ShardAllPlan plan = g.pairs[w];
        const View x = g.tab[s];
        const RankView d = g.rtab[s];
        const sa_hip_token_span* const sp = g.spans + (u64)s * g.P + p0;
        u32 driver = plan.driver, examined = 0, first = 0;
        if (m) {
            if (driver >= m) driver = m - 1;               // (a plan of this launch's own: it is not)
            const Walk k = tq_walk_of(x, sp[driver]);
            first = k.a;
            examined = plan.examined < k.end - k.a ? plan.examined : k.end - k.a;   // first + examined <= n_s whatever the plan holds
        }
        const u64 row = (u64)s * g.G + i;
        u32 candidates = 0;
        const u32 matched = tq_all_walk(x, d, sp, m, driver, first, examined, g.cap, g.docs + row * g.cap, g.offsets + row * g.cap, lane,
                                        candidates);
        if (lane == 0) g.heads[row] = ShardAllPair{matched < g.cap ? matched : g.cap, examined, matched, candidates};
        streamed += examined;
    }
    if (lane == 0 && streamed) atomicAdd(g.streamed, streamed);
}

struct ShardAllMergeArgs {
    const int32_t* docs;               // [S * G * cap] as tq_shard_all_kernel writes them
    const int32_t* offsets;            // [S * G * cap]
    const ShardAllPair* heads;         // [S * G]
    const ShardAllGroup* groups;       // [G]
    const u64* base;                   // [S + 1]
    u64 G;
    u32 S, cap;
    u64* out_docs;                     // [G * cap]; never touched when cap == 0
    int32_t* out_offsets;              // [G * cap]
    sa_hip_token_shards_all* out_heads;   // [G]
};

__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_shard_all_merge_kernel(ShardAllMergeArgs g) {
    const u32 lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    for (u64 i = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); i < g.G; i += waves) {
        u32 wr = 0;
        u64 ex = 0, ma = 0, ca = 0;
        if (lane < g.S) {
            const ShardAllPair h = g.heads[(u64)lane * g.G + i];
            wr = h.written < g.cap ? h.written : g.cap;
            ex = h.examined; ma = h.matched; ca = h.candidates;
        }
        const u64 ma_incl = wave_scan_incl(ma, ScanSum{});
        const u64 slot0 = ma_incl - ma;                    // this shard's first slot
        const u64 matched = __shfl(ma_incl, WAVE - 1);
        const u64 examined = wave_reduce(ex, ScanSum{});
        const u64 candidates = wave_reduce(ca, ScanSum{});
        for (u32 s = 0; s < g.S; ++s) {
            const u64 at = __shfl(slot0, (int)s);
            if (at >= g.cap) break;                        // (wave-uniform; the first slots are non-decreasing in s)
            const u32 n = __shfl(wr, (int)s);
            const u64 row = ((u64)s * g.G + i) * g.cap;
            const u64 b = g.base[s];
            for (u32 j0 = 0; j0 < n; j0 += WAVE) {
                const u32 j = j0 + lane;
                if (j < n && at + j < g.cap) {
                    g.out_docs[i * g.cap + at + j] = b + (u64)(u32)g.docs[row + j];
                    g.out_offsets[i * g.cap + at + j] = g.offsets[row + j];
                }
            }
        }
        if (lane == 0) {
            const ShardAllGroup p = g.groups[i];
            sa_hip_token_shards_all h;
            h.written = matched < g.cap ? (u32)matched : g.cap;
            h.driver = p.driver;
            h.examined = examined;
            h.matched = matched;
            h.candidates = candidates;
            h.count = p.count;
            g.out_heads[i] = h;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// Q >= 1 contexts, cap >= 1, Q * cap < 2^31; every pointer on the device; asynchronous on `stream`
inline int launch_shard_tf(hipStream_t stream, const ShardTfArgs& g) {
    const u64 cells = g.Q * g.cap;
    hipLaunchKernelGGL(tq_shard_tf_kernel, dim3((u32)((cells + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// G >= 1 groups of a chunk
inline int launch_shard_all_plan(hipStream_t stream, const ShardAllPlanArgs& g) {
    hipLaunchKernelGGL(tq_shard_all_plan_kernel, dim3(wave_row_grid(g.G)), dim3(NEXT_WAVES * WAVE), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// the caller has zeroed g.streamed on the stream
inline int launch_shard_all(hipStream_t stream, const ShardAllArgs& g) {
    hipLaunchKernelGGL(tq_shard_all_kernel, dim3(wave_row_grid(g.G * g.S)), dim3(NEXT_WAVES * WAVE), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

inline int launch_shard_all_merge(hipStream_t stream, const ShardAllMergeArgs& g) {
    hipLaunchKernelGGL(tq_shard_all_merge_kernel, dim3(wave_row_grid(g.G)), dim3(NEXT_WAVES * WAVE), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
