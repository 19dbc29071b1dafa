// token_shard_docs.hpp -- documents of a shard set (sa_hip_token_shards_locate_* / _docs_*): which documents of the whole corpus
// hold an n-gram, where in them, and in how many it occurs.
//
// The set is one corpus cut at document boundaries: a document lives in exactly one shard.  With D_s documents in shard s (empty
// ones included), base[0] = 0 and base[s + 1] = base[s] + D_s, the global id of document d of shard s is base[s] + d, a u64.  The
// hits of a context are the concatenation of the shards' rank ranges in shard order, suffix order inside a shard.  Two documents
// of different shards are different documents, so the distinct documents among a prefix of that concatenation are the distinct
// documents of each shard's piece of the prefix, one list after the other, and their number is the plain sum: nothing is
// de-duplicated across shards.
//
// Per context i the span step of the set gives spans[s * stride + i]; c_s is its count after the clamp of tq_walk_of and
// C = sum of the c_s (u64).
//
//   tq_shard_locate_kernel      one lane per cell (context i, j < cap).  The running sum of the S clamped counts finds the shard
//                               of hit j (the lanes of a context read the same S spans); the lane writes base[s] + DA_s[r] and
//                               SA_s[r] - starts_s[doc].  Lane j == 0 writes the head {written = min(C, cap), count = C}.
//   tq_shard_docs_kernel        one wave per (context, shard) pair, NEXT_WAVES per workgroup, pair = i * S + s: the shards of a
//                               context are neighbouring waves, so the S pieces of one long span are walked side by side.  Lane t
//                               loads shard t's clamped count, one wave_scan_incl over u64 gives the ranks in front of shard s,
//                               hence e_s = clamp(budget - that sum, 0, c_s) (tq_budget_share).  The walk is tq_docs_walk
//                               (token_docs.hpp).  The pair's head (sa_hip_token_docs) and its list, local ids, go to scratch of
//                               the set, shard-major [s * qc + i].  One atomic add per wave into a u64 counter: the ranks streamed.
//   tq_shard_docs_merge_kernel  one wave per context, lane s holds pair (s, i)'s head.  An exclusive u64 scan of `distinct` gives
//                               every shard's first slot, wave_reduce gives the sums of the head.  Shard by
//                               shard, while the first slot is below cap, the wave copies that shard's written entries, 64 per
//                               step, adds base[s] and drops slots at or beyond cap.  Lane 0 writes the head.
//
// No kernel uses LDS; the lane operations are scan.hpp's.  Bounds: nothing about the spans is trusted.  first and count are clamped
// to the shard by tq_walk_of, so every rank read is below n_s; DA holds values in [0, D_s) whatever SA holds; a pair's `written` is
// clamped to cap before its list is read; every loop is counted (S, cap / 64) or advances by >= 1 window.
#pragma once
#include "token_docs.hpp"
#include "token_shards.hpp"

namespace sa {
namespace tq {

struct ShardLocateArgs {
    const View* tab;                       // [S]
    const DocView* dtab;                   // [S]
    const u64* base;                       // [S + 1]
    const sa_hip_token_span* spans;        // span of (s, i) at spans[s * Q + i]
    u64 Q;
    u32 S, cap;                            // cap >= 1
    u64* docs;                             // [Q * cap]
    int32_t* offsets;                      // [Q * cap]
    sa_hip_token_shards_locate* heads;     // [Q]
};

// one lane per (context, j), j < cap; Q * cap < 2^31
__global__ __launch_bounds__(BLOCK) void tq_shard_locate_kernel(ShardLocateArgs g) {
    const u64 cell = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const u64 i = cell / g.cap;
    if (i >= g.Q) return;
    const u32 j = (u32)(cell - i * g.cap);
    u64 run = 0;                           // hits of the shards in front
    u32 hs = g.S, hr = 0;                  // the shard and the rank of hit j (hs == S: there is no hit j)
    for (u32 s = 0; s < g.S; ++s) {
        const Walk k = tq_walk_of(g.tab[s], g.spans[(u64)s * g.Q + i]);
        const u32 c = k.end - k.a;
        if (hs == g.S && (u64)j - run < (u64)c) { hs = s; hr = k.a + (u32)((u64)j - run); }   // (run <= j while no shard is found)
        run += c;
    }
    if (j == 0) {
        sa_hip_token_shards_locate h;
        h.written = run < g.cap ? (u32)run : g.cap;
        h.reserved = 0;
        h.count = run;
        g.heads[i] = h;
    }
    if (hs == g.S) return;
    const DocView d = g.dtab[hs];
    const int32_t doc = d.da[hr];
    g.docs[cell] = g.base[hs] + (u64)(u32)doc;
    g.offsets[cell] = (int32_t)(g.tab[hs].sa[hr] - (u32)d.starts[doc]);
}

struct ShardDocsArgs {
    const View* tab;                       // [S]
    const DocView* dtab;                   // [S]
    const sa_hip_token_span* spans;        // span of (s, i) at spans[s * span_stride + i], i < Q
    u64 span_stride;
    u64 Q;                                 // contexts of this chunk
    u32 S, cap;                            // cap == 0: counts only
    u64 budget;                            // 0: none
    int32_t* docs;                         // [S * Q * cap]: the list of pair (s, i) starts at (s * Q + i) * cap; local ids
    int32_t* offsets;                      // [S * Q * cap]
    sa_hip_token_docs* heads;              // [S * Q], at s * Q + i
    unsigned long long* streamed;          // one counter: the sum of the pairs' examined
};

// One wave per (context, shard) pair.
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_shard_docs_kernel(ShardDocsArgs g) {
    const u32 lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    const u64 pairs = g.Q * g.S;
    unsigned long long streamed = 0;
    for (u64 w = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); w < pairs; w += waves) {
        const u64 i = w / g.S;
        const u32 s = (u32)(w - i * g.S);
        u32 a = 0, c = 0;
        if (lane < g.S) {
            const Walk k = tq_walk_of(g.tab[lane], g.spans[(u64)lane * g.span_stride + i]);
            a = k.a;
            c = k.end - k.a;
        }
        const u64 incl = wave_scan_incl((u64)c, ScanSum{});
        const u64 before = __shfl(incl - c, (int)s);       // ranks of the shards in front of s
        const u32 first = __shfl(a, (int)s);
        const u32 count = __shfl(c, (int)s);
        const u32 examined = tq_budget_share(g.budget, before, count);
        const u64 row = (u64)s * g.Q + i;
        const u32 distinct = tq_docs_walk(g.tab[s], g.dtab[s], first, examined, g.cap, g.docs + row * g.cap, g.offsets + row * g.cap, lane);
        if (lane == 0) {
            sa_hip_token_docs h;
            h.written = distinct < g.cap ? distinct : g.cap;
            h.examined = examined;
            h.distinct = distinct;
            h.count = count;
            g.heads[row] = h;
        }
        streamed += examined;
    }
    if (lane == 0 && streamed) atomicAdd(g.streamed, streamed);
}

struct ShardDocsMergeArgs {
    const int32_t* docs;                   // [S * Q * cap] as tq_shard_docs_kernel writes them
    const int32_t* offsets;                // [S * Q * cap]
    const sa_hip_token_docs* heads;        // [S * Q]
    const u64* base;                       // [S + 1]
    u64 Q;
    u32 S, cap;
    u64* out_docs;                         // [Q * cap]; never touched when cap == 0
    int32_t* out_offsets;                  // [Q * cap]
    sa_hip_token_shards_docs* out_heads;   // [Q]
};

__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_shard_docs_merge_kernel(ShardDocsMergeArgs g) {
    const u32 lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    for (u64 i = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); i < g.Q; i += waves) {
        u32 wr = 0;
        u64 ex = 0, di = 0, ct = 0;
        if (lane < g.S) {
            const sa_hip_token_docs h = g.heads[(u64)lane * g.Q + i];
            wr = h.written < g.cap ? h.written : g.cap;
            ex = h.examined; di = h.distinct; ct = h.count;
        }
        const u64 di_incl = wave_scan_incl(di, ScanSum{});
        const u64 slot0 = di_incl - di;                    // this shard's first slot
        const u64 distinct = __shfl(di_incl, WAVE - 1);
        const u64 examined = wave_reduce(ex, ScanSum{});
        const u64 count = wave_reduce(ct, ScanSum{});
        for (u32 s = 0; s < g.S; ++s) {
            const u64 at = __shfl(slot0, (int)s);
            if (at >= g.cap) break;                        // (wave-uniform; the first slots are non-decreasing in s)
            const u32 n = __shfl(wr, (int)s);
            const u64 row = ((u64)s * g.Q + i) * g.cap;
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
            sa_hip_token_shards_docs h;
            h.written = distinct < g.cap ? (u32)distinct : g.cap;
            h.reserved = 0;
            h.examined = examined;
            h.distinct = distinct;
            h.count = count;
            g.out_heads[i] = h;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// Q >= 1 contexts, cap >= 1, Q * cap < 2^31; every pointer on the device; asynchronous on `stream`
inline int launch_shard_locate(hipStream_t stream, const ShardLocateArgs& g) {
    const u64 cells = g.Q * g.cap;
    hipLaunchKernelGGL(tq_shard_locate_kernel, dim3((u32)((cells + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// Q >= 1 contexts of a chunk; the caller has zeroed g.streamed on the stream
inline int launch_shard_docs(hipStream_t stream, const ShardDocsArgs& g) {
    hipLaunchKernelGGL(tq_shard_docs_kernel, dim3(wave_row_grid(g.Q * g.S)), dim3(NEXT_WAVES * WAVE), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

inline int launch_shard_docs_merge(hipStream_t stream, const ShardDocsMergeArgs& g) {
    hipLaunchKernelGGL(tq_shard_docs_merge_kernel, dim3(wave_row_grid(g.Q)), dim3(NEXT_WAVES * WAVE), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
