// token_shards.hpp -- a set of S <= 64 token indexes on one device answered as one corpus (sa_hip_token_shards_*): the steps that
// are not per-shard.  A corpus beyond 2^31 - 1 tokens is cut at document boundaries into shards of int32 size, each with its own
// suffix array; no n-gram spans a cut, so its count is the sum of the shards' counts and no kernel needs a 64-bit rank.
//
// The shard table is View[S] in device memory (token_query.hpp); every per-shard array is shard-major, [s * Q + i].
//
//   tq_shard_range_kernel   one lane per (pattern, shard) pair, the S shards of a pattern in neighbouring lanes: the S dependent
//                           search chains of a pattern run side by side instead of one after the other.
//   tq_shard_total_kernel   totals[i] = sum over s of the counts, one lane per pattern, in shard order: integers, deterministic.
//   tq_shard_span_kernel    one lane per context.  mode 1: binary search over L with "some shard has an effective count >= 1" as
//                           the property -- the sum over the shards is monotone in L because every term is (token_next.hpp), and
//                           the sum is >= 1 iff a term is, so a probe stops at the first shard that qualifies.  Then S range
//                           searches at the L found (mode 0: at the context's length).  <= SPAN_PROBES * S + S range searches.
//   tq_next_merge_kernel    one wave per context, lane s holds the cursor into shard s's list (hence S <= 64).  A step: wave-wide
//                           minimum of the head symbols, wave-wide u64 sum of the counts of the lanes that hold it, those lanes
//                           advance, lane 0 writes the entry.  <= cap steps, no LDS.  Both reductions are wave_reduce of
//                           scan.hpp.  An idle lane (s >= S, or its list exhausted) carries the key 2^64 - 1; a
//                           symbol's key is its value with the sign bit flipped, < 2^32: symbol 2^31 - 1 cannot collide.
//
// The per-shard next symbols are tq_next_kernel as it is: launch_next of every shard on its slice of the spans.
//
// Bounds: every loop is bounded whatever the arrays hold.  The span kernel's loops are counted (SPAN_PROBES, S, STEPS inside
// tq_range); the merge clamps a cursor's end to min(written, cap) and takes <= cap steps; spans are clamped by tq_walk_of inside
// tq_next_kernel.  Lists that are not ascending give unspecified entries, never a read outside the buffers.
#pragma once
#include "token_next.hpp"

namespace sa {
namespace tq {

constexpr u32 SHARDS_MAX = 64;         // one lane of the merge's wave per shard

// a pair index t = row * S + s: the S shards of a row are neighbours; the caller tests the row against its count
struct Pair { u64 row; u32 s; };
__device__ __forceinline__ Pair tq_pair_of(u64 t, u32 S) {
    const u64 row = t / S;
    return Pair{row, (u32)(t - row * S)};
}

// a shard's share (<= count) of a budget of ranks, `before` of them in the shards in front; budget == 0: no budget
__device__ __forceinline__ u32 tq_budget_share(u64 budget, u64 before, u32 count) {
    if (!budget) return count;
    const u64 left = budget > before ? budget - before : 0;
    return left < count ? (u32)left : count;
}

__global__ __launch_bounds__(BLOCK) void tq_shard_range_kernel(const View* __restrict__ tab, u32 S, const int32_t* __restrict__ pat,
                                                               const u64* __restrict__ off, u64 Q, sa_hip_pair_u32* __restrict__ out) {
    const Pair p = tq_pair_of((u64)blockIdx.x * BLOCK + threadIdx.x, S);
    const u64 i = p.row;
    if (i >= Q) return;
    const View x = tab[p.s];
    const u64 o0 = off[i], o1 = off[i + 1];
    out[(u64)p.s * Q + i] = tq_range(x, pat + o0, o1 > o0 ? o1 - o0 : 0);
}

__global__ __launch_bounds__(BLOCK) void tq_shard_total_kernel(const sa_hip_pair_u32* __restrict__ per, u32 S, u64 Q, u64* __restrict__ totals) {
    const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= Q) return;
    u64 sum = 0;
    for (u32 s = 0; s < S; ++s) sum += per[(u64)s * Q + i].second;
    totals[i] = sum;
}

// max_n: the longest shard (no more symbols than that match anywhere)
__global__ __launch_bounds__(BLOCK) void tq_shard_span_kernel(const View* __restrict__ tab, u32 S, u32 max_n, const int32_t* __restrict__ pat,
                                                              const u64* __restrict__ off, u64 Q, int mode, u32 max_length, int need_next,
                                                              u32* __restrict__ length, u64* __restrict__ totals,
                                                              sa_hip_token_span* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= Q) return;
    const u64 o0 = off[i], o1 = off[i + 1];
    const u64 m = o1 > o0 ? o1 - o0 : 0;
    const int32_t* P = pat + o0;
    u64 L = m;
    if (mode != 0) {
        u64 hi = m < max_n ? m : max_n;
        if (max_length && hi > max_length) hi = max_length;
        u64 lo = 0;                                         // L = 0 qualifies wherever a shard holds a symbol, and is the answer otherwise
        for (int probe = 0; probe < SPAN_PROBES && lo < hi; ++probe) {
            const u64 mid = lo + (hi - lo + 1) / 2;
            bool ok = false;
            for (u32 s = 0; s < S && !ok; ++s) {
                const View x = tab[s];
                if (x.n == 0) continue;
                const sa_hip_pair_u32 r = tq_range(x, P + (m - mid), mid);
                u32 eff = r.second;
                if (need_next && r.second == 1) eff -= tq_span_ended(x, r.first, 1u, mid);   // only a lone suffix can be decided by it
                ok = eff != 0;
            }
            if (ok) lo = mid; else hi = mid - 1;
        }
        L = lo;
    }
    u64 sum = 0;
    for (u32 s = 0; s < S; ++s) {
        const View x = tab[s];
        const sa_hip_token_span sp = tq_span_exact(x, P + (m - L), L);
        out[(u64)s * Q + i] = sp;
        sum += sp.count - (need_next ? sp.ended : 0u);
    }
    length[i] = L > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)L;
    totals[i] = sum;
}

struct MergeArgs {
    const int32_t* sym;                  // [S * Q * cap]: the list of (shard s, context i) starts at (s * Q + i) * cap
    const u32* cnt;                      // [S * Q * cap]
    const sa_hip_token_next* heads;      // [S * Q]
    const sa_hip_token_span* spans;      // span of (s, i) at spans[s * span_stride + i]; nullptr: length 0
    u64 span_stride;
    u64 Q;
    u32 S, cap;
    int32_t* out_sym;                    // [Q * cap]
    u64* out_cnt;                        // [Q * cap]
    sa_hip_token_shards_next* out_heads; // [Q]
};

constexpr u64 MERGE_IDLE = ~0ull;

__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_next_merge_kernel(MergeArgs g) {
    const int lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    for (u64 i = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); i < g.Q; i += waves) {
        u32 end = 0, len = 0;
        u64 tot = 0;
        const int32_t* sy = g.sym;
        const u32* ct = g.cnt;
        if ((u32)lane < g.S) {
            const u64 row = (u64)lane * g.Q + i;
            const sa_hip_token_next h = g.heads[row];
            end = h.written < g.cap ? h.written : g.cap;
            tot = h.total;
            sy += row * g.cap;
            ct += row * g.cap;
            if (g.spans) len = g.spans[(u64)lane * g.span_stride + i].length;
        }
        const u64 total = wave_reduce(tot, ScanSum{});
        const u32 length = wave_reduce(len, ScanMax{});
        u32 pos = 0, written = 0;
        u64 covered = 0;
        for (u32 step = 0; step < g.cap; ++step) {
            const bool has = pos < end;
            const u64 key = has ? (u64)((u32)sy[pos] ^ 0x80000000u) : MERGE_IDLE;
            const u64 mn = ~wave_reduce(~key, ScanMax{});                           // the smallest key of the wave
            if (mn == MERGE_IDLE) break;                                            // (wave-uniform) every list is exhausted
            const bool hit = key == mn;
            const u64 sum = wave_reduce(hit ? (u64)ct[pos] : 0ull, ScanSum{});
            if (lane == 0) {
                g.out_sym[i * g.cap + step] = (int32_t)((u32)mn ^ 0x80000000u);
                g.out_cnt[i * g.cap + step] = sum;
            }
            if (hit) ++pos;
            ++written;
            covered += sum;
        }
        if (lane == 0) {
            sa_hip_token_shards_next h;
            h.written = written; h.length = length; h.covered = covered; h.total = total;
            g.out_heads[i] = h;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

constexpr size_t SHARD_SCRATCH_BUDGET = 256ull << 20;   // bytes of per-shard lists per chunk of contexts

// contexts per chunk: S lists of cap (int32 symbol, u32 count) entries and a head each
inline u64 shard_chunk(u64 knob, u32 S, u32 cap, u64 Q) {
    u64 c = knob;
    if (c == 0) {
        const u64 per = (u64)S * ((u64)cap * 8 + sizeof(sa_hip_token_next));
        c = SHARD_SCRATCH_BUDGET / per;
    }
    if (c == 0) c = 1;
    return c < Q ? c : Q;
}

// the workgroups of one lane per (row, shard) pair, rows >= 1; beyond 2^31 - 1: 0, and the error is set under the caller's name
inline u32 shard_pair_grid(u64 rows, u32 S, const char* who, const char* too_many) {
    const u64 g = (rows * S + BLOCK - 1) / BLOCK;
    return g > 0x7FFFFFFFull ? (u32)(fail(SA_HIP_EINVAL, who, too_many), 0) : (u32)g;
}

// Q >= 1 patterns, every pointer on the device, per[S * Q]; asynchronous on `stream`
inline int launch_shard_ranges(const View* tab, u32 S, hipStream_t stream, const int32_t* pat, const u64* off, u64 Q, u64* totals,
                               sa_hip_pair_u32* per) {
    const u32 grid = shard_pair_grid(Q, S, "sa_hip_token_shards_query_batch", "too many patterns for one launch");
    if (!grid) return SA_HIP_EINVAL;
    hipLaunchKernelGGL(tq_shard_range_kernel, dim3(grid), dim3(BLOCK), 0, stream, tab, S, pat, off, Q, per);
    hipLaunchKernelGGL(tq_shard_total_kernel, dim3((u32)((Q + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, (const sa_hip_pair_u32*)per, S, Q, totals);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

inline int launch_shard_spans(const View* tab, u32 S, u32 max_n, hipStream_t stream, const int32_t* pat, const u64* off, u64 Q, int mode,
                              u32 max_length, int need_next, u32* length, u64* totals, sa_hip_token_span* out) {
    const u64 grid = (Q + BLOCK - 1) / BLOCK;
    if (grid > 0x7FFFFFFFull) return fail(SA_HIP_EINVAL, "sa_hip_token_shards_spans_batch", "too many contexts for one launch");
    hipLaunchKernelGGL(tq_shard_span_kernel, dim3((u32)grid), dim3(BLOCK), 0, stream, tab, S, max_n, pat, off, Q, mode, max_length, need_next,
                       length, totals, out);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

inline int launch_merge(hipStream_t stream, const MergeArgs& g) {
    hipLaunchKernelGGL(tq_next_merge_kernel, dim3(wave_row_grid(g.Q)), dim3(NEXT_WAVES * WAVE), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
