// token_top.hpp -- the k most frequent next symbols of a span, and next symbols drawn from a span (sa_hip_token_index_top_* /
// _sample_*, include/sa_hip.h section 6k).  Spans, the walk and s(r) = T[SA[r] + length] are those of token_next.hpp.
//
//   tq_top_kernel     one wave per span, NEXT_WAVES per workgroup, the rows strided as in tq_next_kernel, and the same walk: the
//                     ended suffix stepped over, window steps of 64 ranks (lane_shift_up and a ballot find the run heads), the
//                     jump step over a long run (tq_jump_run) behind one probe of the next 4096 ranks (tq_gallop_run: this walk
//                     meets every run of a span, most of them far shorter than what is left of the span, which is where the
//                     jump step starts from).  It never stops at a cap: every run of the walked part is seen; `budget` (0: none)
//                     cuts the walk to the first `budget` ranks behind the ended suffix, and a run cut by it counts with what
//                     lies inside.  The loop is the device function tq_top_walk, which tq_shard_top_kernel (token_shard_top.hpp)
//                     calls as well for a context whose continuations lie in one shard.
//                     The table: lane j < k holds one entry as the 64-bit key count << 32 | (0xFFFFFFFF - symbol), larger is
//                     better, 0 is empty; lanes >= k hold ~0, which is never the minimum.  Symbols of a text are in
//                     [0, 2^31 - 1] and the runs of a span have distinct symbols, so the keys of a span are distinct and "count
//                     descending, then symbol ascending" is a total order.  The table's minimum and its lane are kept
//                     wave-uniform (scalar registers).  A window's completed runs are the candidates: every head's run but the
//                     last one's, and the carried run that ends at the first head (wave-uniform).  Only the candidates whose key
//                     beats the minimum -- a ballot -- are offered one by one; an insert replaces the minimum's lane and reduces
//                     the minimum again (TopTable::offer).  The span's last run is offered behind the loop.  Then every lane
//                     ranks its key by counting the live keys above it and writes symbols[i * k + rank], counts[i * k + rank].
//                     Bound: every run is offered once, so a span of d runs costs at most d inserts, one 64-lane minimum each.
//                     Runs with ascending counts reach that bound (every run evicts); with descending counts nothing behind the
//                     first k is inserted; on Zipf-like spans the frequent symbols have small ids, stand first, and almost no
//                     later candidate passes the ballot.
//                     No LDS, no array in registers that is indexed at run time, no scratch (profiles/token_top_resources.txt).
//   tq_sample_kernel  one lane per (span, draw): with start = first + ended and total = count - ended (both clamped),
//                     rank = start + floor(draw * total / 2^64) and symbol = s(rank); total == 0 gives -1 / 0xFFFFFFFF.  The
//                     caller supplies the draws, nothing random happens on the device: exact and reproducible, and a uniform
//                     64-bit draw gives every continuation its corpus probability to within 2^-64 * total.
//
// Bounds: as in token_next.hpp -- first and count are clamped to the array, every text index is tested against n, a window step
// advances by >= 1 rank, a jump step is bounded, the offers of a window by its 64 lanes, the final ranking by 64 keys; rank < k in
// every lane that writes.  An in-range array that is not the suffix array gives unspecified entries, never a read or a write
// outside the buffers.
#pragma once
#include "token_next.hpp"

namespace sa {
namespace tq {

constexpr u32 TOP_MAX = 64;            // entries of a table: one per lane

struct TopArgs {
    const sa_hip_token_span* spans;
    u64 Q;
    u32 k;                             // 1 .. TOP_MAX
    u32 budget;                        // ranks walked per span at most; 0: all
    int32_t* symbols;                  // [Q * k]
    u32* counts;                       // [Q * k]
    sa_hip_token_top* heads;           // [Q]
};

struct SampleArgs {
    const sa_hip_token_span* spans;
    u64 Q;
    u32 m;                             // draws per span
    const u64* draws;                  // [Q * m]
    int32_t* symbols;                  // [Q * m]
    u32* ranks;                        // [Q * m], or nullptr
};

__device__ __forceinline__ u64 top_key(int32_t symbol, u32 count) { return (u64)count << 32 | (u64)(0xFFFFFFFFu - (u32)symbol); }
// v of lane j, j wave-uniform: into scalar registers
__device__ __forceinline__ u64 top_readlane(u64 v, int j) {
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, j), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), j);
    return (u64)hi << 32 | lo;
}
__device__ __forceinline__ u64 top_uniform(u64 v) { return top_readlane(v, 0); }

struct TopTable {
    u64 key;        // this lane's entry
    u64 min;        // the smallest key of the wave: an entry of a lane < k, or 0 while one is empty
    int at;         // the lowest lane that holds it
    __device__ __forceinline__ void reset(int lane, u32 k) {
        key = (u32)lane < k ? 0ull : ~0ull;
        min = 0;
        at = 0;
    }
    // c is wave-uniform
    __device__ __forceinline__ void offer(u64 c, int lane) {
        if (c <= min) return;
        if (lane == at) key = c;
        min = top_uniform(~wave_reduce(~key, ScanMax{}));
        at = __ffsll((unsigned long long)__ballot(key == min)) - 1;
    }
};

// One probe in front of the jump step: the 64 ranks lo + 64 * (lane + 1).  Rank lo holds cur and more than NEXT_JUMP_MIN ranks lie
// behind it.  A run that ends within 4096 ranks is narrowed to a slice of 64 by this one step, where tq_jump_run, which starts from
// the whole rest of the span, takes three or four; a longer run goes on to tq_jump_run from rank lo + 4096.  -> as tq_jump_run.
__device__ __forceinline__ u32 tq_gallop_run(const View& x, int lane, int32_t cur, u32 length, u32 lo, u32 hi) {
    const u64 q = (u64)lo + (u64)(lane + 1) * WAVE;
    int32_t sq = 0;
    const bool eq = q < hi && tq_next_symbol(x, (u32)q, length, &sq) && sq == cur;
    const u64 b = __ballot(eq);
    if (b == ~0ull) return tq_jump_run(x, lane, cur, length, lo + (u32)(WAVE * WAVE), hi);   // lane 63's sample: < hi, holds cur
    return lo + ((u32)__ffsll((unsigned long long)~b) - 1u) * (u32)WAVE;                     // the samples still equal
}

// The walk of one wave over the ranks [start, end) of x behind the ended suffix, s(r) read at `length`: every completed run is
// offered to tab (reset by the caller) -> the number of runs.  tq_top_kernel's loop, and the one-shard path of
// tq_shard_top_kernel (token_shard_top.hpp); start, end and length are wave-uniform.
__device__ __forceinline__ u32 tq_top_walk(const View& x, int lane, u32 start, u32 end, u32 length, int jump, TopTable& tab) {
    u32 a = start, distinct = 0, run_start = start;
    int32_t cur = 0;
    bool have = false;
    // every trip advances a by >= 1
    while (a < end) {
        const u32 left_n = end - a;
        const u32 nact = left_n < (u32)WAVE ? left_n : (u32)WAVE;
        const bool act = (u32)lane < nact;
        int32_t s = cur;
        if (act) (void)tq_next_symbol(x, a + lane, length, &s);
        const int32_t left = lane_shift_up(s, 1);
        const bool head = act && (lane == 0 ? (!have || s != cur) : s != left);
        const u64 hb = __ballot(head);
        if (hb == 0) {
            // the window is all the running symbol
            u32 lo = a + nact - 1;                       // known to hold cur; (lo, end): not known
            if (jump && end - lo - 1 > NEXT_JUMP_MIN) lo = tq_gallop_run(x, lane, cur, length, lo, end);
            a = lo + 1;
            continue;
        }
        const int f = __ffsll((unsigned long long)hb) - 1;
        if (have) tab.offer(top_key(cur, a + (u32)f - run_start), lane);         // the carried run ends at the first head
        const u64 above = lane == WAVE - 1 ? 0ull : hb & ~((2ull << lane) - 1ull);
        const u64 ck = head && above ? top_key(s, (u32)(__ffsll((unsigned long long)above) - 1 - lane)) : 0ull;
        // the completed runs that beat the minimum as it stands; it only rises, and offer() tests again (<= 63 trips)
        for (u64 m = __ballot(ck > tab.min); m; m &= m - 1) tab.offer(top_readlane(ck, __ffsll((unsigned long long)m) - 1), lane);
        const int last = 63 - __clzll((unsigned long long)hb);
        cur = __shfl(s, last);
        run_start = a + (u32)last;
        have = true;
        distinct += (u32)__popcll(hb);
        a += nact;
    }
    if (have) tab.offer(top_key(cur, end - run_start), lane);                    // the last run
    return distinct;
}

// One wave per span.
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_top_kernel(View x, TopArgs g, const int jump) {
    const int lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    for (u64 qi = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); qi < g.Q; qi += waves) {
        Walk k = tq_walk_of(x, g.spans[qi]);
        if (k.a < k.end) {                                   // the ended suffix: wave-uniform, every lane reads rank a
            int32_t s0;
            if (!tq_next_symbol(x, k.a, k.length, &s0)) ++k.a;
        }
        const u32 start = k.a;
        const u32 end = g.budget && g.budget < k.end - start ? start + g.budget : k.end;
        TopTable tab;
        tab.reset(lane, g.k);
        const u32 distinct = tq_top_walk(x, lane, start, end, k.length, jump, tab);
        const u64 mine = (u32)lane < g.k ? tab.key : 0ull;
        const u64 live = __ballot(mine != 0);
        u32 rank = 0;                                                                // live keys above mine (<= 64 trips)
        for (u64 m = live; m; m &= m - 1) rank += top_readlane(mine, __ffsll((unsigned long long)m) - 1) > mine ? 1u : 0u;
        const u32 covered = wave_reduce((u32)(mine >> 32), ScanSum{});
        if (mine != 0) {                                                             // rank < popcount(live) <= k
            g.symbols[qi * g.k + rank] = (int32_t)(0xFFFFFFFFu - (u32)mine);
            g.counts[qi * g.k + rank] = (u32)(mine >> 32);
        }
        if (lane == 0) {
            sa_hip_token_top h;
            h.written = (u32)__popcll(live);
            h.distinct = distinct;
            h.covered = covered;
            h.total = k.end - start;
            g.heads[qi] = h;
        }
    }
}

// One lane per (span, draw).
__global__ __launch_bounds__(BLOCK) void tq_sample_kernel(View x, SampleArgs g) {
    const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= g.Q * g.m) return;
    Walk k = tq_walk_of(x, g.spans[i / g.m]);
    int32_t s = -1;
    if (k.a < k.end && !tq_next_symbol(x, k.a, k.length, &s)) ++k.a;   // the ended suffix
    const u32 total = k.end - k.a;
    u32 rank = 0xFFFFFFFFu;
    s = -1;
    if (total) {
        rank = k.a + (u32)__umul64hi(g.draws[i], (u64)total);           // < k.a + total = k.end <= n
        if (!tq_next_symbol(x, rank, k.length, &s)) s = -1;            // (only in an array that is not the suffix array)
    }
    g.symbols[i] = s;
    if (g.ranks) g.ranks[i] = rank;
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// Q >= 1 spans, 1 <= k <= TOP_MAX, Q * k < 2^31; asynchronous on `stream`
inline int launch_top(const Index& x, hipStream_t stream, const NextKnobs& knobs, const TopArgs& g) {
    hipLaunchKernelGGL(tq_top_kernel, dim3(wave_row_grid(g.Q)), dim3(NEXT_WAVES * WAVE), 0, stream, x.view(), g, knobs.jump ? 1 : 0);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// Q >= 1 spans, m >= 1 draws each, Q * m < 2^31
inline int launch_sample(const Index& x, hipStream_t stream, const SampleArgs& g) {
    const u64 grid = (g.Q * g.m + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(tq_sample_kernel, dim3((u32)grid), dim3(BLOCK), 0, stream, x.view(), g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
