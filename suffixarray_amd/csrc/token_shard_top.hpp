// token_shard_top.hpp -- the k most frequent next symbols of a context over a shard set, and next symbols drawn from its S spans
// (sa_hip_token_shards_top_* / _sample_*, include/sa_hip.h section 6l).  Spans are those of token_shards.hpp, [s * Q + i]; the walk
// of one shard, s(r) = T[SA[r] + length] and the table of one index are token_top.hpp's.
//
//   tq_shard_top_kernel     one wave per context, NEXT_WAVES per workgroup, the rows strided as in tq_top_kernel.  Lane s < S loads
//                           shard s's span and View, clamps (tq_walk_of) and steps over the ended suffix; total, length and the
//                           ballot of the shards that have a continuation are wave-wide.
//                           One live shard (the common case behind a long context, and all of S = 1): tq_top_walk of token_top.hpp
//                           over that shard as it is, its 32-bit counts widened on the way out.  A set of one shard with the
//                           fast path on is launched as tq_shard_top_kernel<false>, which holds this path alone: the merge walk's
//                           32 KiB of LDS per workgroup would leave it 5 waves per SIMD where the walk's registers allow 8.
//                           Several: the merge walk.  Lane s keeps shard s's cursor a_s and a queue of completed runs (symbol, count)
//                           in LDS, SHARD_TOP_QUEUE entries per wave cut into S queues of D = shard_top_depth(S) entries.  A refill
//                           of shard s (tq_shard_refill; s wave-uniform, so its View is read into scalar registers) is one window
//                           step of 64 ranks at a_s: every run head's run but the last is complete, a run that reaches the shard's end
//                           is too; the first D of them are written at their ballot-prefix slots and a_s moves to the first head
//                           that was not kept -- the open run is read again by the next refill, nothing is carried.  A window that
//                           is all one symbol and stops short of the end finds the run's end by further window steps, behind
//                           NEXT_JUMP_MIN ranks by tq_gallop_run / tq_jump_run, and yields that one run.  So a refill yields >= 1
//                           run and advances a_s by >= 1 rank.  A merge step refills the lanes whose queue is empty while a_s <
//                           end_s, takes the minimum of the queue heads' symbols (sign bit flipped, as tq_next_merge_kernel; the
//                           lanes without a head are left out by their ballot, which stands in for that kernel's idle key), sums
//                           the counts of the lanes that hold it as uint64, pops them, cuts the sum to what the budget has left and
//                           offers the run to the table.  Minimum and sum are scalar loops over the ballot's <= S bits, one
//                           v_readlane each: the two 64-lane u64 reductions they replace cost about 1 us per step.
//                           <= one step per merged run, <= one refill per run of a shard.
//                           The table is TopTable's scheme with a key of three words (TopKey2: count uint64, 0xFFFFFFFF - symbol):
//                           a sum over 64 shards reaches 2^37 and no longer packs with the symbol into 64 bits.  Lane j < k holds
//                           one entry, count 0 is empty, lanes >= k hold all ones; the minimum (wave_scan_incl of scan.hpp with an
//                           ordered combine, read at lane 63 into scalar registers) and its lane are wave-uniform; a run that does
//                           not beat the minimum costs one scalar compare.  At the end every lane ranks its key by counting the
//                           live keys above it.  No scratch, no register array indexed at run time
//                           (profiles/token_shard_top_resources.txt).
//   tq_shard_sample_kernel  one lane per (context, draw): the S clamped spans summed for total, r = floor(draw * total / 2^64), a
//                           second pass over the spans for the shard that holds r in the shard-major numbering, one gather.
//
// Bounds: spans are clamped per shard, every text index is tested against n (tq_next_symbol), a refill advances its cursor by >= 1
// rank and writes <= D entries into its own queue, a merge step pops >= 1 queue entry, the run search is bounded as in
// token_top.hpp; rank < k in every lane that writes.  Arrays that are not suffix arrays give unspecified entries, never an access
// outside the buffers.
#pragma once
#include "rows_device.hpp"
#include "token_shards.hpp"
#include "token_top.hpp"

namespace sa {
namespace tq {

constexpr u32 SHARD_TOP_QUEUE = 1024;  // (symbol, count) entries of LDS per wave: 8 KiB, 32 KiB per workgroup
// entries of one shard's queue: 64 up to 16 shards, 32 up to 32, 16 beyond
__host__ __device__ inline u32 shard_top_depth(u32 S) { return S <= 16 ? 64u : S <= 32 ? 32u : 16u; }

struct ShardTopArgs {
    const View* tab;                   // [S]
    const sa_hip_token_span* spans;    // [S * Q]
    u64 Q;
    u32 S;
    u32 k;                             // 1 .. TOP_MAX
    u64 budget;                        // merged continuations walked per context at most; 0: all
    int32_t* symbols;                  // [Q * k]
    u64* counts;                       // [Q * k]
    sa_hip_token_shards_top* heads;    // [Q]
    int fast;                          // 1: a context with one live shard takes tq_top_walk
};

struct ShardSampleArgs {
    const View* tab;
    const sa_hip_token_span* spans;    // [S * Q]
    u64 Q;
    u32 S;
    u32 m;                             // draws per context
    const u64* draws;                  // [Q * m]
    int32_t* symbols;                  // [Q * m]
    u32* shards;                       // [Q * m], or nullptr
    u32* ranks;                        // [Q * m], or nullptr
};

// count (lo, hi) and 0xFFFFFFFF - symbol: larger is better; count 0 is empty
struct TopKey2 { u32 lo, hi, inv; };
__device__ __forceinline__ u64 top2_count(const TopKey2& a) { return (u64)a.hi << 32 | a.lo; }
__device__ __forceinline__ TopKey2 top2_key(int32_t symbol, u64 count) { return TopKey2{(u32)count, (u32)(count >> 32), 0xFFFFFFFFu - (u32)symbol}; }
__device__ __forceinline__ bool top2_less(const TopKey2& a, const TopKey2& b) {
    const u64 ca = top2_count(a), cb = top2_count(b);
    return ca != cb ? ca < cb : a.inv < b.inv;
}
__device__ __forceinline__ bool top2_equal(const TopKey2& a, const TopKey2& b) { return a.lo == b.lo && a.hi == b.hi && a.inv == b.inv; }
struct TopKey2Min {
    __device__ __forceinline__ TopKey2 operator()(const TopKey2& x, const TopKey2& y) const { return top2_less(y, x) ? y : x; }
};
// v of lane j, j wave-uniform: into scalar registers
__device__ __forceinline__ TopKey2 top2_readlane(const TopKey2& v, int j) {
    return TopKey2{(u32)__builtin_amdgcn_readlane((int)v.lo, j), (u32)__builtin_amdgcn_readlane((int)v.hi, j),
                   (u32)__builtin_amdgcn_readlane((int)v.inv, j)};
}
__device__ __forceinline__ u32 shard_readlane(u32 v, int j) { return (u32)__builtin_amdgcn_readlane((int)v, j); }

struct TopTable2 {
    TopKey2 key;    // this lane's entry
    TopKey2 min;    // the smallest key of the wave: an entry of a lane < k, or the empty key while one is empty
    int at;         // the lowest lane that holds it
    __device__ __forceinline__ void reset(int lane, u32 k) {
        key = (u32)lane < k ? TopKey2{0u, 0u, 0u} : TopKey2{~0u, ~0u, ~0u};
        min = TopKey2{0u, 0u, 0u};
        at = 0;
    }
    // c is wave-uniform
    __device__ __forceinline__ void offer(const TopKey2& c, int lane) {
        if (!top2_less(min, c)) return;
        if (lane == at) key = c;
        min = top2_readlane(wave_scan_incl(key, TopKey2Min{}), WAVE - 1);
        at = __ffsll((unsigned long long)__ballot(top2_equal(key, min))) - 1;
    }
};

// One refill of a shard's queue `slot` (D entries) by the whole wave: the window of 64 ranks at a < end of x, s(r) read at `length`;
// a, end and length are wave-uniform.  -> the cursor behind the last run kept and the runs kept (>= 1), both wave-uniform.
struct Refill { u32 a, kept; };
__device__ __forceinline__ Refill tq_shard_refill(const View& x, int lane, uint2* slot, u32 D, u32 a, u32 end, u32 length, int jump) {
    const u32 left_n = end - a;
    const u32 nact = left_n < (u32)WAVE ? left_n : (u32)WAVE;
    const bool act = (u32)lane < nact;
    int32_t s = 0;
    if (act) (void)tq_next_symbol(x, a + lane, length, &s);
    const int32_t left = lane_shift_up(s, 1);
    const bool head = act && (lane == 0 || s != left);
    const u64 hb = __ballot(head);                            // bit 0 is set: nact >= 1
    const bool reaches = a + nact == end;
    const u32 nheads = (u32)__popcll(hb);
    if (nheads == 1 && !reaches) {
        // the window is all one symbol and the shard goes on: where that run ends
        const int32_t cur = __shfl(s, 0);
        u32 lo = a + nact - 1;                                // known to hold cur; (lo, end): not known
        u32 run_end = end;
        // every trip advances lo by >= 1
        while (lo + 1 < end) {
            if (jump && end - lo - 1 > NEXT_JUMP_MIN) lo = tq_gallop_run(x, lane, cur, length, lo, end);
            const u32 p = lo + 1;
            if (p >= end) break;
            const u32 n2 = end - p < (u32)WAVE ? end - p : (u32)WAVE;
            int32_t s2 = cur;
            if ((u32)lane < n2) (void)tq_next_symbol(x, p + lane, length, &s2);
            const u64 b = __ballot(s2 != cur);
            if (b) { run_end = p + (u32)(__ffsll((unsigned long long)b) - 1); break; }
            lo = p + n2 - 1;
        }
        if (lane == 0) slot[0] = make_uint2((u32)cur, run_end - a);
        return Refill{run_end, 1u};
    }
    const u32 complete = reaches ? nheads : nheads - 1;       // >= 1
    const u32 kept = complete < D ? complete : D;
    const u32 at = (u32)__popcll(hb & lanemask_lt());
    const u64 above = lane == WAVE - 1 ? 0ull : hb & ~((2ull << lane) - 1ull);
    const u32 next = above ? (u32)(__ffsll((unsigned long long)above) - 1) : nact;   // the next head, or the window's end
    if (head && at < kept) slot[at] = make_uint2((u32)s, next - (u32)lane);
    const u64 cut = __ballot(head && at == kept);             // the first head that is not kept
    return Refill{cut ? a + (u32)(__ffsll((unsigned long long)cut) - 1) : a + nact, kept};
}

// the ranks of shard s's span of context i that have a next symbol: [a, end)
__device__ __forceinline__ Walk tq_shard_walk(const View& x, const sa_hip_token_span& sp) {
    Walk w = tq_walk_of(x, sp);
    int32_t s0;
    if (w.a < w.end && !tq_next_symbol(x, w.a, w.length, &s0)) ++w.a;   // the ended suffix
    return w;
}

// The merge walk of one wave over the shards whose lanes hold a_s < end_s: the first `walked` merged continuations, every merged
// run offered to tab (reset by the caller) -> the number of merged runs.  q: the wave's SHARD_TOP_QUEUE entries of LDS.
__device__ __forceinline__ u32 tq_shard_merge_walk(const ShardTopArgs& g, int lane, uint2* q, u32 a, u32 end, u32 len, u64 walked, int jump,
                                                   TopTable2& tab) {
    const u32 D = shard_top_depth(g.S);
    u32 qpos = 0, qlen = 0, distinct = 0;
    uint2 h = make_uint2(0u, 0u);                             // the head of this lane's queue
    bool reload = false;
    u64 left = walked;
    // every trip pops >= 1 queue entry, every refill advances its shard's cursor by >= 1 rank
    while (left) {
        const u64 need = __ballot(qpos == qlen && a < end);
        for (u64 m = need; m; m &= m - 1) {
            const int s = __ffsll((unsigned long long)m) - 1;
            const View x = g.tab[s];
            const Refill r = tq_shard_refill(x, lane, q + (u32)s * D, D, shard_readlane(a, s), shard_readlane(end, s),
                                             shard_readlane(len, s), jump);
            if (lane == s) { a = r.a; qpos = 0; qlen = r.kept; reload = true; }
        }
        if (need) wave_lds_sync();
        if (reload && qpos < qlen) h = q[(u32)lane * D + qpos];
        reload = false;
        const bool has = qpos < qlen;
        const u32 key = h.x ^ 0x80000000u;                    // signed order as unsigned order
        const u64 heads = __ballot(has);
        if (!heads) break;                                    // every shard is exhausted
        u32 mn = 0xFFFFFFFFu;                                 // the smallest head, over the <= S lanes that have one (scalar)
        for (u64 m = heads; m; m &= m - 1) {
            const u32 v = shard_readlane(key, __ffsll((unsigned long long)m) - 1);
            mn = v < mn ? v : mn;
        }
        const bool hit = has && key == mn;
        u64 sum = 0;                                          // its count over the shards that hold it (scalar, uint64)
        for (u64 m = __ballot(hit); m; m &= m - 1) sum += shard_readlane(h.y, __ffsll((unsigned long long)m) - 1);
        if (hit) { ++qpos; reload = true; }
        if (sum > left) sum = left;                           // the run that the budget cuts counts with what lies inside
        left -= sum;
        ++distinct;
        tab.offer(top2_key((int32_t)(mn ^ 0x80000000u), sum), lane);
    }
    return distinct;
}

// One wave per context.  MERGE false: the form for a set of one shard with the fast path on -- no context has two live shards, the
// merge walk and its LDS are not compiled in, and the occupancy is the registers' (launch_shard_top chooses).
template <bool MERGE>
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_shard_top_kernel(ShardTopArgs g, const int jump) {
    const int lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    for (u64 qi = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); qi < g.Q; qi += waves) {
        u32 a = 0, end = 0, len = 0;
        if ((u32)lane < g.S) {
            const Walk w = tq_shard_walk(g.tab[lane], g.spans[(u64)lane * g.Q + qi]);
            a = w.a; end = w.end; len = w.length;
        }
        const u64 total = top_uniform(wave_reduce((u64)(end - a), ScanSum{}));
        const u32 length = wave_reduce(len, ScanMax{});
        const u64 live_shards = __ballot(end > a);
        const u64 walked = g.budget && g.budget < total ? g.budget : total;
        TopTable2 tab;
        tab.reset(lane, g.k);
        u32 distinct = 0;
        if ((!MERGE || g.fast) && __popcll(live_shards) == 1) {
            const int s = __ffsll((unsigned long long)live_shards) - 1;
            const View x = g.tab[s];
            const u32 start = shard_readlane(a, s);           // total = this shard's end - start, walked <= total
            TopTable one;
            one.reset(lane, g.k);
            distinct = tq_top_walk(x, lane, start, start + (u32)walked, shard_readlane(len, s), jump, one);
            if ((u32)lane < g.k) tab.key = TopKey2{(u32)(one.key >> 32), 0u, (u32)one.key};   // an empty entry stays empty
        } else if constexpr (MERGE) {
            __shared__ uint2 s_q[NEXT_WAVES][SHARD_TOP_QUEUE];
            distinct = tq_shard_merge_walk(g, lane, s_q[threadIdx.x >> 6], a, end, len, walked, jump, tab);
        }
        const TopKey2 mine = (u32)lane < g.k ? tab.key : TopKey2{0u, 0u, 0u};
        const u64 live = __ballot(top2_count(mine) != 0);
        u32 rank = 0;                                                                // live keys above mine (<= 64 trips)
        for (u64 m = live; m; m &= m - 1) rank += top2_less(mine, top2_readlane(mine, __ffsll((unsigned long long)m) - 1)) ? 1u : 0u;
        const u64 covered = wave_reduce(top2_count(mine), ScanSum{});
        if (top2_count(mine) != 0) {                                                 // rank < popcount(live) <= k
            g.symbols[qi * g.k + rank] = (int32_t)(0xFFFFFFFFu - mine.inv);
            g.counts[qi * g.k + rank] = top2_count(mine);
        }
        if (lane == 0) {
            sa_hip_token_shards_top hd;
            hd.written = (u32)__popcll(live);
            hd.distinct = distinct;
            hd.length = length;
            hd.shards = (u32)__popcll(live_shards);
            hd.covered = covered;
            hd.total = total;
            g.heads[qi] = hd;
        }
    }
}

// One lane per (context, draw).
__global__ __launch_bounds__(BLOCK) void tq_shard_sample_kernel(ShardSampleArgs g) {
    const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= g.Q * g.m) return;
    const u64 ctx = i / g.m;
    u64 total = 0;
    for (u32 s = 0; s < g.S; ++s) {
        const Walk w = tq_shard_walk(g.tab[s], g.spans[(u64)s * g.Q + ctx]);
        total += w.end - w.a;
    }
    int32_t sym = -1;
    u32 shard = 0xFFFFFFFFu, rank = 0xFFFFFFFFu;
    if (total) {
        const u64 r = __umul64hi(g.draws[i], total);          // < total
        u64 before = 0;
        for (u32 s = 0; s < g.S; ++s) {
            const View x = g.tab[s];
            const Walk w = tq_shard_walk(x, g.spans[(u64)s * g.Q + ctx]);
            const u64 t = w.end - w.a;
            if (r - before < t) {
                shard = s;
                rank = w.a + (u32)(r - before);               // < w.end <= n
                if (!tq_next_symbol(x, rank, w.length, &sym)) sym = -1;   // (only in an array that is not the suffix array)
                break;
            }
            before += t;
        }
    }
    g.symbols[i] = sym;
    if (g.shards) g.shards[i] = shard;
    if (g.ranks) g.ranks[i] = rank;
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// Q >= 1 contexts, 1 <= k <= TOP_MAX, Q * k < 2^31; asynchronous on `stream`
inline int launch_shard_top(hipStream_t stream, const ShardTopArgs& g, bool jump) {
    if (g.S == 1 && g.fast) {                                // one shard: one live shard or none in every context
        hipLaunchKernelGGL(tq_shard_top_kernel<false>, dim3(wave_row_grid(g.Q)), dim3(NEXT_WAVES * WAVE), 0, stream, g, jump ? 1 : 0);
    } else {
        hipLaunchKernelGGL(tq_shard_top_kernel<true>, dim3(wave_row_grid(g.Q)), dim3(NEXT_WAVES * WAVE), 0, stream, g, jump ? 1 : 0);
    }
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// Q >= 1 contexts, m >= 1 draws each, Q * m < 2^31
inline int launch_shard_sample(hipStream_t stream, const ShardSampleArgs& g) {
    const u64 grid = (g.Q * g.m + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(tq_shard_sample_kernel, dim3((u32)grid), dim3(BLOCK), 0, stream, g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
