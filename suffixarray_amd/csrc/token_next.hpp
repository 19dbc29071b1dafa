// token_next.hpp -- longest-suffix spans and next-symbol counts over the token index (sa_hip_token_index_spans_* / _next_*).
//
// A span is {first, count, length, ended}: the count suffixes SA[first .. first + count) share their first `length` symbols, and
// ended says that SA[first] + length == n (that suffix has no next symbol).  Within a span s(r) = T[SA[r] + length] is
// non-decreasing in r and the one suffix that ends stands first: the next symbols of a span with their multiplicities are the
// run-length encoding of the step function s over [first + ended, first + count).
//
//   tq_span_kernel       one lane per context.  mode 0: one tq_range (tq_span_exact).  mode 1: the largest L such that the
//                        last L symbols of the context occur (need_next: occur with a next symbol) -- that property is
//                        monotone in L, so a binary search over L, <= 64 probes of tq_range.
//   tq_next_kernel       one wave per span, 4 waves per workgroup.  Window step: 64 consecutive ranks, a lane is a run head
//                        when its symbol differs from its left neighbour's (lane_shift_up of scan.hpp; the running symbol is
//                        carried across windows), a ballot gives the heads and a popcount prefix their output slots.  Jump
//                        step: a window that is all the running symbol, with more than NEXT_JUMP_MIN ranks left, samples 64
//                        evenly spaced ranks and narrows to the 1/64 slice where the run ends: a run of R ranks costs about
//                        log64 R steps instead of R / 64.
//   tq_next_lane_kernel  one lane per span: spans of <= NEXT_LANE_MAX suffixes (most spans of a longest-suffix batch) are
//                        answered by their lane, the others are appended to a list by wave-aggregated atomics and
//                        tq_next_kernel runs over that list.  Off by default: it measured 1 % behind the wave form alone.
//
// Short cuts from the key array: length == 1 reads s(r) as the low field of K[r] minus 1 (0 marks the ended suffix), length == 0
// the high field: one read instead of two.
//
// Bounds: the device forms trust nothing.  first and count are clamped to the array, every text index is tested against n, a
// window step advances by >= 1 rank, a jump shrinks its slice 64-fold per step (<= NEXT_JUMP_STEPS steps).  An in-range array
// that is not the suffix array gives unspecified entries from bounded loops, never a read outside the buffers.
#pragma once
#include "token_query.hpp"

namespace sa {
namespace tq {

constexpr u32 NEXT_LANE_MAX = 4;       // suffixes of a span that one lane answers on its own
constexpr int NEXT_WAVES = 4;          // waves (spans in flight) per workgroup of tq_next_kernel
constexpr u32 NEXT_JUMP_MIN = 256;     // ranks left behind an all-equal window before a jump is taken (4 windows)
constexpr int NEXT_JUMP_STEPS = 6;     // 64^6 > 2^31
constexpr int SPAN_PROBES = 64;        // bound of the binary search over L (m < 2^64)
constexpr u32 WAVE_GRID_MAX = 256u * 16u;   // cap of a wave-per-row launch: twice what 256 CUs hold at 8 waves per SIMD
inline u32 wave_row_grid(u64 rows) {   // workgroups for `rows` rows, NEXT_WAVES each; the kernels stride over the rows beyond the cap
    const u64 grid = (rows + NEXT_WAVES - 1) / NEXT_WAVES;
    return (u32)(grid < WAVE_GRID_MAX ? grid : WAVE_GRID_MAX);
}

// s(r) of a span of matched length `length`; false: suffix r has no next symbol (or, in a foreign array, lies outside the text)
__device__ __forceinline__ bool tq_next_symbol(const View& x, u32 r, u32 length, int32_t* s) {
    if (x.K && length <= 1) {
        const u64 k = x.K[r];
        const u32 f = length ? (u32)k : (u32)(k >> 32);
        *s = (int32_t)(f - 1u);
        return f != 0;
    }
    const u64 at = (u64)x.sa[r] + length;
    if (at >= x.n) { *s = -1; return false; }
    *s = x.T[at];
    return true;
}

__device__ __forceinline__ u32 tq_span_ended(const View& x, u32 first, u32 count, u64 length) {
    return (count > 0 && first < x.n && (u64)x.sa[first] + length == x.n) ? 1u : 0u;
}

// the span of the m symbols whose range is r: length saturates at 2^32 - 1 (no text holds a longer pattern: its count is 0)
__device__ __forceinline__ sa_hip_token_span tq_span_of(const View& x, const sa_hip_pair_u32& r, u64 m) {
    sa_hip_token_span s;
    s.first = r.first; s.count = r.second;
    s.length = m > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)m;
    s.ended = tq_span_ended(x, r.first, r.second, m);
    return s;
}
// the exact (mode-0) span of P[0 .. m): one tq_range
__device__ __forceinline__ sa_hip_token_span tq_span_exact(const View& x, const int32_t* __restrict__ P, u64 m) {
    if (x.n == 0) return sa_hip_token_span{0u, 0u, 0u, 0u};   // an empty index: its arrays are not touched
    return tq_span_of(x, tq_range(x, P, m), m);
}

__global__ __launch_bounds__(BLOCK) void tq_span_kernel(View x, const int32_t* __restrict__ pat, const u64* __restrict__ off, u64 Q,
                                                        int mode, u32 max_length, int need_next, sa_hip_token_span* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= Q) return;
    const u64 o0 = off[i], o1 = off[i + 1];
    const u64 m = o1 > o0 ? o1 - o0 : 0;
    const int32_t* P = pat + o0;
    sa_hip_token_span s{0u, 0u, 0u, 0u};
    if (x.n == 0) { out[i] = s; return; }
    if (mode == 0) { out[i] = tq_span_exact(x, P, m); return; }
    u64 hi = m < x.n ? m : x.n;                         // no more than n symbols match
    if (max_length && hi > max_length) hi = max_length;
    u64 lo = 0;                                         // L = 0 always qualifies: {0, n}
    s.count = x.n;
    for (int probe = 0; probe < SPAN_PROBES && lo < hi; ++probe) {
        const u64 L = lo + (hi - lo + 1) / 2;
        const sa_hip_pair_u32 r = tq_range(x, P + (m - L), L);
        u32 eff = r.second;
        if (need_next && r.second == 1) eff -= tq_span_ended(x, r.first, 1u, L);   // only a lone suffix can be decided by it
        if (eff) { lo = L; s.first = r.first; s.count = r.second; } else hi = L - 1;
    }
    s.length = (u32)lo;
    s.ended = tq_span_ended(x, s.first, s.count, lo);
    out[i] = s;
}

struct NextArgs {
    const sa_hip_token_span* spans;
    u64 Q;
    u32 cap;
    int32_t* symbols;            // [Q * cap]
    u32* counts;                 // [Q * cap]
    sa_hip_token_next* heads;    // [Q]
};

// the span as it is walked: clamped to the array, the ended suffix (when it stands first) stepped over
struct Walk { u32 a, end, length; };
__device__ __forceinline__ Walk tq_walk_of(const View& x, const sa_hip_token_span& sp) {
    Walk w;
    w.a = sp.first < x.n ? sp.first : x.n;
    const u32 count = sp.count < x.n - w.a ? sp.count : x.n - w.a;
    w.end = w.a + count;
    w.length = sp.length;
    return w;
}

// The jump step of a wave (tq_next_kernel, tq_top_kernel of token_top.hpp): rank lo holds cur, the ranks (lo, hi) are not known.
// Every step samples 64 evenly spaced ranks and narrows to the 1/64 slice where the run of cur ends, until <= 64 ranks are left
// (<= NEXT_JUMP_STEPS steps); -> the last rank known to hold cur, the same in every lane.
__device__ __forceinline__ u32 tq_jump_run(const View& x, int lane, int32_t cur, u32 length, u32 lo, u32 hi) {
    for (int step = 0; step < NEXT_JUMP_STEPS && hi - lo - 1 > (u32)WAVE; ++step) {
        const u32 stride = (hi - lo - 1 + (u32)WAVE - 1) / (u32)WAVE;
        const u64 q = (u64)lo + (u64)(lane + 1) * stride;
        int32_t sq = 0;
        const bool eq = q < hi && tq_next_symbol(x, (u32)q, length, &sq) && sq == cur;
        const u64 b = __ballot(eq);
        const u32 lead = b == ~0ull ? (u32)WAVE : (u32)__ffsll((unsigned long long)~b) - 1u;   // samples still equal
        const u64 cut = (u64)lo + (u64)(lead + 1) * stride;                                    // the first that is not
        if (lead < (u32)WAVE && cut < hi) hi = (u32)cut;
        lo += lead * stride;
    }
    return lo;
}

// One wave per span.  list == nullptr: span w of all Q; else span list[w] of the *n_list entries tq_next_lane_kernel left.
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_next_kernel(View x, NextArgs g, const u32* __restrict__ list,
                                                                    const u32* __restrict__ n_list, const int jump) {
    const int lane = threadIdx.x & (WAVE - 1);
    const u64 todo = list ? (u64)*n_list : g.Q;
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    for (u64 w = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); w < todo; w += waves) {
        const u64 qi = list ? (u64)list[w] : w;
        if (qi >= g.Q) continue;
        Walk k = tq_walk_of(x, g.spans[qi]);
        int32_t* const sym = g.symbols + qi * g.cap;
        u32* const cnt = g.counts + qi * g.cap;
        if (k.a < k.end) {                                   // the ended suffix: wave-uniform, every lane reads rank a
            int32_t s0;
            if (!tq_next_symbol(x, k.a, k.length, &s0)) ++k.a;
        }
        const u32 start = k.a;
        u32 a = k.a, heads = 0, run_start = k.a, stop_at = k.end;
        int32_t cur = 0;
        bool have = false;
        // every trip advances a by >= 1
        while (a < k.end && heads <= g.cap) {
            const u32 left_n = k.end - a;
            const u32 nact = left_n < (u32)WAVE ? left_n : (u32)WAVE;
            const bool act = (u32)lane < nact;
            int32_t s = cur;
            if (act) (void)tq_next_symbol(x, a + lane, k.length, &s);
            int32_t left = lane_shift_up(s, 1);
            const bool head = act && (lane == 0 ? (!have || s != cur) : s != left);
            const u64 hb = __ballot(head);
            if (hb == 0) {
                // the window is all the running symbol
                u32 lo = a + nact - 1;                       // known to hold cur
                u32 hi = k.end;                              // (lo, hi): not known
                if (jump && hi - lo - 1 > NEXT_JUMP_MIN) lo = tq_jump_run(x, lane, cur, k.length, lo, hi);
                a = lo + 1;
                continue;
            }
            const u32 before = (u32)__popcll(hb & lanemask_lt());
            const u32 slot = heads + before;
            const int f = __ffsll((unsigned long long)hb) - 1;
            if (have && lane == f) cnt[heads - 1] = a + (u32)f - run_start;          // the carried run ends at the first head
            if (head) {
                if (slot < g.cap) sym[slot] = s;
                const u64 above = lane == WAVE - 1 ? 0ull : hb & ~((2ull << lane) - 1ull);
                if (above && slot < g.cap) cnt[slot] = (u32)(__ffsll((unsigned long long)above) - 1 - lane);
            }
            const u64 over = __ballot(head && slot == g.cap);                        // the run behind the last entry: stop there
            if (over) stop_at = a + (u32)(__ffsll((unsigned long long)over) - 1);
            const int last = 63 - __clzll((unsigned long long)hb);
            cur = __shfl(s, last);
            run_start = a + (u32)last;
            have = true;
            heads += (u32)__popcll(hb);
            a += nact;
        }
        if (heads > g.cap) {
            heads = g.cap;
        } else {
            stop_at = k.end;
            if (have && lane == 0) cnt[heads - 1] = k.end - run_start;
        }
        if (lane == 0) {
            sa_hip_token_next h;
            h.written = heads;
            h.covered = heads ? stop_at - start : 0u;
            h.total = k.end - start;
            h.reserved = 0;
            g.heads[qi] = h;
        }
    }
}

// One lane per span: spans of <= NEXT_LANE_MAX suffixes are answered here, the others go to list[] (*n_list of them).
__global__ __launch_bounds__(BLOCK) void tq_next_lane_kernel(View x, NextArgs g, u32* __restrict__ list, u32* __restrict__ n_list) {
    const u64 qi = (u64)blockIdx.x * BLOCK + threadIdx.x;
    bool big = false;
    if (qi < g.Q) {
        const Walk k = tq_walk_of(x, g.spans[qi]);
        if (k.end - k.a <= NEXT_LANE_MAX) {
            int32_t* const sym = g.symbols + qi * g.cap;
            u32* const cnt = g.counts + qi * g.cap;
            u32 written = 0, covered = 0, total = 0, run = 0;
            int32_t cur = 0;
            bool stop = false;
            for (u32 r = k.a; r < k.end; ++r) {
                int32_t s;
                const bool ok = tq_next_symbol(x, r, k.length, &s);
                if (r == k.a && !ok) continue;               // the ended suffix
                ++total;
                if (stop) continue;
                if (run && s == cur) { ++run; continue; }
                if (run) { cnt[written - 1] = run; covered += run; }
                if (written == g.cap) { stop = true; run = 0; continue; }
                sym[written++] = s;
                cur = s; run = 1;
            }
            if (run) { cnt[written - 1] = run; covered += run; }
            sa_hip_token_next h;
            h.written = written; h.covered = covered; h.total = total; h.reserved = 0;
            g.heads[qi] = h;
        } else {
            big = true;
        }
    }
    const int lane = threadIdx.x & (WAVE - 1);
    const u64 m = __ballot(big);
    if (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        u32 base = 0;
        if (lane == leader) base = atomicAdd(n_list, (u32)__popcll(m));
        base = __shfl(base, leader);
        if (big) list[base + (u32)__popcll(m & lanemask_lt())] = (u32)qi;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// test switches (diag_env: only with SA_HIP_DIAG=1), read when the handle is created
struct NextKnobs {
    bool lanes = false;      // SA_HIP_TOKEN_NEXT_LANES=1: spans of <= NEXT_LANE_MAX suffixes by one lane each (measured: no gain)
    bool jump = true;        // SA_HIP_TOKEN_NEXT_JUMP=0: window steps only
    static NextKnobs read() {
        NextKnobs k;
        if (const char* e = diag_env("SA_HIP_TOKEN_NEXT_LANES")) k.lanes = atoi(e) != 0;
        if (const char* e = diag_env("SA_HIP_TOKEN_NEXT_JUMP")) k.jump = atoi(e) != 0;
        return k;
    }
};

// Q >= 1 contexts, every pointer on the device; asynchronous on `stream`
inline int launch_spans(const Index& x, hipStream_t stream, const int32_t* pat, const u64* off, u64 Q, int mode, u32 max_length,
                        int need_next, sa_hip_token_span* out) {
    const u64 grid = (Q + BLOCK - 1) / BLOCK;
    if (grid > 0x7FFFFFFFull) return fail(SA_HIP_EINVAL, "sa_hip_token_index_spans_batch", "too many contexts for one launch");
    hipLaunchKernelGGL(tq_span_kernel, dim3((u32)grid), dim3(BLOCK), 0, stream, x.view(), pat, off, Q, mode, max_length, need_next, out);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// Q >= 1 spans (Q * cap < 2^31); list: Q u32 and n_list: one u32 of the handle, used by the lane form only
inline int launch_next(const Index& x, hipStream_t stream, const NextKnobs& knobs, const NextArgs& g, u32* list, u32* n_list) {
    const u32 grid = wave_row_grid(g.Q);
    if (knobs.lanes) {
        SA_HIP_CHECK(hipMemsetAsync(n_list, 0, sizeof(u32), stream));
        hipLaunchKernelGGL(tq_next_lane_kernel, dim3((u32)((g.Q + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, x.view(), g, list, n_list);
        hipLaunchKernelGGL(tq_next_kernel, dim3(grid), dim3(NEXT_WAVES * WAVE), 0, stream, x.view(), g, (const u32*)list, (const u32*)n_list,
                           knobs.jump ? 1 : 0);
    } else {
        hipLaunchKernelGGL(tq_next_kernel, dim3(grid), dim3(NEXT_WAVES * WAVE), 0, stream, x.view(), g, (const u32*)nullptr,
                           (const u32*)nullptr, knobs.jump ? 1 : 0);
    }
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
