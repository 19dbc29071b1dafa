// token_all.hpp -- per-document counts of an n-gram and the documents that hold ALL n-grams of a group
// (sa_hip_token_index_prepare_doc_ranks / _doc_counts_* / _all_*).
//
// One more structure beside DA and PV of token_docs.hpp, opt-in, 4 bytes per token:
//   RK      the rank-by-document array, int32[n]: RK[starts[d] .. starts[d + 1]) holds the ranks { r : DA[r] == d }, ascending.
//           It is the value array of the sort token_docs.hpp already runs for PV (keys DA[r], values iota, stable), kept instead
//           of freed.  The segments need no offsets of their own: document d owns the text positions [starts[d], starts[d + 1])
//           and every position is one suffix, so the number of ranks with DA[r] == d is starts[d + 1] - starts[d], and the closed
//           starts table bounds the segments.  Equivalently segment d is the sorted set { ISA[p] : p in document d }.  D == 1: iota.
//
// What the queries rest on: "document d has a rank in [a, b)" iff the lower bound of a inside segment d lands inside the segment
// on a value < b, and the number of such ranks is lower_bound(b) - lower_bound(a): two binary searches in one short segment.
//
//   tq_tf_kernel   one lane per cell (span i, slot j < cap): counts[i * cap + j] = the ranks of span i that belong to document
//                  docs[i * cap + j].  Rows may be shorter than cap (a uint32 per span read through a byte stride); slots at or
//                  beyond a row's length are neither read nor written.  A document id outside [0, D) gives 0 without touching RK.
//   tq_all_kernel  one wave per group of 1 .. ALL_MAX spans, NEXT_WAVES per workgroup, no LDS.  The group's counts are loaded one
//                  span per lane; the driver is the span with the smallest count, the lowest index on a tie (one wave scan of
//                  scan.hpp over the inverted key {count, lane}).  The driver's first `examined` ranks are walked as
//                  tq_docs_kernel walks them: PV streamed in DOC_UNROLL windows, a lane is a candidate when PV[r] < a.  Candidate
//                  lanes probe the other spans in index order (their bounds are wave-uniform loads) and stop at the first that
//                  fails; the ballot of the lanes that matched gives the slots, so the order is the driver's rank order.
//
// Bounds: spans are clamped as tq_walk_of does; DA holds values in [0, D) whatever SA holds, so starts[d] and starts[d + 1] exist;
// a segment lies inside [0, n) because the table was checked against n; every search is at most STEPS halvings; a lower bound that
// lands at its segment's end is never dereferenced (in the last document that end is RK[n]).
//
// Not here: OR clauses (CNF with more than one literal), one very long driver split over several waves, a per-wave queue of
// candidates probed 64 at a time.  The shard sets: token_shard_all.hpp.
#pragma once
#include "token_docs.hpp"
#include "scan.hpp"

namespace sa {
namespace tq {

constexpr u32 ALL_MAX = SA_HIP_TOKEN_ALL_MAX;      // spans of one group

struct RankView {             // DocView plus RK
    const int32_t* starts;    // [D + 1]
    const int32_t* da;        // [n]
    const int32_t* pv;        // [n]
    const int32_t* rk;        // [n]
    u32 D;
};

// keys[r] = DA[r] widened: the sort's input, from the DA the handle holds
__global__ __launch_bounds__(BLOCK) void td_widen_kernel(const int32_t* __restrict__ da, u32 n, u64* __restrict__ keys) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) keys[r] = (u64)(u32)da[r];
}

__global__ __launch_bounds__(BLOCK) void td_iota_kernel(int32_t* __restrict__ rk, u32 n) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) rk[r] = (int32_t)r;
}

// the first index in [lo, hi) whose entry is >= key, hi when there is none; entries ascend; at most STEPS halvings
__device__ __forceinline__ u32 tq_seg_lower(const int32_t* __restrict__ rk, u32 lo, u32 hi, u32 key) {
    for (int s = 0; s < STEPS && lo < hi; ++s) {
        const u32 m = lo + ((hi - lo) >> 1);
        if ((u32)rk[m] < key) lo = m + 1; else hi = m;
    }
    return lo;
}

struct TfArgs {
    const sa_hip_token_span* spans;
    u64 Q;
    u32 cap;                       // >= 1
    const int32_t* docs;           // [Q * cap]
    const unsigned char* written;  // nullptr: every row has cap entries; else a uint32 per span, `stride` bytes apart
    u64 stride;
    u32* counts;                   // [Q * cap]
};

// one lane per (span, j), j < cap; Q * cap < 2^31
__global__ __launch_bounds__(BLOCK) void tq_tf_kernel(View x, RankView d, TfArgs g) {
    const u64 cell = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const u64 i = cell / g.cap;
    if (i >= g.Q) return;
    const u32 j = (u32)(cell - i * g.cap);
    if (g.written && j >= *reinterpret_cast<const u32*>(g.written + i * g.stride)) return;
    const Walk k = tq_walk_of(x, g.spans[i]);
    const u32 doc = (u32)g.docs[cell];
    u32 count = 0;
    if (doc < d.D) {                                       // (a negative id is >= 2^31 here)
        const u32 s0 = (u32)d.starts[doc], s1 = (u32)d.starts[doc + 1];
        const u32 lo = tq_seg_lower(d.rk, s0, s1, k.a);
        count = tq_seg_lower(d.rk, lo, s1, k.end) - lo;
    }
    g.counts[cell] = count;
}

struct AllArgs {
    const sa_hip_token_span* spans;   // [S]
    const u32* group_offsets;         // [G + 1], checked on the host: 0 .. S, every group 1 .. ALL_MAX spans
    u64 G;
    u32 cap;                          // 0: counts only
    u32 budget;                       // 0: none
    int32_t* docs;                    // [G * cap]; never touched when cap == 0
    int32_t* offsets;                 // [G * cap]
    sa_hip_token_all* heads;          // [G]
};

// The walk of one wave over the ranks [first_u, first_u + examined) of a group's driver (first_u + examined <= n < 2^31): the
// candidates among them are counted into `candidates`, the matches are returned and the first min(matched, cap) of them go to docs /
// offs (never touched when cap == 0).  sp: the group's m <= ALL_MAX spans.  Every trip advances by DOC_UNROLL windows (the last one
// by what is left, >= 1 rank).  Shared with tq_shard_all_kernel (token_shard_all.hpp).
__device__ __forceinline__ u32 tq_all_walk(const View& x, const RankView& d, const sa_hip_token_span* sp, u32 m, u32 driver, u32 first_u,
                                           u32 examined, u32 cap, int32_t* docs, int32_t* offs, u32 lane, u32& candidates) {
    const u32 end = first_u + examined;                    // <= n < 2^31
    const int32_t first = (int32_t)first_u;
    u32 matched = 0;
    for (u32 a = first_u; a < end; a += (u32)(DOC_UNROLL * WAVE)) {   // (a + 256 < 2^32: no wrap)
        int32_t pv[DOC_UNROLL];
#pragma unroll
        for (int u = 0; u < DOC_UNROLL; ++u) {
            const u32 r = a + (u32)u * WAVE + lane;
            pv[u] = r < end ? d.pv[r] : 0x7FFFFFFF;        // beyond the range: never a candidate
        }
#pragma unroll
        for (int u = 0; u < DOC_UNROLL; ++u) {
            const u32 r = a + (u32)u * WAVE + lane;
            const bool cand = r < end && pv[u] < first;
            const u64 cb = __ballot(cand);
            if (cb == 0) continue;
            candidates += (u32)__popcll(cb);
            bool match = cand;
            int32_t doc = 0;
            if (cand) {                                    // no cross-lane operation inside: the lanes diverge here
                doc = d.da[r];
                const u32 g0 = (u32)d.starts[doc], g1 = (u32)d.starts[doc + 1];
                for (u32 j = 0; j < m && match; ++j) {
                    if (j == driver) continue;
                    const Walk o = tq_walk_of(x, sp[j]);   // the same address in every lane
                    const u32 at = tq_seg_lower(d.rk, g0, g1, o.a);
                    match = at < g1 && (u32)d.rk[at] < o.end;
                }
            }
            const u64 mb = __ballot(match);
            if (mb == 0) continue;
            const u32 slot = matched + (u32)__popcll(mb & lanemask_lt());
            if (match && slot < cap) {
                docs[slot] = doc;
                offs[slot] = (int32_t)(x.sa[r] - (u32)d.starts[doc]);
            }
            matched += (u32)__popcll(mb);
        }
    }
    return matched;
}

// One wave per group.
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_all_kernel(View x, RankView d, AllArgs g) {
    const u32 lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    for (u64 w = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); w < g.G; w += waves) {
        const u32 s0 = g.group_offsets[w];
        u32 m = g.group_offsets[w + 1] - s0;
        if (m > ALL_MAX) m = ALL_MAX;                      // (the host refused such a table)
        const sa_hip_token_span* const sp = g.spans + s0;
        // the driver: the smallest {count, index}; lanes beyond the group hold the largest key there is
        Walk mine{0u, 0u, 0u};
        if (lane < m) mine = tq_walk_of(x, sp[lane]);
        const u64 key = lane < m ? ((u64)(mine.end - mine.a) << 32) | lane : ~0ull;
        const u64 best = ~wave_reduce(~key, ScanMax{});
        const u32 driver = m ? (u32)best : 0u, count = m ? (u32)(best >> 32) : 0u;   // (m == 0: the host refused such a table)
        const u32 first_u = __shfl(mine.a, (int)driver);
        const u32 examined = (g.budget && g.budget < count) ? g.budget : count;
        u32 candidates = 0;
        const u32 matched = tq_all_walk(x, d, sp, m, driver, first_u, examined, g.cap, g.docs + w * g.cap, g.offsets + w * g.cap, lane,
                                        candidates);
        if (lane == 0) {
            sa_hip_token_all h;
            h.written = matched < g.cap ? matched : g.cap;
            h.examined = examined;
            h.matched = matched;
            h.candidates = candidates;
            h.driver = driver;
            h.count = count;
            h.reserved[0] = h.reserved[1] = 0;
            g.heads[w] = h;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// what can be told from the group table alone
inline int all_groups_check(const char* who, const uint64_t* goff, u64 S, u64 G) {
    if (goff[0] != 0) return fail(SA_HIP_EINVAL, who, "group_offsets[0] != 0");
    for (u64 i = 0; i < G; ++i) {
        if (goff[i + 1] <= goff[i]) return fail(SA_HIP_EINVAL, who, "an empty group (group_offsets do not ascend)");
        if (goff[i + 1] - goff[i] > ALL_MAX) return fail(SA_HIP_EINVAL, who, "a group of more than SA_HIP_TOKEN_ALL_MAX spans");
    }
    if (goff[G] != S) return fail(SA_HIP_EINVAL, who, "group_offsets do not end at S");
    return 0;
}

struct DocRanks {
    DevBuf rk;
    hipEvent_t ev[2] = {};
    bool have = false;
    u64 bytes = 0;
    u32 passes = 0;
    float prepare_ms = 0.f;

    void clear() { rk.release(); have = false; bytes = 0; passes = 0; prepare_ms = 0.f; }
    void release() {
        clear();
        for (int j = 0; j < 2; ++j) if (ev[j]) { (void)hipEventDestroy(ev[j]); ev[j] = nullptr; }
    }

    RankView view(const Docs& d) const {
        RankView v{};
        v.starts = d.starts.as<int32_t>(); v.da = d.da.as<int32_t>(); v.pv = d.pv.as<int32_t>(); v.rk = rk.as<int32_t>(); v.D = d.D;
        return v;
    }

    // d has documents.  Synchronous on `stream`; on an error the handle has no RK.
    int build(const Index& x, const Docs& d, hipStream_t stream, const char* who) {
        SA_HIP_CHECK(hipStreamSynchronize(stream));
        clear();
        RadixWorkspace ws;
        DevBuf k0, k1, v0, v1;
        const int rc = build_on(x, d, stream, who, ws, k0, k1, v0, v1);
        (void)hipStreamSynchronize(stream);
        ws.destroy();
        k0.release(); k1.release(); v0.release(); v1.release();
        if (rc) clear(); else have = true;
        return rc;
    }

  private:
    int build_on(const Index& x, const Docs& d, hipStream_t stream, const char* who, RadixWorkspace& ws, DevBuf& k0, DevBuf& k1,
                 DevBuf& v0, DevBuf& v1) {
        int rc;
        const u32 n = x.n;
        for (int j = 0; j < 2; ++j) if (!ev[j]) SA_HIP_CHECK(hipEventCreate(&ev[j]));
        if ((rc = rk.ensure((size_t)n * 4 + 64))) return rc;
        const bool sorted = d.D > 1 && n > 0;
        if (sorted && (rc = rank_sort_reserve(ws, k0, k1, v0, v1, n))) return rc;
        SA_HIP_CHECK(hipEventRecord(ev[0], stream));
        if (sorted) {
            u64* kr = nullptr; u32* vr = nullptr;
            hipLaunchKernelGGL(td_widen_kernel, dim3(stream_grid(n, 1024)), dim3(BLOCK), 0, stream, (const int32_t*)d.da.as<int32_t>(), n,
                               k0.as<u64>());
            SA_HIP_CHECK(hipGetLastError());
            if ((rc = rank_sort(ws, stream, k0, k1, v0, v1, n, d.D, &kr, &vr, &passes))) return rc;
            SA_HIP_CHECK(hipMemcpyAsync(rk.p, vr, (size_t)n * 4, hipMemcpyDeviceToDevice, stream));
        } else if (n) {
            hipLaunchKernelGGL(td_iota_kernel, dim3(stream_grid(n, 1024)), dim3(BLOCK), 0, stream, rk.as<int32_t>(), n);
            SA_HIP_CHECK(hipGetLastError());
        }
        SA_HIP_CHECK(hipEventRecord(ev[1], stream));
        DeviceStatus st{};
        if (sorted) SA_HIP_CHECK(hipMemcpyAsync(&st, ws.dstat, sizeof st, hipMemcpyDeviceToHost, stream));
        SA_HIP_CHECK(hipEventSynchronize(ev[1]));
        SA_HIP_CHECK(hipStreamSynchronize(stream));
        if (st.error) return fail(SA_HIP_EINTERNAL, who, "device look-back spin limit expired");
        if (sorted && (rc = ws.timer.flush())) return rc;
        SA_HIP_CHECK(hipEventElapsedTime(&prepare_ms, ev[0], ev[1]));
        bytes = (u64)n * 4;
        return 0;
    }
};

// Q >= 1 spans, cap >= 1, Q * cap < 2^31; every pointer on the device; asynchronous on `stream`
inline int launch_tf(const Index& x, const Docs& d, const DocRanks& r, hipStream_t stream, const TfArgs& g) {
    const u64 cells = g.Q * g.cap;
    hipLaunchKernelGGL(tq_tf_kernel, dim3((u32)((cells + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, x.view(), r.view(d), g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// G >= 1 groups, G * cap < 2^31 (cap may be 0)
inline int launch_all(const Index& x, const Docs& d, const DocRanks& r, hipStream_t stream, const AllArgs& g) {
    hipLaunchKernelGGL(tq_all_kernel, dim3(wave_row_grid(g.G)), dim3(NEXT_WAVES * WAVE), 0, stream, x.view(), r.view(d), g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
