// token_docs.hpp -- documents of a token index: which documents hold an n-gram, where in them, and in how many it occurs
// (sa_hip_token_index_set_documents / _locate_* / _docs_*).
//
// Documents: a table starts[0 .. D) of text positions, starts[0] == 0, non-decreasing, every entry <= n; document d is
// T[starts[d] .. starts[d + 1]) with starts[D] = n implied.  Equal neighbours are empty documents.  doc(p) is the LARGEST d with
// starts[d] <= p, so an empty document never owns a token.  An occurrence belongs to the document of its FIRST token.  Occurrences
// that run over a boundary are not filtered: callers separate documents with a token of their own, as the shard sets already assume.
//
// Structures, prepared once per table on the handle's stream (Docs::build), 8 bytes per token plus 4 (D + 1):
//   starts  int32[D + 1], closed by n.
//   DA      the document array, DA[r] = doc(SA[r]), int32[n]: one lane per rank, a binary search over starts (<= 32 steps).
//   PV      the previous-rank array, PV[r] = the largest r' < r with DA[r'] == DA[r], -1 when there is none, int32[n].  A stable
//           sort of the ranks by document (radix_sort_pairs over the widened keys DA[r], values = iota, key bits
//           [0, bits_for(D)): the keys are 0 .. D - 1) puts every document's ranks side by side in ascending order; one pass over
//           the sorted order sets PV[vals[i]] = keys[i - 1] == keys[i] ? vals[i - 1] : -1.  D == 1 needs no sort: PV[r] = r - 1.
//           The sort's scratch (two u64 and two u32 arrays of n, 24 n bytes, and a RadixWorkspace of its own) is freed before
//           the call returns.
//
// What the queries rest on: for a rank range [a, b), rank r in it is the FIRST occurrence of its document inside the range iff
// PV[r] < a (signed compare; both sides are below 2^31).  If PV[r] >= a, rank PV[r] is an earlier rank of the range with the
// same document; if PV[r] < a, no rank of [a, r) has that document, because PV[r] is the largest such rank below r.  The
// criterion does not look at b, so it holds for every prefix [a, a + examined) of the range as well.
//
//   tq_locate_kernel  one lane per (span, j), j < min(count, cap): docs[i * cap + j] = DA[first + j], offsets[i * cap + j] =
//                     SA[first + j] - starts[that document]; the head is {written, count}.  Entries come in suffix order.
//   tq_docs_kernel    one wave per span, NEXT_WAVES per workgroup, no LDS.  examined = budget ? min(count, budget) : count.  A
//                     window is 64 consecutive ranks whose PV is read coalesced; a lane is a head when PV[r] < first; the ballot's
//                     popcount is added to `distinct`, the lane's prefix popcount gives its slot, and only lanes with a slot < cap
//                     read DA[r], SA[r] and starts[.] and write.  DOC_UNROLL windows' PV loads are issued before the first ballot.
//                     The head is {written, examined, distinct, count}: the exact document frequency iff examined == count.
//                     cap == 0 counts only and touches neither docs nor offsets.
//
// Bounds: first and count are clamped to the array as tq_walk_of does, every step advances by >= 1 window, DA holds values in
// [0, D) whatever SA holds (it comes from the binary search), SA entries were range-checked when the handle was prepared.  An
// in-range array that is not the suffix array gives unspecified entries, never a spin or a read outside the buffers.
//
// Not here: one very long span split over several waves inside one index.  A wave streams one coalesced array with no gather on the
// counting path; `budget` is the caller's lever.  A shard set walks the S pieces of a span by one wave each
// (token_shard_docs.hpp).
#pragma once
#include "token_next.hpp"
#include "radix_sort.hpp"
#include <vector>

namespace sa {
namespace tq {

constexpr int DOC_UNROLL = 4;          // windows (of 64 ranks) whose PV loads are in flight together in tq_docs_kernel

struct DocView {              // what the document kernels read
    const int32_t* starts;    // [D + 1]
    const int32_t* da;        // [n]
    const int32_t* pv;        // [n]
    u32 D;
};

// the largest d < D with starts[d] <= p (starts[0] == 0: there is one); at most STEPS halvings of [0, D)
__device__ __forceinline__ u32 td_doc_of(const int32_t* __restrict__ starts, u32 D, u32 p) {
    u32 lo = 0, hi = D;                                  // lo = number of entries known to be <= p
    for (int s = 0; s < STEPS && lo < hi; ++s) {
        const u32 m = (lo + hi) >> 1;
        if ((u32)starts[m] <= p) lo = m + 1; else hi = m;
    }
    return lo ? lo - 1 : 0;
}

// DA[r] = doc(SA[r]); keys (may be nullptr: D == 1) receives the same value widened for the sort
__global__ __launch_bounds__(BLOCK) void td_da_kernel(const u32* __restrict__ sa, u32 n, const int32_t* __restrict__ starts, u32 D,
                                                      int32_t* __restrict__ da, u64* __restrict__ keys) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const u32 d = td_doc_of(starts, D, sa[r]);
        da[r] = (int32_t)d;
        if (keys) keys[r] = (u64)d;
    }
}

// keys / vals: the ranks sorted by document, stable (vals ascending within a document); keys == nullptr: one document
__global__ __launch_bounds__(BLOCK) void td_pv_kernel(const u64* __restrict__ keys, const u32* __restrict__ vals, u32 n,
                                                      int32_t* __restrict__ pv) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (!keys) { pv[i] = (int32_t)i - 1; continue; }
        const u32 r = vals[i];
        if (r >= n) continue;                            // (a sort that failed is reported by its status word)
        pv[r] = (i > 0 && keys[i - 1] == keys[i]) ? (int32_t)vals[i - 1] : -1;
    }
}

struct LocateArgs {
    const sa_hip_token_span* spans;
    u64 Q;
    u32 cap;                       // >= 1
    int32_t* docs;                 // [Q * cap]
    int32_t* offsets;              // [Q * cap]
    sa_hip_token_locate* heads;    // [Q]
};

// one lane per (span, j), j < cap; Q * cap < 2^31
__global__ __launch_bounds__(BLOCK) void tq_locate_kernel(View x, DocView d, LocateArgs g) {
    const u64 cell = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const u64 i = cell / g.cap;
    if (i >= g.Q) return;
    const u32 j = (u32)(cell - i * g.cap);
    const Walk k = tq_walk_of(x, g.spans[i]);
    const u32 count = k.end - k.a;
    const u32 written = count < g.cap ? count : g.cap;
    if (j == 0) {
        sa_hip_token_locate h;
        h.written = written; h.count = count;
        g.heads[i] = h;
    }
    if (j >= written) return;
    const u32 r = k.a + j;
    const int32_t doc = d.da[r];
    g.docs[cell] = doc;
    g.offsets[cell] = (int32_t)(x.sa[r] - (u32)d.starts[doc]);
}

struct DocsArgs {
    const sa_hip_token_span* spans;
    u64 Q;
    u32 cap;                       // 0: counts only
    u32 budget;                    // 0: none
    int32_t* docs;                 // [Q * cap]; never touched when cap == 0
    int32_t* offsets;              // [Q * cap]
    sa_hip_token_docs* heads;      // [Q]
    unsigned long long* examined;  // one counter: the sum of the heads' examined, what the launch streamed
};

// The walk of one wave over the ranks [a0, a0 + examined) of a span (a0 + examined <= n < 2^31): the distinct documents among them,
// the first min(distinct, cap) of them to docs / offs (never touched when cap == 0).  Every trip advances by DOC_UNROLL windows
// (the last one by what is left, >= 1 rank).  Shared with tq_shard_docs_kernel (token_shard_docs.hpp).
__device__ __forceinline__ u32 tq_docs_walk(const View& x, const DocView& d, u32 a0, u32 examined, u32 cap, int32_t* docs, int32_t* offs,
                                            u32 lane) {
    const u32 end = a0 + examined;
    const int32_t first = (int32_t)a0;
    u32 distinct = 0;
    for (u32 a = a0; a < end; a += (u32)(DOC_UNROLL * WAVE)) {   // (a + 256 < 2^32: no wrap)
        int32_t pv[DOC_UNROLL];
#pragma unroll
        for (int u = 0; u < DOC_UNROLL; ++u) {
            const u32 r = a + (u32)u * WAVE + lane;
            pv[u] = r < end ? d.pv[r] : 0x7FFFFFFF;    // beyond the range: never a head
        }
#pragma unroll
        for (int u = 0; u < DOC_UNROLL; ++u) {
            const u32 r = a + (u32)u * WAVE + lane;
            const bool head = r < end && pv[u] < first;
            const u64 hb = __ballot(head);
            if (hb == 0) continue;
            const u32 slot = distinct + (u32)__popcll(hb & lanemask_lt());
            if (head && slot < cap) {
                const int32_t doc = d.da[r];
                docs[slot] = doc;
                offs[slot] = (int32_t)(x.sa[r] - (u32)d.starts[doc]);
            }
            distinct += (u32)__popcll(hb);
        }
    }
    return distinct;
}

// One wave per span.
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_docs_kernel(View x, DocView d, DocsArgs g) {
    const u32 lane = threadIdx.x & (WAVE - 1);
    const u64 waves = (u64)gridDim.x * NEXT_WAVES;
    unsigned long long streamed = 0;
    for (u64 w = (u64)blockIdx.x * NEXT_WAVES + (threadIdx.x >> 6); w < g.Q; w += waves) {
        const Walk k = tq_walk_of(x, g.spans[w]);
        const u32 count = k.end - k.a;
        const u32 examined = (g.budget && g.budget < count) ? g.budget : count;
        const u32 distinct = tq_docs_walk(x, d, k.a, examined, g.cap, g.docs + w * g.cap, g.offsets + w * g.cap, lane);
        if (lane == 0) {
            sa_hip_token_docs h;
            h.written = distinct < g.cap ? distinct : g.cap;
            h.examined = examined;
            h.distinct = distinct;
            h.count = count;
            g.heads[w] = h;
        }
        streamed += examined;
    }
    if (lane == 0 && streamed) atomicAdd(g.examined, streamed);
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// what can be told from the table alone: D in range, starts[0] == 0, non-decreasing (hence no negative entry)
inline int docs_table_check(const char* who, const int32_t* starts, u32 D) {
    if (D > 0x7FFFFFFFu) return fail(SA_HIP_EINVAL, who, "more than 2^31 - 1 documents");
    if (starts[0] != 0) return fail(SA_HIP_EINVAL, who, "doc_starts[0] != 0");
    for (u32 d = 1; d < D; ++d) if (starts[d] < starts[d - 1]) return fail(SA_HIP_EINVAL, who, "doc_starts descend");
    return 0;
}

// The sort of the ranks by document, shared by Docs::build (PV) and DocRanks::build (token_all.hpp: RK).  Scratch: two u64 and two
// u32 arrays of n and a RadixWorkspace, the caller's to free.
inline int rank_sort_reserve(RadixWorkspace& ws, DevBuf& k0, DevBuf& k1, DevBuf& v0, DevBuf& v1, u32 n) {
    int rc;
    if ((rc = ws.init(n, 512)) || (rc = k0.ensure((size_t)n * 8)) || (rc = k1.ensure((size_t)n * 8)) ||
        (rc = v0.ensure((size_t)n * 4)) || (rc = v1.ensure((size_t)n * 4))) return rc;
    return 0;
}
// k0: the keys DA[r] widened, n >= 1 of them, D >= 2.  Stable, values = iota, key bits [0, bits_for(D)).  *kr / *vr: the buffers
// that hold the sorted keys and the ranks in document order; *passes: the radix passes it took.
inline int rank_sort(RadixWorkspace& ws, hipStream_t stream, DevBuf& k0, DevBuf& k1, DevBuf& v0, DevBuf& v1, u32 n, u32 D, u64** kr,
                     u32** vr, u32* passes) {
    const u64 before = ws.passes;
    const int rc = radix_sort_pairs(ws, stream, k0.as<u64>(), v0.as<u32>(), k1.as<u64>(), v1.as<u32>(), n, 0, bits_for(D), true, false,
                                    kr, vr);
    if (rc) return rc;
    *passes = (u32)(ws.passes - before);
    return 0;
}

struct Docs {
    DevBuf starts, da, pv, sum;     // sum: the counter of DocsArgs::examined
    hipEvent_t ev[4] = {};          // begin | DA written | ranks sorted | PV written
    u32 D = 0;                      // 0: the handle has no documents
    u64 bytes = 0;
    u32 passes = 0;
    float prepare_ms = 0.f, da_ms = 0.f, sort_ms = 0.f, pv_ms = 0.f;

    void clear() {
        starts.release(); da.release(); pv.release();
        D = 0; bytes = 0; passes = 0;
        prepare_ms = da_ms = sort_ms = pv_ms = 0.f;
    }
    void release() {
        clear();
        sum.release();
        for (int j = 0; j < 4; ++j) if (ev[j]) { (void)hipEventDestroy(ev[j]); ev[j] = nullptr; }
    }

    DocView view() const {
        DocView v{};
        v.starts = starts.as<int32_t>(); v.da = da.as<int32_t>(); v.pv = pv.as<int32_t>(); v.D = D;
        return v;
    }

    // table: D_ >= 1 checked entries, every one <= x.n.  Synchronous on `stream`; on an error the handle has no documents.
    int build(const Index& x, hipStream_t stream, const int32_t* table, u32 D_, const char* who) {
        SA_HIP_CHECK(hipStreamSynchronize(stream));      // launches that read the table being replaced
        clear();
        RadixWorkspace ws;
        DevBuf k0, k1, v0, v1;
        const int rc = build_on(x, stream, table, D_, who, ws, k0, k1, v0, v1);
        (void)hipStreamSynchronize(stream);
        ws.destroy();
        k0.release(); k1.release(); v0.release(); v1.release();
        if (rc) clear();
        return rc;
    }

  private:
    int build_on(const Index& x, hipStream_t stream, const int32_t* table, u32 D_, const char* who, RadixWorkspace& ws, DevBuf& k0,
                 DevBuf& k1, DevBuf& v0, DevBuf& v1) {
        int rc;
        const u32 n = x.n;
        for (int j = 0; j < 4; ++j) if (!ev[j]) SA_HIP_CHECK(hipEventCreate(&ev[j]));
        std::vector<int32_t> closed;
        try { closed.assign(table, table + D_); closed.push_back((int32_t)n); }
        catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, who, "host allocation"); }
        if ((rc = starts.ensure((size_t)(D_ + 1) * 4)) || (rc = da.ensure((size_t)n * 4 + 64)) || (rc = pv.ensure((size_t)n * 4 + 64)) ||
            (rc = sum.ensure(64))) return rc;
        SA_HIP_CHECK(hipMemcpyAsync(starts.p, closed.data(), (size_t)(D_ + 1) * 4, hipMemcpyHostToDevice, stream));
        SA_HIP_CHECK(hipStreamSynchronize(stream));      // (closed is a local)
        const bool sorted = D_ > 1 && n > 0;             // one document: PV[r] = r - 1, and iota with zero passes is refused
        if (sorted && (rc = rank_sort_reserve(ws, k0, k1, v0, v1, n))) return rc;
        SA_HIP_CHECK(hipEventRecord(ev[0], stream));
        u64* kr = nullptr; u32* vr = nullptr;
        if (n) {
            hipLaunchKernelGGL(td_da_kernel, dim3(stream_grid(n, 1024)), dim3(BLOCK), 0, stream, x.sa.as<u32>(), n,
                               (const int32_t*)starts.as<int32_t>(), D_, da.as<int32_t>(), sorted ? k0.as<u64>() : nullptr);
            SA_HIP_CHECK(hipGetLastError());
        }
        SA_HIP_CHECK(hipEventRecord(ev[1], stream));
        if (sorted && (rc = rank_sort(ws, stream, k0, k1, v0, v1, n, D_, &kr, &vr, &passes))) return rc;
        SA_HIP_CHECK(hipEventRecord(ev[2], stream));
        if (n) {
            hipLaunchKernelGGL(td_pv_kernel, dim3(stream_grid(n, 1024)), dim3(BLOCK), 0, stream, (const u64*)kr, (const u32*)vr, n,
                               pv.as<int32_t>());
            SA_HIP_CHECK(hipGetLastError());
        }
        SA_HIP_CHECK(hipEventRecord(ev[3], stream));
        DeviceStatus st{};
        if (sorted) SA_HIP_CHECK(hipMemcpyAsync(&st, ws.dstat, sizeof st, hipMemcpyDeviceToHost, stream));
        SA_HIP_CHECK(hipEventSynchronize(ev[3]));
        SA_HIP_CHECK(hipStreamSynchronize(stream));
        if (st.error) return fail(SA_HIP_EINTERNAL, who, "device look-back spin limit expired");
        if (sorted && (rc = ws.timer.flush())) return rc;
        SA_HIP_CHECK(hipEventElapsedTime(&da_ms, ev[0], ev[1]));
        SA_HIP_CHECK(hipEventElapsedTime(&sort_ms, ev[1], ev[2]));
        SA_HIP_CHECK(hipEventElapsedTime(&pv_ms, ev[2], ev[3]));
        SA_HIP_CHECK(hipEventElapsedTime(&prepare_ms, ev[0], ev[3]));
        D = D_;
        bytes = (u64)n * 8 + (u64)(D_ + 1) * 4;
        return 0;
    }
};

// Q >= 1 spans, cap >= 1, Q * cap < 2^31; every pointer on the device; asynchronous on `stream`
inline int launch_locate(const Index& x, const Docs& d, hipStream_t stream, const LocateArgs& g) {
    const u64 cells = g.Q * g.cap;
    hipLaunchKernelGGL(tq_locate_kernel, dim3((u32)((cells + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, x.view(), d.view(), g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// Q >= 1 spans, Q * cap < 2^31 (cap may be 0); g.examined is zeroed on the stream first
inline int launch_docs(const Index& x, const Docs& d, hipStream_t stream, const DocsArgs& g) {
    SA_HIP_CHECK(hipMemsetAsync(g.examined, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(tq_docs_kernel, dim3(wave_row_grid(g.Q)), dim3(NEXT_WAVES * WAVE), 0, stream, x.view(), d.view(), g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
