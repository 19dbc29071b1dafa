// token_query.hpp -- batched n-gram search over the suffix array of an int32 token text (sa_hip_token_index_*).
//
// What is searched: T (int32[n], symbols in [0, 2^31 - 1]) and SA (int32[n], what sa_hip_libsais_int[_device] produces), n <=
// 2^31 - 1.  A pattern is a sequence of int32 symbols (any value); the answer is {first, count}: first = number of suffixes
// that sort before the pattern (a suffix that ends sorts before one that continues), count = number of suffixes that have the
// pattern as a prefix; they are SA[first .. first + count).
//
// Search structures, prepared once per handle (Index::prepare):
//   dir   first-symbol directory, when max - min + 1 <= 2^24: dir[v - min] = number of suffixes whose first symbol is < v, u32,
//         max - min + 2 entries -- a histogram of the text and its exclusive scan (scan.hpp).  A length-1 pattern is answered
//         from it alone; every longer one starts its search in [dir[v - min], dir[v - min + 1]).
//   K     key array: K[r] = ((T[p] + 1) << 32) | (p + 1 < n ? T[p + 1] + 1 : 0), p = SA[r], u64, 8 n bytes, one gather pass.
//         T[p] + 1 reaches 2^31: both fields are unsigned.  K is non-decreasing in r, so a bound over the first two symbols
//         costs ONE dependent random read per step (K[m]) instead of two (SA[m], then T[SA[m]]) -- a batch of searches is
//         bound by dependent random reads.
//   last  the rank of suffix n - 1.  Its key has a low field of 0, which is no symbol: it is the one suffix that starts with
//         c = T[n - 1] and sorts before [c, x] for EVERY int32 x, negative ones included.  A pattern [c, x < 0, ...] cannot be
//         written as a key; it is answered as "start of c's suffixes, plus one when the last suffix is the first of them".
// Bytes per symbol: 4 (T) + 4 (SA) + 8 (K) + the directory (4 per value of [min, max + 1]).
//
// Search (tq_search_kernel): one lane per pattern, 256-thread workgroups.  The lower and the upper bound are searched in
// one loop whose two loads are issued together.  Every loop is bounded whatever the arrays hold: a binary search halves an
// index range (at most 32 steps, n < 2^31), a comparison reads at most min(pattern length, n) symbols.  SA entries are
// range-checked once (tq_sa_check_kernel), so T[SA[m] + j] with the j < n - SA[m] test never leaves the text.
//
// Longest-suffix spans and the next symbols of a range (with their counts) are token_next.hpp, on top of tq_range below.
//
// Out of scope here: int64 texts and libsais64_long arrays, byte arrays with 64-bit indices, multi-GPU sharding of token
// queries, and anything in bench.py.
#pragma once
#include "int_build.hpp"
#include "scan.hpp"

namespace sa {
namespace tq {

constexpr u64 DIR_CAP = 1ull << 24;   // directory over [min, max] up to this many values
constexpr int BLOCK = 256;
constexpr int STEPS = 32;             // bound of every binary search (n < 2^31: 31 halvings reach an empty range)

struct Check {                        // device, one per handle
    unsigned long long bad;           // SA entries outside [0, n)
    unsigned long long last_rank;     // r with SA[r] == n - 1
};

// every SA entry in [0, n) (a negative entry is >= n as u32), and where suffix n - 1 stands
__global__ __launch_bounds__(BLOCK) void tq_sa_check_kernel(const u32* __restrict__ sa, u32 n, Check* __restrict__ c) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u64 local = 0;
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        const u32 p = sa[j];
        local += p >= n ? 1u : 0u;
        if (p == n - 1) c->last_rank = j;
    }
    if (local) atomicAdd(&c->bad, (unsigned long long)local);
}

// hist[T[i] - min] += 1 (symbols known to lie in [min, max]; bins = max - min + 1).  The first HIST_LDS bins are counted in LDS
// and added to the global table once per workgroup: token ids are Zipf-like, and with global atomics alone the few most
// frequent symbols serialise the pass on their addresses (1e8 Zipf tokens: 105 ms of a 108 ms prepare).
constexpr u32 HIST_LDS = 12288;
__global__ __launch_bounds__(BLOCK) void tq_hist_kernel(const int32_t* __restrict__ T, u32 n, int32_t mn, u32 bins, u32* __restrict__ hist) {
    __shared__ u32 s_h[HIST_LDS];
    const u32 cap = bins < HIST_LDS ? bins : HIST_LDS;
    for (u32 i = threadIdx.x; i < cap; i += BLOCK) s_h[i] = 0;
    __syncthreads();
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u32 b = (u32)(T[i] - mn);
        if (b < cap) atomicAdd(&s_h[b], 1u); else atomicAdd(&hist[b], 1u);
    }
    sync_lds();
    for (u32 i = threadIdx.x; i < cap; i += BLOCK) {
        const u32 c = s_h[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// exclusive scan u32 -> u32 in place, the third step after big::bg_scan_reduce_kernel / bg_scan_parts_kernel (the same tiles)
__global__ __launch_bounds__(big::SC_BLOCK) void tq_scan_apply_kernel(u32* __restrict__ io, u64 len, const u64* __restrict__ part) {
    __shared__ u64 s_w[big::SC_WAVES];
    const u64 base = (u64)blockIdx.x * big::SC_TILE + (u64)threadIdx.x * big::SC_ITEMS;
    u32 v[big::SC_ITEMS];
    u64 s = 0;
#pragma unroll
    for (u32 e = 0; e < big::SC_ITEMS; ++e) { v[e] = (base + e < len) ? io[base + e] : 0u; s += v[e]; }
    u64 run = block_scan_excl<big::SC_WAVES>(s, (u64)0, ScanSum{}, s_w) + part[blockIdx.x];
#pragma unroll
    for (u32 e = 0; e < big::SC_ITEMS; ++e) { if (base + e < len) io[base + e] = (u32)run; run += v[e]; }
}

__global__ __launch_bounds__(BLOCK) void tq_keys_kernel(const int32_t* __restrict__ T, const u32* __restrict__ sa, u32 n, u64* __restrict__ K) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const u32 p = sa[r];
        const u64 hi = (u64)(u32)T[p] + 1;
        const u64 lo = p + 1 < n ? (u64)(u32)T[p + 1] + 1 : 0;
        K[r] = (hi << 32) | lo;
    }
}

struct View {                 // what the search kernel reads
    const int32_t* T;
    const u32* sa;
    const u64* K;             // nullptr: no key array
    const u32* dir;           // nullptr: no directory
    u32 n;
    u32 last_rank;
    int32_t mn, mx;
};

// suffix p against P[j0 .. m), its first j0 symbols known to be equal: -1 the suffix sorts before the pattern (a smaller symbol,
// or it ends first), +1 after, 0 the pattern is a prefix of it.  At most min(m, n - p) - j0 steps.
__device__ __forceinline__ int tq_compare(const int32_t* __restrict__ T, u32 n, u32 p, const int32_t* __restrict__ P, u64 m, u64 j0) {
    const u64 avail = (u64)(n - p);
    const u64 len = m < avail ? m : avail;
    for (u64 j = j0; j < len; ++j) {
        const int32_t a = T[p + j], b = P[j];
        if (a != b) return a < b ? -1 : 1;
    }
    return m > avail ? -1 : 0;
}

// [*lo, *hi) <- the ranks of [lo, hi) whose key is in [a, b): both bounds in one loop, their two loads issued together
__device__ __forceinline__ void tq_key_bounds(const u64* __restrict__ K, u64 a, u64 b, u32* lo, u32* hi) {
    u32 lo1 = *lo, hi1 = *hi, lo2 = *lo, hi2 = *hi;
    for (int s = 0; s < STEPS && (lo1 < hi1 || lo2 < hi2); ++s) {
        const u32 m1 = (lo1 + hi1) >> 1, m2 = (lo2 + hi2) >> 1;
        const u64 k1 = lo1 < hi1 ? K[m1] : 0, k2 = lo2 < hi2 ? K[m2] : 0;
        if (lo1 < hi1) { if (k1 < a) lo1 = m1 + 1; else hi1 = m1; }
        if (lo2 < hi2) { if (k2 < b) lo2 = m2 + 1; else hi2 = m2; }
    }
    *lo = lo1;
    *hi = lo2 < lo1 ? lo1 : lo2;   // an array that is not sorted cannot turn the range inside out
}

// the same by text comparison from symbol j0 on: [*lo, *hi) <- the ranks of [lo, hi) whose suffix has P as a prefix
__device__ __forceinline__ void tq_text_bounds(const View& x, const int32_t* __restrict__ P, u64 m, u64 j0, u32* lo, u32* hi) {
    u32 lo1 = *lo, hi1 = *hi, lo2 = *lo, hi2 = *hi;
    for (int s = 0; s < STEPS && (lo1 < hi1 || lo2 < hi2); ++s) {
        const u32 m1 = (lo1 + hi1) >> 1, m2 = (lo2 + hi2) >> 1;
        const bool live1 = lo1 < hi1, live2 = lo2 < hi2;
        const u32 p1 = live1 ? x.sa[m1] : 0, p2 = live2 ? x.sa[m2] : 0;
        int c1 = 0;
        if (live1) { c1 = tq_compare(x.T, x.n, p1, P, m, j0); if (c1 < 0) lo1 = m1 + 1; else hi1 = m1; }
        if (live2) {
            const int c2 = (live1 && m2 == m1) ? c1 : tq_compare(x.T, x.n, p2, P, m, j0);   // while both searches walk together
            if (c2 <= 0) lo2 = m2 + 1; else hi2 = m2;
        }
    }
    *lo = lo1;
    *hi = lo2 < lo1 ? lo1 : lo2;
}

// {first, count} of the pattern P[0 .. m): what one lane of tq_search_kernel computes (token_next.hpp probes with it as well)
__device__ __forceinline__ sa_hip_pair_u32 tq_range(const View& x, const int32_t* __restrict__ P, u64 m) {
    sa_hip_pair_u32 res{0u, 0u};
    if (m == 0) { res.second = x.n; return res; }
    if (x.n == 0) return res;
    const int32_t v = P[0];
    if (v < x.mn) return res;                                    // below every suffix (a negative symbol among them)
    if (v > x.mx) { res.first = x.n; return res; }               // above every suffix
    u32 lo = 0, hi = x.n;
    if (x.dir) {
        lo = x.dir[(u32)(v - x.mn)];
        hi = x.dir[(u32)(v - x.mn) + 1];
        if (hi < lo) hi = lo;
        if (hi > x.n) hi = x.n;   // (a directory of this handle spans [0, n]; a bound for the loads all the same)
        if (lo > hi) lo = hi;
        if (m == 1 || lo == hi) { res.first = lo; res.second = hi - lo; return res; }
    }
    if (x.K) {
        const int32_t w = m >= 2 ? P[1] : 0;
        const bool first_only = m == 1 || w < 0;   // the key holds no negative symbol: only the first symbol goes through it
        if (!(first_only && x.dir)) {
            const u64 a = first_only ? ((u64)(u32)v + 1) << 32 : ((((u64)(u32)v + 1) << 32) | ((u64)(u32)w + 1));
            const u64 b = first_only ? ((u64)(u32)v + 2) << 32 : a + 1;
            tq_key_bounds(x.K, a, b, &lo, &hi);
        }
        if (m >= 2 && w < 0) {
            // [v, negative, ...]: after the suffix that ends behind v (the first of v's suffixes when v = T[n - 1]), before every other
            res.first = lo + ((lo < hi && x.last_rank == lo) ? 1u : 0u);
            return res;
        }
        if (m > 2 && lo < hi) tq_text_bounds(x, P, m, 2, &lo, &hi);
    } else {
        tq_text_bounds(x, P, m, x.dir ? 1 : 0, &lo, &hi);
    }
    res.first = lo;
    res.second = hi - lo;
    return res;
}

__global__ __launch_bounds__(BLOCK) void tq_search_kernel(View x, const int32_t* __restrict__ pat, const u64* __restrict__ off, u64 Q,
                                                          sa_hip_pair_u32* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= Q) return;
    const u64 o0 = off[i], o1 = off[i + 1];
    out[i] = tq_range(x, pat + o0, o1 > o0 ? o1 - o0 : 0);
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// test switches (diag_env: only with SA_HIP_DIAG=1), read when the handle is created
struct Knobs {
    bool keys = true;        // SA_HIP_TOKEN_KEYS=0: no key array, bounds by text comparison alone
    bool dir = true;         // SA_HIP_TOKEN_DIR=0: no directory
    static Knobs read() {
        Knobs k;
        if (const char* e = diag_env("SA_HIP_TOKEN_KEYS")) k.keys = atoi(e) != 0;
        if (const char* e = diag_env("SA_HIP_TOKEN_DIR")) k.dir = atoi(e) != 0;
        return k;
    }
};

struct Index {
    DevBuf text, sa, keys, dir, part, small;
    hipEvent_t ev[2] = {};
    Knobs knobs;
    u32 n = 0;
    int32_t mn = 0, mx = 0;
    u64 dir_entries = 0;
    u32 key_bytes = 0;
    u32 last_rank = 0;
    float prepare_ms = 0.f;

    void release() {
        text.release(); sa.release(); keys.release(); dir.release(); part.release(); small.release();
        for (int j = 0; j < 2; ++j) if (ev[j]) { (void)hipEventDestroy(ev[j]); ev[j] = nullptr; }
    }

    int reserve(u32 n_) {
        int rc;
        n = n_;
        for (int j = 0; j < 2; ++j) if (!ev[j]) SA_HIP_CHECK(hipEventCreate(&ev[j]));
        if ((rc = text.ensure((size_t)n * 4 + 64)) || (rc = sa.ensure((size_t)n * 4 + 64)) || (rc = small.ensure(256))) return rc;
        return 0;
    }

    // text and sa hold n entries each: alphabet, range check, directory, keys.  Synchronous on `stream`.
    int prepare(hipStream_t stream, const char* who) {
        int rc;
        mn = mx = 0; dir_entries = 0; key_bytes = 0; last_rank = 0; prepare_ms = 0.f;
        if (n == 0) return 0;
        const int32_t* T = text.as<int32_t>();
        const u32* S = sa.as<u32>();
        ints::Range* r = small.as<ints::Range>();
        Check* c = reinterpret_cast<Check*>(small.as<u8>() + 64);
        const ints::Range rinit{~0ull, 0ull, ~0ull, 0ull};
        const Check cinit{0ull, 0ull};
        SA_HIP_CHECK(hipEventRecord(ev[0], stream));
        SA_HIP_CHECK(hipMemcpyAsync(r, &rinit, sizeof rinit, hipMemcpyHostToDevice, stream));
        SA_HIP_CHECK(hipMemcpyAsync(c, &cinit, sizeof cinit, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL((ints::int_range_kernel<int32_t>), dim3(stream_grid(n, 256 * 16)), dim3(256), 0, stream, T, (u64)n, r);
        hipLaunchKernelGGL(tq_sa_check_kernel, dim3(stream_grid(n, 1024)), dim3(BLOCK), 0, stream, S, n, c);
        SA_HIP_CHECK(hipGetLastError());
        ints::Range rh{};
        Check ch{};
        SA_HIP_CHECK(hipMemcpyAsync(&rh, r, sizeof rh, hipMemcpyDeviceToHost, stream));
        SA_HIP_CHECK(hipMemcpyAsync(&ch, c, sizeof ch, hipMemcpyDeviceToHost, stream));
        SA_HIP_CHECK(hipStreamSynchronize(stream));
        const int64_t lo = (int64_t)(rh.lo ^ (1ull << 63)), hi = (int64_t)(rh.hi ^ (1ull << 63));
        if (lo < 0) {
            char b[96];
            snprintf(b, sizeof b, "smallest symbol %lld", (long long)lo);
            return fail(SA_HIP_EINVAL, who, (std::string("negative text symbol: ") + b).c_str());
        }
        if (ch.bad) return fail(SA_HIP_EINVAL, who, "suffix array holds entries outside [0, n)");
        mn = (int32_t)lo; mx = (int32_t)hi;
        last_rank = (u32)ch.last_rank;
        const u64 range = (u64)(hi - lo) + 1;
        if (knobs.dir && range <= DIR_CAP) {
            const u64 len = range + 1;
            const u64 nparts = (len + big::SC_TILE - 1) / big::SC_TILE;
            if ((rc = dir.ensure(len * 4 + 64)) || (rc = part.ensure((nparts + 1) * 8 + 64))) return rc;
            SA_HIP_CHECK(hipMemsetAsync(dir.p, 0, len * 4, stream));
            hipLaunchKernelGGL(tq_hist_kernel, dim3(stream_grid(n, 256 * 64)), dim3(BLOCK), 0, stream, T, n, mn, (u32)range, dir.as<u32>());
            hipLaunchKernelGGL(big::bg_scan_reduce_kernel, dim3((u32)nparts), dim3(big::SC_BLOCK), 0, stream, (const u32*)dir.as<u32>(), len, part.as<u64>());
            hipLaunchKernelGGL(big::bg_scan_parts_kernel, dim3(1), dim3(big::SC_BLOCK), 0, stream, part.as<u64>(), nparts);
            hipLaunchKernelGGL(tq_scan_apply_kernel, dim3((u32)nparts), dim3(big::SC_BLOCK), 0, stream, dir.as<u32>(), len, (const u64*)part.as<u64>());
            SA_HIP_CHECK(hipGetLastError());
            dir_entries = len;
        } else {
            dir.release(); part.release();
        }
        if (knobs.keys) {
            if ((rc = keys.ensure((size_t)n * 8 + 64))) return rc;
            hipLaunchKernelGGL(tq_keys_kernel, dim3(stream_grid(n, 1024)), dim3(BLOCK), 0, stream, T, S, n, keys.as<u64>());
            SA_HIP_CHECK(hipGetLastError());
            key_bytes = 8;
        } else {
            keys.release();
        }
        SA_HIP_CHECK(hipEventRecord(ev[1], stream));
        SA_HIP_CHECK(hipEventSynchronize(ev[1]));
        SA_HIP_CHECK(hipEventElapsedTime(&prepare_ms, ev[0], ev[1]));
        return 0;
    }

    View view() const {
        View v{};
        v.T = text.as<int32_t>();
        v.sa = sa.as<u32>();
        v.K = key_bytes ? keys.as<u64>() : nullptr;
        v.dir = dir_entries ? dir.as<u32>() : nullptr;
        v.n = n; v.last_rank = last_rank; v.mn = mn; v.mx = mx;
        return v;
    }

    // Q >= 1 patterns, every pointer on the device; asynchronous on `stream`
    int search(hipStream_t stream, const int32_t* pat, const u64* off, u64 Q, sa_hip_pair_u32* out) const {
        const u64 grid = (Q + BLOCK - 1) / BLOCK;
        if (grid > 0x7FFFFFFFull) return fail(SA_HIP_EINVAL, "sa_hip_token_index_query_batch", "too many patterns for one launch");
        hipLaunchKernelGGL(tq_search_kernel, dim3((u32)grid), dim3(BLOCK), 0, stream, view(), pat, off, Q, out);
        SA_HIP_CHECK(hipGetLastError());
        return 0;
    }
};

}  // namespace tq
}  // namespace sa
