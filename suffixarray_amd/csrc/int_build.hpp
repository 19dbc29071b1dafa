// int_build.hpp -- suffix arrays of integer texts (sa_hip_libsais_int, sa_hip_libsais64_long and their device forms).
//
// libsais_int / libsais64_long (libsais.h:96, libsais64.h:73) take a text of int32 / int64 symbols in [0, k).  Here:
//   1. alphabet pass: one streaming read of T -- min and max by wave reductions, one atomic per workgroup.  A symbol outside
//      [0, k) is an error (the reference's behaviour is undefined there).  When max + 1 <= DENSE_CAP a presence table over
//      [0, max] and its exclusive scan give dense codes (code = 1 + rank; 0 = past the end) and sigma; above the cap the codes
//      are the raw v + 1 (sigma not counted).
//   2. route A (sigma <= 256, n <= 2^32 - 2): rank(v) as one byte per symbol into the text buffer of a device index, then the
//      product's own byte build -- its alphabet compaction is order-preserving, so the suffix array is the integer text's.
//   3. route B (everything else): s = floor(64 / b) codes of b bits per suffix, MSB first, as the initial key, then the sort,
//      flags and prefix doubling of big_build.hpp unchanged (BigBuilder::build_with), doubling from h = s.  The int32 form
//      narrows the 64-bit result.
// Memory of route B: 8 n (64-bit SA) + 32 n (BigBuilder during the initial sort) + the text (4 n or 8 n) + the int32 result of
// the int32 device form (the drop-in narrows into its text buffer) -- 44 to 48 n bytes.
#pragma once
#include "big_build.hpp"

namespace sa {
namespace ints {

constexpr u64 DENSE_CAP = 1ull << 24;   // presence table / rank table over [0, max] up to this many values
constexpr u32 KG_TILE = 2048;           // keygen: positions per workgroup (256 threads)
constexpr u32 KG_HALO = 64;             // codes past the tile a key may cover (s <= 64)

// biased order: (v ^ sign bit) as u64 orders like the signed value
template <class S>
__device__ __forceinline__ u64 biased(S v) { return (u64)(int64_t)v ^ (1ull << 63); }

struct Range {                          // device, one per call
    unsigned long long lo, hi;          // biased min / max
    unsigned long long bad_pos;         // first position with a symbol outside [0, k) (~0: none); filled on the error path only
    unsigned long long pad;
};

template <class S>
__global__ __launch_bounds__(256) void int_range_kernel(const S* __restrict__ T, u64 n, Range* __restrict__ r) {
    __shared__ u64 s_lo[256 / WAVE], s_hi[256 / WAVE];
    u64 lo = ~0ull, hi = 0;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 b = biased(T[i]);
        lo = b < lo ? b : lo;
        hi = b > hi ? b : hi;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 a = __shfl_xor(lo, o), c = __shfl_xor(hi, o);
        lo = a < lo ? a : lo;
        hi = c > hi ? c : hi;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 256 / WAVE; ++w) { lo = s_lo[w] < lo ? s_lo[w] : lo; hi = s_hi[w] > hi ? s_hi[w] : hi; }
        atomicMin(&r->lo, (unsigned long long)lo);
        atomicMax(&r->hi, (unsigned long long)hi);
    }
}

// error path only: the first position whose symbol lies outside [0, k)
template <class S>
__global__ __launch_bounds__(256) void int_first_bad_kernel(const S* __restrict__ T, u64 n, int64_t k, Range* __restrict__ r) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t v = (int64_t)T[i];
        if (v < 0 || v >= k) { atomicMin(&r->bad_pos, (unsigned long long)i); break; }
    }
}

// presence over [0, max] (symbols checked in range; a plain store of the same value from every lane that sees it)
template <class S>
__global__ __launch_bounds__(256) void int_presence_kernel(const S* __restrict__ T, u64 n, u32* __restrict__ pres) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) pres[(u64)T[i]] = 1u;
}

// route A: rank(v) as a byte (sigma <= 256)
template <class S>
__global__ __launch_bounds__(256) void int_bytes_kernel(const S* __restrict__ T, u64 n, const u64* __restrict__ rank, u8* __restrict__ out) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (u8)rank[(u64)T[i]];
}

// route B: key[p] = codes of T[p .. p + s) MSB first, b bits each, 0 past the end; the tile's codes (and s - 1 past it) are
// staged in LDS with coalesced reads, every key is then assembled from LDS and written coalesced.  b * s <= 64.
template <class S, bool DENSE>
__global__ __launch_bounds__(256) void int_keygen_kernel(const S* __restrict__ T, u64 n, const u64* __restrict__ rank, int b, int s,
                                                         u64* __restrict__ keys, u64* __restrict__ idx) {
    __shared__ u64 s_c[KG_TILE + KG_HALO];
    const u64 base = (u64)blockIdx.x * KG_TILE;
    const u32 span = KG_TILE + (u32)s - 1;
    for (u32 j = threadIdx.x; j < span; j += 256) {
        const u64 x = base + j;
        u64 c = 0;
        if (x < n) c = DENSE ? rank[(u64)T[x]] + 1 : (u64)T[x] + 1;
        s_c[j] = c;
    }
    __syncthreads();
    for (u32 j = threadIdx.x; j < KG_TILE; j += 256) {
        const u64 p = base + j;
        if (p >= n) break;
        u64 key = s_c[j];
        for (int c = 1; c < s; ++c) key = (key << b) | s_c[j + c];   // (s >= 2: b <= 32)
        keys[p] = key;
        idx[p] = p;
    }
}

__global__ __launch_bounds__(256) void int_narrow_kernel(const u64* __restrict__ sa, u64 n, int32_t* __restrict__ out) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (int32_t)sa[i];
}

__global__ __launch_bounds__(256) void int_widen_kernel(const u32* __restrict__ sa, u64 n, int64_t* __restrict__ out) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (int64_t)sa[i];
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// diagnostic switches (diag_env: only with SA_HIP_DIAG=1), read per call
struct Knobs {
    bool bytes = true;       // SA_HIP_INT_BYTES=0: never route A
    bool compact = true;     // SA_HIP_INT_COMPACT=0: raw v + 1 codes
    int key_symbols = 64;    // SA_HIP_INT_KEY_SYMBOLS=s: at most s symbols per initial key
    static Knobs read() {
        Knobs k;
        if (const char* e = diag_env("SA_HIP_INT_BYTES")) k.bytes = atoi(e) != 0;
        if (const char* e = diag_env("SA_HIP_INT_COMPACT")) k.compact = atoi(e) != 0;
        if (const char* e = diag_env("SA_HIP_INT_KEY_SYMBOLS")) { const int v = atoi(e); if (v >= 1 && v <= 64) k.key_symbols = v; }
        return k;
    }
};

struct Alphabet {
    int64_t min = 0, max = 0;
    u32 sigma = 0;           // distinct symbols (0: not counted)
    bool dense = false;      // rank table built: code = 1 + rank
    int bits = 0;            // code width of route B
    int s = 0;               // symbols per initial key of route B
};

struct Workspace {
    DevBuf range, pres, rank, part, sa64;
    hipEvent_t ev[2] = {};
    big::BigBuilder big;
    void release() {
        range.release(); pres.release(); rank.release(); part.release(); sa64.release();
        big.destroy();
        for (int j = 0; j < 2; ++j) if (ev[j]) { (void)hipEventDestroy(ev[j]); ev[j] = nullptr; }
    }
};

// The alphabet pass over T[0..n) (n >= 2) on `stream`, synchronous.  Returns SA_HIP_EINVAL naming the first symbol outside
// [0, k).  *ms = its device time.
template <class S>
int alphabet(Workspace& ws, hipStream_t stream, const S* T, u64 n, int64_t k, const Knobs& kn, Alphabet* a, float* ms) {
    int rc;
    for (int j = 0; j < 2; ++j) if (!ws.ev[j]) SA_HIP_CHECK(hipEventCreate(&ws.ev[j]));
    if ((rc = ws.range.ensure(sizeof(Range) + 64))) return rc;
    Range* r = ws.range.as<Range>();
    const Range init{~0ull, 0ull, ~0ull, 0ull};
    SA_HIP_CHECK(hipEventRecord(ws.ev[0], stream));
    SA_HIP_CHECK(hipMemcpyAsync(r, &init, sizeof init, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL((int_range_kernel<S>), dim3(stream_grid(n, 256 * 16)), dim3(256), 0, stream, T, n, r);
    SA_HIP_CHECK(hipGetLastError());
    Range h{};
    SA_HIP_CHECK(hipMemcpyAsync(&h, r, sizeof h, hipMemcpyDeviceToHost, stream));
    SA_HIP_CHECK(hipStreamSynchronize(stream));
    a->min = (int64_t)(h.lo ^ (1ull << 63));
    a->max = (int64_t)(h.hi ^ (1ull << 63));
    if (a->min < 0 || a->max >= k) {
        hipLaunchKernelGGL((int_first_bad_kernel<S>), dim3(stream_grid(n, 256 * 16)), dim3(256), 0, stream, T, n, k, r);
        SA_HIP_CHECK(hipGetLastError());
        SA_HIP_CHECK(hipMemcpyAsync(&h, r, sizeof h, hipMemcpyDeviceToHost, stream));
        SA_HIP_CHECK(hipStreamSynchronize(stream));
        S v = 0;
        if (h.bad_pos < n) SA_HIP_CHECK(hipMemcpy(&v, T + h.bad_pos, sizeof v, hipMemcpyDeviceToHost));
        char b[160];
        snprintf(b, sizeof b, "T[%llu] = %lld, k = %lld", (unsigned long long)h.bad_pos, (long long)v, (long long)k);
        return fail(SA_HIP_EINVAL, "symbol outside [0, k)", b);
    }
    const u64 range = (u64)a->max + 1;
    a->dense = kn.compact && range <= DENSE_CAP;
    a->sigma = 0;
    if (a->dense) {
        const u64 nparts = (range + big::SC_TILE - 1) / big::SC_TILE;
        if ((rc = ws.pres.ensure(range * 4 + 64)) || (rc = ws.rank.ensure(range * 8 + 64)) || (rc = ws.part.ensure((nparts + 1) * 8 + 64))) return rc;
        SA_HIP_CHECK(hipMemsetAsync(ws.pres.p, 0, range * 4, stream));
        hipLaunchKernelGGL((int_presence_kernel<S>), dim3(stream_grid(n, 256 * 16)), dim3(256), 0, stream, T, n, ws.pres.as<u32>());
        hipLaunchKernelGGL(big::bg_scan_reduce_kernel, dim3((u32)nparts), dim3(big::SC_BLOCK), 0, stream, (const u32*)ws.pres.as<u32>(), range,
                           ws.part.as<u64>());
        hipLaunchKernelGGL(big::bg_scan_parts_kernel, dim3(1), dim3(big::SC_BLOCK), 0, stream, ws.part.as<u64>(), nparts);
        hipLaunchKernelGGL(big::bg_scan_apply_kernel, dim3((u32)nparts), dim3(big::SC_BLOCK), 0, stream, (const u32*)ws.pres.as<u32>(), range,
                           (const u64*)ws.part.as<u64>(), ws.rank.as<u64>());
        SA_HIP_CHECK(hipGetLastError());
        u64 sigma = 0;
        SA_HIP_CHECK(hipMemcpyAsync(&sigma, ws.part.as<u64>() + nparts, 8, hipMemcpyDeviceToHost, stream));
        SA_HIP_CHECK(hipStreamSynchronize(stream));
        a->sigma = (u32)sigma;
        a->bits = bits_for(sigma + 1);
    } else {
        a->bits = bits_for(range + 1);   // codes 0 .. max + 1
    }
    if (a->bits < 1) a->bits = 1;
    int s = 64 / a->bits;
    if (s > kn.key_symbols) s = kn.key_symbols;
    if ((u64)s > n) s = (int)n;
    if (s < 1) s = 1;
    a->s = s;
    SA_HIP_CHECK(hipEventRecord(ws.ev[1], stream));
    SA_HIP_CHECK(hipEventSynchronize(ws.ev[1]));
    SA_HIP_CHECK(hipEventElapsedTime(ms, ws.ev[0], ws.ev[1]));
    return 0;
}

inline bool route_bytes(const Alphabet& a, u64 n, const Knobs& kn) {
    return kn.bytes && a.dense && a.sigma <= 256 && n <= 0xFFFFFFFEull;
}

// route A's map: T -> rank bytes in `out` (n bytes) on `stream`
template <class S>
int map_bytes(Workspace& ws, hipStream_t stream, const S* T, u64 n, u8* out) {
    hipLaunchKernelGGL((int_bytes_kernel<S>), dim3(stream_grid(n, 256 * 4)), dim3(256), 0, stream, T, n, (const u64*)ws.rank.as<u64>(), out);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// route B: the 64-bit suffix array of T into sa_out (n entries) on `stream` (ws.big.stream is set to it)
template <class S>
int build_keys(Workspace& ws, hipStream_t stream, const S* T, u64 n, const Alphabet& a, u64* sa_out) {
    ws.big.stream = stream;
    const u64* rank = ws.rank.as<u64>();
    return ws.big.build_with(n, sa_out, [&](u64* keys, u64* idx, int* key_bits, u64* h0) -> int {
        ws.big.stats.sigma = a.sigma; ws.big.stats.bits_per_symbol = (u32)a.bits; ws.big.stats.initial_chars = (u32)a.s;
        const dim3 grid((u32)((n + KG_TILE - 1) / KG_TILE));
        if (a.dense) hipLaunchKernelGGL((int_keygen_kernel<S, true>), grid, dim3(256), 0, stream, T, n, rank, a.bits, a.s, keys, idx);
        else hipLaunchKernelGGL((int_keygen_kernel<S, false>), grid, dim3(256), 0, stream, T, n, rank, a.bits, a.s, keys, idx);
        SA_HIP_CHECK(hipGetLastError());
        *key_bits = a.bits * a.s;
        *h0 = (u64)a.s;
        return 0;
    });
}

inline int narrow(hipStream_t stream, const u64* sa, u64 n, int32_t* out) {
    hipLaunchKernelGGL(int_narrow_kernel, dim3(stream_grid(n, 1024)), dim3(256), 0, stream, sa, n, out);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

inline int widen(hipStream_t stream, const u32* sa, u64 n, int64_t* out) {
    hipLaunchKernelGGL(int_widen_kernel, dim3(stream_grid(n, 1024)), dim3(256), 0, stream, sa, n, out);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ints
}  // namespace sa
