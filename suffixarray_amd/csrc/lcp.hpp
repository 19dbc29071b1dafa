// lcp.hpp -- PLCP / LCP arrays on the device (sa_hip_libsais[64]_plcp / _lcp, sa_hip_index_[p]lcp_device,
// sa_hip_[p]lcp64_device).  Irreducible-LCP formulation (Kärkkäinen, Manzini, Puglisi, CPM 2009), fully parallel:
//
//   Phi[SA[r]] = SA[r-1] (SA[0] has no predecessor).  PLCP[i] is REDUCIBLE when i > 0, Phi[i] > 0 and
//   T[i-1] == T[Phi[i]-1]; then PLCP[i] = PLCP[i-1] - 1.  Only the irreducible positions are compared against the
//   text (their PLCP values sum to O(n log n)).  PLCP[i] + i never decreases, so W[i] = i + PLCP[i] at irreducible
//   positions, 0 elsewhere, and an inclusive max-scan over W in text order gives PLCP[i] = scan[i] - i everywhere.
//   LCP[r] = PLCP[SA[r]] is a gather.  End of text as in libsais (libsais.c:7721-7744): a comparison of i and k stops
//   at n - max(i, k).
//
// Phases (every launch on the caller's stream; no host synchronisation inside):
//   phi    one thread per rank r: range check of SA[r] and SA[r-1], reducibility test, up to lane_bytes compared with
//          8-byte loads; longer pairs are queued (rank only: i and k are re-read from SA)
//   wave   one wave per queued pair, 1 KB per step (16 bytes per lane), up to wave_bytes; longer pairs are queued again
//   split  every pair still open is cut into 4 KB chunks over all workgroups; the first mismatch is taken by a vector
//          atomicMin on W[i] itself (W[i] = all ones while open).  Segment lengths double from round to round, so a
//          pair of PLCP p costs O(p) bytes and O(log p) rounds; rounds without open pairs return at once
//   scan   tile maxima, one-workgroup exclusive scan of them, per-tile scan + subtraction (in place or into out)
//   gather LCP[r] = PLCP[SA[r]]
//
// Key shortcut (index handles): the index keeps the first k0 characters of every suffix as packed keys in SA order
// (sa_build.hpp: qkeys / qkeys32, q_b bits per code, code 0 = past the end).  Adjacent keys that differ in their first
// k0 codes give PLCP[SA[r]] exactly; equal ones ("tied") mean PLCP >= k0, and their comparison starts at depth k0.  A
// reducible position with PLCP >= k0 has a predecessor with PLCP >= k0, so the reducibility chains of tied positions
// stay among tied positions: for the LCP output only the tied ranks are scattered, scanned values are used only at
// tied positions, and only tied ranks are gathered (the others are written by the phi kernel straight from the keys).
// For the PLCP output every untied position gets W[i] = i + (key LCP) directly (a true value, so the scan stays exact).
//
// Every SA entry is range-checked by the thread that uses it: an entry >= n sets Counters::error and is skipped, so no
// scatter or gather ever leaves [0, n).  With an in-range array that is not a suffix array the output is unspecified,
// but every loop is bounded by n - max(i, k) and by the fixed number of split rounds.
#pragma once
#include "common.hpp"
#include "sa_build.hpp"

namespace sa {
namespace lcp {

constexpr u32 BLOCK = 256;
constexpr u32 SCAN_ITEMS = 16;                        // per thread in the scan kernels
constexpr u32 SCAN_TILE = BLOCK * SCAN_ITEMS;         // 4096 positions per tile
constexpr u32 SPLIT_CHUNK = BLOCK * 16;               // bytes per workgroup step of a split comparison
constexpr u32 WAVE_STEP = WAVE * 16;                  // bytes per wave step
constexpr u32 MAX_ROUNDS = 64;
constexpr u32 TIED = 0xFFFFFFFFu;                     // LCP output of the key path: rank left for the gather

struct Counters {                                     // device, zeroed per call
    unsigned long long positions;                     // irreducible positions compared against the text
    unsigned long long bytes;                         // bytes compared
    unsigned long long waves;                         // pairs queued for the wave kernel (= length of that queue)
    unsigned long long splits;                        // pairs queued for split comparison (= length of that queue)
    unsigned long long tied;                          // ranks whose key equals the predecessor's
    unsigned long long remaining[MAX_ROUNDS];         // split pairs still open after round j
    u32 error;                                        // an SA entry >= n was seen
    u32 pad[3];
};

// packed keys of an index in SA order (sa_build.hpp; exactly one of keys / keys32 is set)
struct KeyView {
    const u64* keys;
    const u32* keys32;
    const u32* bstart;                                // [257] with keys32
    int lo_shift, b, k0;
};

// ---- text access: aligned 8-byte words; words past the last one holding a text byte read as 0 ----------------------
__device__ __forceinline__ u64 tword(const u64* __restrict__ t, u64 w, u64 nw) { return w < nw ? t[w] : 0ull; }
__device__ __forceinline__ u64 tload8(const u64* __restrict__ t, u64 p, u64 nw) {   // T[p..p+8) little-endian
    const u64 w = p >> 3;
    const u32 s = (u32)(p & 7u) * 8u;
    const u64 lo = tword(t, w, nw);
    return s ? (lo >> s) | (tword(t, w + 1, nw) << (64u - s)) : lo;
}
// first offset o in [0, 16) with T[a+o] != T[b+o], 16 if none
__device__ __forceinline__ u32 mismatch16(const u64* __restrict__ t, u64 nw, u64 a, u64 b) {
    const u64 x0 = tload8(t, a, nw) ^ tload8(t, b, nw);
    if (x0) return (u32)__builtin_ctzll(x0) >> 3;
    const u64 x1 = tload8(t, a + 8, nw) ^ tload8(t, b + 8, nw);
    return x1 ? 8u + ((u32)__builtin_ctzll(x1) >> 3) : 16u;
}

template <class Idx>
__device__ __forceinline__ void wave_add(unsigned long long* ctr, u64 v) {   // one atomic per wave
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(ctr, (unsigned long long)v);
}

__device__ __forceinline__ u64 key_at(const KeyView& kv, const u32* s_b, u64 r) {
    if (kv.keys) return kv.keys[r];
    u32 lo = 0, hi = 256;                             // last b with bstart[b] <= r (empty buckets share their bound)
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if ((u64)s_b[mid] <= r) lo = mid; else hi = mid; }
    return ((u64)lo << 56) | ((u64)kv.keys32[r] << kv.lo_shift);
}

// Symbols: S = u8 (byte texts) or u32 (integer texts, sa_hip_libsais_plcp_int).  A text of S symbols is compared as the
// bytes of its words: suffix i starts at byte i * sizeof(S), a pair of m symbols spans m * sizeof(S) bytes, and the first
// differing byte o gives LCP o / sizeof(S) -- the same first mismatch whatever the byte order inside a symbol.  Depths,
// budgets and chunks below are in bytes; PLCP values in symbols.

// phase 1: one thread per rank.  KEYS: key shortcut (u8 only); LCP_OUT (with KEYS): untied ranks written to lcp_out directly.
template <class Idx, class S, bool KEYS, bool LCP_OUT>
__global__ __launch_bounds__(BLOCK) void lcp_phi_kernel(const u8* __restrict__ T, u64 nw, const Idx* __restrict__ SA, u64 n,
                                                         Idx* __restrict__ W, Idx* __restrict__ queue, u32* __restrict__ lcp_out,
                                                         KeyView kv, u32 lane_bytes, Counters* __restrict__ c) {
    __shared__ u32 s_b[257];
    if (KEYS && kv.keys32) {
        for (u32 j = threadIdx.x; j <= 256; j += BLOCK) s_b[j] = kv.bstart[j];
        __syncthreads();
    }
    static_assert(!KEYS || sizeof(S) == 1, "the key shortcut is byte-only");
    constexpr u64 SB = sizeof(S);
    const u64* T64 = reinterpret_cast<const u64*>(T);
    const S* Ts = reinterpret_cast<const S*>(T);
    u64 positions = 0, bytes = 0, tied = 0;
    u32 bad = 0;
    const u64 stride = (u64)gridDim.x * BLOCK;
    const u64 n_round = (n + 63) & ~63ull;            // whole waves iterate together (wave-aggregated queue pushes)
    for (u64 r = (u64)blockIdx.x * BLOCK + threadIdx.x; r < n_round; r += stride) {
        bool push = false;
        if (r < n) {
            const u64 i = (u64)SA[r];
            if (i >= n) bad = 1;
            else if (r == 0) {
                W[i] = (Idx)i;                        // no predecessor: PLCP 0
                if (LCP_OUT) lcp_out[0] = 0;
            } else {
                const u64 k = (u64)SA[r - 1];
                if (k >= n) bad = 1;
                else {
                    const u64 m = n - (i > k ? i : k);
                    u64 d0 = 0;
                    bool go = true;
                    if (KEYS) {
                        const u64 x = key_at(kv, s_b, r) ^ key_at(kv, s_b, r - 1);
                        const u32 j = x ? (u32)__builtin_clzll(x) / (u32)kv.b : 64u;
                        if (j < (u32)kv.k0) {         // differ inside the first k0 codes: exact
                            if (LCP_OUT) lcp_out[r] = j;
                            else W[i] = (Idx)(i + j);
                            go = false;
                        } else {
                            if (LCP_OUT) lcp_out[r] = TIED;
                            d0 = (u64)kv.k0 < m ? (u64)kv.k0 : m;
                            ++tied;
                        }
                    }
                    if (go && (i == 0 || k == 0 || Ts[i - 1] != Ts[k - 1])) {   // irreducible
                        ++positions;
                        const u64 mb = m * SB;
                        const u64 lim = (d0 + lane_bytes < mb) ? d0 + lane_bytes : mb;
                        u64 d = d0, l = lim;
                        while (d < lim) {
                            const u64 x = tload8(T64, i * SB + d, nw) ^ tload8(T64, k * SB + d, nw);
                            bytes += 8;
                            if (x) { const u64 p = d + ((u32)__builtin_ctzll(x) >> 3); l = p < lim ? p : lim; break; }
                            d += 8;
                        }
                        if (l < lim || l == mb) W[i] = (Idx)(i + l / SB);
                        else push = true;
                    }
                }
            }
        }
        const u64 mask = __ballot(push);
        if (mask) {
            const int leader = __ffsll((long long)mask) - 1;
            u64 base = 0;
            if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(&c->waves, (unsigned long long)__popcll(mask));
            base = __shfl(base, leader);
            if (push) queue[base + (u64)__popcll(mask & lanemask_lt())] = (Idx)r;
        }
    }
    wave_add<Idx>(&c->positions, positions);
    wave_add<Idx>(&c->bytes, bytes);
    if (KEYS) wave_add<Idx>(&c->tied, tied);
    if (bad) atomicOr(&c->error, 1u);
}

// phase 2: one wave per queued pair, comparison from depth d_start (uniform: every queued pair ran out of the same
// lane budget), 1 KB per step, up to wave_bytes; pairs still equal then are queued for the split phase with W[i] open.
template <class Idx, class S>
__global__ __launch_bounds__(BLOCK) void lcp_wave_kernel(const u8* __restrict__ T, u64 nw, const Idx* __restrict__ SA, u64 n,
                                                          Idx* __restrict__ W, const Idx* __restrict__ queue, Idx* __restrict__ split,
                                                          u64 d_start, u64 wave_bytes, Counters* __restrict__ c) {
    constexpr u64 SB = sizeof(S);
    const u64* T64 = reinterpret_cast<const u64*>(T);
    const u64 nq = c->waves;
    const u32 lane = threadIdx.x & 63;
    const u64 nwaves = (u64)gridDim.x * (BLOCK / WAVE);
    u64 bytes = 0;
    for (u64 e = (u64)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6); e < nq; e += nwaves) {
        const u64 r = (u64)queue[e];
        const u64 i = (u64)SA[r], k = (u64)SA[r - 1];   // both range-checked by the phi kernel
        const u64 m = n - (i > k ? i : k), mb = m * SB;
        u64 d = d_start < mb ? d_start : mb;
        const u64 end = (d + wave_bytes < mb) ? d + wave_bytes : mb;
        u64 res = ~0ull;
        while (d < end) {
            const u64 p = d + (u64)lane * 16;
            u32 off = 16;
            if (p < end) {
                off = mismatch16(T64, nw, i * SB + p, k * SB + p);
                if (off < 16 && p + off >= end) off = 16;
                const u64 span = end - p;
                bytes += (off < 16) ? off + 1 : (span < 16 ? span : 16);
            }
            const u64 mm = __ballot(off < 16);
            if (mm) {
                const int f = __ffsll((long long)mm) - 1;
                res = d + (u64)f * 16 + (u64)__shfl((int)off, f);
                break;
            }
            d += WAVE_STEP;
        }
        if (lane == 0) {
            if (res != ~0ull) W[i] = (Idx)(i + res / SB);
            else if (end >= mb) W[i] = (Idx)(i + m);
            else {
                W[i] = (Idx)~(Idx)0;                  // open: the split phase takes the minimum into it
                split[atomicAdd(&c->splits, 1ull)] = (Idx)r;
            }
        }
    }
    wave_add<Idx>(&c->bytes, bytes);
}

// phase 3, round j: [d_lo, d_lo + seg) of every open pair, 4 KB chunks spread over all workgroups.
template <class Idx, class S>
__global__ __launch_bounds__(BLOCK) void lcp_split_kernel(const u8* __restrict__ T, u64 nw, const Idx* __restrict__ SA, u64 n,
                                                           Idx* __restrict__ W, const Idx* __restrict__ split, u32 round,
                                                           u64 d_lo, u64 seg, Counters* __restrict__ c) {
    const u64 ns = c->splits;
    if (ns == 0 || (round > 0 && c->remaining[round - 1] == 0)) return;
    constexpr u64 SB = sizeof(S);
    const u64* T64 = reinterpret_cast<const u64*>(T);
    const Idx OPEN = (Idx)~(Idx)0;
    const u64 cpe = (seg + SPLIT_CHUNK - 1) / SPLIT_CHUNK;
    const u64 total = ns * cpe;
    u64 bytes = 0;
    for (u64 t = blockIdx.x; t < total; t += gridDim.x) {
        const u64 e = t / cpe, ch = t - e * cpe;
        const u64 r = (u64)split[e];
        const u64 i = (u64)SA[r], k = (u64)SA[r - 1];
        const u64 mb = (n - (i > k ? i : k)) * SB;
        const u64 lo = d_lo + ch * SPLIT_CHUNK;
        u64 hi = d_lo + seg < mb ? d_lo + seg : mb;
        if (lo + SPLIT_CHUNK < hi) hi = lo + SPLIT_CHUNK;
        if (lo >= hi) continue;
        const Idx cur = __atomic_load_n(&W[i], __ATOMIC_RELAXED);
        if (cur != OPEN && (u64)cur < i + lo / SB) continue;   // a mismatch before this chunk is known (its symbol ends before lo)
        const u64 p = lo + (u64)threadIdx.x * 16;
        if (p < hi) {
            u32 off = mismatch16(T64, nw, i * SB + p, k * SB + p);
            const u64 span = hi - p;
            bytes += span < 16 ? span : 16;
            if (off < 16 && p + off < hi) atomicMin(&W[i], (Idx)(i + (p + off) / SB));
        }
    }
    wave_add<Idx>(&c->bytes, bytes);
}

// end of round j: pairs without a mismatch in [.., d_hi) that reached n - max(i, k) are closed with that length
template <class Idx, class S>
__global__ __launch_bounds__(BLOCK) void lcp_split_advance_kernel(const Idx* __restrict__ SA, u64 n, Idx* __restrict__ W,
                                                                   const Idx* __restrict__ split, u32 round, u64 d_hi,
                                                                   Counters* __restrict__ c) {
    const u64 ns = c->splits;
    if (ns == 0 || (round > 0 && c->remaining[round - 1] == 0)) return;
    const Idx OPEN = (Idx)~(Idx)0;
    u64 open = 0;
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < ns; e += (u64)gridDim.x * BLOCK) {
        const u64 r = (u64)split[e];
        const u64 i = (u64)SA[r], k = (u64)SA[r - 1];
        const u64 m = n - (i > k ? i : k);
        if (W[i] == OPEN) {
            if (d_hi >= m * sizeof(S)) W[i] = (Idx)(i + m);
            else ++open;
        }
    }
    wave_add<Idx>(&c->remaining[round], open);
}

// ---- inclusive max-scan over W in text order ---------------------------------------------------------------------
// (block_scan_excl with ScanMax and identity 0: W holds no smaller value)
constexpr int SCAN_WAVES = BLOCK / WAVE;

// SCAN_ITEMS consecutive entries of W from `base` (W is the workspace's own buffer: 16-byte aligned, as is every tile)
template <class Idx>
__device__ __forceinline__ void load_items(const Idx* W, u64 base, u64 n, Idx (&v)[SCAN_ITEMS]) {
    if (base + SCAN_ITEMS <= n) {
        const uint4* p = reinterpret_cast<const uint4*>(W + base);
#pragma unroll
        for (u32 q = 0; q < SCAN_ITEMS * sizeof(Idx) / 16; ++q) { const uint4 x = p[q]; memcpy(&v[q * 16 / sizeof(Idx)], &x, 16); }
    } else {
        for (u32 q = 0; q < SCAN_ITEMS; ++q) v[q] = (base + q < n) ? W[base + q] : (Idx)0;
    }
}

template <class Idx>
__global__ __launch_bounds__(BLOCK) void lcp_tile_max_kernel(const Idx* __restrict__ W, u64 n, Idx* __restrict__ tmax) {
    __shared__ Idx s_w[SCAN_WAVES];
    const u64 base = (u64)blockIdx.x * SCAN_TILE + (u64)threadIdx.x * SCAN_ITEMS;
    Idx it[SCAN_ITEMS];
    load_items<Idx>(W, base, n, it);
    Idx v = 0;
    for (u32 q = 0; q < SCAN_ITEMS; ++q) if (it[q] > v) v = it[q];
    Idx all;
    (void)block_scan_excl<SCAN_WAVES>(v, (Idx)0, ScanMax{}, s_w, &all);
    if (threadIdx.x == 0) tmax[blockIdx.x] = all;
}

// one workgroup: exclusive max-scan of the tile maxima, in place
template <class Idx>
__global__ __launch_bounds__(BLOCK) void lcp_tile_scan_kernel(Idx* __restrict__ tmax, u64 nt) {
    __shared__ Idx s_w[SCAN_WAVES];
    Idx carry = 0;
    for (u64 base = 0; base < nt; base += SCAN_TILE) {
        const u64 b = base + (u64)threadIdx.x * SCAN_ITEMS;
        Idx v[SCAN_ITEMS];
        Idx mx = 0;
        for (u32 q = 0; q < SCAN_ITEMS; ++q) { v[q] = (b + q < nt) ? tmax[b + q] : 0; if (v[q] > mx) mx = v[q]; }
        Idx all;
        Idx run = block_scan_excl<SCAN_WAVES>(mx, (Idx)0, ScanMax{}, s_w, &all);
        if (carry > run) run = carry;
        for (u32 q = 0; q < SCAN_ITEMS; ++q) {
            if (b + q < nt) tmax[b + q] = run;
            if (v[q] > run) run = v[q];
        }
        if (all > carry) carry = all;
    }
}

// PLCP[j] = max(prefix of the tile, W[..j]) - j, written to out (may be W)
template <class Idx>
__global__ __launch_bounds__(BLOCK) void lcp_scan_apply_kernel(const Idx* W, u64 n, const Idx* __restrict__ tpre, Idx* out) {
    __shared__ Idx s_w[SCAN_WAVES];
    const u64 base = (u64)blockIdx.x * SCAN_TILE + (u64)threadIdx.x * SCAN_ITEMS;
    Idx v[SCAN_ITEMS];
    load_items<Idx>(W, base, n, v);
    Idx mx = 0;
    for (u32 q = 0; q < SCAN_ITEMS; ++q) if (v[q] > mx) mx = v[q];
    Idx run = block_scan_excl<SCAN_WAVES>(mx, (Idx)0, ScanMax{}, s_w);
    const Idx pre = tpre[blockIdx.x];
    if (pre > run) run = pre;
    for (u32 q = 0; q < SCAN_ITEMS; ++q) {
        if (v[q] > run) run = v[q];
        v[q] = (Idx)(run - (Idx)(base + q));
    }
    if (base + SCAN_ITEMS <= n && ((uintptr_t)out & 15u) == 0) {   // 16-byte stores (out may be a caller's buffer: checked)
        uint4* o = reinterpret_cast<uint4*>(out + base);
#pragma unroll
        for (u32 q = 0; q < SCAN_ITEMS * sizeof(Idx) / 16; ++q) { uint4 x; memcpy(&x, &v[q * 16 / sizeof(Idx)], 16); o[q] = x; }
    } else {
        for (u32 q = 0; q < SCAN_ITEMS; ++q) if (base + q < n) out[base + q] = v[q];
    }
}

// LCP[r] = PLCP[SA[r]].  KEYED: only the ranks the phi kernel left TIED.
template <class Idx, bool KEYED>
__global__ __launch_bounds__(BLOCK) void lcp_gather_kernel(const Idx* __restrict__ plcp, const Idx* __restrict__ SA, u64 n,
                                                            Idx* __restrict__ out, Counters* __restrict__ c) {
    u32 bad = 0;
    for (u64 r = (u64)blockIdx.x * BLOCK + threadIdx.x; r < n; r += (u64)gridDim.x * BLOCK) {
        if (KEYED && (u32)out[r] != TIED) continue;
        const u64 i = (u64)SA[r];
        if (i >= n) { bad = 1; continue; }
        out[r] = plcp[i];
    }
    if (bad) atomicOr(&c->error, 1u);
}

// ---- host side -----------------------------------------------------------------------------------------------------

struct Knobs {
    bool keys = true;
    u32 lane_bytes = 64;
    u64 wave_bytes = 16384;
    static Knobs read() {   // at call start (diag_env: only with SA_HIP_DIAG=1)
        Knobs k;
        if (const char* e = diag_env("SA_HIP_LCP_KEYS")) k.keys = atoi(e) != 0;
        if (const char* e = diag_env("SA_HIP_LCP_LANE_BYTES")) { const long v = atol(e); if (v >= 0 && v <= (1 << 20)) k.lane_bytes = (u32)v; }
        if (const char* e = diag_env("SA_HIP_LCP_WAVE_BYTES")) { const long long v = atoll(e); if (v >= 1 && v <= (1ll << 30)) k.wave_bytes = (u64)v; }
        return k;
    }
};

struct Workspace {
    DevBuf w, queue, split, tiles, ctr;
    hipEvent_t ev[6] = {};
    int ensure(u64 n, size_t idx_bytes) {
        for (int j = 0; j < 6; ++j) if (!ev[j]) SA_HIP_CHECK(hipEventCreate(&ev[j]));
        int rc;
        const u64 nt = (n + SCAN_TILE - 1) / SCAN_TILE + 1;
        if ((rc = w.ensure(n * idx_bytes + 64)) || (rc = queue.ensure(n * idx_bytes + 64)) || (rc = split.ensure(n * idx_bytes + 64)) ||
            (rc = tiles.ensure(nt * idx_bytes + 64)) || (rc = ctr.ensure(sizeof(Counters)))) return rc;
        return 0;
    }
    void release() {
        w.release(); queue.release(); split.release(); tiles.release(); ctr.release();
        for (int j = 0; j < 6; ++j) if (ev[j]) { (void)hipEventDestroy(ev[j]); ev[j] = nullptr; }
    }
};

enum class Out { PLCP, LCP };

inline u32 lcp_grid(u64 items) {   // grid-stride kernels: 8 workgroups per CU at most
    u64 g = (items + BLOCK - 1) / BLOCK;
    if (g > 2048) g = 2048;
    return g ? (u32)g : 1u;
}

// PLCP or LCP of (text, SA) on `stream`; n >= 2.  text: n symbols of S, 8-byte aligned (readable up to the 8-byte word
// that holds its last byte).  out: n entries of Idx.  keys: nullptr = no key shortcut (LCP with keys: Idx = u32, S = u8).
// When counters_host is non-NULL the call waits and copies the counters there; otherwise it only enqueues.
template <class Idx, class S = u8>
int run(Workspace& ws, hipStream_t stream, const u8* text, const Idx* sa, u64 n, Idx* out, Out what, const KeyView* keys,
        const Knobs& kn, Counters* counters_host, sa_hip_lcp_stats* stats) {
    int rc = ws.ensure(n, sizeof(Idx));
    if (rc) return rc;
    constexpr u64 SB = sizeof(S);
    const u64 nw = (n * SB + 7) / 8;
    Idx* W = ws.w.as<Idx>();
    Idx* queue = ws.queue.as<Idx>();
    Idx* split = ws.split.as<Idx>();
    Counters* c = ws.ctr.as<Counters>();
    const bool use_keys = keys != nullptr;
    const bool lcp_keyed = use_keys && what == Out::LCP;
    SA_HIP_CHECK(hipEventRecord(ws.ev[0], stream));
    SA_HIP_CHECK(hipMemsetAsync(c, 0, sizeof(Counters), stream));
    SA_HIP_CHECK(hipMemsetAsync(W, 0, n * sizeof(Idx), stream));
    const u32 g = lcp_grid(n);
    KeyView kv = use_keys ? *keys : KeyView{};
    u32* lcp32 = reinterpret_cast<u32*>(out);
    if constexpr (sizeof(Idx) == 4 && SB == 1) {   // the key shortcut exists for index handles (32-bit, bytes) only
        if (use_keys && what == Out::LCP)
            hipLaunchKernelGGL((lcp_phi_kernel<Idx, S, true, true>), dim3(g), dim3(BLOCK), 0, stream, text, nw, sa, n, W, queue, lcp32, kv, kn.lane_bytes, c);
        else if (use_keys)
            hipLaunchKernelGGL((lcp_phi_kernel<Idx, S, true, false>), dim3(g), dim3(BLOCK), 0, stream, text, nw, sa, n, W, queue, lcp32, kv, kn.lane_bytes, c);
    } else if (use_keys) return fail(SA_HIP_EINTERNAL, "lcp: key shortcut with 64-bit indices or integer symbols");
    if (!use_keys)
        hipLaunchKernelGGL((lcp_phi_kernel<Idx, S, false, false>), dim3(g), dim3(BLOCK), 0, stream, text, nw, sa, n, W, queue, lcp32, kv, kn.lane_bytes, c);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipEventRecord(ws.ev[1], stream));
    const u64 d_wave = (use_keys ? (u64)kv.k0 : 0ull) + kn.lane_bytes;
    hipLaunchKernelGGL((lcp_wave_kernel<Idx, S>), dim3(2048), dim3(BLOCK), 0, stream, text, nw, sa, n, W, queue, split, d_wave, kn.wave_bytes, c);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipEventRecord(ws.ev[2], stream));
    // split rounds: segment lengths double; round j covers [d_lo, d_lo + seg); no pair is longer than n symbols
    u64 d_lo = d_wave + kn.wave_bytes;
    u64 seg = ((kn.wave_bytes + SPLIT_CHUNK - 1) / SPLIT_CHUNK) * SPLIT_CHUNK;
    u32 rounds = 0;
    for (u32 j = 0; j < MAX_ROUNDS && d_lo < n * SB; ++j) {
        hipLaunchKernelGGL((lcp_split_kernel<Idx, S>), dim3(2048), dim3(BLOCK), 0, stream, text, nw, sa, n, W, split, j, d_lo, seg, c);
        hipLaunchKernelGGL((lcp_split_advance_kernel<Idx, S>), dim3(256), dim3(BLOCK), 0, stream, sa, n, W, split, j, d_lo + seg, c);
        SA_HIP_CHECK(hipGetLastError());
        d_lo += seg;
        seg *= 2;
        ++rounds;
    }
    SA_HIP_CHECK(hipEventRecord(ws.ev[3], stream));
    const u64 nt = (n + SCAN_TILE - 1) / SCAN_TILE;
    Idx* tiles = ws.tiles.as<Idx>();
    Idx* plcp = (what == Out::PLCP) ? out : W;        // the LCP output keeps PLCP in W for the gather
    hipLaunchKernelGGL((lcp_tile_max_kernel<Idx>), dim3(nt), dim3(BLOCK), 0, stream, W, n, tiles);
    hipLaunchKernelGGL((lcp_tile_scan_kernel<Idx>), dim3(1), dim3(BLOCK), 0, stream, tiles, nt);
    hipLaunchKernelGGL((lcp_scan_apply_kernel<Idx>), dim3(nt), dim3(BLOCK), 0, stream, W, n, tiles, plcp);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipEventRecord(ws.ev[4], stream));
    if (what == Out::LCP) {
        if constexpr (sizeof(Idx) == 4) {
            if (lcp_keyed) hipLaunchKernelGGL((lcp_gather_kernel<Idx, true>), dim3(lcp_grid(n)), dim3(BLOCK), 0, stream, W, sa, n, out, c);
        }
        if (!lcp_keyed) hipLaunchKernelGGL((lcp_gather_kernel<Idx, false>), dim3(lcp_grid(n)), dim3(BLOCK), 0, stream, W, sa, n, out, c);
        SA_HIP_CHECK(hipGetLastError());
    }
    SA_HIP_CHECK(hipEventRecord(ws.ev[5], stream));
    if (!counters_host && !stats) return 0;
    Counters h{};
    SA_HIP_CHECK(hipMemcpyAsync(&h, c, sizeof h, hipMemcpyDeviceToHost, stream));
    SA_HIP_CHECK(hipStreamSynchronize(stream));
    if (counters_host) *counters_host = h;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->n = n;
        stats->tied = h.tied;
        stats->compared_positions = h.positions;
        stats->compared_bytes = h.bytes;
        stats->wave_compares = h.waves;
        stats->split_compares = h.splits;
        stats->split_rounds = rounds;
        stats->keys = use_keys ? 1u : 0u;
        float ms[5] = {};
        for (int j = 0; j < 5; ++j) SA_HIP_CHECK(hipEventElapsedTime(&ms[j], ws.ev[j], ws.ev[j + 1]));
        float tot = 0.f;
        SA_HIP_CHECK(hipEventElapsedTime(&tot, ws.ev[0], ws.ev[5]));
        stats->phi_ms = ms[0]; stats->wave_ms = ms[1]; stats->split_ms = ms[2]; stats->scan_ms = ms[3]; stats->gather_ms = ms[4];
        stats->total_ms = tot;
    }
    return 0;
}

// LCP from a given PLCP (the drop-ins' *_lcp): a gather only
template <class Idx>
int gather_only(Workspace& ws, hipStream_t stream, const Idx* plcp, const Idx* sa, u64 n, Idx* out, u32* error) {
    int rc = ws.ctr.ensure(sizeof(Counters));
    if (rc) return rc;
    Counters* c = ws.ctr.as<Counters>();
    SA_HIP_CHECK(hipMemsetAsync(c, 0, sizeof(Counters), stream));
    hipLaunchKernelGGL((lcp_gather_kernel<Idx, false>), dim3(lcp_grid(n)), dim3(BLOCK), 0, stream, plcp, sa, n, out, c);
    SA_HIP_CHECK(hipGetLastError());
    Counters h{};
    SA_HIP_CHECK(hipMemcpyAsync(&h, c, sizeof h, hipMemcpyDeviceToHost, stream));
    SA_HIP_CHECK(hipStreamSynchronize(stream));
    *error = h.error;
    return 0;
}

}  // namespace lcp
}  // namespace sa
