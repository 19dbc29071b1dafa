// bwt.hpp -- Burrows-Wheeler transform and its inverse on the device (sa_hip_libsais[64]_bwt[_aux] / _unbwt[_aux],
// sa_hip_index_bwt_device, sa_hip_bwt64_device / sa_hip_unbwt64_device).  Conventions of libsais (libsais.c:6665-6714,
// 7588-7614): with SA the suffix array and p the rank with SA[p] = 0, the primary index is p + 1, U[0] = T[n-1] and
// U[r + (r < p)] = T[SA[r]-1] for every r != p (the '$' row is left out); the aux form adds I[t] = ISA[t*r_aux] + 1.
//
// Forward (one thread per 16 output bytes, one uint4 store each):
//   find    every SA entry range-checked (an entry >= n sets Counters::error and is never used for an access), the rank
//           of suffix 0, and I[SA[r] / r_aux] = r + 1 where r_aux divides SA[r]
//   gather  U[q] = T[SA[q - (q <= p)] - 1] for q >= 1, U[0] = T[n-1]: the SA read is sequential, the text read a random
//           byte per rank
//
// Inverse, in rank space (rank = matrix row - 1, the '$' row dropped): rank d of suffix i has psi(d) = rank of suffix
// (i + 1) mod n, and T[k] = F(psi^k(I[0] - 1)) where F(d) is the first character of rank d (the bucket of d among the
// 257 bounds of the byte histogram).  With row(u) = I[0] - 1 for u = 0, u - 1 for u < I[0], u otherwise (the row of U[u],
// libsais' calculate_biPSI skips `index` the same way), psi[cum[U[u]] + #{u' < u : U[u'] = U[u]}] = row(u): a stable
// counting sort of U by its byte --
//   hist    per-tile 256-bin counts, digit-major
//   scan    exclusive scan of them (big_build.hpp's three kernels): every (byte, tile) destination; bounds[c] = cum[c]
//   psi     per-wave ballot ranking (wave_rank, radix_sort.hpp), wave prefixes in LDS, psi[dest] = row(u)
// psi is a permutation of [0, n) whatever U holds: it comes from a histogram this file computes itself (an input freq
// table is never read) and row() is a bijection for every primary index in [1, n].
//
// The walk is list ranking over ruler sets.  Rulers: the aux rows I[t] - 1 (deduplicated), and, unless those are many
// and close ("aux-only"), every rank whose mixed hash is 0 mod s.  Each ruler follows psi for at most B steps, writing
// the characters it decodes; it stops at the next ruler (its successor).  A walk that uses up B claims the row it has
// reached as a new ruler, walked in the next round (the host reads the ruler count after every round; more rounds than
// ceil(n / B) + 1, or more rulers than the slots allow, return -2 -- never expected).  Paths of distinct rulers never
// share a row (psi is a permutation), so every walk is bounded and every claim is unique.
//   aux-only  text offsets are known (t * r_aux, a claim: its claimer's + B): walks write the output directly
//   ranked    walks write B-byte staging slots; Wyllie pointer jumping from the primary ruler over the successor list
//             (ceil(log2 S) + 1 rounds) gives each ruler its offset, then one wave per ruler copies its slot
// With input that is not the BWT of any text (psi has more than one cycle, or inconsistent aux rows), the output is
// unspecified, but every walk is bounded by B steps per round and every write lands inside a slot or inside [0, n).
#pragma once
#include "common.hpp"
#include "radix_sort.hpp"
#include "sa_build.hpp"
#include "big_build.hpp"

namespace sa {
namespace bwt {

constexpr u32 BLOCK = 256;
constexpr u32 ITEMS = 16;
constexpr u32 TILE = BLOCK * ITEMS;                   // 4096 bytes of U per workgroup in hist / psi
constexpr u32 WAVES = BLOCK / WAVE;
constexpr u64 NIL = ~0ull;

struct Counters {                                     // device, zeroed per call (primary: all ones)
    unsigned long long primary;                       // forward: smallest rank with SA = 0 (all ones: none)
    unsigned long long next_id;                       // rulers allocated so far
    unsigned long long aux_active;                    // aux rows that became rulers (duplicates do not)
    unsigned long long longest;                       // most psi steps of one lane in one launch
    u32 error;                                        // an SA entry >= n, or an aux row outside (0, n]
    u32 overflow;                                     // a claim found no free slot
    u32 pad[2];
};

// ---- forward ---------------------------------------------------------------------------------------------------------
template <class Idx>
__global__ __launch_bounds__(BLOCK) void bwt_find_kernel(const Idx* __restrict__ SA, u64 n, u64 r_aux, Idx* __restrict__ I,
                                                          Counters* __restrict__ c) {
    u32 bad = 0;
    const u64 mask = r_aux - 1;
    for (u64 r = (u64)blockIdx.x * BLOCK + threadIdx.x; r < n; r += (u64)gridDim.x * BLOCK) {
        const u64 s = (u64)SA[r];
        if (s >= n) { bad = 1; continue; }
        if (s == 0) atomicMin(&c->primary, (unsigned long long)r);
        if (I && (s & mask) == 0) I[s / r_aux] = (Idx)(r + 1);
    }
    if (bad) atomicOr(&c->error, 1u);
}

// U[q] for q in [16 t, 16 t + 16): whole 16-byte stores where U is 16-byte aligned and the group is complete
template <class Idx>
__global__ __launch_bounds__(BLOCK) void bwt_gather_kernel(const u8* __restrict__ T, const Idx* __restrict__ SA, u64 n,
                                                            u8* __restrict__ U, const Counters* __restrict__ c) {
    const u64 p = c->primary;                         // all ones (no SA entry 0: not a suffix array) -> q - 1 throughout
    const bool vec = ((uintptr_t)U & 15u) == 0;
    const u64 groups = (n + 15) / 16;
    for (u64 g = (u64)blockIdx.x * BLOCK + threadIdx.x; g < groups; g += (u64)gridDim.x * BLOCK) {
        const u64 q0 = g * 16;
        u32 w[4] = {0, 0, 0, 0};
#pragma unroll
        for (u32 j = 0; j < 16; ++j) {
            const u64 q = q0 + j;
            u32 ch = 0;
            if (q < n) {
                if (q == 0) ch = T[n - 1];
                else {
                    const u64 s = (u64)SA[q - (q <= p ? 1 : 0)];
                    ch = (s >= 1 && s < n) ? T[s - 1] : 0u;   // out-of-range entries: flagged by the find kernel
                }
            }
            w[j >> 2] |= ch << (8 * (j & 3));
        }
        if (vec && q0 + 16 <= n) {
            *reinterpret_cast<uint4*>(U + q0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (u32 j = 0; j < 16 && q0 + j < n; ++j) U[q0 + j] = (u8)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

// ---- inverse: psi by a stable counting sort of U ---------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void unbwt_hist_kernel(const u8* __restrict__ U, u64 n, u32 ntiles, u32* __restrict__ th) {
    constexpr int CS = 257;
    __shared__ u32 s_h[4 * CS];
    for (u32 i = threadIdx.x; i < 4 * CS; i += BLOCK) s_h[i] = 0;
    __syncthreads();
    u32* my = s_h + (threadIdx.x & 3) * CS;
    const u64 base = (u64)blockIdx.x * TILE;
#pragma unroll 4
    for (u32 it = 0; it < ITEMS; ++it) {
        const u64 j = base + (u64)it * BLOCK + threadIdx.x;
        if (j < n) atomicAdd(&my[U[j]], 1u);
    }
    sync_lds();
    if (threadIdx.x < 256) {
        u32 v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v += s_h[k * CS + threadIdx.x];
        th[(u64)threadIdx.x * ntiles + blockIdx.x] = v;
    }
}

// bounds[c] = number of bytes < c (the exclusive scan at digit c's first tile), bounds[256] = n
__global__ void unbwt_bounds_kernel(const u64* __restrict__ off, u32 ntiles, u64 n, u64* __restrict__ bounds) {
    const u32 c = threadIdx.x;
    if (c < 256) bounds[c] = off[(u64)c * ntiles];
    if (c == 0) bounds[256] = n;
}

template <class Idx>
__global__ __launch_bounds__(BLOCK) void unbwt_psi_kernel(const u8* __restrict__ U, u64 n, u64 primary, u32 ntiles,
                                                           const u64* __restrict__ off, Idx* __restrict__ psi) {
    __shared__ u32 s_wh[WAVES * 256];
    __shared__ u64 s_gd[256];
    for (u32 i = threadIdx.x; i < WAVES * 256; i += BLOCK) s_wh[i] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 base = (u64)blockIdx.x * TILE;
    const u32 tile_n = (u32)((n - base) < TILE ? (n - base) : TILE);
    const u32 woff = wave * (WAVE * ITEMS) + lane;
    u32 key[ITEMS], rd[ITEMS];
#pragma unroll
    for (u32 j = 0; j < ITEMS; ++j) { const u32 q = woff + j * WAVE; key[j] = q < tile_n ? (u32)U[base + q] : 0u; }
    if (tile_n == TILE) wave_rank<true, u32, ITEMS>(key, 0, 255u, woff, tile_n, s_wh + wave * 256, rd);
    else wave_rank<false, u32, ITEMS>(key, 0, 255u, woff, tile_n, s_wh + wave * 256, rd);
    sync_lds();
    if (threadIdx.x < 256) {                          // per digit: wave counts -> wave prefixes; the tile's base
        u32 run = 0;
#pragma unroll
        for (u32 w = 0; w < WAVES; ++w) { const u32 t = s_wh[w * 256 + threadIdx.x]; s_wh[w * 256 + threadIdx.x] = run; run += t; }
        s_gd[threadIdx.x] = off[(u64)threadIdx.x * ntiles + blockIdx.x];
    }
    __syncthreads();
    const u32* wh = s_wh + wave * 256;
#pragma unroll
    for (u32 j = 0; j < ITEMS; ++j) {
        const u32 q = woff + j * WAVE;
        if (q >= tile_n) continue;
        const u32 d = rd[j] >> 16;
        const u64 dest = s_gd[d] + wh[d] + (rd[j] & 0xFFFFu);
        const u64 u = base + q;
        const u64 row = (u == 0) ? primary - 1 : (u < primary ? u - 1 : u);
        if (dest < n) psi[dest] = (Idx)row;           // always true: the scan covers exactly n bytes
    }
}

// ---- rulers ------------------------------------------------------------------------------------------------------------
struct Rulers {                                       // per ruler id (capacity cap)
    u64* start;                                       // rank the walk begins at (NIL: duplicate, never walked)
    u64* succ;                                        // successor ruler id (NIL: none)
    u64* len;                                         // characters of its segment
    u64* off;                                         // text offset (aux-only: known; ranked: after the ranking)
    u32* mark;                                        // per rank: ruler id + 1, 0 = none (read only where bit is set)
    u32* bits;                                        // per rank: is a ruler
    u64 cap;
};

__device__ __forceinline__ u64 mix64(u64 x) {       // splitmix64 finaliser: hash rulers independent of the text's order
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ void set_bit(u32* bits, u64 x) { atomicOr(&bits[x >> 5], 1u << (x & 31)); }
__device__ __forceinline__ bool get_bit(const u32* bits, u64 x) { return (bits[x >> 5] >> (x & 31)) & 1u; }

// aux rows I[t] - 1 as rulers 0..m-1 (ruler 0 = the primary row); an entry outside (0, n] sets error; a duplicate row
// stays with the first id that claimed it
template <class Idx>
__global__ __launch_bounds__(BLOCK) void unbwt_aux_rulers_kernel(const Idx* __restrict__ I, u64 m, u64 n, u64 r_aux, Rulers R,
                                                                  Counters* __restrict__ c) {
    u32 bad = 0;
    u64 act = 0;
    for (u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x; t < m; t += (u64)gridDim.x * BLOCK) {
        const u64 v = (u64)I[t];
        R.succ[t] = NIL; R.len[t] = 0;
        R.off[t] = t * r_aux;
        if (v == 0 || v > n) { bad = 1; R.start[t] = NIL; continue; }
        const u64 x = v - 1;
        if (atomicCAS(&R.mark[x], 0u, (u32)(t + 1)) == 0u) { set_bit(R.bits, x); R.start[t] = x; ++act; }
        else R.start[t] = NIL;
    }
    for (int o = 32; o > 0; o >>= 1) act += __shfl_xor(act, o);
    if ((threadIdx.x & 63) == 0 && act) atomicAdd(&c->aux_active, (unsigned long long)act);
    if (bad) atomicOr(&c->error, 1u);
}

__device__ __forceinline__ bool hash_ruler(u64 x, u64 smask, u64 salt) { return (mix64(x ^ salt) & smask) == 0; }

// COUNT: how many ranks the hash selects (a bound for the slots); else: those not yet rulers get ids from next_id
template <bool COUNT>
__global__ __launch_bounds__(BLOCK) void unbwt_hash_rulers_kernel(u64 n, u64 smask, u64 salt, Rulers R, Counters* __restrict__ c) {
    const u64 n_round = (n + 63) & ~63ull;
    u64 cnt = 0;
    for (u64 x = (u64)blockIdx.x * BLOCK + threadIdx.x; x < n_round; x += (u64)gridDim.x * BLOCK) {
        bool take = x < n && hash_ruler(x, smask, salt);
        if (COUNT) { cnt += take; continue; }
        if (take && R.mark[x] != 0u) take = false;   // already an aux ruler (aux rulers were placed by an earlier launch)
        const u64 mask = __ballot(take);
        if (!mask) continue;
        const int leader = __ffsll((long long)mask) - 1;
        u64 base = 0;
        if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(&c->next_id, (unsigned long long)__popcll(mask));
        base = __shfl(base, leader);
        if (take) {
            const u64 id = base + (u64)__popcll(mask & lanemask_lt());
            if (id < R.cap) {
                R.mark[x] = (u32)(id + 1); set_bit(R.bits, x);
                R.start[id] = x; R.succ[id] = NIL; R.len[id] = 0; R.off[id] = NIL;
            } else atomicOr(&c->overflow, 1u);
        }
    }
    if (COUNT) {
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&c->next_id, (unsigned long long)cnt);
    }
}

// F(d): the byte whose bucket holds rank d (last c with bounds[c] <= d; empty buckets share their bound)
__device__ __forceinline__ u32 f_char(const u64* s_b, u64 d) {
    u32 lo = 0, hi = 256;
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (s_b[mid] <= d) lo = mid; else hi = mid; }
    return lo;
}

// byte writer: dst[pos], pos < lim; 8-byte stores where the word lies wholly inside this walk's span and dst is aligned
struct Writer {
    u8* dst; u64 pos0, pos, lim; u64 acc; bool al;
    __device__ __forceinline__ void flush_bytes(u64 wpos, u32 cnt) {   // bytes [wpos, wpos + cnt) from acc (by pos & 7)
        for (u32 j = 0; j < cnt; ++j) { const u64 q = wpos + j; if (q < lim) dst[q] = (u8)(acc >> (8 * (q & 7))); }
    }
    __device__ __forceinline__ void put(u32 ch) {
        acc |= (u64)ch << (8 * (pos & 7));
        if ((pos & 7) == 7) {
            const u64 w0 = pos - 7;
            if (al && w0 >= pos0 && pos < lim) *reinterpret_cast<u64*>(dst + w0) = acc;
            else { const u64 s = w0 >= pos0 ? w0 : pos0; flush_bytes(s, (u32)(pos + 1 - s)); }
            acc = 0;
        }
        ++pos;
    }
    __device__ __forceinline__ void finish() {
        if (pos & 7) { const u64 w0 = pos & ~7ull; const u64 s = w0 >= pos0 ? w0 : pos0; flush_bytes(s, (u32)(pos - s)); }
    }
};

// one lane per ruler of this round, ids [lo, hi): at most B psi steps.  DIRECT: into out at the ruler's known offset;
// else into its staging slot.
template <class Idx, bool DIRECT>
__global__ __launch_bounds__(BLOCK) void unbwt_walk_kernel(const Idx* __restrict__ psi, const u64* __restrict__ bounds, u64 n,
                                                            Rulers R, u64 lo, u64 hi, u32 B, u8* __restrict__ out,
                                                            u8* __restrict__ staging, Counters* __restrict__ c) {
    __shared__ u64 s_b[257];
    for (u32 j = threadIdx.x; j <= 256; j += BLOCK) s_b[j] = bounds[j];
    __syncthreads();
    u64 longest = 0;
    const u64 n1 = n - 1;
    for (u64 id = lo + (u64)blockIdx.x * BLOCK + threadIdx.x; id < hi; id += (u64)gridDim.x * BLOCK) {
        const u64 x0 = R.start[id];
        if (x0 == NIL) continue;
        Writer w;
        if (DIRECT) { const u64 o = R.off[id]; w.dst = out; w.pos0 = w.pos = o; w.lim = n; w.al = ((uintptr_t)out & 7u) == 0; }
        else { w.dst = staging + id * (u64)B; w.pos0 = w.pos = 0; w.lim = B; w.al = true; }
        w.acc = 0;
        u64 x = x0;
        u64 nxt = (u64)psi[x];
        u64 succ = NIL;
        u32 k = 0;
        for (;;) {
            w.put(f_char(s_b, x));
            ++k;
            const u64 y = nxt < n1 ? nxt : n1;        // psi entries are < n by construction; clamped all the same
            const bool is_r = get_bit(R.bits, y);
            const u64 nn = (u64)psi[y];               // issued with the bit test: one round trip per step
            if (is_r) { succ = (u64)R.mark[y] - 1; break; }
            if (k >= B) {
                const u64 id2 = atomicAdd(&c->next_id, 1ull);
                if (id2 < R.cap) {
                    R.mark[y] = (u32)(id2 + 1); set_bit(R.bits, y);
                    R.start[id2] = y; R.succ[id2] = NIL; R.len[id2] = 0;
                    R.off[id2] = DIRECT ? R.off[id] + B : NIL;
                    succ = id2;
                } else atomicOr(&c->overflow, 1u);
                break;
            }
            x = y;
            nxt = nn;
        }
        w.finish();
        R.len[id] = k;
        R.succ[id] = succ;
        if (k > longest) longest = k;
    }
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(longest, o); if (t > longest) longest = t; }
    if ((threadIdx.x & 63) == 0 && longest) atomicMax(&c->longest, (unsigned long long)longest);
}

// ---- ranking (Wyllie): distance to the end of the successor list, cut before the primary ruler (id 0) --------------
__global__ __launch_bounds__(BLOCK) void unbwt_rank_init_kernel(Rulers R, u64 S, u64* __restrict__ val, u64* __restrict__ nx) {
    for (u64 id = (u64)blockIdx.x * BLOCK + threadIdx.x; id < S; id += (u64)gridDim.x * BLOCK) {
        if (R.start[id] == NIL) { val[id] = 0; nx[id] = NIL; continue; }
        const u64 s = R.succ[id];
        val[id] = R.len[id];
        nx[id] = (s == 0 || s >= S) ? NIL : s;
    }
}
__global__ __launch_bounds__(BLOCK) void unbwt_rank_step_kernel(u64 S, const u64* __restrict__ vi, const u64* __restrict__ ni,
                                                                 u64* __restrict__ vo, u64* __restrict__ no) {
    for (u64 id = (u64)blockIdx.x * BLOCK + threadIdx.x; id < S; id += (u64)gridDim.x * BLOCK) {
        const u64 j = ni[id];
        if (j == NIL) { vo[id] = vi[id]; no[id] = NIL; }
        else { vo[id] = vi[id] + vi[j]; no[id] = ni[j]; }
    }
}
// off = n - (distance to the end); a ruler off the primary's list (not a BWT) keeps no offset
__global__ __launch_bounds__(BLOCK) void unbwt_rank_final_kernel(Rulers R, u64 S, u64 n, const u64* __restrict__ val, const u64* __restrict__ nx) {
    for (u64 id = (u64)blockIdx.x * BLOCK + threadIdx.x; id < S; id += (u64)gridDim.x * BLOCK) {
        const u64 d = val[id];
        R.off[id] = (nx[id] == NIL && d <= n) ? n - d : NIL;
    }
}

// one wave per ruler: its slot to out[off, off + len) when that lies inside [0, n)
__global__ __launch_bounds__(BLOCK) void unbwt_copy_kernel(Rulers R, u64 S, u64 n, u32 B, const u8* __restrict__ staging, u8* __restrict__ out) {
    const u32 lane = threadIdx.x & 63;
    const u64 nwaves = (u64)gridDim.x * WAVES;
    for (u64 id = (u64)blockIdx.x * WAVES + (threadIdx.x >> 6); id < S; id += nwaves) {
        if (R.start[id] == NIL) continue;
        const u64 o = R.off[id], len = R.len[id];
        if (o == NIL || o > n || len > n - o || len > B) continue;
        const u8* src = staging + id * (u64)B;
        for (u64 j = lane; j < len; j += WAVE) out[o + j] = src[j];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------

struct Knobs {
    u32 walk = 2048;                                  // B: psi steps per walk and round (multiple of 8)
    u32 ruler = 1024;                                 // s: one hash ruler per s ranks (power of two)
    u64 aux_min = 1ull << 18;                         // aux rows that make the aux-only plan (with r_aux <= 8 B)
    static Knobs read() {   // at call start (diag_env: only with SA_HIP_DIAG=1)
        Knobs k;
        if (const char* e = diag_env("SA_HIP_UNBWT_WALK")) { const long v = atol(e); if (v >= 8 && v <= (1 << 20)) k.walk = (u32)(v & ~7l); }
        if (const char* e = diag_env("SA_HIP_UNBWT_RULER")) { const long v = atol(e); if (v >= 1 && v <= (1 << 30) && (v & (v - 1)) == 0) k.ruler = (u32)v; }
        if (const char* e = diag_env("SA_HIP_UNBWT_AUX_MIN")) { const long long v = atoll(e); if (v >= 1) k.aux_min = (u64)v; }
        return k;
    }
};

struct Workspace {
    DevBuf ctr, th, part, off, bounds, psi, aux;
    DevBuf start, succ, len, roff, mark, bits, staging, rank[4], tmp;
    hipEvent_t ev[6] = {};
    int events() {
        for (int j = 0; j < 6; ++j) if (!ev[j]) SA_HIP_CHECK(hipEventCreate(&ev[j]));
        return 0;
    }
    void release() {
        DevBuf* all[] = {&ctr, &th, &part, &off, &bounds, &psi, &aux, &start, &succ, &len, &roff, &mark, &bits, &staging,
                         &rank[0], &rank[1], &rank[2], &rank[3], &tmp};
        for (DevBuf* b : all) b->release();
        for (int j = 0; j < 6; ++j) if (ev[j]) { (void)hipEventDestroy(ev[j]); ev[j] = nullptr; }
    }
};

inline u32 grid_for(u64 items) {
    u64 g = (items + BLOCK - 1) / BLOCK;
    if (g > 2048) g = 2048;
    return g ? (u32)g : 1u;
}

// Forward BWT of (text, SA) on `stream`, n >= 2: U (n bytes), I (aux rows, (n-1)/r_aux + 1 entries of Idx) when non-NULL.
// Waits; *primary = rank of suffix 0 + 1.  -1 (SA_HIP_EINVAL) when an SA entry is out of range or none is 0.
template <class Idx>
int run_bwt(Workspace& ws, hipStream_t stream, const u8* text, const Idx* sa, u64 n, u64 r_aux, Idx* I, u8* U, u64* primary,
            sa_hip_bwt_stats* stats) {
    int rc;
    if ((rc = ws.events()) || (rc = ws.ctr.ensure(sizeof(Counters)))) return rc;
    Counters* c = ws.ctr.as<Counters>();
    SA_HIP_CHECK(hipEventRecord(ws.ev[0], stream));
    SA_HIP_CHECK(hipMemsetAsync(c, 0, sizeof(Counters), stream));
    SA_HIP_CHECK(hipMemsetAsync(&c->primary, 0xFF, 8, stream));
    hipLaunchKernelGGL((bwt_find_kernel<Idx>), dim3(grid_for(n)), dim3(BLOCK), 0, stream, sa, n, I ? r_aux : 1ull, I, c);
    hipLaunchKernelGGL((bwt_gather_kernel<Idx>), dim3(grid_for((n + 15) / 16)), dim3(BLOCK), 0, stream, text, sa, n, U, c);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipEventRecord(ws.ev[1], stream));
    Counters h{};
    SA_HIP_CHECK(hipMemcpyAsync(&h, c, sizeof h, hipMemcpyDeviceToHost, stream));
    SA_HIP_CHECK(hipStreamSynchronize(stream));
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->n = n;
        float ms = 0.f;
        SA_HIP_CHECK(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]));
        stats->gather_ms = ms; stats->total_ms = ms;
    }
    if (h.error) return fail(SA_HIP_EINVAL, "bwt: suffix array entry out of range [0, n)");
    if (h.primary >= n) return fail(SA_HIP_EINVAL, "bwt: no suffix array entry is 0 (not a suffix array)");
    *primary = h.primary + 1;
    return 0;
}

// Inverse BWT on `stream`, n >= 2: U (n bytes, device), I (m = (n-1)/r_aux + 1 aux rows of Idx on the device, I[0] the
// primary index; r_aux = n for the plain form) -> out (n bytes; may not overlap U).  Waits.  Returns 0, -1 (an aux row
// outside (0, n]: nothing is written), -2 (more rounds or rulers than the bounds allow; never expected).
template <class Idx>
int run_unbwt(Workspace& ws, hipStream_t stream, const u8* U, u64 n, const Idx* I, u64 r_aux, u8* out, const Knobs& kn,
              sa_hip_bwt_stats* stats) {
    int rc;
    const u64 m = (n - 1) / r_aux + 1;
    const u64 nt64 = (n + TILE - 1) / TILE;
    if (nt64 > 0x7FFFFFFFull) return fail(SA_HIP_EINVAL, "unbwt: too many tiles");
    const u32 ntiles = (u32)nt64;
    const u64 len = 256ull * ntiles;
    const u64 nparts = (len + big::SC_TILE - 1) / big::SC_TILE;
    const u64 nbits = (n + 31) / 32;
    if ((rc = ws.events()) || (rc = ws.ctr.ensure(sizeof(Counters))) || (rc = ws.th.ensure(len * 4 + 64)) ||
        (rc = ws.part.ensure((nparts + 1) * 8 + 64)) || (rc = ws.off.ensure(len * 8 + 64)) || (rc = ws.bounds.ensure(257 * 8 + 64)) ||
        (rc = ws.psi.ensure(n * sizeof(Idx) + 64)) || (rc = ws.mark.ensure(n * 4 + 64)) || (rc = ws.bits.ensure(nbits * 4 + 64)))
        return rc;
    Counters* c = ws.ctr.as<Counters>();
    u64* bounds = ws.bounds.as<u64>();
    Idx* psi = ws.psi.as<Idx>();
    // primary index for row(): I[0], read back (m entries are checked on the device below)
    Idx i0 = 0;
    SA_HIP_CHECK(hipMemcpyAsync(&i0, I, sizeof(Idx), hipMemcpyDeviceToHost, stream));
    SA_HIP_CHECK(hipStreamSynchronize(stream));
    const u64 primary = (u64)i0;
    if (primary == 0 || primary > n) return fail(SA_HIP_EINVAL, "unbwt: primary index outside (0, n]");
    SA_HIP_CHECK(hipEventRecord(ws.ev[0], stream));
    SA_HIP_CHECK(hipMemsetAsync(c, 0, sizeof(Counters), stream));
    hipLaunchKernelGGL(unbwt_hist_kernel, dim3(ntiles), dim3(BLOCK), 0, stream, U, n, ntiles, ws.th.as<u32>());
    hipLaunchKernelGGL(big::bg_scan_reduce_kernel, dim3((u32)nparts), dim3(big::SC_BLOCK), 0, stream, (const u32*)ws.th.as<u32>(), len, ws.part.as<u64>());
    hipLaunchKernelGGL(big::bg_scan_parts_kernel, dim3(1), dim3(big::SC_BLOCK), 0, stream, ws.part.as<u64>(), nparts);
    hipLaunchKernelGGL(big::bg_scan_apply_kernel, dim3((u32)nparts), dim3(big::SC_BLOCK), 0, stream, (const u32*)ws.th.as<u32>(), len,
                       (const u64*)ws.part.as<u64>(), ws.off.as<u64>());
    hipLaunchKernelGGL(unbwt_bounds_kernel, dim3(1), dim3(BLOCK), 0, stream, (const u64*)ws.off.as<u64>(), ntiles, n, bounds);
    hipLaunchKernelGGL((unbwt_psi_kernel<Idx>), dim3(ntiles), dim3(BLOCK), 0, stream, U, n, primary, ntiles, (const u64*)ws.off.as<u64>(), psi);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipEventRecord(ws.ev[1], stream));

    // rulers: aux rows first (ids 0..m-1; their count bounds the slots before anything is placed)
    SA_HIP_CHECK(hipMemsetAsync(ws.mark.p, 0, n * 4, stream));
    SA_HIP_CHECK(hipMemsetAsync(ws.bits.p, 0, nbits * 4, stream));
    const u64 smask = (u64)kn.ruler - 1;
    const u64 salt = 0x5851f42d4c957f2dull ^ n;
    hipLaunchKernelGGL((unbwt_hash_rulers_kernel<true>), dim3(grid_for(n)), dim3(BLOCK), 0, stream, n, smask, salt, Rulers{}, c);
    SA_HIP_CHECK(hipGetLastError());
    Counters h{};
    SA_HIP_CHECK(hipMemcpyAsync(&h, c, sizeof h, hipMemcpyDeviceToHost, stream));
    SA_HIP_CHECK(hipStreamSynchronize(stream));
    const u64 hash_count = h.next_id;
    const u64 B = kn.walk;
    const u64 cap = m + hash_count + (n + B - 1) / B + 2;
    if (cap >= 0xFFFFFFFFull) return fail(SA_HIP_EINVAL, "unbwt: too many rulers");
    if ((rc = ws.start.ensure(cap * 8 + 64)) || (rc = ws.succ.ensure(cap * 8 + 64)) || (rc = ws.len.ensure(cap * 8 + 64)) ||
        (rc = ws.roff.ensure(cap * 8 + 64))) return rc;
    Rulers R{ws.start.as<u64>(), ws.succ.as<u64>(), ws.len.as<u64>(), ws.roff.as<u64>(), ws.mark.as<u32>(), ws.bits.as<u32>(), cap};
    SA_HIP_CHECK(hipMemsetAsync(c, 0, sizeof(Counters), stream));
    hipLaunchKernelGGL((unbwt_aux_rulers_kernel<Idx>), dim3(grid_for(m)), dim3(BLOCK), 0, stream, I, m, n, r_aux, R, c);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipMemcpyAsync(&h, c, sizeof h, hipMemcpyDeviceToHost, stream));
    SA_HIP_CHECK(hipStreamSynchronize(stream));
    if (h.error) return fail(SA_HIP_EINVAL, "unbwt: an aux index is outside (0, n]");
    const bool direct = h.aux_active >= kn.aux_min && r_aux <= 8 * B;   // aux-only: offsets known, no ranking
    const u64 nid0 = m;
    SA_HIP_CHECK(hipMemcpyAsync(&c->next_id, &nid0, 8, hipMemcpyHostToDevice, stream));
    if (!direct)
        hipLaunchKernelGGL((unbwt_hash_rulers_kernel<false>), dim3(grid_for(n)), dim3(BLOCK), 0, stream, n, smask, salt, R, c);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipMemcpyAsync(&h, c, sizeof h, hipMemcpyDeviceToHost, stream));
    SA_HIP_CHECK(hipStreamSynchronize(stream));
    if (h.overflow) return fail(SA_HIP_EINTERNAL, "unbwt: ruler slots exhausted");
    u64 S0 = h.next_id;
    u8* staging = nullptr;
    if (!direct) {
        if ((rc = ws.staging.ensure(cap * B + 64))) return rc;
        staging = ws.staging.as<u8>();
    }
    SA_HIP_CHECK(hipEventRecord(ws.ev[2], stream));

    // walks, round by round
    const u64 max_rounds = (n + B - 1) / B + 1;
    u64 lo = 0, hi = S0;
    u32 rounds = 0;
    while (lo < hi) {
        if (rounds >= max_rounds) return fail(-2, "unbwt: more walk rounds than the bound (not expected)");
        const u32 g = grid_for(hi - lo);
        if (direct) hipLaunchKernelGGL((unbwt_walk_kernel<Idx, true>), dim3(g), dim3(BLOCK), 0, stream, psi, bounds, n, R, lo, hi, (u32)B, out, staging, c);
        else hipLaunchKernelGGL((unbwt_walk_kernel<Idx, false>), dim3(g), dim3(BLOCK), 0, stream, psi, bounds, n, R, lo, hi, (u32)B, out, staging, c);
        SA_HIP_CHECK(hipGetLastError());
        SA_HIP_CHECK(hipMemcpyAsync(&h, c, sizeof h, hipMemcpyDeviceToHost, stream));
        SA_HIP_CHECK(hipStreamSynchronize(stream));
        if (h.overflow) return fail(-2, "unbwt: ruler slots exhausted (not expected)");
        ++rounds;
        lo = hi;
        hi = h.next_id < cap ? h.next_id : cap;
    }
    const u64 S = hi;
    SA_HIP_CHECK(hipEventRecord(ws.ev[3], stream));

    // ranking and copy (ranked plan only)
    u32 rank_rounds = 0;
    if (!direct) {
        for (int j = 0; j < 4; ++j) if ((rc = ws.rank[j].ensure(S * 8 + 64))) return rc;
        u64 *vi = ws.rank[0].as<u64>(), *ni = ws.rank[1].as<u64>(), *vo = ws.rank[2].as<u64>(), *no = ws.rank[3].as<u64>();
        hipLaunchKernelGGL(unbwt_rank_init_kernel, dim3(grid_for(S)), dim3(BLOCK), 0, stream, R, S, vi, ni);
        const u32 steps = (u32)bits_for(S + 1) + 1;
        for (u32 j = 0; j < steps; ++j) {
            hipLaunchKernelGGL(unbwt_rank_step_kernel, dim3(grid_for(S)), dim3(BLOCK), 0, stream, S, (const u64*)vi, (const u64*)ni, vo, no);
            u64* t = vi; vi = vo; vo = t;
            t = ni; ni = no; no = t;
            ++rank_rounds;
        }
        hipLaunchKernelGGL(unbwt_rank_final_kernel, dim3(grid_for(S)), dim3(BLOCK), 0, stream, R, S, n, (const u64*)vi, (const u64*)ni);
        SA_HIP_CHECK(hipGetLastError());
    }
    SA_HIP_CHECK(hipEventRecord(ws.ev[4], stream));
    if (!direct) {
        u64 g = (S + WAVES - 1) / WAVES;
        if (g > 4096) g = 4096;
        hipLaunchKernelGGL(unbwt_copy_kernel, dim3((u32)(g ? g : 1)), dim3(BLOCK), 0, stream, R, S, n, (u32)B, (const u8*)staging, out);
        SA_HIP_CHECK(hipGetLastError());
    }
    SA_HIP_CHECK(hipEventRecord(ws.ev[5], stream));
    SA_HIP_CHECK(hipStreamSynchronize(stream));
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->n = n;
        stats->rulers = S;
        stats->longest_walk = h.longest;
        stats->ruler_rounds = rounds;
        stats->rank_rounds = rank_rounds;
        stats->aux_only = direct ? 1u : 0u;
        float ms[5] = {};
        for (int j = 0; j < 5; ++j) SA_HIP_CHECK(hipEventElapsedTime(&ms[j], ws.ev[j], ws.ev[j + 1]));
        // ev[1..2] (ruler placement) is counted with the walk
        stats->psi_ms = ms[0]; stats->walk_ms = ms[1] + ms[2]; stats->rank_ms = ms[3]; stats->copy_ms = ms[4];
        float tot = 0.f;
        SA_HIP_CHECK(hipEventElapsedTime(&tot, ws.ev[0], ws.ev[5]));
        stats->total_ms = tot;
    }
    return 0;
}

}  // namespace bwt
}  // namespace sa
