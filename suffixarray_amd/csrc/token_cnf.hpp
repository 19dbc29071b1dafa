// token_cnf.hpp -- the documents that satisfy a CNF query: an AND of clauses, every clause an OR of n-grams (literals), some clauses
// negated (sa_hip_token_index_cnf_*; include/sa_hip.h section 6m).  The single-literal case is tq_all_kernel of token_all.hpp; this
// is its general form on the same three arrays PV, DA and RK and the same two facts: a rank r of a range [a, b) is the first rank of
// its document there iff PV[r] < a, and "document d has a rank in [a, b)" is one bounded binary search in segment d of RK.
//
//   tq_cnf_kernel  one wave per group (one query), NEXT_WAVES per workgroup.  Lane l < L loads literal l's clamped range; the bounds
//                  go to LDS once per group (2 * 64 words per wave) and are read from there at addresses that are the same in every
//                  lane, so the divergent part needs no register array indexed by a literal number.  The literal counts are summed in
//                  u64 by one wave scan of scan.hpp; clause j's sum is the difference of two scan values.  The driver is the positive
//                  clause with the smallest {sum, index} (one wave reduce over the inverted key); a negated clause never drives.
//                  The driver's literals are walked one after the other, each from its own first rank, `examined` ranks in all: PV
//                  is streamed in DOC_UNROLL windows as tq_all_walk streams it.  A lane whose rank is the first of its document in
//                  its literal looks the document up in the driver's earlier literals (a duplicate when one holds it: the document
//                  was a candidate there), then in every other clause in clause order: a positive clause stops at its first literal
//                  that holds the document, a negated one fails at it.  The lanes diverge there; nothing in that part is a cross-lane
//                  operation.  Three ballots follow it: duplicates, candidates, matches; the prefix popcount of the last gives the
//                  slots, so the list is in literal order and then rank order.
//
// Bounds: literal ranges are clamped as tq_walk_of does; clauses per group are clamped to CNF_MAX_CLAUSES, literals to
// CNF_MAX_LITERALS and every clause offset to [0, L] (the host refused any table that needs it); DA holds values in [0, D); every
// search is at most STEPS halvings and a lower bound that lands at its segment's end is never dereferenced; a window loop advances
// by >= 1 rank per trip; docs and offsets are written below cap only and never when cap == 0.
//
// Not here: the shard-set form, a proximity constraint between clauses, a per-wave queue of candidates probed 64 at a time
// (DESIGN.md 9z).
#pragma once
#include "token_all.hpp"

namespace sa {
namespace tq {

constexpr u32 CNF_MAX_CLAUSES = SA_HIP_TOKEN_CNF_MAX_CLAUSES;     // clauses of one group
constexpr u32 CNF_MAX_LITERALS = SA_HIP_TOKEN_CNF_MAX_LITERALS;   // literals of one group: one per lane
static_assert(CNF_MAX_LITERALS == (u32)WAVE && CNF_MAX_CLAUSES < (u32)WAVE, "one lane per literal, one lane per clause offset");

struct CnfArgs {
    const sa_hip_token_span* spans;   // [S]
    const u32* group_offsets;         // [G + 1] into the clauses, checked on the host
    const u32* clause_offsets;        // [C + 1] into the spans, checked on the host
    const unsigned char* negated;     // [C], 0 / 1
    u64 G;
    u32 cap;                          // 0: counts only
    u32 budget;                       // 0: none
    int32_t* docs;                    // [G * cap]; never touched when cap == 0
    int32_t* offsets;                 // [G * cap]
    sa_hip_token_cnf* heads;          // [G]
};

// whether document segment [g0, g1) of RK holds a rank of [a, end)
__device__ __forceinline__ bool tq_cnf_holds(const int32_t* __restrict__ rk, u32 g0, u32 g1, u32 a, u32 end) {
    const u32 at = tq_seg_lower(rk, g0, g1, a);
    return at < g1 && (u32)rk[at] < end;
}

// One wave per group.
__global__ __launch_bounds__(NEXT_WAVES * WAVE) void tq_cnf_kernel(View x, RankView d, CnfArgs g) {
    __shared__ u32 s_a[NEXT_WAVES][CNF_MAX_LITERALS], s_end[NEXT_WAVES][CNF_MAX_LITERALS];   // the literals' bounds
    __shared__ u32 s_cl[NEXT_WAVES][CNF_MAX_CLAUSES + 1];                                    // clause offsets inside the group
    const u32 lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
    // the groups beyond the launch cap of wave_row_grid are served by this loop (test_gpu_token_cnf.py runs it past the cap; the table
    // of row loops in tests/token_walk_cases.py lists the kernels of test_gpu_token_launch_cap.py and is left as it stands)
    const u64 stride = (u64)gridDim.x * NEXT_WAVES;
    for (u64 w = (u64)blockIdx.x * NEXT_WAVES + wv; w < g.G; w += stride) {
        const u32 c0 = g.group_offsets[w];
        u32 nc = g.group_offsets[w + 1] - c0;
        if (nc > CNF_MAX_CLAUSES) nc = CNF_MAX_CLAUSES;    // (the host refused such a table)
        const u32 l0 = g.clause_offsets[c0];
        u32 L = g.clause_offsets[c0 + nc] - l0;
        if (L > CNF_MAX_LITERALS) L = CNF_MAX_LITERALS;    // (likewise)
        const sa_hip_token_span* const sp = g.spans + l0;
        // lane l: literal l; lane j <= nc: clause offset j; lane j < nc: whether clause j is negated
        Walk mine{0u, 0u, 0u};
        if (lane < L) mine = tq_walk_of(x, sp[lane]);
        u32 cut = 0;
        if (lane <= nc) {
            cut = g.clause_offsets[c0 + lane] - l0;
            if (cut > L) cut = L;
        }
        const u32 negmask = (u32)__ballot(lane < nc && g.negated[c0 + lane] != 0);           // (nc <= 16)
        __builtin_amdgcn_wave_barrier();                   // the group before this one has been read
        s_a[wv][lane] = mine.a;
        s_end[wv][lane] = mine.end;
        if (lane <= nc) s_cl[wv][lane] = cut;
        __builtin_amdgcn_wave_barrier();
        // clause sums in 64 bits: 64 literals of up to 2^31 - 1 ranks
        const u64 upto = wave_scan_incl((u64)(mine.end - mine.a), ScanSum{});
        const u32 lo = lane < nc ? cut : 0u;
        const u32 hi = lane < nc ? s_cl[wv][lane + 1] : 0u;
        const u64 below = __shfl(upto, (int)(lo ? lo - 1 : 0u)), through = __shfl(upto, (int)(hi ? hi - 1 : 0u));
        const u64 sum = hi > lo ? through - (lo ? below : 0ull) : 0ull;                      // < 2^37
        // the driver: the smallest {sum, clause} over the positive clauses; every other lane holds the largest key there is
        const bool positive = lane < nc && !((negmask >> lane) & 1);
        const u64 key = positive ? (sum << 6) | lane : ~0ull;
        const u64 best = ~wave_reduce(~key, ScanMax{});
        const bool any = best != ~0ull;                    // (no positive clause: the host refused such a table)
        const u32 driver = any ? (u32)(best & 63) : 0u;
        const u64 count = any ? best >> 6 : 0ull;
        const u64 examined = (g.budget && g.budget < count) ? g.budget : count;
        const u32 d0 = any ? s_cl[wv][driver] : 0u, d1 = any ? s_cl[wv][driver + 1] : 0u;
        if (lane == 0) {                                   // what is known before the walk; the four counters follow it
            sa_hip_token_cnf& h = g.heads[w];
            h.driver = driver;
            h.literals = d1 - d0;
            h.examined = examined;
            h.count = count;
            h.reserved = 0;
        }
        int32_t* const docs = g.docs + w * g.cap;
        int32_t* const offs = g.offsets + w * g.cap;
        u32 matched = 0, candidates = 0, duplicates = 0;
        u64 left = examined;
        for (u32 l = d0; l < d1 && left; ++l) {            // the driver's literals in order: an earlier one is walked whole first
            const u32 first_u = s_a[wv][l];
            const u32 have = s_end[wv][l] - first_u;
            const u32 take = have < left ? have : (u32)left;
            left -= take;
            const u32 end = first_u + take;                // <= n < 2^31
            const int32_t first = (int32_t)first_u;
            for (u32 a = first_u; a < end; a += (u32)(DOC_UNROLL * WAVE)) {   // (a + 256 < 2^32: no wrap)
                int32_t pv[DOC_UNROLL];
#pragma unroll
                for (int u = 0; u < DOC_UNROLL; ++u) {
                    const u32 r = a + (u32)u * WAVE + lane;
                    pv[u] = r < end ? d.pv[r] : 0x7FFFFFFF;                   // beyond the piece: never a first occurrence
                }
#pragma unroll 1
                for (int u = 0; u < DOC_UNROLL; ++u) {     // one copy of the probes: the window's PV by a select, not by an index
                    static_assert(DOC_UNROLL == 4, "the select below names every window");
                    const int32_t p = u == 0 ? pv[0] : u == 1 ? pv[1] : u == 2 ? pv[2] : pv[3];
                    const u32 r = a + (u32)u * WAVE + lane;
                    const bool head = r < end && p < first;
                    if (__ballot(head) == 0) continue;
                    bool dup = false, match = false;
                    int32_t doc = 0;
                    if (head) {                            // no cross-lane operation inside: the lanes diverge here
                        doc = d.da[r];
                        const u32 g0 = (u32)d.starts[doc], g1 = (u32)d.starts[doc + 1];
                        // pass 0: the driver's earlier literals [d0, l) as an exclusion (one of them holds it: a duplicate, the
                        // document was a candidate there); pass j + 1: clause j.  A positive clause stops at its first literal that
                        // holds the document, a negated one fails at it.
                        match = true;
                        for (u32 pass = 0; pass <= nc && match; ++pass) {
                            if (pass == driver + 1) continue;
                            const u32 j = pass ? pass - 1 : 0u;
                            const u32 e0 = pass ? s_cl[wv][j] : d0, e1 = pass ? s_cl[wv][j + 1] : l;
                            const bool neg = pass ? (negmask >> j) & 1 : true;
                            bool holds = false;
                            for (u32 e = e0; e < e1 && !holds; ++e)
                                holds = tq_cnf_holds(d.rk, g0, g1, s_a[wv][e], s_end[wv][e]);   // the same address in every lane
                            match = holds != neg;
                            if (pass == 0) dup = holds;
                        }
                    }
                    duplicates += (u32)__popcll(__ballot(dup));
                    candidates += (u32)__popcll(__ballot(head && !dup));
                    const u64 mb = __ballot(match);
                    if (mb == 0) continue;
                    const u32 slot = matched + (u32)__popcll(mb & lanemask_lt());
                    if (match && slot < g.cap) {
                        docs[slot] = doc;
                        offs[slot] = (int32_t)(x.sa[r] - (u32)d.starts[doc]);
                    }
                    matched += (u32)__popcll(mb);
                }
            }
        }
        if (lane == 0) {
            sa_hip_token_cnf& h = g.heads[w];
            h.written = matched < g.cap ? matched : g.cap;
            h.matched = matched;
            h.candidates = candidates;
            h.duplicates = duplicates;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// What can be told from the three tables alone (G >= 1; C and S below 2^31): the clause table cuts [0, S) into C clauses of >= 1
// literal, the group table cuts [0, C) into G groups of 1 .. CNF_MAX_CLAUSES clauses and at most CNF_MAX_LITERALS literals, negated
// (nullptr: none) holds 0 / 1 and leaves every group a positive clause.
inline int cnf_tables_check(const char* who, const uint64_t* coff, u64 C, u64 S, const uint8_t* negated, const uint64_t* goff, u64 G) {
    if (coff[0] != 0) return fail(SA_HIP_EINVAL, who, "clause_offsets[0] != 0");
    for (u64 c = 0; c < C; ++c)
        if (coff[c + 1] <= coff[c]) return fail(SA_HIP_EINVAL, who, "an empty clause (clause_offsets do not ascend)");
    if (coff[C] != S) return fail(SA_HIP_EINVAL, who, "clause_offsets do not end at S");
    if (negated)
        for (u64 c = 0; c < C; ++c)
            if (negated[c] > 1) return fail(SA_HIP_EINVAL, who, "negated holds 0 or 1");
    if (goff[0] != 0) return fail(SA_HIP_EINVAL, who, "group_offsets[0] != 0");
    for (u64 i = 0; i < G; ++i) {
        if (goff[i + 1] <= goff[i]) return fail(SA_HIP_EINVAL, who, "an empty group (group_offsets do not ascend)");
        if (goff[i + 1] > C) return fail(SA_HIP_EINVAL, who, "group_offsets do not end at C");
        if (goff[i + 1] - goff[i] > CNF_MAX_CLAUSES) return fail(SA_HIP_EINVAL, who, "a group of more than SA_HIP_TOKEN_CNF_MAX_CLAUSES clauses");
        if (coff[goff[i + 1]] - coff[goff[i]] > CNF_MAX_LITERALS)
            return fail(SA_HIP_EINVAL, who, "a group of more than SA_HIP_TOKEN_CNF_MAX_LITERALS literals");
        bool positive = !negated;
        for (u64 c = goff[i]; c < goff[i + 1] && !positive; ++c) positive = negated[c] == 0;
        if (!positive) return fail(SA_HIP_EINVAL, who, "a group with no positive clause");
    }
    if (goff[G] != C) return fail(SA_HIP_EINVAL, who, "group_offsets do not end at C");
    return 0;
}

// G >= 1 groups, G * cap < 2^31 (cap may be 0)
inline int launch_cnf(const Index& x, const Docs& d, const DocRanks& r, hipStream_t stream, const CnfArgs& g) {
    hipLaunchKernelGGL(tq_cnf_kernel, dim3(wave_row_grid(g.G)), dim3(NEXT_WAVES * WAVE), 0, stream, x.view(), r.view(d), g);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tq
}  // namespace sa
