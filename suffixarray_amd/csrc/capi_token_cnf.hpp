// capi_token_cnf.hpp -- the C ABI of CNF document queries (include/sa_hip.h section 6m), included by sa_capi.hip behind
// capi_token_all.hpp (same translation unit).  The kernel and the table check are csrc/token_cnf.hpp.
// Argument checks come first and touch neither the handle nor the device; the three host tables are checked by one function that the
// device form and the host form share; whether the handle has documents and RK is looked up under its mutex, still before any HIP
// call.  The tables travel through one pinned buffer of the handle, so the caller's arrays are free when the call returns and the
// launch stays asynchronous.  The stopwatch is a LaunchTimer member of the handle; cnf_batch returns through capi_token.hpp's
// token_rows_out.
#pragma once
#include "capi_token_all.hpp"
#include "token_cnf.hpp"

namespace {

// S, C and G as they are, the tables only when there are groups
int token_cnf_args(const char* who, u64 S, const uint64_t* coff, u64 C, const uint8_t* negated, const uint64_t* goff, u64 G, u32 cap) {
    if (S >= 0x80000000ull) return fail(SA_HIP_EINVAL, who, "S >= 2^31");
    if (C >= 0x80000000ull) return fail(SA_HIP_EINVAL, who, "C >= 2^31");
    if (G >= 0x80000000ull) return fail(SA_HIP_EINVAL, who, "G >= 2^31");
    int rc = token_cells_args(who, G, cap);
    if (rc || G == 0) return rc;
    if (!coff) return fail(SA_HIP_EINVAL, who, "NULL clause_offsets");
    if (!goff) return fail(SA_HIP_EINVAL, who, "NULL group_offsets");
    return tq::cnf_tables_check(who, coff, C, S, negated, goff, G);
}

// where the three checked tables lie in c_tab (and in its pinned twin): uint32 group offsets, uint32 clause offsets, the bytes
struct CnfTables {
    size_t goff, coff, neg, bytes;
    CnfTables(u64 C, u64 G) : goff(0), coff((size_t)(G + 1) * 4), neg(coff + (size_t)(C + 1) * 4), bytes(neg + (size_t)C) {}
};

int token_stage_cnf(sa_hip_token_index* t, const uint64_t* coff, u64 C, const uint8_t* negated, const uint64_t* goff, u64 G) {
    int rc;
    const CnfTables at(C, G);
    if (t->c_copy_pending) {
        SA_HIP_CHECK(hipEventSynchronize(t->c_copied));
        t->c_copy_pending = false;
    }
    if (t->c_pin_cap < at.bytes) {
        if (t->c_pin) (void)hipHostFree(t->c_pin);
        t->c_pin = nullptr; t->c_pin_cap = 0;
        SA_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&t->c_pin), at.bytes, hipHostMallocDefault));
        t->c_pin_cap = at.bytes;
    }
    if ((rc = t->c_tab.ensure(at.bytes))) return rc;
    u32* const pg = reinterpret_cast<u32*>(t->c_pin + at.goff);
    u32* const pc = reinterpret_cast<u32*>(t->c_pin + at.coff);
    for (u64 i = 0; i <= G; ++i) pg[i] = (u32)goff[i];
    for (u64 c = 0; c <= C; ++c) pc[c] = (u32)coff[c];
    if (negated) memcpy(t->c_pin + at.neg, negated, (size_t)C); else memset(t->c_pin + at.neg, 0, (size_t)C);
    SA_HIP_CHECK(hipMemcpyAsync(t->c_tab.p, t->c_pin, at.bytes, hipMemcpyHostToDevice, t->stream));
    SA_HIP_CHECK(hipEventRecord(t->c_copied, t->stream));
    t->c_copy_pending = true;
    return 0;
}

int token_launch_cnf(sa_hip_token_index* t, const sa_hip_token_span* spans, const uint64_t* coff, u64 C, const uint8_t* negated,
                     const uint64_t* goff, u64 G, u32 cap, u32 budget, int32_t* docs, int32_t* offs, sa_hip_token_cnf* heads) {
    int rc;
    if ((rc = token_stage_cnf(t, coff, C, negated, goff, G))) return rc;
    const CnfTables at(C, G);
    const unsigned char* const tab = t->c_tab.as<unsigned char>();
    const tq::CnfArgs g{spans, reinterpret_cast<const u32*>(tab + at.goff), reinterpret_cast<const u32*>(tab + at.coff), tab + at.neg, G, cap,
                        budget, docs, offs, heads};
    if ((rc = t->tm_cnf.begin(t->stream)) || (rc = tq::launch_cnf(t->x, t->docs, t->ranks, t->stream, g))) return rc;
    return t->tm_cnf.end(t->stream, G);
}

}  // namespace

extern "C" {

int sa_hip_token_index_cnf_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t S, const uint64_t* clause_offsets_host,
                                        uint64_t C, const uint8_t* negated_host, const uint64_t* group_offsets_host, uint64_t G,
                                        uint32_t cap, uint32_t budget, void* docs_dev, void* offsets_dev, void* heads_dev) {
    const char* who = "sa_hip_token_index_cnf_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_cnf_args(who, S, clause_offsets_host, C, negated_host, group_offsets_host, G, cap);
    if (rc || G == 0) return rc;
    if (!spans_dev || !heads_dev || (cap && (!docs_dev || !offsets_dev))) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = token_has_ranks(t, who)) || (rc = set_device(t->device))) return rc;
    return token_launch_cnf(t, static_cast<const sa_hip_token_span*>(spans_dev), clause_offsets_host, C, negated_host, group_offsets_host, G,
                            cap, budget, static_cast<int32_t*>(docs_dev), static_cast<int32_t*>(offsets_dev),
                            static_cast<sa_hip_token_cnf*>(heads_dev));
}

int sa_hip_token_index_cnf_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t S,
                                 const uint64_t* clause_offsets, uint64_t C, const uint8_t* negated, const uint64_t* group_offsets,
                                 uint64_t G, int mode, uint32_t max_length, int need_next, uint32_t cap, uint32_t budget,
                                 sa_hip_token_span* spans, int32_t* docs, int32_t* offs, sa_hip_token_cnf* heads) {
    const char* who = "sa_hip_token_index_cnf_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_cnf_args(who, S, clause_offsets, C, negated, group_offsets, G, cap)) || G == 0) return rc;
    if (!offsets || !heads || (cap && (!docs || !offs))) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, S))) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = token_has_ranks(t, who)) || (rc = set_device(t->device))) return rc;
    const size_t cells = (size_t)G * cap;
    if ((rc = t->d_docs.ensure(cells * 4)) || (rc = t->d_offs.ensure(cells * 4)) || (rc = t->d_heads.ensure((size_t)G * sizeof(sa_hip_token_cnf)))) return rc;
    if ((rc = token_stage_spans(t, patterns, offsets, S, mode, max_length, need_next))) return rc;
    if (spans) SA_HIP_CHECK(hipMemcpyAsync(spans, t->s_spans.p, (size_t)S * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, t->stream));
    if ((rc = token_launch_cnf(t, t->s_spans.as<sa_hip_token_span>(), clause_offsets, C, negated, group_offsets, G, cap, budget,
                               cap ? t->d_docs.as<int32_t>() : nullptr, cap ? t->d_offs.as<int32_t>() : nullptr,
                               t->d_heads.as<sa_hip_token_cnf>()))) return rc;
    return token_rows_out(t->stream, who, G, cap, t->d_heads.p, heads, t->d_docs.p, docs, t->d_offs.p, offs);
}

int sa_hip_token_index_cnf_info(const sa_hip_token_index* ct, sa_hip_token_cnf_info* out) {
    if (!ct || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_index_cnf_info", "NULL argument");
    sa_hip_token_index* t = const_cast<sa_hip_token_index*>(ct);
    std::lock_guard<std::mutex> g(t->mu);
    if (t->tm_cnf.pending) {
        int rc = set_device(t->device);
        if (rc || (rc = t->tm_cnf.resolve())) return rc;
    }
    memset(out, 0, sizeof *out);
    out->q = t->tm_cnf.q;
    out->ms = t->tm_cnf.ms;
    return 0;
}

}  // extern "C"
