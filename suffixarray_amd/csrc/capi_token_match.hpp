// capi_token_match.hpp -- the C ABI of matching statistics over a token index (include/sa_hip.h section 6f), included by sa_capi.hip
// behind capi_token_all.hpp (same translation unit).  The kernels are csrc/token_match.hpp.
// Argument checks come first and touch neither the handle nor the device.  The two stopwatches are LaunchTimer members of the handle
// (launch_timer.hpp), the documents of a host form go up through token_upload, and the heads and written rows come back through
// token_rows_out (capi_token.hpp).
#pragma once
#include "capi_token_docs.hpp"
#include "token_match.hpp"

namespace {

int token_match_total(const char* who, u64 total) {
    return total >= 0x80000000ull ? fail(SA_HIP_EINVAL, who, "total >= 2^31 positions") : 0;
}
int token_match_docs_args(const char* who, u64 Q, u32 min_length, u32 cap) {
    if (min_length == 0) return fail(SA_HIP_EINVAL, who, "min_length == 0");
    return token_cells_args(who, Q, cap);
}

// total >= 1
int token_launch_match(sa_hip_token_index* t, const int32_t* pat, const u64* off, u64 Q, u64 total, u32 max_length,
                       sa_hip_token_span* spans) {
    const tq::MatchArgs g{pat, off, Q, total, max_length, spans};
    int rc;
    if ((rc = t->tm_mt.begin(t->stream)) || (rc = tq::launch_match(t->x, t->stream, g)) || (rc = t->tm_mt.end(t->stream, total))) return rc;
    t->m_last = Q;
    return 0;
}

int token_launch_match_docs(sa_hip_token_index* t, const sa_hip_token_span* spans, const u64* off, u64 Q, u32 min_length, u32 cap,
                            u32* positions, sa_hip_token_span* out_spans, sa_hip_token_match_head* heads) {
    const tq::MatchDocsArgs<sa_hip_token_span> g{spans, off, Q, min_length, cap, positions, out_spans, heads};
    int rc;
    if ((rc = t->tm_md.begin(t->stream)) || (rc = tq::launch_match_docs(t->stream, g)) || (rc = t->tm_md.end(t->stream, Q))) return rc;
    t->m_last = Q;
    return 0;
}

// documents from the host into the handle's staging buffers, their matches into m_spans
int token_stage_match(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, u64 Q, u32 max_length) {
    int rc;
    const u64 total = offsets[Q];
    if ((rc = t->m_spans.ensure((size_t)total * sizeof(sa_hip_token_span) + 64)) ||
        (rc = token_upload(t->q_pat, t->q_off, t->stream, patterns, offsets, Q))) return rc;
    if (total == 0) return 0;
    return token_launch_match(t, t->q_pat.as<int32_t>(), t->q_off.as<u64>(), Q, total, max_length, t->m_spans.as<sa_hip_token_span>());
}

}  // namespace

extern "C" {

int sa_hip_token_index_match_batch_device(sa_hip_token_index* t, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                          uint64_t total, uint32_t max_length, void* spans_dev) {
    const char* who = "sa_hip_token_index_match_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_match_total(who, total);
    if (rc || Q == 0) return rc;
    if (!offsets_dev || (total && (!patterns_dev || !spans_dev))) return fail(SA_HIP_EINVAL, who, "NULL argument");
    if (total == 0) return 0;                            // a batch of empty documents: no position to answer
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    return token_launch_match(t, static_cast<const int32_t*>(patterns_dev), static_cast<const u64*>(offsets_dev), Q, total, max_length,
                              static_cast<sa_hip_token_span*>(spans_dev));
}

int sa_hip_token_index_match_docs_batch_device(sa_hip_token_index* t, const void* spans_dev, const void* offsets_dev, uint64_t Q,
                                               uint32_t min_length, uint32_t cap, void* positions_dev, void* out_spans_dev,
                                               void* heads_dev) {
    const char* who = "sa_hip_token_index_match_docs_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_match_docs_args(who, Q, min_length, cap);
    if (rc || Q == 0) return rc;
    // (spans may be NULL: a batch of empty documents has none)
    if (!offsets_dev || !heads_dev || (cap && (!positions_dev || !out_spans_dev))) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    return token_launch_match_docs(t, static_cast<const sa_hip_token_span*>(spans_dev), static_cast<const u64*>(offsets_dev), Q, min_length,
                                   cap, static_cast<u32*>(positions_dev), static_cast<sa_hip_token_span*>(out_spans_dev),
                                   static_cast<sa_hip_token_match_head*>(heads_dev));
}

int sa_hip_token_index_match_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                   uint32_t max_length, sa_hip_token_span* spans) {
    const char* who = "sa_hip_token_index_match_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (Q == 0) return 0;
    if (!offsets) return fail(SA_HIP_EINVAL, who, "NULL argument");
    int rc = token_offsets_args(who, patterns, offsets, Q);
    if (rc || (rc = token_match_total(who, offsets[Q]))) return rc;
    const u64 total = offsets[Q];
    if (total == 0) return 0;
    if (!spans) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    if ((rc = token_stage_match(t, patterns, offsets, Q, max_length))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(spans, t->m_spans.p, (size_t)total * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    return 0;
}

int sa_hip_token_index_match_docs_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                        uint32_t max_length, uint32_t min_length, uint32_t cap, sa_hip_token_span* spans,
                                        uint32_t* positions, sa_hip_token_span* out_spans, sa_hip_token_match_head* heads) {
    const char* who = "sa_hip_token_index_match_docs_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_match_docs_args(who, Q, min_length, cap);
    if (rc || Q == 0) return rc;
    if (!offsets || !heads || (cap && (!positions || !out_spans))) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q)) || (rc = token_match_total(who, offsets[Q]))) return rc;
    const u64 total = offsets[Q];
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    const size_t cells = (size_t)Q * cap;
    if ((rc = t->m_pos.ensure(cells * 4)) || (rc = t->m_out.ensure(cells * sizeof(sa_hip_token_span))) ||
        (rc = t->m_heads.ensure((size_t)Q * sizeof(sa_hip_token_match_head)))) return rc;
    if ((rc = token_stage_match(t, patterns, offsets, Q, max_length))) return rc;
    if (spans && total) SA_HIP_CHECK(hipMemcpyAsync(spans, t->m_spans.p, (size_t)total * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, t->stream));
    if ((rc = token_launch_match_docs(t, t->m_spans.as<sa_hip_token_span>(), t->q_off.as<u64>(), Q, min_length, cap,
                                      cap ? t->m_pos.as<u32>() : nullptr, cap ? t->m_out.as<sa_hip_token_span>() : nullptr,
                                      t->m_heads.as<sa_hip_token_match_head>()))) return rc;
    return token_rows_out(t->stream, who, Q, cap, t->m_heads.p, heads, t->m_pos.p, positions, t->m_out.p, out_spans);
}

int sa_hip_token_index_match_info(const sa_hip_token_index* ct, sa_hip_token_match_info* out) {
    if (!ct || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_index_match_info", "NULL argument");
    sa_hip_token_index* t = const_cast<sa_hip_token_index*>(ct);
    std::lock_guard<std::mutex> g(t->mu);
    if (t->tm_mt.pending || t->tm_md.pending) {
        int rc = set_device(t->device);
        if (rc || (rc = t->tm_mt.resolve()) || (rc = t->tm_md.resolve())) return rc;
    }
    memset(out, 0, sizeof *out);
    out->q = t->m_last;
    out->positions = t->tm_mt.q;
    out->match_ms = t->tm_mt.ms;
    out->docs_ms = t->tm_md.ms;
    return 0;
}

}  // extern "C"
