// capi_token_score.hpp -- the C ABI of infinity-gram scores over a token index (include/sa_hip.h section 6i), included by sa_capi.hip
// behind capi_token_match.hpp (same translation unit).  The kernels are csrc/token_score.hpp.
// Argument checks come first and touch neither the handle nor the device.  The two stopwatches are LaunchTimer members of the handle
// (launch_timer.hpp), the match launch of the host form is capi_token_match.hpp's with its stopwatch and its buffer, and the documents
// of the host form go up through token_upload.
#pragma once
#include "capi_token_match.hpp"
#include "token_score.hpp"

namespace {

// which way the host form takes: true runs the match launch first and hands its records to the score launch (DESIGN.md 9s has the
// measurement behind the choice)
constexpr bool SCORE_HOST_MATCHES = true;

// total >= 1
int token_launch_score(sa_hip_token_index* t, const int32_t* pat, const u64* off, u64 Q, u64 total, u32 max_length,
                       const sa_hip_token_span* ms, sa_hip_token_score* scores) {
    const tq::ScoreArgs g{pat, off, Q, total, max_length, ms, scores};
    int rc;
    if ((rc = t->tm_sc.begin(t->stream)) || (rc = tq::launch_score(t->x, t->stream, g)) || (rc = t->tm_sc.end(t->stream, total))) return rc;
    t->sc_last = Q;
    return 0;
}

int token_launch_score_docs(sa_hip_token_index* t, const sa_hip_token_score* scores, const u64* off, u64 Q, sa_hip_token_score_head* heads) {
    const tq::ScoreDocsArgs g{scores, off, Q, heads};
    int rc;
    if ((rc = t->tm_sd.begin(t->stream)) || (rc = tq::launch_score_docs(t->stream, g)) || (rc = t->tm_sd.end(t->stream, Q))) return rc;
    t->sc_last = Q;
    return 0;
}

}  // namespace

extern "C" {

int sa_hip_token_index_score_batch_device(sa_hip_token_index* t, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                          uint64_t total, uint32_t max_length, const void* spans_dev, void* scores_dev) {
    const char* who = "sa_hip_token_index_score_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_match_total(who, total);
    if (rc || Q == 0) return rc;
    if (!offsets_dev || (total && (!patterns_dev || !scores_dev))) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL: way 2)
    if (total == 0) return 0;                            // a batch of empty documents: no position to answer
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    return token_launch_score(t, static_cast<const int32_t*>(patterns_dev), static_cast<const u64*>(offsets_dev), Q, total, max_length,
                              static_cast<const sa_hip_token_span*>(spans_dev), static_cast<sa_hip_token_score*>(scores_dev));
}

int sa_hip_token_index_score_docs_batch_device(sa_hip_token_index* t, const void* scores_dev, const void* offsets_dev, uint64_t Q,
                                               void* heads_dev) {
    const char* who = "sa_hip_token_index_score_docs_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (Q == 0) return 0;
    if (!offsets_dev || !heads_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (scores may be NULL: a batch of empty documents has none)
    std::lock_guard<std::mutex> g(t->mu);
    int rc = set_device(t->device);
    if (rc) return rc;
    return token_launch_score_docs(t, static_cast<const sa_hip_token_score*>(scores_dev), static_cast<const u64*>(offsets_dev), Q,
                                   static_cast<sa_hip_token_score_head*>(heads_dev));
}

int sa_hip_token_index_score_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                   uint32_t max_length, sa_hip_token_score* scores, sa_hip_token_score_head* heads) {
    const char* who = "sa_hip_token_index_score_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (Q == 0) return 0;
    if (!offsets || (!scores && !heads)) return fail(SA_HIP_EINVAL, who, "NULL argument");
    int rc = token_offsets_args(who, patterns, offsets, Q);
    if (rc || (rc = token_match_total(who, offsets[Q]))) return rc;
    const u64 total = offsets[Q];
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    if ((rc = t->sc_scores.ensure((size_t)total * sizeof(sa_hip_token_score) + 64)) ||
        (rc = t->sc_heads.ensure((size_t)Q * sizeof(sa_hip_token_score_head)))) return rc;
    if (SCORE_HOST_MATCHES) rc = token_stage_match(t, patterns, offsets, Q, max_length);
    else rc = token_upload(t->q_pat, t->q_off, t->stream, patterns, offsets, Q);
    if (rc) return rc;
    if (total) {
        if ((rc = token_launch_score(t, t->q_pat.as<int32_t>(), t->q_off.as<u64>(), Q, total, max_length,
                                     SCORE_HOST_MATCHES ? t->m_spans.as<sa_hip_token_span>() : nullptr,
                                     t->sc_scores.as<sa_hip_token_score>()))) return rc;
        if (scores) SA_HIP_CHECK(hipMemcpyAsync(scores, t->sc_scores.p, (size_t)total * sizeof(sa_hip_token_score), hipMemcpyDeviceToHost, t->stream));
    }
    if (heads) {
        if ((rc = token_launch_score_docs(t, t->sc_scores.as<sa_hip_token_score>(), t->q_off.as<u64>(), Q,
                                          t->sc_heads.as<sa_hip_token_score_head>()))) return rc;
        SA_HIP_CHECK(hipMemcpyAsync(heads, t->sc_heads.p, (size_t)Q * sizeof(sa_hip_token_score_head), hipMemcpyDeviceToHost, t->stream));
    }
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    return 0;
}

int sa_hip_token_index_score_info(const sa_hip_token_index* ct, sa_hip_token_score_info* out) {
    if (!ct || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_index_score_info", "NULL argument");
    sa_hip_token_index* t = const_cast<sa_hip_token_index*>(ct);
    std::lock_guard<std::mutex> g(t->mu);
    if (t->tm_mt.pending || t->tm_sc.pending || t->tm_sd.pending) {
        int rc = set_device(t->device);
        if (rc || (rc = t->tm_mt.resolve()) || (rc = t->tm_sc.resolve()) || (rc = t->tm_sd.resolve())) return rc;
    }
    memset(out, 0, sizeof *out);
    out->q = t->sc_last;
    out->positions = t->tm_sc.q;
    out->match_ms = t->tm_mt.ms;
    out->score_ms = t->tm_sc.ms;
    out->docs_ms = t->tm_sd.ms;
    return 0;
}

}  // extern "C"
