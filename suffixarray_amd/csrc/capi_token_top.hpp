// capi_token_top.hpp -- the C ABI of top-k next symbols and of draws from a span over a token index (include/sa_hip.h section 6k),
// included by sa_capi.hip behind capi_token_score.hpp (same translation unit).  The kernels are csrc/token_top.hpp.
// Argument checks come first and touch neither the handle nor the device.  The two stopwatches are LaunchTimer members of the handle
// (launch_timer.hpp); the host forms take the contexts up and the spans through capi_token.hpp's token_stage_spans, stage in the
// buffers of the next-symbol host forms (s_sym, s_cnt, s_heads) and return heads and rows through token_rows_out.
#pragma once
#include "capi_token.hpp"
#include "token_top.hpp"

namespace {

int token_top_args(const char* who, u64 Q, u32 k) {
    if (k == 0 || k > tq::TOP_MAX) return fail(SA_HIP_EINVAL, who, "k is 1 .. 64");
    if (Q > 0x7FFFFFFFull / k || Q * k >= 0x80000000ull) return fail(SA_HIP_EINVAL, who, "Q * k >= 2^31");
    return 0;
}
int token_sample_args(const char* who, u64 Q, u32 m) {
    if (m == 0) return fail(SA_HIP_EINVAL, who, "m == 0");
    if (Q > 0x7FFFFFFFull / m || Q * m >= 0x80000000ull) return fail(SA_HIP_EINVAL, who, "Q * m >= 2^31");
    return 0;
}

int token_launch_top(sa_hip_token_index* t, const sa_hip_token_span* spans, u64 Q, u32 k, u32 budget, int32_t* symbols, u32* counts,
                     sa_hip_token_top* heads) {
    const tq::TopArgs g{spans, Q, k, budget, symbols, counts, heads};
    int rc;
    if ((rc = t->tm_tp.begin(t->stream)) || (rc = tq::launch_top(t->x, t->stream, t->next_knobs, g)) || (rc = t->tm_tp.end(t->stream, Q))) return rc;
    t->tp_last = Q;
    return 0;
}

int token_launch_sample(sa_hip_token_index* t, const sa_hip_token_span* spans, u64 Q, const u64* draws, u32 m, int32_t* symbols, u32* ranks) {
    const tq::SampleArgs g{spans, Q, m, draws, symbols, ranks};
    int rc;
    if ((rc = t->tm_sm.begin(t->stream)) || (rc = tq::launch_sample(t->x, t->stream, g)) || (rc = t->tm_sm.end(t->stream, Q))) return rc;
    t->tp_last = Q;
    return 0;
}

}  // namespace

extern "C" {

int sa_hip_token_index_top_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, uint32_t k, uint32_t budget,
                                        void* symbols_dev, void* counts_dev, void* heads_dev) {
    const char* who = "sa_hip_token_index_top_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_top_args(who, Q, k);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !symbols_dev || !counts_dev || !heads_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    return token_launch_top(t, static_cast<const sa_hip_token_span*>(spans_dev), Q, k, budget, static_cast<int32_t*>(symbols_dev),
                            static_cast<u32*>(counts_dev), static_cast<sa_hip_token_top*>(heads_dev));
}

int sa_hip_token_index_top_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                 uint32_t max_length, int need_next, uint32_t k, uint32_t budget, sa_hip_token_span* spans,
                                 int32_t* symbols, uint32_t* counts, sa_hip_token_top* heads) {
    const char* who = "sa_hip_token_index_top_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_top_args(who, Q, k)) || Q == 0) return rc;
    if (!offsets || !symbols || !counts || !heads) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    if ((rc = token_stage_spans(t, patterns, offsets, Q, mode, max_length, need_next))) return rc;
    if (spans) SA_HIP_CHECK(hipMemcpyAsync(spans, t->s_spans.p, (size_t)Q * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, t->stream));
    const size_t cells = (size_t)Q * k;
    if ((rc = t->s_sym.ensure(cells * 4)) || (rc = t->s_cnt.ensure(cells * 4)) || (rc = t->s_heads.ensure((size_t)Q * sizeof(sa_hip_token_top)))) return rc;
    if ((rc = token_launch_top(t, t->s_spans.as<sa_hip_token_span>(), Q, k, budget, t->s_sym.as<int32_t>(), t->s_cnt.as<u32>(),
                               t->s_heads.as<sa_hip_token_top>()))) return rc;
    return token_rows_out(t->stream, who, Q, k, t->s_heads.p, heads, t->s_sym.p, symbols, t->s_cnt.p, counts);
}

int sa_hip_token_index_sample_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, const void* draws_dev, uint32_t m,
                                           void* symbols_dev, void* ranks_dev) {
    const char* who = "sa_hip_token_index_sample_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_sample_args(who, Q, m);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !draws_dev || !symbols_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (ranks may be NULL)
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    return token_launch_sample(t, static_cast<const sa_hip_token_span*>(spans_dev), Q, static_cast<const u64*>(draws_dev), m,
                               static_cast<int32_t*>(symbols_dev), static_cast<u32*>(ranks_dev));
}

int sa_hip_token_index_sample_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                    uint32_t max_length, int need_next, const uint64_t* draws, uint32_t m, sa_hip_token_span* spans,
                                    int32_t* symbols, uint32_t* ranks) {
    const char* who = "sa_hip_token_index_sample_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_sample_args(who, Q, m)) || Q == 0) return rc;
    if (!offsets || !draws || !symbols) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans and ranks may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    const size_t cells = (size_t)Q * m;
    if ((rc = t->tp_draws.ensure(cells * 8)) || (rc = t->s_sym.ensure(cells * 4)) || (rc = t->s_cnt.ensure(cells * 4))) return rc;
    if ((rc = token_stage_spans(t, patterns, offsets, Q, mode, max_length, need_next))) return rc;
    if (spans) SA_HIP_CHECK(hipMemcpyAsync(spans, t->s_spans.p, (size_t)Q * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipMemcpyAsync(t->tp_draws.p, draws, cells * 8, hipMemcpyHostToDevice, t->stream));
    if ((rc = token_launch_sample(t, t->s_spans.as<sa_hip_token_span>(), Q, t->tp_draws.as<u64>(), m, t->s_sym.as<int32_t>(),
                                  ranks ? t->s_cnt.as<u32>() : nullptr))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(symbols, t->s_sym.p, cells * 4, hipMemcpyDeviceToHost, t->stream));   // every cell is written
    if (ranks) SA_HIP_CHECK(hipMemcpyAsync(ranks, t->s_cnt.p, cells * 4, hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    return 0;
}

int sa_hip_token_index_top_info(const sa_hip_token_index* ct, sa_hip_token_top_info* out) {
    if (!ct || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_index_top_info", "NULL argument");
    sa_hip_token_index* t = const_cast<sa_hip_token_index*>(ct);
    std::lock_guard<std::mutex> g(t->mu);
    if (t->tm_sp.pending || t->tm_tp.pending || t->tm_sm.pending) {
        int rc = set_device(t->device);
        if (rc || (rc = t->tm_sp.resolve()) || (rc = t->tm_tp.resolve()) || (rc = t->tm_sm.resolve())) return rc;
    }
    memset(out, 0, sizeof *out);
    out->q = t->tp_last;
    out->spans_ms = t->tm_sp.ms;
    out->top_ms = t->tm_tp.ms;
    out->sample_ms = t->tm_sm.ms;
    return 0;
}

}  // extern "C"
