// capi_token_docs.hpp -- the C ABI of a token index's documents (include/sa_hip.h section 6d), included by sa_capi.hip behind
// capi_token.hpp (same translation unit).  The structures and the kernels are csrc/token_docs.hpp.
// Argument checks come first and touch neither the handle nor the device; whether the handle has documents is looked up under its
// mutex, still before any HIP call.  The two stopwatches are LaunchTimer members of the handle (launch_timer.hpp), the contexts of a
// host form go up through token_stage_spans, and the heads and written rows come back through token_rows_out (both capi_token.hpp's).
#pragma once
#include "capi_token.hpp"
#include "token_docs.hpp"

namespace {

// cap == 0 is the caller's to refuse (locate) or to allow (docs)
int token_cells_args(const char* who, u64 Q, u32 cap) {
    if (cap && (Q > 0x7FFFFFFFull / cap || Q * cap >= 0x80000000ull)) return fail(SA_HIP_EINVAL, who, "Q * cap >= 2^31");
    return 0;
}
int token_has_docs(const sa_hip_token_index* t, const char* who) {
    return t->docs.D ? 0 : fail(SA_HIP_EINVAL, who, "the handle has no documents (sa_hip_token_index_set_documents)");
}

int token_launch_locate(sa_hip_token_index* t, const sa_hip_token_span* spans, u64 Q, u32 cap, int32_t* docs, int32_t* offs,
                        sa_hip_token_locate* heads) {
    const tq::LocateArgs g{spans, Q, cap, docs, offs, heads};
    int rc;
    if ((rc = t->tm_lc.begin(t->stream)) || (rc = tq::launch_locate(t->x, t->docs, t->stream, g))) return rc;
    return t->tm_lc.end(t->stream, Q);
}

int token_launch_docs(sa_hip_token_index* t, const sa_hip_token_span* spans, u64 Q, u32 cap, u32 budget, int32_t* docs, int32_t* offs,
                      sa_hip_token_docs* heads) {
    const tq::DocsArgs g{spans, Q, cap, budget, docs, offs, heads, t->docs.sum.as<unsigned long long>()};
    int rc;
    if ((rc = t->tm_dc.begin(t->stream)) || (rc = tq::launch_docs(t->x, t->docs, t->stream, g))) return rc;
    return t->tm_dc.end(t->stream, Q);
}

}  // namespace

extern "C" {

int sa_hip_token_index_set_documents(sa_hip_token_index* t, const int32_t* doc_starts_host, uint32_t D) {
    const char* who = "sa_hip_token_index_set_documents";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (D == 0 && doc_starts_host) return fail(SA_HIP_EINVAL, who, "D == 0 (a NULL table with D == 0 removes the documents)");
    if (D != 0 && !doc_starts_host) return fail(SA_HIP_EINVAL, who, "NULL doc_starts");
    int rc;
    if (D && (rc = tq::docs_table_check(who, doc_starts_host, D))) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if (D && (u32)doc_starts_host[D - 1] > t->x.n) return fail(SA_HIP_EINVAL, who, "doc_starts beyond the text");
    ++t->docs_gen;                                       // whatever follows: a shard set that recorded the old one asks again
    if (D == 0 && t->docs.D == 0) return 0;
    if ((rc = set_device(t->device))) return rc;
    if (D == 0) {
        SA_HIP_CHECK(hipStreamSynchronize(t->stream));   // launches that read the table
        t->docs.clear();
        if (t->ranks.have) ++t->ranks_gen;
        t->ranks.clear();
        return 0;
    }
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));       // launches that read the rank-by-document array of the table being replaced
    if (t->ranks.have) ++t->ranks_gen;
    t->ranks.clear();
    return t->docs.build(t->x, t->stream, doc_starts_host, D, who);
}

int sa_hip_token_index_get_doc_range(sa_hip_token_index* t, uint64_t first, uint64_t count, int32_t* docs_out, int32_t* prev_out) {
    const char* who = "sa_hip_token_index_get_doc_range";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    std::lock_guard<std::mutex> g(t->mu);
    int rc = token_has_docs(t, who);
    if (rc) return rc;
    if (first > t->x.n || count > t->x.n - first) return fail(SA_HIP_EINVAL, who, "range beyond the suffix array");
    if (count == 0 || (!docs_out && !prev_out)) return 0;
    if ((rc = set_device(t->device))) return rc;
    if (docs_out) SA_HIP_CHECK(hipMemcpyAsync(docs_out, t->docs.da.as<int32_t>() + first, (size_t)count * 4, hipMemcpyDeviceToHost, t->stream));
    if (prev_out) SA_HIP_CHECK(hipMemcpyAsync(prev_out, t->docs.pv.as<int32_t>() + first, (size_t)count * 4, hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    return 0;
}

int sa_hip_token_index_docs_info(const sa_hip_token_index* ct, sa_hip_token_docs_info* out) {
    if (!ct || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_index_docs_info", "NULL argument");
    sa_hip_token_index* t = const_cast<sa_hip_token_index*>(ct);
    std::lock_guard<std::mutex> g(t->mu);
    if (t->tm_lc.pending || t->tm_dc.pending) {
        int rc = set_device(t->device);
        if (rc || (rc = t->tm_lc.resolve())) return rc;
        if (t->tm_dc.pending) {
            unsigned long long sum = 0;
            if (t->docs.sum.p) {
                SA_HIP_CHECK(hipMemcpyAsync(&sum, t->docs.sum.p, sizeof sum, hipMemcpyDeviceToHost, t->stream));
                SA_HIP_CHECK(hipStreamSynchronize(t->stream));
            }
            if ((rc = t->tm_dc.resolve())) return rc;
            t->dc_examined = sum;
        }
    }
    memset(out, 0, sizeof *out);
    out->documents = t->docs.D;
    out->bytes = t->docs.bytes;
    out->prepare_ms = t->docs.prepare_ms;
    out->da_ms = t->docs.da_ms;
    out->sort_ms = t->docs.sort_ms;
    out->pv_ms = t->docs.pv_ms;
    out->sort_passes = t->docs.passes;
    out->locate_q = t->tm_lc.q;
    out->locate_ms = t->tm_lc.ms;
    out->docs_q = t->tm_dc.q;
    out->docs_ms = t->tm_dc.ms;
    out->examined = t->dc_examined;
    return 0;
}

int sa_hip_token_index_locate_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, uint32_t cap, void* docs_dev,
                                           void* offsets_dev, void* heads_dev) {
    const char* who = "sa_hip_token_index_locate_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (cap == 0) return fail(SA_HIP_EINVAL, who, "cap == 0");
    int rc = token_cells_args(who, Q, cap);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !docs_dev || !offsets_dev || !heads_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = token_has_docs(t, who)) || (rc = set_device(t->device))) return rc;
    return token_launch_locate(t, static_cast<const sa_hip_token_span*>(spans_dev), Q, cap, static_cast<int32_t*>(docs_dev),
                               static_cast<int32_t*>(offsets_dev), static_cast<sa_hip_token_locate*>(heads_dev));
}

int sa_hip_token_index_locate_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, uint32_t cap,
                                    sa_hip_token_span* spans, int32_t* docs, int32_t* offs, sa_hip_token_locate* heads) {
    const char* who = "sa_hip_token_index_locate_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (cap == 0) return fail(SA_HIP_EINVAL, who, "cap == 0");
    int rc = token_cells_args(who, Q, cap);
    if (rc || Q == 0) return rc;
    if (!offsets || !docs || !offs || !heads) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = token_has_docs(t, who)) || (rc = set_device(t->device))) return rc;
    const size_t cells = (size_t)Q * cap;
    if ((rc = t->d_docs.ensure(cells * 4)) || (rc = t->d_offs.ensure(cells * 4)) || (rc = t->d_heads.ensure((size_t)Q * sizeof(sa_hip_token_docs)))) return rc;
    if ((rc = token_stage_spans(t, patterns, offsets, Q, 0, 0, 0))) return rc;
    if (spans) SA_HIP_CHECK(hipMemcpyAsync(spans, t->s_spans.p, (size_t)Q * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, t->stream));
    if ((rc = token_launch_locate(t, t->s_spans.as<sa_hip_token_span>(), Q, cap, t->d_docs.as<int32_t>(), t->d_offs.as<int32_t>(),
                                  t->d_heads.as<sa_hip_token_locate>()))) return rc;
    return token_rows_out(t->stream, who, Q, cap, t->d_heads.p, heads, t->d_docs.p, docs, t->d_offs.p, offs);
}

int sa_hip_token_index_docs_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, uint32_t cap, uint32_t budget,
                                         void* docs_dev, void* offsets_dev, void* heads_dev) {
    const char* who = "sa_hip_token_index_docs_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_cells_args(who, Q, cap);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !heads_dev || (cap && (!docs_dev || !offsets_dev))) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = token_has_docs(t, who)) || (rc = set_device(t->device))) return rc;
    return token_launch_docs(t, static_cast<const sa_hip_token_span*>(spans_dev), Q, cap, budget, static_cast<int32_t*>(docs_dev),
                             static_cast<int32_t*>(offsets_dev), static_cast<sa_hip_token_docs*>(heads_dev));
}

int sa_hip_token_index_docs_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                  uint32_t max_length, int need_next, uint32_t cap, uint32_t budget, sa_hip_token_span* spans,
                                  int32_t* docs, int32_t* offs, sa_hip_token_docs* heads) {
    const char* who = "sa_hip_token_index_docs_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_cells_args(who, Q, cap)) || Q == 0) return rc;
    if (!offsets || !heads || (cap && (!docs || !offs))) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = token_has_docs(t, who)) || (rc = set_device(t->device))) return rc;
    const size_t cells = (size_t)Q * cap;
    if ((rc = t->d_docs.ensure(cells * 4)) || (rc = t->d_offs.ensure(cells * 4)) || (rc = t->d_heads.ensure((size_t)Q * sizeof(sa_hip_token_docs)))) return rc;
    if ((rc = token_stage_spans(t, patterns, offsets, Q, mode, max_length, need_next))) return rc;
    if (spans) SA_HIP_CHECK(hipMemcpyAsync(spans, t->s_spans.p, (size_t)Q * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, t->stream));
    if ((rc = token_launch_docs(t, t->s_spans.as<sa_hip_token_span>(), Q, cap, budget, cap ? t->d_docs.as<int32_t>() : nullptr,
                                cap ? t->d_offs.as<int32_t>() : nullptr, t->d_heads.as<sa_hip_token_docs>()))) return rc;
    return token_rows_out(t->stream, who, Q, cap, t->d_heads.p, heads, t->d_docs.p, docs, t->d_offs.p, offs);
}

}  // extern "C"
