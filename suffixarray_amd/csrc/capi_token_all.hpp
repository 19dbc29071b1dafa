// capi_token_all.hpp -- the C ABI of per-document counts and of the documents that hold all n-grams of a group
// (include/sa_hip.h section 6e), included by sa_capi.hip behind capi_token_docs.hpp (same translation unit).  The rank-by-document
// array and the kernels are csrc/token_all.hpp.
// Argument checks come first and touch neither the handle nor the device; whether the handle has documents and the array is looked
// up under its mutex, still before any HIP call.  The two stopwatches are LaunchTimer members of the handle (launch_timer.hpp); the
// host doc_counts form moves the caller's rows in and the counts out with copy_written_rows (host_rows.hpp), all_batch returns
// through capi_token.hpp's token_rows_out.
#pragma once
#include "capi_token_docs.hpp"
#include "token_all.hpp"

namespace {

int token_has_ranks(const sa_hip_token_index* t, const char* who) {
    const int rc = token_has_docs(t, who);
    if (rc) return rc;
    return t->ranks.have ? 0 : fail(SA_HIP_EINVAL, who, "the handle has no rank-by-document array (sa_hip_token_index_prepare_doc_ranks)");
}

int token_counts_args(const char* who, u64 Q, u32 cap, const void* written, u64 stride) {
    if (cap == 0) return fail(SA_HIP_EINVAL, who, "cap == 0");
    if (written && (stride < 4 || (stride & 3))) return fail(SA_HIP_EINVAL, who, "written_stride is a multiple of 4, at least 4");
    return token_cells_args(who, Q, cap);
}

// S and G as they are, the table only when there are groups
int token_all_args(const char* who, u64 S, const uint64_t* goff, u64 G, u32 cap) {
    if (S >= 0x80000000ull) return fail(SA_HIP_EINVAL, who, "S >= 2^31");
    if (G >= 0x80000000ull) return fail(SA_HIP_EINVAL, who, "G >= 2^31");
    int rc = token_cells_args(who, G, cap);
    if (rc || G == 0) return rc;
    if (!goff) return fail(SA_HIP_EINVAL, who, "NULL group_offsets");
    return tq::all_groups_check(who, goff, S, G);
}

int token_launch_tf(sa_hip_token_index* t, const sa_hip_token_span* spans, u64 Q, u32 cap, const int32_t* docs, const void* written,
                    u64 stride, u32* counts) {
    const tq::TfArgs g{spans, Q, cap, docs, static_cast<const unsigned char*>(written), stride, counts};
    int rc;
    if ((rc = t->tm_tf.begin(t->stream)) || (rc = tq::launch_tf(t->x, t->docs, t->ranks, t->stream, g))) return rc;
    return t->tm_tf.end(t->stream, Q);
}

// The checked group table of a handle or of a shard set (both name the members alike) into a_goff through its pinned buffer, so
// the caller's array is free when the call returns and the launch stays asynchronous.
template <class Owner>
int token_stage_groups(Owner* t, const uint64_t* goff, u64 G) {
    int rc;
    if (t->a_copy_pending) {
        SA_HIP_CHECK(hipEventSynchronize(t->a_copied));
        t->a_copy_pending = false;
    }
    if (t->a_goff_pin_cap < G + 1) {
        if (t->a_goff_pin) (void)hipHostFree(t->a_goff_pin);
        t->a_goff_pin = nullptr; t->a_goff_pin_cap = 0;
        SA_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&t->a_goff_pin), (size_t)(G + 1) * 4, hipHostMallocDefault));
        t->a_goff_pin_cap = (size_t)(G + 1);
    }
    if ((rc = t->a_goff.ensure((size_t)(G + 1) * 4))) return rc;
    for (u64 i = 0; i <= G; ++i) t->a_goff_pin[i] = (u32)goff[i];
    SA_HIP_CHECK(hipMemcpyAsync(t->a_goff.p, t->a_goff_pin, (size_t)(G + 1) * 4, hipMemcpyHostToDevice, t->stream));
    SA_HIP_CHECK(hipEventRecord(t->a_copied, t->stream));
    t->a_copy_pending = true;
    return 0;
}

int token_launch_all(sa_hip_token_index* t, const sa_hip_token_span* spans, const uint64_t* goff, u64 G, u32 cap, u32 budget,
                     int32_t* docs, int32_t* offs, sa_hip_token_all* heads) {
    int rc;
    if ((rc = token_stage_groups(t, goff, G))) return rc;
    const tq::AllArgs g{spans, t->a_goff.as<u32>(), G, cap, budget, docs, offs, heads};
    if ((rc = t->tm_al.begin(t->stream)) || (rc = tq::launch_all(t->x, t->docs, t->ranks, t->stream, g))) return rc;
    return t->tm_al.end(t->stream, G);
}

}  // namespace

extern "C" {

int sa_hip_token_index_prepare_doc_ranks(sa_hip_token_index* t, int on) {
    const char* who = "sa_hip_token_index_prepare_doc_ranks";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (on != 0 && on != 1) return fail(SA_HIP_EINVAL, who, "on is 0 or 1");
    std::lock_guard<std::mutex> g(t->mu);
    int rc;
    if (on == 0) {
        if (!t->ranks.have) return 0;
        if ((rc = set_device(t->device))) return rc;
        SA_HIP_CHECK(hipStreamSynchronize(t->stream));   // launches that read the array
        ++t->ranks_gen;
        t->ranks.clear();
        return 0;
    }
    if ((rc = token_has_docs(t, who))) return rc;
    if (t->ranks.have) return 0;
    if ((rc = set_device(t->device))) return rc;
    ++t->ranks_gen;                                      // whatever follows: a shard set that recorded the old one asks again
    return t->ranks.build(t->x, t->docs, t->stream, who);
}

int sa_hip_token_index_get_doc_ranks(sa_hip_token_index* t, uint64_t first, uint64_t count, int32_t* out) {
    const char* who = "sa_hip_token_index_get_doc_ranks";
    if (!t || (!out && count)) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    int rc = token_has_ranks(t, who);
    if (rc) return rc;
    if (first > t->x.n || count > t->x.n - first) return fail(SA_HIP_EINVAL, who, "range beyond the suffix array");
    if (count == 0) return 0;
    if ((rc = set_device(t->device))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(out, t->ranks.rk.as<int32_t>() + first, (size_t)count * 4, hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    return 0;
}

int sa_hip_token_index_doc_ranks_info(const sa_hip_token_index* ct, sa_hip_token_doc_ranks_info* out) {
    if (!ct || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_index_doc_ranks_info", "NULL argument");
    sa_hip_token_index* t = const_cast<sa_hip_token_index*>(ct);
    std::lock_guard<std::mutex> g(t->mu);
    if (t->tm_tf.pending || t->tm_al.pending) {
        int rc = set_device(t->device);
        if (rc || (rc = t->tm_tf.resolve()) || (rc = t->tm_al.resolve())) return rc;
    }
    memset(out, 0, sizeof *out);
    out->present = t->ranks.have ? 1u : 0u;
    out->sort_passes = t->ranks.passes;
    out->bytes = t->ranks.bytes;
    out->prepare_ms = t->ranks.prepare_ms;
    out->counts_q = t->tm_tf.q;
    out->counts_ms = t->tm_tf.ms;
    out->all_q = t->tm_al.q;
    out->all_ms = t->tm_al.ms;
    return 0;
}

int sa_hip_token_index_doc_counts_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, uint32_t cap,
                                               const void* docs_dev, const void* written_dev, uint64_t written_stride,
                                               void* counts_dev) {
    const char* who = "sa_hip_token_index_doc_counts_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_counts_args(who, Q, cap, written_dev, written_stride);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !docs_dev || !counts_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (written may be NULL)
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = token_has_ranks(t, who)) || (rc = set_device(t->device))) return rc;
    return token_launch_tf(t, static_cast<const sa_hip_token_span*>(spans_dev), Q, cap, static_cast<const int32_t*>(docs_dev), written_dev,
                           written_stride, static_cast<u32*>(counts_dev));
}

int sa_hip_token_index_doc_counts_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                        uint32_t max_length, int need_next, uint32_t cap, const int32_t* docs,
                                        const uint32_t* written, uint32_t* counts, sa_hip_token_span* spans) {
    const char* who = "sa_hip_token_index_doc_counts_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_counts_args(who, Q, cap, nullptr, 0)) || Q == 0) return rc;
    if (!offsets || !docs || !counts) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (written and spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = token_has_ranks(t, who)) || (rc = set_device(t->device))) return rc;
    const size_t cells = (size_t)Q * cap;
    if ((rc = t->d_docs.ensure(cells * 4)) || (rc = t->a_cnt.ensure(cells * 4)) || (rc = t->a_wr.ensure((size_t)Q * 4))) return rc;
    // only the slots of a row are read: the others may be anything on the host, and stay as they are in counts
    std::vector<int32_t> hd;
    std::vector<u32> hc;
    try { hd.assign(cells, 0); hc.resize(cells); } catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, who, "host allocation"); }
    auto slots = [&](u64 i) { return written ? written[i] : cap; };
    copy_written_rows(hd.data(), docs, Q, cap, slots);
    if ((rc = token_stage_spans(t, patterns, offsets, Q, mode, max_length, need_next))) return rc;
    if (spans) SA_HIP_CHECK(hipMemcpyAsync(spans, t->s_spans.p, (size_t)Q * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipMemcpyAsync(t->d_docs.p, hd.data(), cells * 4, hipMemcpyHostToDevice, t->stream));
    if (written) SA_HIP_CHECK(hipMemcpyAsync(t->a_wr.p, written, (size_t)Q * 4, hipMemcpyHostToDevice, t->stream));
    if ((rc = token_launch_tf(t, t->s_spans.as<sa_hip_token_span>(), Q, cap, t->d_docs.as<int32_t>(), written ? t->a_wr.p : nullptr, 4,
                              t->a_cnt.as<u32>()))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(hc.data(), t->a_cnt.p, cells * 4, hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    copy_written_rows(counts, hc.data(), Q, cap, slots);
    return 0;
}

int sa_hip_token_index_all_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t S, const uint64_t* group_offsets_host,
                                        uint64_t G, uint32_t cap, uint32_t budget, void* docs_dev, void* offsets_dev, void* heads_dev) {
    const char* who = "sa_hip_token_index_all_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_all_args(who, S, group_offsets_host, G, cap);
    if (rc || G == 0) return rc;
    if (!spans_dev || !heads_dev || (cap && (!docs_dev || !offsets_dev))) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = token_has_ranks(t, who)) || (rc = set_device(t->device))) return rc;
    return token_launch_all(t, static_cast<const sa_hip_token_span*>(spans_dev), group_offsets_host, G, cap, budget,
                            static_cast<int32_t*>(docs_dev), static_cast<int32_t*>(offsets_dev), static_cast<sa_hip_token_all*>(heads_dev));
}

int sa_hip_token_index_all_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t S,
                                 const uint64_t* group_offsets, uint64_t G, int mode, uint32_t max_length, int need_next,
                                 uint32_t cap, uint32_t budget, sa_hip_token_span* spans, int32_t* docs, int32_t* offs,
                                 sa_hip_token_all* heads) {
    const char* who = "sa_hip_token_index_all_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_all_args(who, S, group_offsets, G, cap)) || G == 0) return rc;
    if (!offsets || !heads || (cap && (!docs || !offs))) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, S))) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = token_has_ranks(t, who)) || (rc = set_device(t->device))) return rc;
    const size_t cells = (size_t)G * cap;
    if ((rc = t->d_docs.ensure(cells * 4)) || (rc = t->d_offs.ensure(cells * 4)) || (rc = t->d_heads.ensure((size_t)G * sizeof(sa_hip_token_all)))) return rc;
    if ((rc = token_stage_spans(t, patterns, offsets, S, mode, max_length, need_next))) return rc;
    if (spans) SA_HIP_CHECK(hipMemcpyAsync(spans, t->s_spans.p, (size_t)S * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, t->stream));
    if ((rc = token_launch_all(t, t->s_spans.as<sa_hip_token_span>(), group_offsets, G, cap, budget, cap ? t->d_docs.as<int32_t>() : nullptr,
                               cap ? t->d_offs.as<int32_t>() : nullptr, t->d_heads.as<sa_hip_token_all>()))) return rc;
    return token_rows_out(t->stream, who, G, cap, t->d_heads.p, heads, t->d_docs.p, docs, t->d_offs.p, offs);
}

}  // extern "C"
