// capi_token_shard_all.hpp -- the C ABI of per-document counts and AND groups over a shard set (include/sa_hip.h section 6h),
// included by sa_capi.hip behind capi_token_shard_docs.hpp (same translation unit).  The kernels are csrc/token_shard_all.hpp; the
// shards' own rank-by-document arrays are built by sa_hip_token_index_prepare_doc_ranks (capi_token_all.hpp).
// Argument checks come first and touch neither the set nor the device; whether the set has documents and a table of rank arrays,
// and whether the shards' documents and arrays are still the ones the tables describe, is looked up under the mutexes, still before
// any HIP call.  The doc_counts stopwatch is a LaunchTimer of the set, the plan, pair and merge launches are the three stages of a
// ChunkTimer (launch_timer.hpp).  The contexts of a host form go up through shards_stage_spans, the chunks of groups are walked by
// shards_chunks (both capi_token_shards.hpp's), and the heads and written rows come back through token_rows_out (capi_token.hpp);
// the host doc_counts form moves the caller's rows in and the counts out with copy_written_rows (host_rows.hpp) as
// capi_token_all.hpp's does.  The group table goes through a pinned buffer of the set (token_stage_groups of capi_token_all.hpp),
// so the device form stays asynchronous.
#pragma once
#include "capi_token_all.hpp"
#include "capi_token_shard_docs.hpp"
#include "token_shard_all.hpp"

static_assert(sizeof(sa_hip_token_shards_all) == 40, "sa_hip_token_shards_all is 40 bytes");
static_assert(sizeof(tq::ShardAllPair) == 16 && sizeof(tq::ShardAllPlan) == 8 && sizeof(tq::ShardAllGroup) == 16, "scratch records");

namespace {

// under the set's mutex, before any HIP call: documents and rank arrays of every shard are the ones the set's tables were built from
int shards_ranks_current(sa_hip_token_shards* g, const char* who) {
    int rc = shards_docs_current(g, who);
    if (rc) return rc;
    if (!g->has_ranks) return fail(SA_HIP_EINVAL, who, "the set has no rank arrays (sa_hip_token_shards_prepare_doc_ranks)");
    for (u32 s = 0; s < g->S; ++s) {
        sa_hip_token_index* t = g->shard[s];
        std::lock_guard<std::mutex> lk(t->mu);
        if (t->ranks_gen != g->rank_gen[s] || !t->ranks.have)
            return fail(SA_HIP_EINVAL, who, "a shard's rank arrays changed behind the set (sa_hip_token_shards_prepare_doc_ranks)");
    }
    return 0;
}

// under the set's mutex, the device set: the table of the shards' rank views from what the shards hold now
int shards_ranks_table(sa_hip_token_shards* g, const char* who) {
    g->has_ranks = false;
    tq::RankView v[tq::SHARDS_MAX];
    for (u32 s = 0; s < g->S; ++s) {
        sa_hip_token_index* t = g->shard[s];
        std::lock_guard<std::mutex> lk(t->mu);
        if (t->docs.D == 0 || !t->ranks.have) return fail(SA_HIP_EINVAL, who, "a shard has no rank-by-document array");
        v[s] = t->ranks.view(t->docs);
        g->rank_gen[s] = t->ranks_gen;
    }
    int rc;
    if ((rc = g->rtab.ensure(sizeof(tq::RankView) * tq::SHARDS_MAX)) || (rc = g->a_sum.ensure(64))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(g->rtab.p, v, sizeof(tq::RankView) * g->S, hipMemcpyHostToDevice, g->stream));   // (behind the launches that read the old one)
    SA_HIP_CHECK(hipMemsetAsync(g->a_sum.p, 0, sizeof(unsigned long long), g->stream));
    SA_HIP_CHECK(hipStreamSynchronize(g->stream));       // (v is a local)
    g->has_ranks = true;
    return 0;
}

// P and G as they are, the table only when there are groups
int shards_all_args(const char* who, u64 P, const uint64_t* goff, u64 G, u32 cap) {
    if (P >= 0x80000000ull) return fail(SA_HIP_EINVAL, who, "P >= 2^31");
    if (G >= 0x80000000ull) return fail(SA_HIP_EINVAL, who, "G >= 2^31");
    int rc = token_cells_args(who, G, cap);
    if (rc || G == 0) return rc;
    if (!goff) return fail(SA_HIP_EINVAL, who, "NULL group_offsets");
    return tq::all_groups_check(who, goff, P, G);
}

int shards_launch_tf(sa_hip_token_shards* g, const sa_hip_token_span* spans, u64 Q, u32 cap, const u64* docs, const void* written,
                     u64 stride, u32* counts) {
    const tq::ShardTfArgs a{g->table(), g->rtab.as<tq::RankView>(), g->dbase.as<u64>(), spans, Q, g->S, cap, docs,
                            static_cast<const unsigned char*>(written), stride, counts};
    int rc;
    if ((rc = g->tm_tf.begin(g->stream)) || (rc = tq::launch_shard_tf(g->stream, a))) return rc;
    return g->tm_tf.end(g->stream, Q);
}

int shards_launch_all_merge(sa_hip_token_shards* g, const int32_t* docs, const int32_t* offs, const tq::ShardAllPair* heads,
                            const tq::ShardAllGroup* groups, const u64* base, u64 G, u32 cap, u64* out_docs, int32_t* out_offs,
                            sa_hip_token_shards_all* out_heads) {
    const tq::ShardAllMergeArgs m{docs, offs, heads, groups, base, G, g->S, cap, out_docs, out_offs, out_heads};
    return tq::launch_shard_all_merge(g->stream, m);
}

// AND groups over the device spans [S * P], chunk by chunk: the plan (one wave per group), one wave per (group, shard) pair into
// the set's scratch, then the merge.  Device outputs (to_host false): written in place.  Host outputs: every chunk is merged into
// od_docs / od_offs / oa_heads and its written entries copied out.
int shards_all(sa_hip_token_shards* g, const char* who, const sa_hip_token_span* spans, u64 P, const uint64_t* goff, u64 G, u32 cap,
               u64 budget, u64* docs, int32_t* offs, sa_hip_token_shards_all* heads, bool to_host) {
    int rc;
    const u32 S = g->S;
    const u64 chunk = shards_chunk(g, cap, G);
    const size_t cells = (size_t)chunk * cap;
    if ((rc = g->a_docs.ensure(cells * S * 4)) || (rc = g->a_offs.ensure(cells * S * 4)) ||
        (rc = g->a_heads.ensure((size_t)chunk * S * sizeof(tq::ShardAllPair))) ||
        (rc = g->a_plan.ensure((size_t)chunk * S * sizeof(tq::ShardAllPlan))) ||
        (rc = g->a_groups.ensure((size_t)chunk * sizeof(tq::ShardAllGroup)))) return rc;
    if ((rc = token_stage_groups(g, goff, G))) return rc;
    SA_HIP_CHECK(hipMemsetAsync(g->a_sum.p, 0, sizeof(unsigned long long), g->stream));
    int32_t* const p_docs = cap ? g->a_docs.as<int32_t>() : nullptr;
    int32_t* const p_offs = cap ? g->a_offs.as<int32_t>() : nullptr;
    auto plan = [&](const auto& c) -> int {
        tq::ShardAllPlanArgs p{};
        p.tab = g->table(); p.spans = spans; p.P = P;
        p.group_offsets = g->a_goff.as<u32>() + c.c0; p.G = c.n; p.S = S; p.budget = budget;
        p.pairs = g->a_plan.as<tq::ShardAllPlan>(); p.groups = g->a_groups.as<tq::ShardAllGroup>();
        return tq::launch_shard_all_plan(g->stream, p);
    };
    auto pairs = [&](const auto& c) -> int {
        tq::ShardAllArgs a{};
        a.tab = g->table(); a.rtab = g->rtab.as<tq::RankView>();
        a.spans = spans; a.P = P; a.group_offsets = g->a_goff.as<u32>() + c.c0; a.pairs = g->a_plan.as<tq::ShardAllPlan>();
        a.G = c.n; a.S = S; a.cap = cap;
        a.docs = p_docs; a.offsets = p_offs;
        a.heads = g->a_heads.as<tq::ShardAllPair>();
        a.streamed = g->a_sum.as<unsigned long long>();
        return tq::launch_shard_all(g->stream, a);
    };
    auto merge = [&](const auto& c) -> int {
        return shards_launch_all_merge(g, p_docs, p_offs, g->a_heads.as<tq::ShardAllPair>(), g->a_groups.as<tq::ShardAllGroup>(),
                                       g->dbase.as<u64>(), c.n, cap, c.a, c.b, c.heads);
    };
    return shards_chunks(g, who, g->tm_al, G, cap, chunk, to_host, g->oa_heads, heads, g->od_docs, docs, g->od_offs, offs, plan, pairs, merge);
}

}  // namespace

extern "C" {

int sa_hip_token_shards_prepare_doc_ranks(sa_hip_token_shards* g, int on) {
    const char* who = "sa_hip_token_shards_prepare_doc_ranks";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (on != 0 && on != 1) return fail(SA_HIP_EINVAL, who, "on is 0 or 1");
    std::lock_guard<std::mutex> lk(g->mu);
    int rc;
    if (on == 0) {
        if (!g->has_docs) return fail(SA_HIP_EINVAL, who, "the set has no documents (sa_hip_token_shards_set_documents)");
        if ((rc = set_device(g->device))) return rc;
        SA_HIP_CHECK(hipStreamSynchronize(g->stream));   // launches of the set that read the arrays
        g->has_ranks = false;
        for (u32 s = 0; s < g->S; ++s)
            if ((rc = sa_hip_token_index_prepare_doc_ranks(g->shard[s], 0))) return rc;
        return 0;
    }
    if ((rc = shards_docs_current(g, who)) || (rc = set_device(g->device))) return rc;
    SA_HIP_CHECK(hipStreamSynchronize(g->stream));       // launches of the set that read the table being replaced
    g->has_ranks = false;
    for (u32 s = 0; s < g->S; ++s)                       // one after another: the sort scratch of one shard at a time
        if ((rc = sa_hip_token_index_prepare_doc_ranks(g->shard[s], 1))) return rc;
    return shards_ranks_table(g, who);
}

int sa_hip_token_shards_doc_ranks_info(const sa_hip_token_shards* cg, sa_hip_token_shards_ranks_stats* out) {
    if (!cg || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_shards_doc_ranks_info", "NULL argument");
    sa_hip_token_shards* g = const_cast<sa_hip_token_shards*>(cg);
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->tm_tf.pending || g->tm_al.pending) {
        int rc = set_device(g->device);
        if (rc || (rc = g->tm_tf.resolve())) return rc;
        if (g->tm_al.pending) {
            unsigned long long sum = 0;
            SA_HIP_CHECK(hipMemcpyAsync(&sum, g->a_sum.p, sizeof sum, hipMemcpyDeviceToHost, g->stream));
            SA_HIP_CHECK(hipStreamSynchronize(g->stream));
            if ((rc = g->tm_al.resolve())) return rc;
            g->al_streamed = sum;
        }
    }
    memset(out, 0, sizeof *out);
    out->present = g->has_ranks ? 1u : 0u;
    out->chunk = g->tm_al.chunk;
    for (u32 s = 0; s < g->S; ++s) {
        sa_hip_token_index* t = g->shard[s];
        std::lock_guard<std::mutex> ls(t->mu);
        out->bytes += t->ranks.bytes;
        out->prepare_ms += t->ranks.prepare_ms;
    }
    out->counts_q = g->tm_tf.q;
    out->counts_ms = g->tm_tf.ms;
    out->plan_q = g->tm_al.q;
    out->plan_ms = g->tm_al.ms[0];
    out->pairs_q = g->tm_al.q * g->S;
    out->pairs_ms = g->tm_al.ms[1];
    out->merge_q = g->tm_al.q;
    out->merge_ms = g->tm_al.ms[2];
    out->streamed = g->al_streamed;
    return 0;
}

int sa_hip_token_shards_doc_counts_batch_device(sa_hip_token_shards* g, const void* spans_dev, uint64_t Q, uint32_t cap,
                                                const void* docs_dev, const void* written_dev, uint64_t written_stride,
                                                void* counts_dev) {
    const char* who = "sa_hip_token_shards_doc_counts_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_counts_args(who, Q, cap, written_dev, written_stride);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !docs_dev || !counts_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (written may be NULL)
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = shards_ranks_current(g, who)) || (rc = set_device(g->device))) return rc;
    return shards_launch_tf(g, static_cast<const sa_hip_token_span*>(spans_dev), Q, cap, static_cast<const u64*>(docs_dev), written_dev,
                            written_stride, static_cast<u32*>(counts_dev));
}

int sa_hip_token_shards_doc_counts_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                         int mode, uint32_t max_length, int need_next, uint32_t cap, const uint64_t* docs,
                                         const uint32_t* written, uint32_t* counts, sa_hip_token_span* spans) {
    const char* who = "sa_hip_token_shards_doc_counts_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_counts_args(who, Q, cap, nullptr, 0)) || Q == 0) return rc;
    if (!offsets || !docs || !counts) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (written and spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = shards_ranks_current(g, who)) || (rc = set_device(g->device))) return rc;
    const size_t cells = (size_t)Q * cap;
    if ((rc = g->c_docs.ensure(cells * 8)) || (rc = g->c_cnt.ensure(cells * 4)) || (rc = g->c_wr.ensure((size_t)Q * 4))) return rc;
    // only the slots of a row are read: the others may be anything on the host, and stay as they are in counts
    std::vector<u64> hd;
    std::vector<u32> hc;
    try { hd.assign(cells, 0); hc.resize(cells); } catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, who, "host allocation"); }
    auto slots = [&](u64 i) { return written ? written[i] : cap; };
    copy_written_rows(hd.data(), docs, Q, cap, slots);
    if ((rc = shards_stage_spans(g, patterns, offsets, Q, mode, max_length, need_next, spans))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(g->c_docs.p, hd.data(), cells * 8, hipMemcpyHostToDevice, g->stream));
    if (written) SA_HIP_CHECK(hipMemcpyAsync(g->c_wr.p, written, (size_t)Q * 4, hipMemcpyHostToDevice, g->stream));
    if ((rc = shards_launch_tf(g, g->s_spans.as<sa_hip_token_span>(), Q, cap, g->c_docs.as<u64>(), written ? g->c_wr.p : nullptr, 4,
                               g->c_cnt.as<u32>()))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(hc.data(), g->c_cnt.p, cells * 4, hipMemcpyDeviceToHost, g->stream));
    SA_HIP_CHECK(hipStreamSynchronize(g->stream));
    copy_written_rows(counts, hc.data(), Q, cap, slots);
    return 0;
}

int sa_hip_token_shards_all_batch_device(sa_hip_token_shards* g, const void* spans_dev, uint64_t P,
                                         const uint64_t* group_offsets_host, uint64_t G, uint32_t cap, uint64_t budget,
                                         void* docs_dev, void* offsets_dev, void* heads_dev) {
    const char* who = "sa_hip_token_shards_all_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = shards_all_args(who, P, group_offsets_host, G, cap);
    if (rc || G == 0) return rc;
    if (!spans_dev || !heads_dev || (cap && (!docs_dev || !offsets_dev))) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = shards_ranks_current(g, who)) || (rc = set_device(g->device))) return rc;
    return shards_all(g, who, static_cast<const sa_hip_token_span*>(spans_dev), P, group_offsets_host, G, cap, budget,
                      static_cast<u64*>(docs_dev), static_cast<int32_t*>(offsets_dev), static_cast<sa_hip_token_shards_all*>(heads_dev), false);
}

int sa_hip_token_shards_all_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t P,
                                  const uint64_t* group_offsets, uint64_t G, int mode, uint32_t max_length, int need_next,
                                  uint32_t cap, uint64_t budget, sa_hip_token_span* spans, uint64_t* docs, int32_t* offs,
                                  sa_hip_token_shards_all* heads) {
    const char* who = "sa_hip_token_shards_all_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = shards_all_args(who, P, group_offsets, G, cap)) || G == 0) return rc;
    if (!offsets || !heads || (cap && (!docs || !offs))) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, P))) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = shards_ranks_current(g, who)) || (rc = set_device(g->device))) return rc;
    if ((rc = shards_stage_spans(g, patterns, offsets, P, mode, max_length, need_next, spans))) return rc;
    return shards_all(g, who, g->s_spans.as<sa_hip_token_span>(), P, group_offsets, G, cap, budget, docs, offs, heads, true);
}

int sa_hip_token_shards_all_merge_device(sa_hip_token_shards* g, const void* docs_dev, const void* offsets_dev, const void* heads_dev,
                                         const void* plan_dev, const void* bases_dev, uint64_t G, uint32_t cap, void* out_docs_dev,
                                         void* out_offsets_dev, void* out_heads_dev) {
    const char* who = "sa_hip_token_shards_all_merge_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_cells_args(who, G, cap);
    if (rc || G == 0) return rc;
    if (!heads_dev || !plan_dev || !out_heads_dev || (cap && (!docs_dev || !offsets_dev || !out_docs_dev || !out_offsets_dev)))
        return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if (!bases_dev && (rc = shards_docs_current(g, who))) return rc;
    if ((rc = set_device(g->device))) return rc;
    return shards_launch_all_merge(g, static_cast<const int32_t*>(docs_dev), static_cast<const int32_t*>(offsets_dev),
                                   static_cast<const tq::ShardAllPair*>(heads_dev), static_cast<const tq::ShardAllGroup*>(plan_dev),
                                   bases_dev ? static_cast<const u64*>(bases_dev) : g->dbase.as<u64>(), G, cap,
                                   static_cast<u64*>(out_docs_dev), static_cast<int32_t*>(out_offsets_dev),
                                   static_cast<sa_hip_token_shards_all*>(out_heads_dev));
}

}  // extern "C"
