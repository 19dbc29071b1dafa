// capi_token_shard_docs.hpp -- the C ABI of documents over a shard set (include/sa_hip.h section 6g), included by sa_capi.hip behind
// capi_token_shards.hpp (same translation unit).  The kernels are csrc/token_shard_docs.hpp; the shards' own structures are built by
// sa_hip_token_index_set_documents (capi_token_docs.hpp).
// Argument checks come first and touch neither the set nor the device; whether the set has documents, and whether the shards'
// documents are still the ones its table describes, is looked up under the mutexes, still before any HIP call.  The locate stopwatch
// is a LaunchTimer of the set, the pair and merge launches are the two stages of a ChunkTimer (launch_timer.hpp).  The contexts of
// a host form go up through shards_stage_spans, the chunks are walked by shards_chunks (both capi_token_shards.hpp's), and the
// heads and written rows come back through token_rows_out (capi_token.hpp).  Only the scratch of a chunk of pairs and the two
// launches are this file's.
#pragma once
#include "capi_token_docs.hpp"
#include "capi_token_shards.hpp"
#include "token_shard_docs.hpp"

namespace {

// under the set's mutex, before any HIP call: the set has a table and every shard's documents are the ones it was built from
int shards_docs_current(sa_hip_token_shards* g, const char* who) {
    if (!g->has_docs) return fail(SA_HIP_EINVAL, who, "the set has no documents (sa_hip_token_shards_set_documents)");
    for (u32 s = 0; s < g->S; ++s) {
        sa_hip_token_index* t = g->shard[s];
        std::lock_guard<std::mutex> lk(t->mu);
        if (t->docs_gen != g->doc_gen[s] || t->docs.D == 0)
            return fail(SA_HIP_EINVAL, who, "a shard's documents changed behind the set (sa_hip_token_shards_adopt_documents)");
    }
    return 0;
}

// under the set's mutex, the device set: the table of the shards' document views and the bases, from what the shards hold now
int shards_docs_table(sa_hip_token_shards* g, const char* who) {
    g->has_docs = false;
    tq::DocView v[tq::SHARDS_MAX];
    g->doc_base[0] = 0;
    for (u32 s = 0; s < g->S; ++s) {
        sa_hip_token_index* t = g->shard[s];
        std::lock_guard<std::mutex> lk(t->mu);
        if (t->docs.D == 0) return fail(SA_HIP_EINVAL, who, "a shard has no documents (sa_hip_token_index_set_documents)");
        v[s] = t->docs.view();
        g->doc_gen[s] = t->docs_gen;
        g->doc_base[s + 1] = g->doc_base[s] + t->docs.D;
    }
    int rc;
    if ((rc = g->dtab.ensure(sizeof(tq::DocView) * tq::SHARDS_MAX)) || (rc = g->dbase.ensure(sizeof(u64) * (tq::SHARDS_MAX + 1))) ||
        (rc = g->d_sum.ensure(64))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(g->dtab.p, v, sizeof(tq::DocView) * g->S, hipMemcpyHostToDevice, g->stream));   // (behind the launches that read the old one)
    SA_HIP_CHECK(hipMemcpyAsync(g->dbase.p, g->doc_base, sizeof(u64) * (g->S + 1), hipMemcpyHostToDevice, g->stream));
    SA_HIP_CHECK(hipMemsetAsync(g->d_sum.p, 0, sizeof(unsigned long long), g->stream));
    SA_HIP_CHECK(hipStreamSynchronize(g->stream));       // (v is a local)
    g->has_docs = true;
    return 0;
}

int shards_launch_locate(sa_hip_token_shards* g, const sa_hip_token_span* spans, u64 Q, u32 cap, u64* docs, int32_t* offs,
                         sa_hip_token_shards_locate* heads) {
    const tq::ShardLocateArgs a{g->table(), g->dtab.as<tq::DocView>(), g->dbase.as<u64>(), spans, Q, g->S, cap, docs, offs, heads};
    int rc;
    if ((rc = g->tm_lc.begin(g->stream)) || (rc = tq::launch_shard_locate(g->stream, a))) return rc;
    return g->tm_lc.end(g->stream, Q);
}

int shards_launch_docs_merge(sa_hip_token_shards* g, const int32_t* docs, const int32_t* offs, const sa_hip_token_docs* heads,
                             const u64* base, u64 Q, u32 cap, u64* out_docs, int32_t* out_offs, sa_hip_token_shards_docs* out_heads) {
    const tq::ShardDocsMergeArgs m{docs, offs, heads, base, Q, g->S, cap, out_docs, out_offs, out_heads};
    return tq::launch_shard_docs_merge(g->stream, m);
}

// Documents of the device spans [S * Q], chunk by chunk: one wave per (context, shard) pair into the set's scratch, then the
// merge.  Device outputs (to_host false): written in place.  Host outputs: every chunk is merged into od_* and its written
// entries copied out.
int shards_docs(sa_hip_token_shards* g, const char* who, const sa_hip_token_span* spans, u64 Q, u32 cap, u64 budget, u64* docs,
                int32_t* offs, sa_hip_token_shards_docs* heads, bool to_host) {
    int rc;
    const u32 S = g->S;
    const u64 chunk = shards_chunk(g, cap, Q);
    const size_t cells = (size_t)chunk * cap;
    if ((rc = g->d_docs.ensure(cells * S * 4)) || (rc = g->d_offs.ensure(cells * S * 4)) ||
        (rc = g->d_heads.ensure((size_t)chunk * S * sizeof(sa_hip_token_docs)))) return rc;
    SA_HIP_CHECK(hipMemsetAsync(g->d_sum.p, 0, sizeof(unsigned long long), g->stream));
    int32_t* const p_docs = cap ? g->d_docs.as<int32_t>() : nullptr;
    int32_t* const p_offs = cap ? g->d_offs.as<int32_t>() : nullptr;
    auto pairs = [&](const auto& c) -> int {
        tq::ShardDocsArgs a{};
        a.tab = g->table(); a.dtab = g->dtab.as<tq::DocView>();
        a.spans = spans + c.c0; a.span_stride = Q;
        a.Q = c.n; a.S = S; a.cap = cap; a.budget = budget;
        a.docs = p_docs; a.offsets = p_offs;
        a.heads = g->d_heads.as<sa_hip_token_docs>();
        a.streamed = g->d_sum.as<unsigned long long>();
        return tq::launch_shard_docs(g->stream, a);
    };
    auto merge = [&](const auto& c) -> int {
        return shards_launch_docs_merge(g, p_docs, p_offs, g->d_heads.as<sa_hip_token_docs>(), g->dbase.as<u64>(), c.n, cap, c.a, c.b, c.heads);
    };
    return shards_chunks(g, who, g->tm_dc, Q, cap, chunk, to_host, g->od_heads, heads, g->od_docs, docs, g->od_offs, offs, pairs, merge);
}

}  // namespace

extern "C" {

int sa_hip_token_shards_set_documents(sa_hip_token_shards* g, const int32_t* const* starts, const uint32_t* D) {
    const char* who = "sa_hip_token_shards_set_documents";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (!starts != !D) return fail(SA_HIP_EINVAL, who, "starts and D are both given, or both NULL (which removes the documents)");
    int rc;
    if (starts) {                                        // every table before the first shard is touched
        for (u32 s = 0; s < g->S; ++s) {
            if (!starts[s]) return fail(SA_HIP_EINVAL, who, "NULL doc_starts of a shard");
            if (D[s] == 0) return fail(SA_HIP_EINVAL, who, "D == 0 for a shard");
            if ((rc = tq::docs_table_check(who, starts[s], D[s]))) return rc;
            if ((u32)starts[s][D[s] - 1] > g->shard[s]->x.n) return fail(SA_HIP_EINVAL, who, "doc_starts beyond the shard's text");
        }
    }
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    SA_HIP_CHECK(hipStreamSynchronize(g->stream));       // launches of the set that read the tables being replaced
    g->has_docs = false;
    g->has_ranks = false;                                // every shard drops its rank-by-document array with its documents
    for (u32 s = 0; s < g->S; ++s)
        if ((rc = sa_hip_token_index_set_documents(g->shard[s], starts ? starts[s] : nullptr, starts ? D[s] : 0))) return rc;
    if (!starts) { g->doc_base[g->S] = 0; return 0; }
    return shards_docs_table(g, who);
}

int sa_hip_token_shards_adopt_documents(sa_hip_token_shards* g) {
    const char* who = "sa_hip_token_shards_adopt_documents";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    std::lock_guard<std::mutex> lk(g->mu);
    for (u32 s = 0; s < g->S; ++s) {                     // before any HIP call
        std::lock_guard<std::mutex> ls(g->shard[s]->mu);
        if (g->shard[s]->docs.D == 0) { g->has_docs = false; return fail(SA_HIP_EINVAL, who, "a shard has no documents (sa_hip_token_index_set_documents)"); }
    }
    int rc = set_device(g->device);
    if (rc) return rc;
    return shards_docs_table(g, who);
}

int sa_hip_token_shards_doc_bases(sa_hip_token_shards* g, uint64_t* out) {
    const char* who = "sa_hip_token_shards_doc_bases";
    if (!g || !out) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    int rc = shards_docs_current(g, who);
    if (rc) return rc;
    memcpy(out, g->doc_base, sizeof(u64) * (g->S + 1));
    return 0;
}

int sa_hip_token_shards_docs_info(const sa_hip_token_shards* cg, sa_hip_token_shards_docs_stats* out) {
    if (!cg || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_shards_docs_info", "NULL argument");
    sa_hip_token_shards* g = const_cast<sa_hip_token_shards*>(cg);
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->tm_lc.pending || g->tm_dc.pending) {
        int rc = set_device(g->device);
        if (rc || (rc = g->tm_lc.resolve())) return rc;
        if (g->tm_dc.pending) {
            unsigned long long sum = 0;
            SA_HIP_CHECK(hipMemcpyAsync(&sum, g->d_sum.p, sizeof sum, hipMemcpyDeviceToHost, g->stream));
            SA_HIP_CHECK(hipStreamSynchronize(g->stream));
            if ((rc = g->tm_dc.resolve())) return rc;
            g->dc_streamed = sum;
        }
    }
    memset(out, 0, sizeof *out);
    out->documents = g->has_docs ? g->doc_base[g->S] : 0;
    out->chunk = g->tm_dc.chunk;
    out->locate_q = g->tm_lc.q;
    out->locate_ms = g->tm_lc.ms;
    out->pairs_q = g->tm_dc.q * g->S;
    out->pairs_ms = g->tm_dc.ms[0];
    out->merge_q = g->tm_dc.q;
    out->merge_ms = g->tm_dc.ms[1];
    out->streamed = g->dc_streamed;
    return 0;
}

int sa_hip_token_shards_locate_batch_device(sa_hip_token_shards* g, const void* spans_dev, uint64_t Q, uint32_t cap, void* docs_dev,
                                            void* offsets_dev, void* heads_dev) {
    const char* who = "sa_hip_token_shards_locate_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (cap == 0) return fail(SA_HIP_EINVAL, who, "cap == 0");
    int rc = token_cells_args(who, Q, cap);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !docs_dev || !offsets_dev || !heads_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = shards_docs_current(g, who)) || (rc = set_device(g->device))) return rc;
    return shards_launch_locate(g, static_cast<const sa_hip_token_span*>(spans_dev), Q, cap, static_cast<u64*>(docs_dev),
                                static_cast<int32_t*>(offsets_dev), static_cast<sa_hip_token_shards_locate*>(heads_dev));
}

int sa_hip_token_shards_locate_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                     uint32_t cap, sa_hip_token_span* spans, uint64_t* docs, int32_t* offs,
                                     sa_hip_token_shards_locate* heads) {
    const char* who = "sa_hip_token_shards_locate_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (cap == 0) return fail(SA_HIP_EINVAL, who, "cap == 0");
    int rc = token_cells_args(who, Q, cap);
    if (rc || Q == 0) return rc;
    if (!offsets || !docs || !offs || !heads) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = shards_docs_current(g, who)) || (rc = set_device(g->device))) return rc;
    const size_t cells = (size_t)Q * cap;
    if ((rc = g->od_docs.ensure(cells * 8)) || (rc = g->od_offs.ensure(cells * 4)) ||
        (rc = g->od_heads.ensure((size_t)Q * sizeof(sa_hip_token_shards_docs)))) return rc;
    if ((rc = shards_stage_spans(g, patterns, offsets, Q, 0, 0, 0, spans))) return rc;
    if ((rc = shards_launch_locate(g, g->s_spans.as<sa_hip_token_span>(), Q, cap, g->od_docs.as<u64>(), g->od_offs.as<int32_t>(),
                                   g->od_heads.as<sa_hip_token_shards_locate>()))) return rc;
    return token_rows_out(g->stream, who, Q, cap, g->od_heads.p, heads, g->od_docs.p, docs, g->od_offs.p, offs);
}

int sa_hip_token_shards_docs_batch_device(sa_hip_token_shards* g, const void* spans_dev, uint64_t Q, uint32_t cap, uint64_t budget,
                                          void* docs_dev, void* offsets_dev, void* heads_dev) {
    const char* who = "sa_hip_token_shards_docs_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_cells_args(who, Q, cap);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !heads_dev || (cap && (!docs_dev || !offsets_dev))) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = shards_docs_current(g, who)) || (rc = set_device(g->device))) return rc;
    return shards_docs(g, who, static_cast<const sa_hip_token_span*>(spans_dev), Q, cap, budget, static_cast<u64*>(docs_dev),
                       static_cast<int32_t*>(offsets_dev), static_cast<sa_hip_token_shards_docs*>(heads_dev), false);
}

int sa_hip_token_shards_docs_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                   uint32_t max_length, int need_next, uint32_t cap, uint64_t budget, sa_hip_token_span* spans,
                                   uint64_t* docs, int32_t* offs, sa_hip_token_shards_docs* heads) {
    const char* who = "sa_hip_token_shards_docs_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_cells_args(who, Q, cap)) || Q == 0) return rc;
    if (!offsets || !heads || (cap && (!docs || !offs))) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = shards_docs_current(g, who)) || (rc = set_device(g->device))) return rc;
    if ((rc = shards_stage_spans(g, patterns, offsets, Q, mode, max_length, need_next, spans))) return rc;
    return shards_docs(g, who, g->s_spans.as<sa_hip_token_span>(), Q, cap, budget, docs, offs, heads, true);
}

int sa_hip_token_shards_docs_merge_device(sa_hip_token_shards* g, const void* docs_dev, const void* offsets_dev, const void* heads_dev,
                                          const void* bases_dev, uint64_t Q, uint32_t cap, void* out_docs_dev, void* out_offsets_dev,
                                          void* out_heads_dev) {
    const char* who = "sa_hip_token_shards_docs_merge_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_cells_args(who, Q, cap);
    if (rc || Q == 0) return rc;
    if (!heads_dev || !out_heads_dev || (cap && (!docs_dev || !offsets_dev || !out_docs_dev || !out_offsets_dev)))
        return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if (!bases_dev && (rc = shards_docs_current(g, who))) return rc;
    if ((rc = set_device(g->device))) return rc;
    return shards_launch_docs_merge(g, static_cast<const int32_t*>(docs_dev), static_cast<const int32_t*>(offsets_dev),
                                    static_cast<const sa_hip_token_docs*>(heads_dev),
                                    bases_dev ? static_cast<const u64*>(bases_dev) : g->dbase.as<u64>(), Q, cap,
                                    static_cast<u64*>(out_docs_dev), static_cast<int32_t*>(out_offsets_dev),
                                    static_cast<sa_hip_token_shards_docs*>(out_heads_dev));
}

}  // extern "C"
