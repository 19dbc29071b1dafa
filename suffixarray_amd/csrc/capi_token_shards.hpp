// capi_token_shards.hpp -- the C ABI of the shard set (include/sa_hip.h section 6c), included by sa_capi.hip behind capi_token.hpp
// (same translation unit).  The kernels are csrc/token_shards.hpp; the per-shard next symbols are tq::launch_next of every shard.
// Matching statistics over the set: capi_token_shard_match.hpp; documents over the set: capi_token_shard_docs.hpp; per-document
// counts and AND groups over the set: capi_token_shard_all.hpp; infinity-gram scores over the set: capi_token_shard_score.hpp;
// top-k next symbols and draws over the set: capi_token_shard_top.hpp.
// The stopwatches, the upload of a host batch and token_rows_out are capi_token.hpp's.  What the families of the set share is here:
// the spans of a host batch (shards_stage_spans) and the walk of a chunked call (shards_chunks: chunk size, per-chunk stopwatch,
// output pointers of the host and the device form, the way of a chunk's rows to the caller), which the next symbols, the documents
// and the AND groups hand their launches to.
#pragma once
#include "capi_token.hpp"
#include "token_shards.hpp"

struct sa_hip_token_shards {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    u32 S = 0;
    sa_hip_token_index* shard[tq::SHARDS_MAX] = {};
    u64 tokens = 0;
    u32 max_n = 0;
    u64 chunk_knob = 0;                      // SA_HIP_TOKEN_SHARD_CHUNK: contexts per chunk, 0: from the scratch budget
    DevBuf tab;                              // tq::View[S]
    DevBuf q_pat, q_off;                     // staging of the host forms
    DevBuf r_per, r_tot;                     // ranges: per shard (also when the caller wants none), totals
    DevBuf s_spans, s_len, s_tot;            // spans of the host forms
    DevBuf l_sym, l_cnt, l_heads, l_list;    // the per-shard lists of one chunk; l_list as sa_hip_token_index::s_list
    DevBuf o_sym, o_cnt, o_heads;            // merged output of one chunk (host form)
    LaunchTimer tm_r, tm_sp;                 // the last ranges / spans launch
    ChunkTimer<2> tm_nx;                     // the last next-symbol call: the shards' launches, the merge (q: contexts)
    u64 q_last = 0;                          // contexts of the last launch of any kind
    // matching statistics (token_shard_match.hpp, capi_token_shard_match.hpp)
    DevBuf m_ms;                             // u32[total * S]: the per-shard lengths of the last match launch, position-major
    DevBuf m_per, m_merged;                  // staging of the host forms
    DevBuf m_pos, m_out, m_heads;
    LaunchTimer tm_mt, tm_md;                // the last match launches (q: positions) / match docs launch (q: documents)
    u64 m_last = 0;                          // documents of the last launch of either kind
    // documents (token_shard_docs.hpp, capi_token_shard_docs.hpp)
    bool has_docs = false;                   // dtab and dbase describe the shards' documents as of doc_gen
    u64 doc_gen[tq::SHARDS_MAX] = {};        // every shard's docs_gen when the table was built
    u64 doc_base[tq::SHARDS_MAX + 1] = {};   // base[s]: documents of the shards in front of s; base[S]: of the set
    DevBuf dtab, dbase;                      // tq::DocView[S], u64[S + 1]
    DevBuf d_docs, d_offs, d_heads, d_sum;   // the per-pair lists and heads of one chunk; the counter of the streamed ranks
    DevBuf od_docs, od_offs, od_heads;       // merged output of one chunk / the locate output (host forms)
    LaunchTimer tm_lc;                       // the last locate launch
    ChunkTimer<2> tm_dc;                     // the last docs call: the pair launch, the merge (q: contexts)
    u64 dc_streamed = 0;
    // per-document counts and AND groups (token_shard_all.hpp, capi_token_shard_all.hpp)
    bool has_ranks = false;                  // rtab describes the shards' rank-by-document arrays as of rank_gen
    u64 rank_gen[tq::SHARDS_MAX] = {};       // every shard's ranks_gen when the table was built
    DevBuf rtab;                             // tq::RankView[S]
    DevBuf a_docs, a_offs, a_heads;          // the per-pair lists and heads of one chunk
    DevBuf a_plan, a_groups, a_sum;          // the plan of one chunk: per pair, per group; the counter of the streamed ranks
    DevBuf oa_heads;                         // merged heads of one chunk (host form; the lists go through od_docs / od_offs)
    DevBuf c_docs, c_cnt, c_wr;              // staging of the host doc_counts form
    DevBuf a_goff;                           // group offsets of the last all call
    u32* a_goff_pin = nullptr;               // pinned: what the asynchronous copy into a_goff reads
    size_t a_goff_pin_cap = 0;               // ... in entries
    hipEvent_t a_copied = nullptr;           // that copy is done: the pinned buffer may be rewritten
    bool a_copy_pending = false;
    LaunchTimer tm_tf;                       // the last doc_counts launch
    ChunkTimer<3> tm_al;                     // the last all call: the plan launch, the pair launch, the merge (q: groups)
    u64 al_streamed = 0;
    // infinity-gram scores (token_shard_score.hpp, capi_token_shard_score.hpp)
    DevBuf sc_w;                             // u32[3 * total * S]: the scratch planes of the last score launches, position-major
    DevBuf sc_scores, sc_heads;              // staging of the host form (its per-shard spans go through m_per)
    LaunchTimer tm_sc, tm_sd;                // the last score launches (q: positions) / score docs launch (q: documents)
    u64 sc_last = 0;                         // documents of the last launch of either kind
    // top-k next symbols and draws (token_shard_top.hpp, capi_token_shard_top.hpp); the host forms stage through o_sym, o_cnt, o_heads
    bool top_fast = true;                    // SA_HIP_TOKEN_SHARD_TOP_FAST=0: every context through the merge walk, one live shard or not
    DevBuf tp_draws, tp_at;                  // staging of the host sample form: its draws; shards and ranks, u32[Q * m] each
    LaunchTimer tm_tp, tm_sm;                // the last top / sample launch
    u64 tp_last = 0;                         // contexts of the last launch of either kind

    const tq::View* table() const { return tab.as<tq::View>(); }
    std::array<LaunchTimer*, 10> timers() { return {&tm_r, &tm_sp, &tm_mt, &tm_md, &tm_lc, &tm_tf, &tm_sc, &tm_sd, &tm_tp, &tm_sm}; }
    auto buffers() {                         // every DevBuf member above
        return std::array{&tab, &q_pat, &q_off, &r_per, &r_tot, &s_spans, &s_len, &s_tot, &l_sym, &l_cnt, &l_heads, &l_list, &o_sym, &o_cnt,
                          &o_heads, &m_ms, &m_per, &m_merged, &m_pos, &m_out, &m_heads, &dtab, &dbase, &d_docs, &d_offs, &d_heads, &d_sum,
                          &od_docs, &od_offs, &od_heads, &rtab, &a_docs, &a_offs, &a_heads, &a_plan, &a_groups, &a_sum, &oa_heads, &c_docs,
                          &c_cnt, &c_wr, &a_goff, &sc_w, &sc_scores, &sc_heads, &tp_draws, &tp_at};
    }
};

namespace {

int shards_launch_ranges(sa_hip_token_shards* g, const int32_t* pat, const u64* off, u64 Q, u64* totals, sa_hip_pair_u32* per) {
    int rc;
    if (!per) {
        if ((rc = g->r_per.ensure((size_t)Q * g->S * sizeof(sa_hip_pair_u32)))) return rc;
        per = g->r_per.as<sa_hip_pair_u32>();
    }
    if ((rc = g->tm_r.begin(g->stream)) || (rc = tq::launch_shard_ranges(g->table(), g->S, g->stream, pat, off, Q, totals, per)) ||
        (rc = g->tm_r.end(g->stream, Q))) return rc;
    g->q_last = Q;
    return 0;
}

int shards_launch_spans(sa_hip_token_shards* g, const int32_t* pat, const u64* off, u64 Q, int mode, u32 max_length, int need_next,
                        u32* length, u64* totals, sa_hip_token_span* spans) {
    int rc;
    if ((rc = g->tm_sp.begin(g->stream)) ||
        (rc = tq::launch_shard_spans(g->table(), g->S, g->max_n, g->stream, pat, off, Q, mode, max_length, need_next, length, totals, spans)) ||
        (rc = g->tm_sp.end(g->stream, Q))) return rc;
    g->q_last = Q;
    return 0;
}

// contexts from the host into the set's staging buffers, their spans into s_spans (and to the caller when asked), lengths and
// totals into s_len and s_tot
int shards_stage_spans(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, u64 Q, int mode, u32 max_length,
                       int need_next, sa_hip_token_span* spans) {
    int rc;
    const size_t span_bytes = (size_t)Q * g->S * sizeof(sa_hip_token_span);
    if ((rc = token_upload(g->q_pat, g->q_off, g->stream, patterns, offsets, Q)) || (rc = g->s_spans.ensure(span_bytes)) ||
        (rc = g->s_len.ensure((size_t)Q * 4)) || (rc = g->s_tot.ensure((size_t)Q * 8))) return rc;
    if ((rc = shards_launch_spans(g, g->q_pat.as<int32_t>(), g->q_off.as<u64>(), Q, mode, max_length, need_next, g->s_len.as<u32>(),
                                  g->s_tot.as<u64>(), g->s_spans.as<sa_hip_token_span>()))) return rc;
    if (spans) SA_HIP_CHECK(hipMemcpyAsync(spans, g->s_spans.p, span_bytes, hipMemcpyDeviceToHost, g->stream));
    return 0;
}

// Rows (contexts, groups) per chunk of a chunked call over Q rows: every family sizes its per-chunk scratch by it.  A (row, shard)
// pair costs cap * 8 bytes of list and a 16-byte head in each of them.
u64 shards_chunk(const sa_hip_token_shards* g, u32 cap, u64 Q) { return tq::shard_chunk(g->chunk_knob, g->S, cap, Q); }

// rows [c0, c0 + n) of a chunked call, and where the merge of this chunk writes them: the caller's device arrays in place, or the
// set's staging of one chunk (host form); a and b are NULL when cap == 0
template <class Head, class A, class B>
struct ShardChunk {
    u64 c0, n;
    Head* heads;
    A* a;
    B* b;
};

// The walk of a chunked call over Q rows, chunk (from shards_chunk, by which the caller sized its scratch) rows at a time.  Every
// chunk runs its stages in order, as many as tm counts, with a mark of tm in front of the first and behind each, and is published;
// in the host form it comes back through token_rows_out before the next chunk overwrites the staging s_heads / s_a / s_b, which
// grows here with the host scratch, once per call.
template <class Head, class A, class B, u32 STAGES, class... Stage>
int shards_chunks(sa_hip_token_shards* g, const char* who, ChunkTimer<STAGES>& tm, u64 Q, u32 cap, u64 chunk, bool to_host, DevBuf& s_heads,
                  Head* heads, DevBuf& s_a, A* a, DevBuf& s_b, B* b, Stage&&... stage) {
    static_assert(sizeof...(Stage) == STAGES, "one launch per stage of the stopwatch");
    int rc;
    const size_t cells = (size_t)chunk * cap;
    HostRows<A, B> h;
    if (to_host && ((rc = s_heads.ensure((size_t)chunk * sizeof(Head))) || (rc = s_a.ensure(cells * sizeof(A))) ||
                    (rc = s_b.ensure(cells * sizeof(B))) || (rc = h.reserve(who, cells)))) return rc;
    tm.restart();
    for (u64 c0 = 0; c0 < Q; c0 += chunk) {
        const ShardChunk<Head, A, B> c{c0, Q - c0 < chunk ? Q - c0 : chunk, to_host ? s_heads.as<Head>() : heads + c0,
                                       !cap ? nullptr : to_host ? s_a.as<A>() : a + c0 * cap, !cap ? nullptr : to_host ? s_b.as<B>() : b + c0 * cap};
        auto timed = [&](auto& launch) { return (rc = launch(c)) || (rc = tm.mark(g->stream)); };   // true: failed, rc says how
        if ((rc = tm.mark(g->stream)) || (timed(stage) || ...)) return rc;   // the stages from left to right, up to the first that fails
        tm.publish();
        if (to_host && (rc = token_rows_out(g->stream, c.n, cap, c.heads, heads + c0, c.a, a + c0 * cap, c.b, b + c0 * cap, h))) return rc;
    }
    tm.finish(Q, (u32)chunk);
    return 0;
}

// Next symbols of the device spans [S * Q], chunk by chunk: every shard's launch_next on its slice, then the merge.  Device
// outputs (to_host false): written in place.  Host outputs: every chunk is merged into o_* and its written entries copied out.
int shards_next(sa_hip_token_shards* g, const sa_hip_token_span* spans, u64 Q, u32 cap, int32_t* symbols, u64* counts,
                sa_hip_token_shards_next* heads, bool to_host) {
    int rc;
    const u32 S = g->S;
    const u64 chunk = shards_chunk(g, cap, Q);
    const size_t cells = (size_t)chunk * cap;
    bool lanes = false;
    for (u32 s = 0; s < S; ++s) lanes = lanes || g->shard[s]->next_knobs.lanes;
    if ((rc = g->l_sym.ensure(cells * S * 4)) || (rc = g->l_cnt.ensure(cells * S * 4)) ||
        (rc = g->l_heads.ensure((size_t)chunk * S * sizeof(sa_hip_token_next))) || (lanes && (rc = g->l_list.ensure(64 + (size_t)chunk * 4)))) return rc;
    u32* n_list = lanes ? g->l_list.as<u32>() : nullptr;
    auto lists = [&](const auto& c) -> int {
        for (u32 s = 0; s < S; ++s) {
            const sa_hip_token_index* t = g->shard[s];
            const tq::NextArgs a{spans + (u64)s * Q + c.c0, c.n, cap, g->l_sym.as<int32_t>() + (u64)s * c.n * cap,
                                 g->l_cnt.as<u32>() + (u64)s * c.n * cap, g->l_heads.as<sa_hip_token_next>() + (u64)s * c.n};
            if (int r = tq::launch_next(t->x, g->stream, t->next_knobs, a, n_list ? n_list + 16 : nullptr, n_list)) return r;
        }
        return 0;
    };
    auto merge = [&](const auto& c) -> int {
        tq::MergeArgs m{};
        m.sym = g->l_sym.as<int32_t>(); m.cnt = g->l_cnt.as<u32>(); m.heads = g->l_heads.as<sa_hip_token_next>();
        m.spans = spans + c.c0; m.span_stride = Q;
        m.Q = c.n; m.S = S; m.cap = cap;
        m.out_sym = c.a; m.out_cnt = c.b; m.out_heads = c.heads;
        return tq::launch_merge(g->stream, m);
    };
    if ((rc = shards_chunks(g, "sa_hip_token_shards_next_batch", g->tm_nx, Q, cap, chunk, to_host, g->o_heads, heads, g->o_sym, symbols, g->o_cnt, counts,
                            lists, merge))) return rc;
    g->q_last = Q;
    return 0;
}

}  // namespace

extern "C" {

void sa_hip_token_shards_destroy(sa_hip_token_shards* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (u32 s = 0; s < g->S; ++s) sa_hip_token_index_destroy(g->shard[s]);
    for (DevBuf* b : g->buffers()) b->release();
    if (g->a_goff_pin) (void)hipHostFree(g->a_goff_pin);
    if (g->a_copied) (void)hipEventDestroy(g->a_copied);
    for (LaunchTimer* w : g->timers()) w->destroy();
    g->tm_nx.destroy(); g->tm_dc.destroy(); g->tm_al.destroy();
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

int sa_hip_token_shards_create(sa_hip_token_shards** out, sa_hip_token_index* const* shards, uint32_t S) {
    const char* who = "sa_hip_token_shards_create";
    if (!out) return fail(SA_HIP_EINVAL, who, "out == NULL");
    *out = nullptr;
    if (!shards) return fail(SA_HIP_EINVAL, who, "NULL shard list");
    if (S == 0 || S > tq::SHARDS_MAX) return fail(SA_HIP_EINVAL, who, "a set holds 1 to 64 shards");
    for (u32 s = 0; s < S; ++s) if (!shards[s]) return fail(SA_HIP_EINVAL, who, "NULL shard");
    for (u32 s = 1; s < S; ++s)
        for (u32 r = 0; r < s; ++r) if (shards[s] == shards[r]) return fail(SA_HIP_EINVAL, who, "a shard is listed twice");
    for (u32 s = 1; s < S; ++s) if (shards[s]->device != shards[0]->device) return fail(SA_HIP_EINVAL, who, "shards on different devices");
    const int device = shards[0]->device;
    int rc = set_device(device);
    if (rc) return rc;
    sa_hip_token_shards* g = new (std::nothrow) sa_hip_token_shards();
    if (!g) return fail(SA_HIP_ENOMEM, who, "host allocation");
    g->device = device;
    if (const char* e = diag_env("SA_HIP_TOKEN_SHARD_CHUNK")) g->chunk_knob = strtoull(e, nullptr, 10);
    if (const char* e = diag_env("SA_HIP_TOKEN_SHARD_TOP_FAST")) g->top_fast = atoi(e) != 0;
    auto run = [&]() -> int {
        SA_HIP_CHECK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
        for (LaunchTimer* w : g->timers()) SA_HIP_CHECK(w->create());
        SA_HIP_CHECK(hipEventCreate(&g->a_copied));
        tq::View v[tq::SHARDS_MAX];
        for (u32 s = 0; s < S; ++s) {
            std::lock_guard<std::mutex> lk(shards[s]->mu);
            SA_HIP_CHECK(hipStreamSynchronize(shards[s]->stream));   // whatever the shard was asked before it joined
            v[s] = shards[s]->x.view();
            g->tokens += v[s].n;
            if (v[s].n > g->max_n) g->max_n = v[s].n;
        }
        int r2 = g->tab.ensure(sizeof(tq::View) * tq::SHARDS_MAX);
        if (r2) return r2;
        SA_HIP_CHECK(hipMemcpyAsync(g->tab.p, v, sizeof(tq::View) * S, hipMemcpyHostToDevice, g->stream));
        SA_HIP_CHECK(hipStreamSynchronize(g->stream));
        return 0;
    };
    rc = run();
    if (rc) { sa_hip_token_shards_destroy(g); return rc; }   // g->S is still 0: no shard is adopted
    g->S = S;
    for (u32 s = 0; s < S; ++s) g->shard[s] = shards[s];
    *out = g;
    return 0;
}

sa_hip_token_index* sa_hip_token_shards_shard(sa_hip_token_shards* g, uint32_t s) {
    return g && s < g->S ? g->shard[s] : nullptr;
}

int sa_hip_token_shards_sync(sa_hip_token_shards* g) {
    if (!g) return fail(SA_HIP_EINVAL, "sa_hip_token_shards_sync", "NULL handle");
    std::lock_guard<std::mutex> lk(g->mu);
    int rc = set_device(g->device);
    if (rc) return rc;
    SA_HIP_CHECK(hipStreamSynchronize(g->stream));
    return 0;
}

int sa_hip_token_shards_info(const sa_hip_token_shards* cg, sa_hip_token_shards_stats* out) {
    if (!cg || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_shards_info", "NULL argument");
    sa_hip_token_shards* g = const_cast<sa_hip_token_shards*>(cg);
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->tm_r.pending || g->tm_sp.pending || g->tm_nx.pending) {
        int rc = set_device(g->device);
        if (rc || (rc = g->tm_r.resolve()) || (rc = g->tm_sp.resolve()) || (rc = g->tm_nx.resolve())) return rc;
    }
    memset(out, 0, sizeof *out);
    out->shards = g->S;
    out->chunk = g->tm_nx.chunk;
    out->tokens = g->tokens;
    out->q = g->q_last;
    out->ranges_ms = g->tm_r.ms;
    out->spans_ms = g->tm_sp.ms;
    out->next_ms = g->tm_nx.ms[0];
    out->merge_ms = g->tm_nx.ms[1];
    return 0;
}

// ---- ranges.  Argument checks come first and touch neither the handle nor the device. --------------------------------------

int sa_hip_token_shards_query_batch_device(sa_hip_token_shards* g, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                           void* totals_dev, void* per_shard_dev) {
    const char* who = "sa_hip_token_shards_query_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (Q == 0) return 0;
    if (!offsets_dev || !totals_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (patterns may be NULL: a batch of empty patterns)
    std::lock_guard<std::mutex> lk(g->mu);
    int rc = set_device(g->device);
    if (rc) return rc;
    return shards_launch_ranges(g, static_cast<const int32_t*>(patterns_dev), static_cast<const u64*>(offsets_dev), Q, static_cast<u64*>(totals_dev),
                                static_cast<sa_hip_pair_u32*>(per_shard_dev));
}

int sa_hip_token_shards_query_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, uint64_t* totals,
                                    sa_hip_pair_u32* per_shard) {
    const char* who = "sa_hip_token_shards_query_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (Q == 0) return 0;
    if (!offsets || !totals) return fail(SA_HIP_EINVAL, who, "NULL argument");
    int rc = token_offsets_args(who, patterns, offsets, Q);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    const size_t per_bytes = (size_t)Q * g->S * sizeof(sa_hip_pair_u32);
    if ((rc = token_upload(g->q_pat, g->q_off, g->stream, patterns, offsets, Q)) || (rc = g->r_per.ensure(per_bytes)) || (rc = g->r_tot.ensure((size_t)Q * 8))) return rc;
    if ((rc = shards_launch_ranges(g, g->q_pat.as<int32_t>(), g->q_off.as<u64>(), Q, g->r_tot.as<u64>(), g->r_per.as<sa_hip_pair_u32>()))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(totals, g->r_tot.p, (size_t)Q * 8, hipMemcpyDeviceToHost, g->stream));
    if (per_shard) SA_HIP_CHECK(hipMemcpyAsync(per_shard, g->r_per.p, per_bytes, hipMemcpyDeviceToHost, g->stream));
    SA_HIP_CHECK(hipStreamSynchronize(g->stream));
    return 0;
}

// ---- spans ----------------------------------------------------------------------------------------------------------------

int sa_hip_token_shards_spans_batch_device(sa_hip_token_shards* g, const void* patterns_dev, const void* offsets_dev, uint64_t Q, int mode,
                                           uint32_t max_length, int need_next, void* length_dev, void* totals_dev, void* spans_dev) {
    const char* who = "sa_hip_token_shards_spans_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || Q == 0) return rc;
    if (!offsets_dev || !length_dev || !totals_dev || !spans_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (patterns may be NULL)
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    return shards_launch_spans(g, static_cast<const int32_t*>(patterns_dev), static_cast<const u64*>(offsets_dev), Q, mode, max_length, need_next,
                               static_cast<u32*>(length_dev), static_cast<u64*>(totals_dev), static_cast<sa_hip_token_span*>(spans_dev));
}

int sa_hip_token_shards_spans_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                    uint32_t max_length, int need_next, uint32_t* length, uint64_t* totals, sa_hip_token_span* spans) {
    const char* who = "sa_hip_token_shards_spans_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || Q == 0) return rc;
    if (!offsets || !length || !totals || !spans) return fail(SA_HIP_EINVAL, who, "NULL argument");
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    if ((rc = shards_stage_spans(g, patterns, offsets, Q, mode, max_length, need_next, spans))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(length, g->s_len.p, (size_t)Q * 4, hipMemcpyDeviceToHost, g->stream));
    SA_HIP_CHECK(hipMemcpyAsync(totals, g->s_tot.p, (size_t)Q * 8, hipMemcpyDeviceToHost, g->stream));
    SA_HIP_CHECK(hipStreamSynchronize(g->stream));
    return 0;
}

// ---- next symbols ---------------------------------------------------------------------------------------------------------

int sa_hip_token_shards_next_batch_device(sa_hip_token_shards* g, const void* spans_dev, uint64_t Q, uint32_t cap, void* symbols_dev,
                                          void* counts_dev, void* heads_dev) {
    const char* who = "sa_hip_token_shards_next_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_next_args(who, Q, cap);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !symbols_dev || !counts_dev || !heads_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    return shards_next(g, static_cast<const sa_hip_token_span*>(spans_dev), Q, cap, static_cast<int32_t*>(symbols_dev), static_cast<u64*>(counts_dev),
                       static_cast<sa_hip_token_shards_next*>(heads_dev), false);
}

int sa_hip_token_shards_next_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                   uint32_t max_length, int need_next, uint32_t cap, sa_hip_token_span* spans, int32_t* symbols,
                                   uint64_t* counts, sa_hip_token_shards_next* heads) {
    const char* who = "sa_hip_token_shards_next_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_next_args(who, Q, cap)) || Q == 0) return rc;
    if (!offsets || !symbols || !counts || !heads) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    if ((rc = shards_stage_spans(g, patterns, offsets, Q, mode, max_length, need_next, spans))) return rc;
    return shards_next(g, g->s_spans.as<sa_hip_token_span>(), Q, cap, symbols, counts, heads, true);
}

int sa_hip_token_shards_merge_device(sa_hip_token_shards* g, const void* symbols_dev, const void* counts_dev, const void* heads_dev, uint64_t Q,
                                     uint32_t cap, void* out_symbols_dev, void* out_counts_dev, void* out_heads_dev) {
    const char* who = "sa_hip_token_shards_merge_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_next_args(who, Q, cap);
    if (rc || Q == 0) return rc;
    if (!symbols_dev || !counts_dev || !heads_dev || !out_symbols_dev || !out_counts_dev || !out_heads_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    tq::MergeArgs m{};
    m.sym = static_cast<const int32_t*>(symbols_dev); m.cnt = static_cast<const u32*>(counts_dev);
    m.heads = static_cast<const sa_hip_token_next*>(heads_dev);
    m.spans = nullptr; m.span_stride = 0;
    m.Q = Q; m.S = g->S; m.cap = cap;
    m.out_sym = static_cast<int32_t*>(out_symbols_dev); m.out_cnt = static_cast<u64*>(out_counts_dev);
    m.out_heads = static_cast<sa_hip_token_shards_next*>(out_heads_dev);
    return tq::launch_merge(g->stream, m);
}

}  // extern "C"
