// capi_token_shards.hpp -- the C ABI of the shard set (include/sa_hip.h section 6c), included by sa_capi.hip behind capi_token.hpp
// (same translation unit).  The kernels are csrc/token_shards.hpp; the per-shard next symbols are tq::launch_next of every shard.
// Matching statistics over the set: capi_token_shard_match.hpp; documents over the set: capi_token_shard_docs.hpp; per-document
// counts and AND groups over the set: capi_token_shard_all.hpp.
// The stopwatches, the upload of a host batch and the row copy are capi_token.hpp's; the per-chunk events of the next symbols, summed
// into two figures, are the set's own.
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
    std::vector<hipEvent_t> nx_ev;           // 3 per chunk: before the shards' launches, behind them, behind the merge
    size_t nx_used = 0;                      // events of the last next-symbol call
    bool nx_pending = false;
    u64 q_last = 0;                          // contexts of the last launch of any kind
    u32 chunk_last = 0;
    double nx_ms = 0.0, mg_ms = 0.0;
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
    std::vector<hipEvent_t> dc_ev;           // 3 per chunk, as nx_ev: before the pair launch, behind it, behind the merge
    size_t dc_used = 0;
    bool dc_pending = false;
    u64 dc_q = 0, dm_q = 0;                  // pairs / contexts of the last pair / merge launches
    u32 dc_chunk = 0;
    double dc_ms = 0.0, dm_ms = 0.0;
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
    std::vector<hipEvent_t> al_ev;           // 4 per chunk: before the plan launch, behind it, behind the pair launch, behind the merge
    size_t al_used = 0;
    bool al_pending = false;
    u64 al_q = 0, al_pairs_q = 0;            // groups / pairs of the last all call
    u32 al_chunk = 0;
    double al_plan_ms = 0.0, al_pairs_ms = 0.0, al_merge_ms = 0.0;
    u64 al_streamed = 0;

    const tq::View* table() const { return tab.as<tq::View>(); }
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

// event k of a per-chunk list (nx_ev, dc_ev), created on demand, recorded on the set's stream
int shards_event(sa_hip_token_shards* g, std::vector<hipEvent_t>& list, size_t k) {
    while (list.size() <= k) {
        hipEvent_t e = nullptr;
        SA_HIP_CHECK(hipEventCreate(&e));
        list.push_back(e);
    }
    SA_HIP_CHECK(hipEventRecord(list[k], g->stream));
    return 0;
}
int shards_event(sa_hip_token_shards* g, size_t k) { return shards_event(g, g->nx_ev, k); }

// Next symbols of the device spans [S * Q], chunk by chunk: every shard's launch_next on its slice, then the merge.  Device
// outputs (to_host false): written in place.  Host outputs: every chunk is merged into o_* and its written entries copied out.
int shards_next(sa_hip_token_shards* g, const sa_hip_token_span* spans, u64 Q, u32 cap, int32_t* symbols, u64* counts,
                sa_hip_token_shards_next* heads, bool to_host) {
    const char* who = "sa_hip_token_shards_next_batch";
    int rc;
    const u32 S = g->S;
    const u64 chunk = tq::shard_chunk(g->chunk_knob, S, cap, Q);
    const size_t cells = (size_t)chunk * cap;
    bool lanes = false;
    for (u32 s = 0; s < S; ++s) lanes = lanes || g->shard[s]->next_knobs.lanes;
    if ((rc = g->l_sym.ensure(cells * S * 4)) || (rc = g->l_cnt.ensure(cells * S * 4)) ||
        (rc = g->l_heads.ensure((size_t)chunk * S * sizeof(sa_hip_token_next))) || (lanes && (rc = g->l_list.ensure(64 + (size_t)chunk * 4)))) return rc;
    std::vector<int32_t> hs;
    std::vector<u64> hc;
    if (to_host) {
        if ((rc = g->o_sym.ensure(cells * 4)) || (rc = g->o_cnt.ensure(cells * 8)) || (rc = g->o_heads.ensure((size_t)chunk * sizeof(sa_hip_token_shards_next)))) return rc;
        try { hs.resize(cells); hc.resize(cells); } catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, who, "host allocation"); }
    }
    u32* n_list = lanes ? g->l_list.as<u32>() : nullptr;
    size_t ev = 0;
    for (u64 c0 = 0; c0 < Q; c0 += chunk) {
        const u64 qc = Q - c0 < chunk ? Q - c0 : chunk;
        if ((rc = shards_event(g, ev++))) return rc;
        for (u32 s = 0; s < S; ++s) {
            const sa_hip_token_index* t = g->shard[s];
            const tq::NextArgs a{spans + (u64)s * Q + c0, qc, cap, g->l_sym.as<int32_t>() + (u64)s * qc * cap, g->l_cnt.as<u32>() + (u64)s * qc * cap,
                                 g->l_heads.as<sa_hip_token_next>() + (u64)s * qc};
            if ((rc = tq::launch_next(t->x, g->stream, t->next_knobs, a, n_list ? n_list + 16 : nullptr, n_list))) return rc;
        }
        if ((rc = shards_event(g, ev++))) return rc;
        tq::MergeArgs m{};
        m.sym = g->l_sym.as<int32_t>(); m.cnt = g->l_cnt.as<u32>(); m.heads = g->l_heads.as<sa_hip_token_next>();
        m.spans = spans + c0; m.span_stride = Q;
        m.Q = qc; m.S = S; m.cap = cap;
        m.out_sym = to_host ? g->o_sym.as<int32_t>() : symbols + c0 * cap;
        m.out_cnt = to_host ? g->o_cnt.as<u64>() : counts + c0 * cap;
        m.out_heads = to_host ? g->o_heads.as<sa_hip_token_shards_next>() : heads + c0;
        if ((rc = tq::launch_merge(g->stream, m))) return rc;
        if ((rc = shards_event(g, ev++))) return rc;
        g->nx_used = ev;
        g->nx_pending = true;
        if (to_host) {
            SA_HIP_CHECK(hipMemcpyAsync(heads + c0, g->o_heads.p, (size_t)qc * sizeof(sa_hip_token_shards_next), hipMemcpyDeviceToHost, g->stream));
            SA_HIP_CHECK(hipMemcpyAsync(hs.data(), g->o_sym.p, (size_t)qc * cap * 4, hipMemcpyDeviceToHost, g->stream));
            SA_HIP_CHECK(hipMemcpyAsync(hc.data(), g->o_cnt.p, (size_t)qc * cap * 8, hipMemcpyDeviceToHost, g->stream));
            SA_HIP_CHECK(hipStreamSynchronize(g->stream));
            const StridedLen written{&heads[c0].written, sizeof heads[0]};
            copy_written_rows(symbols + c0 * cap, hs.data(), qc, cap, written);
            copy_written_rows(counts + c0 * cap, hc.data(), qc, cap, written);
        }
    }
    g->q_last = Q;
    g->chunk_last = (u32)chunk;
    return 0;
}

}  // namespace

extern "C" {

void sa_hip_token_shards_destroy(sa_hip_token_shards* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (u32 s = 0; s < g->S; ++s) sa_hip_token_index_destroy(g->shard[s]);
    g->tab.release(); g->q_pat.release(); g->q_off.release(); g->r_per.release(); g->r_tot.release();
    g->s_spans.release(); g->s_len.release(); g->s_tot.release();
    g->l_sym.release(); g->l_cnt.release(); g->l_heads.release(); g->l_list.release();
    g->o_sym.release(); g->o_cnt.release(); g->o_heads.release();
    g->m_ms.release(); g->m_per.release(); g->m_merged.release(); g->m_pos.release(); g->m_out.release(); g->m_heads.release();
    g->dtab.release(); g->dbase.release(); g->d_docs.release(); g->d_offs.release(); g->d_heads.release(); g->d_sum.release();
    g->od_docs.release(); g->od_offs.release(); g->od_heads.release();
    g->rtab.release(); g->a_docs.release(); g->a_offs.release(); g->a_heads.release(); g->a_plan.release(); g->a_groups.release();
    g->a_sum.release(); g->oa_heads.release(); g->c_docs.release(); g->c_cnt.release(); g->c_wr.release(); g->a_goff.release();
    if (g->a_goff_pin) (void)hipHostFree(g->a_goff_pin);
    if (g->a_copied) (void)hipEventDestroy(g->a_copied);
    g->tm_tf.destroy();
    for (hipEvent_t e : g->al_ev) (void)hipEventDestroy(e);
    g->tm_r.destroy(); g->tm_sp.destroy(); g->tm_mt.destroy(); g->tm_md.destroy(); g->tm_lc.destroy();
    for (hipEvent_t e : g->nx_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->dc_ev) (void)hipEventDestroy(e);
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
    auto run = [&]() -> int {
        SA_HIP_CHECK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
        SA_HIP_CHECK(g->tm_r.create());
        SA_HIP_CHECK(g->tm_sp.create());
        SA_HIP_CHECK(g->tm_mt.create());
        SA_HIP_CHECK(g->tm_md.create());
        SA_HIP_CHECK(g->tm_lc.create());
        SA_HIP_CHECK(g->tm_tf.create());
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
    if (g->tm_r.pending || g->tm_sp.pending || g->nx_pending) {
        int rc = set_device(g->device);
        if (rc || (rc = g->tm_r.resolve()) || (rc = g->tm_sp.resolve())) return rc;
        if (g->nx_pending) {
            float ms = 0.f;
            SA_HIP_CHECK(hipEventSynchronize(g->nx_ev[g->nx_used - 1]));
            g->nx_ms = g->mg_ms = 0.0;
            for (size_t k = 0; k + 3 <= g->nx_used; k += 3) {
                SA_HIP_CHECK(hipEventElapsedTime(&ms, g->nx_ev[k], g->nx_ev[k + 1]));
                g->nx_ms += ms;
                SA_HIP_CHECK(hipEventElapsedTime(&ms, g->nx_ev[k + 1], g->nx_ev[k + 2]));
                g->mg_ms += ms;
            }
            g->nx_pending = false;
        }
    }
    memset(out, 0, sizeof *out);
    out->shards = g->S;
    out->chunk = g->chunk_last;
    out->tokens = g->tokens;
    out->q = g->q_last;
    out->ranges_ms = g->tm_r.ms;
    out->spans_ms = g->tm_sp.ms;
    out->next_ms = g->nx_ms;
    out->merge_ms = g->mg_ms;
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
    const size_t span_bytes = (size_t)Q * g->S * sizeof(sa_hip_token_span);
    if ((rc = token_upload(g->q_pat, g->q_off, g->stream, patterns, offsets, Q)) || (rc = g->s_spans.ensure(span_bytes)) || (rc = g->s_len.ensure((size_t)Q * 4)) ||
        (rc = g->s_tot.ensure((size_t)Q * 8))) return rc;
    if ((rc = shards_launch_spans(g, g->q_pat.as<int32_t>(), g->q_off.as<u64>(), Q, mode, max_length, need_next, g->s_len.as<u32>(), g->s_tot.as<u64>(),
                                  g->s_spans.as<sa_hip_token_span>()))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(length, g->s_len.p, (size_t)Q * 4, hipMemcpyDeviceToHost, g->stream));
    SA_HIP_CHECK(hipMemcpyAsync(totals, g->s_tot.p, (size_t)Q * 8, hipMemcpyDeviceToHost, g->stream));
    SA_HIP_CHECK(hipMemcpyAsync(spans, g->s_spans.p, span_bytes, hipMemcpyDeviceToHost, g->stream));
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
    const size_t span_bytes = (size_t)Q * g->S * sizeof(sa_hip_token_span);
    if ((rc = token_upload(g->q_pat, g->q_off, g->stream, patterns, offsets, Q)) || (rc = g->s_spans.ensure(span_bytes)) || (rc = g->s_len.ensure((size_t)Q * 4)) ||
        (rc = g->s_tot.ensure((size_t)Q * 8))) return rc;
    if ((rc = shards_launch_spans(g, g->q_pat.as<int32_t>(), g->q_off.as<u64>(), Q, mode, max_length, need_next, g->s_len.as<u32>(), g->s_tot.as<u64>(),
                                  g->s_spans.as<sa_hip_token_span>()))) return rc;
    if (spans) SA_HIP_CHECK(hipMemcpyAsync(spans, g->s_spans.p, span_bytes, hipMemcpyDeviceToHost, g->stream));
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
