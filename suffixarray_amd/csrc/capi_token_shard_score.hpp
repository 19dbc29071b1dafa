// capi_token_shard_score.hpp -- the C ABI of infinity-gram scores over a shard set (include/sa_hip.h section 6j), included by
// sa_capi.hip behind capi_token_shard_match.hpp (same translation unit).  The kernels are csrc/token_shard_score.hpp.
// Argument checks come first and touch neither the set nor the device.  The two stopwatches are LaunchTimer members of the set
// (launch_timer.hpp); the host form goes through shards_stage_match of capi_token_shard_match.hpp, which uploads the documents
// (token_upload) and runs the match launches with their stopwatch into m_merged, and lets the score launches write their per-shard
// spans over m_per, which the match launches are done with by then.
#pragma once
#include "capi_token_shard_match.hpp"
#include "token_shard_score.hpp"

static_assert(sizeof(sa_hip_token_shards_score) == 24 && alignof(sa_hip_token_shards_score) == 8, "sa_hip_token_shards_score is 24 bytes");

namespace {

// which way the host form takes: true runs the match launches first and hands the merged records to the score launches (DESIGN.md
// 9u: until the table there says otherwise, by 9s's result for the single index)
constexpr bool SHARDS_SCORE_HOST_MATCHES = true;

// total >= 1; the three scratch planes grow here, under the set's mutex
int shards_launch_score(sa_hip_token_shards* g, const int32_t* pat, const u64* off, u64 Q, u64 total, u32 max_length,
                        const sa_hip_token_shards_match* merged, sa_hip_token_shards_score* scores, sa_hip_token_span* per) {
    int rc;
    if ((rc = g->sc_w.ensure((size_t)total * g->S * 3 * sizeof(u32)))) return rc;
    tq::ShardScoreArgs a{};
    a.tab = g->table(); a.S = g->S; a.max_n = g->max_n; a.max_length = max_length;
    a.pat = pat; a.off = off; a.Q = Q; a.total = total;
    a.merged = merged; a.w = g->sc_w.as<u32>(); a.scores = scores; a.per = per;
    if ((rc = g->tm_sc.begin(g->stream)) || (rc = tq::launch_shard_score(g->stream, a)) || (rc = g->tm_sc.end(g->stream, total))) return rc;
    g->sc_last = Q;
    return 0;
}

int shards_launch_score_docs(sa_hip_token_shards* g, const sa_hip_token_shards_score* scores, const u64* off, u64 Q,
                             sa_hip_token_score_head* heads) {
    const tq::ShardScoreDocsArgs a{scores, off, Q, heads};
    int rc;
    if ((rc = g->tm_sd.begin(g->stream)) || (rc = tq::launch_shard_score_docs(g->stream, a)) || (rc = g->tm_sd.end(g->stream, Q))) return rc;
    g->sc_last = Q;
    return 0;
}

}  // namespace

extern "C" {

int sa_hip_token_shards_score_batch_device(sa_hip_token_shards* g, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                           uint64_t total, uint32_t max_length, const void* merged_dev, void* scores_dev,
                                           void* per_shard_dev) {
    const char* who = "sa_hip_token_shards_score_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_match_total(who, total);
    if (rc || Q == 0) return rc;
    if (!offsets_dev || (total && (!patterns_dev || !scores_dev || !per_shard_dev))) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (merged may be NULL: way 2)
    if (total == 0) return 0;                            // a batch of empty documents: no position to answer
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    return shards_launch_score(g, static_cast<const int32_t*>(patterns_dev), static_cast<const u64*>(offsets_dev), Q, total, max_length,
                               static_cast<const sa_hip_token_shards_match*>(merged_dev), static_cast<sa_hip_token_shards_score*>(scores_dev),
                               static_cast<sa_hip_token_span*>(per_shard_dev));
}

int sa_hip_token_shards_score_docs_batch_device(sa_hip_token_shards* g, const void* scores_dev, const void* offsets_dev, uint64_t Q,
                                                void* heads_dev) {
    const char* who = "sa_hip_token_shards_score_docs_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (Q == 0) return 0;
    if (!offsets_dev || !heads_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (scores may be NULL: a batch of empty documents has none)
    std::lock_guard<std::mutex> lk(g->mu);
    int rc = set_device(g->device);
    if (rc) return rc;
    return shards_launch_score_docs(g, static_cast<const sa_hip_token_shards_score*>(scores_dev), static_cast<const u64*>(offsets_dev), Q,
                                    static_cast<sa_hip_token_score_head*>(heads_dev));
}

int sa_hip_token_shards_score_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                    uint32_t max_length, sa_hip_token_shards_score* scores, sa_hip_token_span* per_shard,
                                    sa_hip_token_score_head* heads) {
    const char* who = "sa_hip_token_shards_score_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (Q == 0) return 0;
    if (!offsets || (!scores && !per_shard && !heads)) return fail(SA_HIP_EINVAL, who, "NULL argument");
    int rc = token_offsets_args(who, patterns, offsets, Q);
    if (rc || (rc = token_match_total(who, offsets[Q]))) return rc;
    const u64 total = offsets[Q];
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    const size_t per_bytes = (size_t)total * g->S * sizeof(sa_hip_token_span);
    if ((rc = g->sc_scores.ensure((size_t)total * sizeof(sa_hip_token_shards_score) + 64)) ||
        (rc = g->sc_heads.ensure((size_t)Q * sizeof(sa_hip_token_score_head)))) return rc;
    if (SHARDS_SCORE_HOST_MATCHES) rc = shards_stage_match(g, patterns, offsets, Q, max_length);
    else if (!(rc = g->m_per.ensure(per_bytes + 64))) rc = token_upload(g->q_pat, g->q_off, g->stream, patterns, offsets, Q);
    if (rc) return rc;
    if (total) {
        if ((rc = shards_launch_score(g, g->q_pat.as<int32_t>(), g->q_off.as<u64>(), Q, total, max_length,
                                      SHARDS_SCORE_HOST_MATCHES ? g->m_merged.as<sa_hip_token_shards_match>() : nullptr,
                                      g->sc_scores.as<sa_hip_token_shards_score>(), g->m_per.as<sa_hip_token_span>()))) return rc;
        if (scores) SA_HIP_CHECK(hipMemcpyAsync(scores, g->sc_scores.p, (size_t)total * sizeof(sa_hip_token_shards_score), hipMemcpyDeviceToHost, g->stream));
        if (per_shard) SA_HIP_CHECK(hipMemcpyAsync(per_shard, g->m_per.p, per_bytes, hipMemcpyDeviceToHost, g->stream));
    }
    if (heads) {
        if ((rc = shards_launch_score_docs(g, g->sc_scores.as<sa_hip_token_shards_score>(), g->q_off.as<u64>(), Q,
                                           g->sc_heads.as<sa_hip_token_score_head>()))) return rc;
        SA_HIP_CHECK(hipMemcpyAsync(heads, g->sc_heads.p, (size_t)Q * sizeof(sa_hip_token_score_head), hipMemcpyDeviceToHost, g->stream));
    }
    SA_HIP_CHECK(hipStreamSynchronize(g->stream));
    return 0;
}

int sa_hip_token_shards_score_info(const sa_hip_token_shards* cg, sa_hip_token_shards_score_stats* out) {
    if (!cg || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_shards_score_info", "NULL argument");
    sa_hip_token_shards* g = const_cast<sa_hip_token_shards*>(cg);
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->tm_mt.pending || g->tm_sc.pending || g->tm_sd.pending) {
        int rc = set_device(g->device);
        if (rc || (rc = g->tm_mt.resolve()) || (rc = g->tm_sc.resolve()) || (rc = g->tm_sd.resolve())) return rc;
    }
    memset(out, 0, sizeof *out);
    out->q = g->sc_last;
    out->positions = g->tm_sc.q;
    out->match_ms = g->tm_mt.ms;
    out->score_ms = g->tm_sc.ms;
    out->docs_ms = g->tm_sd.ms;
    return 0;
}

}  // extern "C"
