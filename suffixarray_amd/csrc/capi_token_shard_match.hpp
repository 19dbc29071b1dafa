// capi_token_shard_match.hpp -- the C ABI of matching statistics over a shard set (include/sa_hip.h section 6c, matching statistics),
// included by sa_capi.hip behind capi_token_shards.hpp (same translation unit).  The kernels are csrc/token_shard_match.hpp and, for
// the documents step, csrc/token_match.hpp's tq_match_docs_kernel over the merged record.
// Argument checks come first and touch neither the set nor the device (token_match_total and token_match_docs_args are
// capi_token_match.hpp's).  The two stopwatches are LaunchTimer members of the set (launch_timer.hpp), the documents of a host form
// go up through token_upload, and the heads and written rows come back through token_rows_out (both capi_token.hpp's).
#pragma once
#include "capi_token_match.hpp"
#include "capi_token_shards.hpp"
#include "token_shard_match.hpp"

namespace {

// total >= 1; the scratch of the per-shard lengths grows here, under the set's mutex
int shards_launch_match(sa_hip_token_shards* g, const int32_t* pat, const u64* off, u64 Q, u64 total, u32 max_length,
                        sa_hip_token_shards_match* merged, sa_hip_token_span* per) {
    int rc;
    if ((rc = g->m_ms.ensure((size_t)total * g->S * sizeof(u32)))) return rc;
    tq::ShardMatchArgs a{};
    a.tab = g->table(); a.S = g->S; a.max_length = max_length;
    a.pat = pat; a.off = off; a.Q = Q; a.total = total;
    a.ms = g->m_ms.as<u32>(); a.per = per; a.merged = merged;
    if ((rc = g->tm_mt.begin(g->stream)) || (rc = tq::launch_shard_match(g->stream, a)) || (rc = g->tm_mt.end(g->stream, total))) return rc;
    g->m_last = Q;
    return 0;
}

int shards_launch_match_docs(sa_hip_token_shards* g, const sa_hip_token_shards_match* merged, const u64* off, u64 Q, u32 min_length,
                             u32 cap, u32* positions, sa_hip_token_shards_match* out_matches, sa_hip_token_match_head* heads) {
    const tq::MatchDocsArgs<sa_hip_token_shards_match> a{merged, off, Q, min_length, cap, positions, out_matches, heads};
    int rc;
    if ((rc = g->tm_md.begin(g->stream)) || (rc = tq::launch_match_docs(g->stream, a)) || (rc = g->tm_md.end(g->stream, Q))) return rc;
    g->m_last = Q;
    return 0;
}

// documents from the host into the set's staging buffers, their matches into m_merged and m_per
int shards_stage_match(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, u64 Q, u32 max_length) {
    int rc;
    const u64 total = offsets[Q];
    if ((rc = g->m_merged.ensure((size_t)total * sizeof(sa_hip_token_shards_match) + 64)) ||
        (rc = g->m_per.ensure((size_t)total * g->S * sizeof(sa_hip_token_span) + 64)) ||
        (rc = token_upload(g->q_pat, g->q_off, g->stream, patterns, offsets, Q))) return rc;
    if (total == 0) return 0;
    return shards_launch_match(g, g->q_pat.as<int32_t>(), g->q_off.as<u64>(), Q, total, max_length,
                               g->m_merged.as<sa_hip_token_shards_match>(), g->m_per.as<sa_hip_token_span>());
}

}  // namespace

extern "C" {

int sa_hip_token_shards_match_batch_device(sa_hip_token_shards* g, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                           uint64_t total, uint32_t max_length, void* merged_dev, void* per_shard_dev) {
    const char* who = "sa_hip_token_shards_match_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_match_total(who, total);
    if (rc || Q == 0) return rc;
    if (!offsets_dev || (total && (!patterns_dev || !merged_dev || !per_shard_dev))) return fail(SA_HIP_EINVAL, who, "NULL argument");
    if (total == 0) return 0;                            // a batch of empty documents: no position to answer
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    return shards_launch_match(g, static_cast<const int32_t*>(patterns_dev), static_cast<const u64*>(offsets_dev), Q, total, max_length,
                               static_cast<sa_hip_token_shards_match*>(merged_dev), static_cast<sa_hip_token_span*>(per_shard_dev));
}

int sa_hip_token_shards_match_docs_batch_device(sa_hip_token_shards* g, const void* merged_dev, const void* offsets_dev, uint64_t Q,
                                                uint32_t min_length, uint32_t cap, void* positions_dev, void* out_matches_dev,
                                                void* heads_dev) {
    const char* who = "sa_hip_token_shards_match_docs_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_match_docs_args(who, Q, min_length, cap);
    if (rc || Q == 0) return rc;
    // (merged may be NULL: a batch of empty documents has none)
    if (!offsets_dev || !heads_dev || (cap && (!positions_dev || !out_matches_dev))) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    return shards_launch_match_docs(g, static_cast<const sa_hip_token_shards_match*>(merged_dev), static_cast<const u64*>(offsets_dev), Q,
                                    min_length, cap, static_cast<u32*>(positions_dev), static_cast<sa_hip_token_shards_match*>(out_matches_dev),
                                    static_cast<sa_hip_token_match_head*>(heads_dev));
}

int sa_hip_token_shards_match_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                    uint32_t max_length, sa_hip_token_shards_match* merged, sa_hip_token_span* per_shard) {
    const char* who = "sa_hip_token_shards_match_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (Q == 0) return 0;
    if (!offsets) return fail(SA_HIP_EINVAL, who, "NULL argument");
    int rc = token_offsets_args(who, patterns, offsets, Q);
    if (rc || (rc = token_match_total(who, offsets[Q]))) return rc;
    const u64 total = offsets[Q];
    if (total == 0) return 0;
    if (!merged) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (per_shard may be NULL)
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    if ((rc = shards_stage_match(g, patterns, offsets, Q, max_length))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(merged, g->m_merged.p, (size_t)total * sizeof(sa_hip_token_shards_match), hipMemcpyDeviceToHost, g->stream));
    if (per_shard) SA_HIP_CHECK(hipMemcpyAsync(per_shard, g->m_per.p, (size_t)total * g->S * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, g->stream));
    SA_HIP_CHECK(hipStreamSynchronize(g->stream));
    return 0;
}

int sa_hip_token_shards_match_docs_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                         uint32_t max_length, uint32_t min_length, uint32_t cap, sa_hip_token_shards_match* merged,
                                         uint32_t* positions, sa_hip_token_shards_match* out_matches, sa_hip_token_match_head* heads) {
    const char* who = "sa_hip_token_shards_match_docs_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_match_docs_args(who, Q, min_length, cap);
    if (rc || Q == 0) return rc;
    if (!offsets || !heads || (cap && (!positions || !out_matches))) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (merged may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q)) || (rc = token_match_total(who, offsets[Q]))) return rc;
    const u64 total = offsets[Q];
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    const size_t cells = (size_t)Q * cap;
    if ((rc = g->m_pos.ensure(cells * 4)) || (rc = g->m_out.ensure(cells * sizeof(sa_hip_token_shards_match))) ||
        (rc = g->m_heads.ensure((size_t)Q * sizeof(sa_hip_token_match_head)))) return rc;
    if ((rc = shards_stage_match(g, patterns, offsets, Q, max_length))) return rc;
    if (merged && total) SA_HIP_CHECK(hipMemcpyAsync(merged, g->m_merged.p, (size_t)total * sizeof(sa_hip_token_shards_match), hipMemcpyDeviceToHost, g->stream));
    if ((rc = shards_launch_match_docs(g, g->m_merged.as<sa_hip_token_shards_match>(), g->q_off.as<u64>(), Q, min_length, cap,
                                       cap ? g->m_pos.as<u32>() : nullptr, cap ? g->m_out.as<sa_hip_token_shards_match>() : nullptr,
                                       g->m_heads.as<sa_hip_token_match_head>()))) return rc;
    return token_rows_out(g->stream, who, Q, cap, g->m_heads.p, heads, g->m_pos.p, positions, g->m_out.p, out_matches);
}

int sa_hip_token_shards_match_info(const sa_hip_token_shards* cg, sa_hip_token_shards_match_stats* out) {
    if (!cg || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_shards_match_info", "NULL argument");
    sa_hip_token_shards* g = const_cast<sa_hip_token_shards*>(cg);
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->tm_mt.pending || g->tm_md.pending) {
        int rc = set_device(g->device);
        if (rc || (rc = g->tm_mt.resolve()) || (rc = g->tm_md.resolve())) return rc;
    }
    memset(out, 0, sizeof *out);
    out->q = g->m_last;
    out->positions = g->tm_mt.q;
    out->match_ms = g->tm_mt.ms;
    out->docs_ms = g->tm_md.ms;
    return 0;
}

}  // extern "C"
