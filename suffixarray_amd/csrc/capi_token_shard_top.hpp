// capi_token_shard_top.hpp -- the C ABI of top-k next symbols and of draws over a shard set (include/sa_hip.h section 6l), included by
// sa_capi.hip behind capi_token_shards.hpp (same translation unit).  The kernels are csrc/token_shard_top.hpp.  Argument checks come
// first and touch neither the handle nor the device (token_top_args, token_sample_args: capi_token_top.hpp).  The two stopwatches are
// LaunchTimer members of the set; the host forms take the contexts up and the spans through shards_stage_spans, stage the rows in the
// merged-output buffers of the next-symbol host form (o_sym, o_cnt, o_heads) and return heads and rows through token_rows_out.
// One launch per call: the kernel keeps no per-shard lists, so there is no scratch budget and no chunk walk.
#pragma once
#include "capi_token_shards.hpp"
#include "capi_token_top.hpp"
#include "token_shard_top.hpp"

namespace {

int shards_launch_top(sa_hip_token_shards* g, const sa_hip_token_span* spans, u64 Q, u32 k, u64 budget, int32_t* symbols, u64* counts,
                      sa_hip_token_shards_top* heads) {
    bool jump = true;                                        // the walk obeys the shards' SA_HIP_TOKEN_NEXT_JUMP
    for (u32 s = 0; s < g->S; ++s) jump = jump && g->shard[s]->next_knobs.jump;
    const tq::ShardTopArgs a{g->table(), spans, Q, g->S, k, budget, symbols, counts, heads, g->top_fast ? 1 : 0};
    int rc;
    if ((rc = g->tm_tp.begin(g->stream)) || (rc = tq::launch_shard_top(g->stream, a, jump)) || (rc = g->tm_tp.end(g->stream, Q))) return rc;
    g->tp_last = Q;
    return 0;
}

int shards_launch_sample(sa_hip_token_shards* g, const sa_hip_token_span* spans, u64 Q, const u64* draws, u32 m, int32_t* symbols,
                         u32* shards, u32* ranks) {
    const tq::ShardSampleArgs a{g->table(), spans, Q, g->S, m, draws, symbols, shards, ranks};
    int rc;
    if ((rc = g->tm_sm.begin(g->stream)) || (rc = tq::launch_shard_sample(g->stream, a)) || (rc = g->tm_sm.end(g->stream, Q))) return rc;
    g->tp_last = Q;
    return 0;
}

}  // namespace

extern "C" {

int sa_hip_token_shards_top_batch_device(sa_hip_token_shards* g, const void* spans_dev, uint64_t Q, uint32_t k, uint64_t budget,
                                         void* symbols_dev, void* counts_dev, void* heads_dev) {
    const char* who = "sa_hip_token_shards_top_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_top_args(who, Q, k);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !symbols_dev || !counts_dev || !heads_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    return shards_launch_top(g, static_cast<const sa_hip_token_span*>(spans_dev), Q, k, budget, static_cast<int32_t*>(symbols_dev),
                             static_cast<u64*>(counts_dev), static_cast<sa_hip_token_shards_top*>(heads_dev));
}

int sa_hip_token_shards_top_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                  uint32_t max_length, int need_next, uint32_t k, uint64_t budget, sa_hip_token_span* spans,
                                  int32_t* symbols, uint64_t* counts, sa_hip_token_shards_top* heads) {
    const char* who = "sa_hip_token_shards_top_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_top_args(who, Q, k)) || Q == 0) return rc;
    if (!offsets || !symbols || !counts || !heads) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    if ((rc = shards_stage_spans(g, patterns, offsets, Q, mode, max_length, need_next, spans))) return rc;
    const size_t cells = (size_t)Q * k;
    if ((rc = g->o_sym.ensure(cells * 4)) || (rc = g->o_cnt.ensure(cells * 8)) ||
        (rc = g->o_heads.ensure((size_t)Q * sizeof(sa_hip_token_shards_top)))) return rc;
    if ((rc = shards_launch_top(g, g->s_spans.as<sa_hip_token_span>(), Q, k, budget, g->o_sym.as<int32_t>(), g->o_cnt.as<u64>(),
                                g->o_heads.as<sa_hip_token_shards_top>()))) return rc;
    return token_rows_out(g->stream, who, Q, k, g->o_heads.p, heads, g->o_sym.p, symbols, g->o_cnt.p, counts);
}

int sa_hip_token_shards_sample_batch_device(sa_hip_token_shards* g, const void* spans_dev, uint64_t Q, const void* draws_dev, uint32_t m,
                                            void* symbols_dev, void* shards_dev, void* ranks_dev) {
    const char* who = "sa_hip_token_shards_sample_batch_device";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_sample_args(who, Q, m);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !draws_dev || !symbols_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (shards and ranks may be NULL)
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    return shards_launch_sample(g, static_cast<const sa_hip_token_span*>(spans_dev), Q, static_cast<const u64*>(draws_dev), m,
                                static_cast<int32_t*>(symbols_dev), static_cast<u32*>(shards_dev), static_cast<u32*>(ranks_dev));
}

int sa_hip_token_shards_sample_batch(sa_hip_token_shards* g, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                     uint32_t max_length, int need_next, const uint64_t* draws, uint32_t m, sa_hip_token_span* spans,
                                     int32_t* symbols, uint32_t* shards_out, uint32_t* ranks) {
    const char* who = "sa_hip_token_shards_sample_batch";
    if (!g) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_sample_args(who, Q, m)) || Q == 0) return rc;
    if (!offsets || !draws || !symbols) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans, shards_out and ranks may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    if ((rc = set_device(g->device))) return rc;
    const size_t cells = (size_t)Q * m;
    if ((rc = g->tp_draws.ensure(cells * 8)) || (rc = g->o_sym.ensure(cells * 4)) || (rc = g->tp_at.ensure(cells * 8))) return rc;
    if ((rc = shards_stage_spans(g, patterns, offsets, Q, mode, max_length, need_next, spans))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(g->tp_draws.p, draws, cells * 8, hipMemcpyHostToDevice, g->stream));
    u32* const sh_dev = g->tp_at.as<u32>();
    u32* const rk_dev = sh_dev + cells;
    if ((rc = shards_launch_sample(g, g->s_spans.as<sa_hip_token_span>(), Q, g->tp_draws.as<u64>(), m, g->o_sym.as<int32_t>(),
                                   shards_out ? sh_dev : nullptr, ranks ? rk_dev : nullptr))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(symbols, g->o_sym.p, cells * 4, hipMemcpyDeviceToHost, g->stream));   // every cell is written
    if (shards_out) SA_HIP_CHECK(hipMemcpyAsync(shards_out, sh_dev, cells * 4, hipMemcpyDeviceToHost, g->stream));
    if (ranks) SA_HIP_CHECK(hipMemcpyAsync(ranks, rk_dev, cells * 4, hipMemcpyDeviceToHost, g->stream));
    SA_HIP_CHECK(hipStreamSynchronize(g->stream));
    return 0;
}

int sa_hip_token_shards_top_info(const sa_hip_token_shards* cg, sa_hip_token_shards_top_stats* out) {
    if (!cg || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_shards_top_info", "NULL argument");
    sa_hip_token_shards* g = const_cast<sa_hip_token_shards*>(cg);
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->tm_sp.pending || g->tm_tp.pending || g->tm_sm.pending) {
        int rc = set_device(g->device);
        if (rc || (rc = g->tm_sp.resolve()) || (rc = g->tm_tp.resolve()) || (rc = g->tm_sm.resolve())) return rc;
    }
    memset(out, 0, sizeof *out);
    out->q = g->tp_last;
    out->spans_ms = g->tm_sp.ms;
    out->top_ms = g->tm_tp.ms;
    out->sample_ms = g->tm_sm.ms;
    return 0;
}

}  // extern "C"
