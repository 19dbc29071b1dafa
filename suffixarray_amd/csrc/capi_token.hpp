// capi_token.hpp -- the C ABI of the token index (include/sa_hip.h section 6), included by sa_capi.hip (same translation unit).
// The kernels and the search structures are csrc/token_query.hpp, spans and next symbols csrc/token_next.hpp, documents csrc/token_docs.hpp (their entry points:
// capi_token_docs.hpp), per-document counts and AND groups csrc/token_all.hpp (capi_token_all.hpp), CNF queries csrc/token_cnf.hpp (capi_token_cnf.hpp), matching statistics csrc/token_match.hpp
// (capi_token_match.hpp), infinity-gram scores csrc/token_score.hpp (capi_token_score.hpp), top-k next symbols and draws
// csrc/token_top.hpp (capi_token_top.hpp); the suffix array of sa_hip_token_index_build comes from
// the build behind sa_hip_libsais_int_device (capi_dropins.hpp: int_device).
// What the capi_token*.hpp files share is here and in two small headers: the stopwatches (launch_timer.hpp), the upload of a host
// batch of contexts (token_upload), and the way of staged heads and rows to the caller (token_rows_out; its row copy is
// host_rows.hpp).  A handle lists its stopwatches and its staging buffers once (timers(), buffers()): create and destroy walk the lists.
#pragma once
#include "launch_timer.hpp"
#include "host_rows.hpp"
#include "token_query.hpp"
#include "token_next.hpp"
#include "token_docs.hpp"
#include "token_all.hpp"
#include <array>
#include <vector>

struct sa_hip_token_index {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    tq::Index x;
    DevBuf q_pat, q_off, q_out;          // staging of the host-pointer query
    LaunchTimer tm_q;                    // the last search launch
    // spans and next symbols (token_next.hpp)
    tq::NextKnobs next_knobs;
    DevBuf s_spans, s_sym, s_cnt, s_heads;   // staging of the host forms
    DevBuf s_list;                           // [0, 64): the list's length, [64, ..): ranks of the spans left to the wave form
    LaunchTimer tm_sp, tm_nx;                // the last spans / next launch
    u64 s_last = 0;                          // contexts / spans of the last launch of either kind
    bool nx_lanes = false;                   // whether the last next launch went through the lane form
    u64 nx_lane_spans = 0, nx_wave_spans = 0;
    // documents (token_docs.hpp, capi_token_docs.hpp)
    tq::Docs docs;
    DevBuf d_docs, d_offs, d_heads;          // staging of the host forms
    LaunchTimer tm_lc, tm_dc;                // the last locate / documents launch
    u64 dc_examined = 0;
    u64 docs_gen = 0;                        // bumped by every set_documents: a shard set compares it with the one it recorded
    // the rank-by-document array, per-document counts and AND groups (token_all.hpp, capi_token_all.hpp)
    tq::DocRanks ranks;
    u64 ranks_gen = 0;                       // bumped whenever RK is built, freed or dropped: a shard set compares it as it does docs_gen
    DevBuf a_goff, a_cnt, a_wr;              // group offsets of the last all launch; staging of the host doc_counts form
    u32* a_goff_pin = nullptr;               // pinned: what the asynchronous copy into a_goff reads
    size_t a_goff_pin_cap = 0;               // ... in entries
    hipEvent_t a_copied = nullptr;           // that copy is done: the pinned buffer may be rewritten
    bool a_copy_pending = false;
    LaunchTimer tm_tf, tm_al;                // the last doc_counts launch (q: spans) / all launch (q: groups)
    // matching statistics (token_match.hpp, capi_token_match.hpp)
    DevBuf m_spans, m_pos, m_out, m_heads;   // staging of the host forms
    LaunchTimer tm_mt, tm_md;                // the last match launch (q: positions) / match docs launch (q: documents)
    u64 m_last = 0;                          // documents of the last launch of either kind
    // infinity-gram scores (token_score.hpp, capi_token_score.hpp)
    DevBuf sc_scores, sc_heads;              // staging of the host form (its matches go to m_spans)
    LaunchTimer tm_sc, tm_sd;                // the last score launch (q: positions) / score docs launch (q: documents)
    u64 sc_last = 0;                         // documents of the last launch of either kind
    // top-k next symbols and draws (token_top.hpp, capi_token_top.hpp); the host forms stage through s_spans, s_sym, s_cnt, s_heads
    DevBuf tp_draws;                         // staging of the host form's draws
    LaunchTimer tm_tp, tm_sm;                // the last top / sample launch
    u64 tp_last = 0;                         // spans of the last launch of either kind
    // CNF document queries (token_cnf.hpp, capi_token_cnf.hpp); the host form stages through s_spans, d_docs, d_offs, d_heads
    DevBuf c_tab;                            // group offsets, clause offsets and negated bytes of the last cnf launch
    unsigned char* c_pin = nullptr;          // pinned: what the asynchronous copy into c_tab reads
    size_t c_pin_cap = 0;                    // ... in bytes
    hipEvent_t c_copied = nullptr;           // that copy is done: the pinned buffer may be rewritten
    bool c_copy_pending = false;
    LaunchTimer tm_cnf;                      // the last cnf launch (q: groups)

    std::array<LaunchTimer*, 14> timers() {
        return {&tm_q, &tm_sp, &tm_nx, &tm_lc, &tm_dc, &tm_tf, &tm_al, &tm_mt, &tm_md, &tm_sc, &tm_sd, &tm_tp, &tm_sm, &tm_cnf};
    }
    auto buffers() {                         // every DevBuf member above (x, docs and ranks release their own)
        return std::array{&q_pat, &q_off, &q_out, &s_spans, &s_sym, &s_cnt, &s_heads, &s_list, &d_docs, &d_offs, &d_heads, &a_goff, &a_cnt,
                          &a_wr, &m_spans, &m_pos, &m_out, &m_heads, &sc_scores, &sc_heads, &tp_draws, &c_tab};
    }
};

namespace {

int token_create(sa_hip_token_index** out, int device, const char* who) {
    const int cnt = sa_hip_device_count();
    if (cnt < 0) return cnt;
    if (device < 0 || device >= cnt) return fail(SA_HIP_EHIP, who, "no such HIP device");
    int rc = set_device(device);
    if (rc) return rc;
    sa_hip_token_index* t = new (std::nothrow) sa_hip_token_index();
    if (!t) return fail(SA_HIP_ENOMEM, who, "host allocation");
    t->device = device;
    t->x.knobs = tq::Knobs::read();
    t->next_knobs = tq::NextKnobs::read();
    hipError_t e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    for (LaunchTimer* w : t->timers()) if (e == hipSuccess) e = w->create();
    if (e == hipSuccess) e = hipEventCreate(&t->a_copied);
    if (e == hipSuccess) e = hipEventCreate(&t->c_copied);
    if (e != hipSuccess) {
        sa_hip_token_index_destroy(t);
        return fail(e == hipErrorOutOfMemory ? SA_HIP_ENOMEM : SA_HIP_EHIP, who, hipGetErrorString(e));
    }
    *out = t;
    return 0;
}

int token_launch(sa_hip_token_index* t, const int32_t* pat, const u64* off, u64 Q, sa_hip_pair_u32* out) {
    int rc;
    if ((rc = t->tm_q.begin(t->stream)) || (rc = t->x.search(t->stream, pat, off, Q, out))) return rc;
    return t->tm_q.end(t->stream, Q);
}

// what every spans / next entry point refuses before it touches the handle or the device
int token_span_args(const char* who, int mode, int need_next) {
    if (mode != 0 && mode != 1) return fail(SA_HIP_EINVAL, who, "mode is 0 (exact) or 1 (longest suffix)");
    if (need_next != 0 && need_next != 1) return fail(SA_HIP_EINVAL, who, "need_next is 0 or 1");
    return 0;
}
int token_next_args(const char* who, u64 Q, u32 cap) {
    if (cap == 0) return fail(SA_HIP_EINVAL, who, "cap == 0");
    if (Q > 0x7FFFFFFFull / cap || Q * cap >= 0x80000000ull) return fail(SA_HIP_EINVAL, who, "Q * cap >= 2^31");
    return 0;
}
int token_offsets_args(const char* who, const int32_t* patterns, const uint64_t* offsets, u64 Q) {
    for (u64 i = 0; i < Q; ++i) if (offsets[i + 1] < offsets[i]) return fail(SA_HIP_EINVAL, who, "offsets descend");
    if (!patterns && offsets[Q]) return fail(SA_HIP_EINVAL, who, "NULL patterns");
    return 0;
}

int token_launch_spans(sa_hip_token_index* t, const int32_t* pat, const u64* off, u64 Q, int mode, u32 max_length, int need_next,
                       sa_hip_token_span* out) {
    int rc;
    if ((rc = t->tm_sp.begin(t->stream)) || (rc = tq::launch_spans(t->x, t->stream, pat, off, Q, mode, max_length, need_next, out)) ||
        (rc = t->tm_sp.end(t->stream, Q))) return rc;
    t->s_last = Q;
    return 0;
}

int token_launch_next(sa_hip_token_index* t, const sa_hip_token_span* spans, u64 Q, u32 cap, int32_t* symbols, u32* counts,
                      sa_hip_token_next* heads) {
    int rc;
    if (t->next_knobs.lanes && (rc = t->s_list.ensure(64 + (size_t)Q * 4))) return rc;
    const tq::NextArgs g{spans, Q, cap, symbols, counts, heads};
    u32* n_list = t->next_knobs.lanes ? t->s_list.as<u32>() : nullptr;
    if ((rc = t->tm_nx.begin(t->stream)) || (rc = tq::launch_next(t->x, t->stream, t->next_knobs, g, n_list ? n_list + 16 : nullptr, n_list)) ||
        (rc = t->tm_nx.end(t->stream, Q))) return rc;
    t->s_last = Q;
    t->nx_lanes = t->next_knobs.lanes;
    return 0;
}

// a host batch of contexts into staging buffers (of a handle or of a shard set): the symbols [0, offsets[Q]) are staged, nothing beyond
// them is read
int token_upload(DevBuf& pat, DevBuf& off, hipStream_t stream, const int32_t* patterns, const uint64_t* offsets, u64 Q) {
    int rc;
    const u64 total = offsets[Q];
    if ((rc = pat.ensure((size_t)total * 4 + 64)) || (rc = off.ensure((size_t)(Q + 1) * 8))) return rc;
    if (total) SA_HIP_CHECK(hipMemcpyAsync(pat.p, patterns, (size_t)total * 4, hipMemcpyHostToDevice, stream));
    SA_HIP_CHECK(hipMemcpyAsync(off.p, offsets, (size_t)(Q + 1) * 8, hipMemcpyHostToDevice, stream));
    return 0;
}

// contexts from the host into the handle's staging buffers, spans into s_spans
int token_stage_spans(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, u64 Q, int mode, u32 max_length,
                      int need_next) {
    int rc;
    if ((rc = t->s_spans.ensure((size_t)Q * sizeof(sa_hip_token_span))) || (rc = token_upload(t->q_pat, t->q_off, t->stream, patterns, offsets, Q))) return rc;
    return token_launch_spans(t, t->q_pat.as<int32_t>(), t->q_off.as<u64>(), Q, mode, max_length, need_next, t->s_spans.as<sa_hip_token_span>());
}

// Host scratch of the two row arrays of one call or, in the chunked forms of a shard set, of one chunk: reserved once per call.
template <class A, class B>
struct HostRows {
    std::vector<A> a;
    std::vector<B> b;
    int reserve(const char* who, size_t cells) {
        try { a.resize(cells); b.resize(cells); } catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, who, "host allocation"); }
        return 0;
    }
};

// Staged heads [Q] and two staged [Q, cap] row arrays to the caller: the heads as they are, of every row only the entries that its
// head says were written (host_rows.hpp).  Synchronises the stream.  h holds at least Q * cap cells.
template <class Head, class A, class B>
int token_rows_out(hipStream_t stream, u64 Q, u32 cap, const void* heads_dev, Head* heads, const void* a_dev, A* a, const void* b_dev, B* b,
                   HostRows<A, B>& h) {
    const size_t cells = (size_t)Q * cap;
    SA_HIP_CHECK(hipMemcpyAsync(heads, heads_dev, (size_t)Q * sizeof(Head), hipMemcpyDeviceToHost, stream));
    if (cells) {
        SA_HIP_CHECK(hipMemcpyAsync(h.a.data(), a_dev, cells * sizeof(A), hipMemcpyDeviceToHost, stream));
        SA_HIP_CHECK(hipMemcpyAsync(h.b.data(), b_dev, cells * sizeof(B), hipMemcpyDeviceToHost, stream));
    }
    SA_HIP_CHECK(hipStreamSynchronize(stream));
    const StridedLen written{&heads[0].written, sizeof(Head)};
    copy_written_rows(a, h.a.data(), Q, cap, written);
    copy_written_rows(b, h.b.data(), Q, cap, written);
    return 0;
}
// ... of a call that is not chunked: the scratch is its own
template <class Head, class A, class B>
int token_rows_out(hipStream_t stream, const char* who, u64 Q, u32 cap, const void* heads_dev, Head* heads, const void* a_dev, A* a,
                   const void* b_dev, B* b) {
    HostRows<A, B> h;
    const int rc = h.reserve(who, (size_t)Q * cap);
    return rc ? rc : token_rows_out(stream, Q, cap, heads_dev, heads, a_dev, a, b_dev, b, h);
}

// next symbols of the spans in s_spans to the host
int token_stage_next(sa_hip_token_index* t, const char* who, u64 Q, u32 cap, int32_t* symbols, u32* counts, sa_hip_token_next* heads) {
    int rc;
    const size_t cells = (size_t)Q * cap;
    if ((rc = t->s_sym.ensure(cells * 4)) || (rc = t->s_cnt.ensure(cells * 4)) || (rc = t->s_heads.ensure((size_t)Q * sizeof(sa_hip_token_next)))) return rc;
    if ((rc = token_launch_next(t, t->s_spans.as<sa_hip_token_span>(), Q, cap, t->s_sym.as<int32_t>(), t->s_cnt.as<u32>(), t->s_heads.as<sa_hip_token_next>()))) return rc;
    return token_rows_out(t->stream, who, Q, cap, t->s_heads.p, heads, t->s_sym.p, symbols, t->s_cnt.p, counts);
}

}  // namespace

extern "C" {

void sa_hip_token_index_destroy(sa_hip_token_index* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    t->x.release();
    t->docs.release();
    t->ranks.release();
    for (DevBuf* b : t->buffers()) b->release();
    if (t->a_goff_pin) (void)hipHostFree(t->a_goff_pin);
    if (t->a_copied) (void)hipEventDestroy(t->a_copied);
    if (t->c_pin) (void)hipHostFree(t->c_pin);
    if (t->c_copied) (void)hipEventDestroy(t->c_copied);
    for (LaunchTimer* w : t->timers()) w->destroy();
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
}

int sa_hip_token_index_build(sa_hip_token_index** out, const int32_t* T_host, int32_t n, int32_t k, int device) {
    const char* who = "sa_hip_token_index_build";
    if (!out) return fail(SA_HIP_EINVAL, who, "out == NULL");
    *out = nullptr;
    if (n < 0) return fail(SA_HIP_EINVAL, who, "negative length");
    if (!T_host && n) return fail(SA_HIP_EINVAL, who, "NULL text");
    if (n >= 2 && k < 1) return fail(SA_HIP_EINVAL, who, "k < 1");
    sa_hip_token_index* t = nullptr;
    int rc = token_create(&t, device, who);
    if (rc) return rc;
    auto run = [&]() -> int {
        int r2 = t->x.reserve((u32)n);
        if (r2 || n == 0) return r2;
        SA_HIP_CHECK(hipMemcpyAsync(t->x.text.p, T_host, (size_t)n * 4, hipMemcpyHostToDevice, t->stream));
        SA_HIP_CHECK(hipMemsetAsync(t->x.sa.p, 0, 4, t->stream));   // n == 1: SA = {0}
        SA_HIP_CHECK(hipStreamSynchronize(t->stream));
        // k = INT32_MAX admits every non-negative symbol: the build underneath takes a 64-bit k, and 2^31 - 1 is a symbol here
        const int64_t k64 = k == INT32_MAX ? (int64_t)INT32_MAX + 1 : (int64_t)k;
        if (n >= 2 && (r2 = int_device<int32_t, int32_t>(t->x.text.as<int32_t>(), t->x.sa.as<int32_t>(), n, k64, device, nullptr, who))) return r2;
        return t->x.prepare(t->stream, who);
    };
    rc = run();
    if (rc) { sa_hip_token_index_destroy(t); return rc; }
    *out = t;
    return 0;
}

int sa_hip_token_index_load_device(sa_hip_token_index** out, const int32_t* T_dev, const int32_t* SA_dev, int32_t n, int device) {
    const char* who = "sa_hip_token_index_load_device";
    if (!out) return fail(SA_HIP_EINVAL, who, "out == NULL");
    *out = nullptr;
    if (n < 0) return fail(SA_HIP_EINVAL, who, "negative length");
    if ((!T_dev || !SA_dev) && n) return fail(SA_HIP_EINVAL, who, "NULL argument");
    sa_hip_token_index* t = nullptr;
    int rc = token_create(&t, device, who);
    if (rc) return rc;
    auto run = [&]() -> int {
        int r2 = t->x.reserve((u32)n);
        if (r2 || n == 0) return r2;
        SA_HIP_CHECK(hipMemcpyAsync(t->x.text.p, T_dev, (size_t)n * 4, hipMemcpyDeviceToDevice, t->stream));
        SA_HIP_CHECK(hipMemcpyAsync(t->x.sa.p, SA_dev, (size_t)n * 4, hipMemcpyDeviceToDevice, t->stream));
        return t->x.prepare(t->stream, who);
    };
    rc = run();
    if (rc) { sa_hip_token_index_destroy(t); return rc; }
    *out = t;
    return 0;
}

int sa_hip_token_index_query_batch_device(sa_hip_token_index* t, const void* patterns_dev, const void* offsets_dev, uint64_t Q, void* out_dev) {
    const char* who = "sa_hip_token_index_query_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (Q == 0) return 0;
    if (!offsets_dev || !out_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (patterns may be NULL: a batch of empty patterns)
    std::lock_guard<std::mutex> g(t->mu);
    int rc = set_device(t->device);
    if (rc) return rc;
    return token_launch(t, static_cast<const int32_t*>(patterns_dev), static_cast<const u64*>(offsets_dev), Q, static_cast<sa_hip_pair_u32*>(out_dev));
}

int sa_hip_token_index_query_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, sa_hip_pair_u32* out) {
    const char* who = "sa_hip_token_index_query_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    if (Q == 0) return 0;
    if (!offsets || !out) return fail(SA_HIP_EINVAL, who, "NULL argument");
    int rc = token_offsets_args(who, patterns, offsets, Q);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    if ((rc = t->q_out.ensure((size_t)Q * 8)) || (rc = token_upload(t->q_pat, t->q_off, t->stream, patterns, offsets, Q))) return rc;
    if ((rc = token_launch(t, t->q_pat.as<int32_t>(), t->q_off.as<u64>(), Q, t->q_out.as<sa_hip_pair_u32>()))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(out, t->q_out.p, (size_t)Q * 8, hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    return 0;
}

int sa_hip_token_index_sync(sa_hip_token_index* t) {
    if (!t) return fail(SA_HIP_EINVAL, "sa_hip_token_index_sync", "NULL handle");
    std::lock_guard<std::mutex> g(t->mu);
    int rc = set_device(t->device);
    if (rc) return rc;
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    return 0;
}

const void* sa_hip_token_index_text_dev(const sa_hip_token_index* t) { return t ? t->x.text.p : nullptr; }
const void* sa_hip_token_index_sa_dev(const sa_hip_token_index* t) { return t ? t->x.sa.p : nullptr; }

int sa_hip_token_index_get_sa_range(sa_hip_token_index* t, uint64_t first, uint64_t count, int32_t* out_host) {
    const char* who = "sa_hip_token_index_get_sa_range";
    if (!t || (!out_host && count)) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    if (first > t->x.n || count > t->x.n - first) return fail(SA_HIP_EINVAL, who, "range beyond the suffix array");
    if (count == 0) return 0;
    int rc = set_device(t->device);
    if (rc) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(out_host, t->x.sa.as<int32_t>() + first, (size_t)count * 4, hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    return 0;
}

// the two search structures as prepare() left them (tests compare them entry by entry with their definitions)
int sa_hip_token_index_get_dir_range(sa_hip_token_index* t, uint64_t first, uint64_t count, uint32_t* out_host) {
    const char* who = "sa_hip_token_index_get_dir_range";
    if (!t || !out_host) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    if (!t->x.dir_entries) return fail(SA_HIP_EINVAL, who, "the handle has no directory");
    if (first > t->x.dir_entries || count > t->x.dir_entries - first) return fail(SA_HIP_EINVAL, who, "range beyond the directory");
    if (count == 0) return 0;
    int rc = set_device(t->device);
    if (rc) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(out_host, t->x.dir.as<u32>() + first, (size_t)count * 4, hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    return 0;
}

int sa_hip_token_index_get_key_range(sa_hip_token_index* t, uint64_t first, uint64_t count, uint64_t* out_host) {
    const char* who = "sa_hip_token_index_get_key_range";
    if (!t || !out_host) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    if (!t->x.key_bytes) return fail(SA_HIP_EINVAL, who, "the handle has no key array");
    if (first > t->x.n || count > t->x.n - first) return fail(SA_HIP_EINVAL, who, "range beyond the key array");
    if (count == 0) return 0;
    int rc = set_device(t->device);
    if (rc) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(out_host, t->x.keys.as<u64>() + first, (size_t)count * 8, hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    return 0;
}

int sa_hip_token_index_info(const sa_hip_token_index* ct, sa_hip_token_info* out) {
    if (!ct || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_index_info", "NULL argument");
    sa_hip_token_index* t = const_cast<sa_hip_token_index*>(ct);
    std::lock_guard<std::mutex> g(t->mu);
    if (t->tm_q.pending) {
        int rc = set_device(t->device);
        if (rc || (rc = t->tm_q.resolve())) return rc;
    }
    memset(out, 0, sizeof *out);
    out->n = t->x.n;
    out->min_symbol = t->x.mn;
    out->max_symbol = t->x.mx;
    out->dir_entries = t->x.dir_entries;
    out->key_bytes = t->x.key_bytes;
    out->last_rank = t->x.last_rank;
    out->prepare_ms = t->x.prepare_ms;
    out->q = t->tm_q.q;
    out->kernel_ms = t->tm_q.ms;
    return 0;
}

// ---- spans and next symbols.  Argument checks come first and touch neither the handle nor the device. ----------------------

int sa_hip_token_index_spans_batch_device(sa_hip_token_index* t, const void* patterns_dev, const void* offsets_dev, uint64_t Q, int mode,
                                          uint32_t max_length, int need_next, void* spans_dev) {
    const char* who = "sa_hip_token_index_spans_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || Q == 0) return rc;
    if (!offsets_dev || !spans_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (patterns may be NULL: a batch of empty contexts)
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    return token_launch_spans(t, static_cast<const int32_t*>(patterns_dev), static_cast<const u64*>(offsets_dev), Q, mode, max_length, need_next,
                              static_cast<sa_hip_token_span*>(spans_dev));
}

int sa_hip_token_index_spans_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                   uint32_t max_length, int need_next, sa_hip_token_span* spans) {
    const char* who = "sa_hip_token_index_spans_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || Q == 0) return rc;
    if (!offsets || !spans) return fail(SA_HIP_EINVAL, who, "NULL argument");
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    if ((rc = token_stage_spans(t, patterns, offsets, Q, mode, max_length, need_next))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(spans, t->s_spans.p, (size_t)Q * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, t->stream));
    SA_HIP_CHECK(hipStreamSynchronize(t->stream));
    return 0;
}

int sa_hip_token_index_next_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, uint32_t cap, void* symbols_dev,
                                         void* counts_dev, void* heads_dev) {
    const char* who = "sa_hip_token_index_next_batch_device";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_next_args(who, Q, cap);
    if (rc || Q == 0) return rc;
    if (!spans_dev || !symbols_dev || !counts_dev || !heads_dev) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    return token_launch_next(t, static_cast<const sa_hip_token_span*>(spans_dev), Q, cap, static_cast<int32_t*>(symbols_dev),
                             static_cast<u32*>(counts_dev), static_cast<sa_hip_token_next*>(heads_dev));
}

int sa_hip_token_index_next_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                  uint32_t max_length, int need_next, uint32_t cap, sa_hip_token_span* spans, int32_t* symbols,
                                  uint32_t* counts, sa_hip_token_next* heads) {
    const char* who = "sa_hip_token_index_next_batch";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_span_args(who, mode, need_next);
    if (rc || (rc = token_next_args(who, Q, cap)) || Q == 0) return rc;
    if (!offsets || !symbols || !counts || !heads) return fail(SA_HIP_EINVAL, who, "NULL argument");   // (spans may be NULL)
    if ((rc = token_offsets_args(who, patterns, offsets, Q))) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if ((rc = set_device(t->device))) return rc;
    if ((rc = token_stage_spans(t, patterns, offsets, Q, mode, max_length, need_next))) return rc;
    if (spans) SA_HIP_CHECK(hipMemcpyAsync(spans, t->s_spans.p, (size_t)Q * sizeof(sa_hip_token_span), hipMemcpyDeviceToHost, t->stream));
    return token_stage_next(t, who, Q, cap, symbols, counts, heads);
}

int sa_hip_token_index_next_of_spans(sa_hip_token_index* t, const sa_hip_token_span* spans, uint64_t Q, uint32_t cap, int32_t* symbols,
                                     uint32_t* counts, sa_hip_token_next* heads) {
    const char* who = "sa_hip_token_index_next_of_spans";
    if (!t) return fail(SA_HIP_EINVAL, who, "NULL handle");
    int rc = token_next_args(who, Q, cap);
    if (rc || Q == 0) return rc;
    if (!spans || !symbols || !counts || !heads) return fail(SA_HIP_EINVAL, who, "NULL argument");
    std::lock_guard<std::mutex> g(t->mu);
    for (u64 i = 0; i < Q; ++i)
        if (spans[i].first > t->x.n || spans[i].count > t->x.n - spans[i].first) return fail(SA_HIP_EINVAL, who, "span beyond the suffix array");
    if ((rc = set_device(t->device))) return rc;
    if ((rc = t->s_spans.ensure((size_t)Q * sizeof(sa_hip_token_span)))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(t->s_spans.p, spans, (size_t)Q * sizeof(sa_hip_token_span), hipMemcpyHostToDevice, t->stream));
    return token_stage_next(t, who, Q, cap, symbols, counts, heads);
}

int sa_hip_token_index_next_info(const sa_hip_token_index* ct, sa_hip_token_next_info* out) {
    if (!ct || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_index_next_info", "NULL argument");
    sa_hip_token_index* t = const_cast<sa_hip_token_index*>(ct);
    std::lock_guard<std::mutex> g(t->mu);
    if (t->tm_sp.pending || t->tm_nx.pending) {
        int rc = set_device(t->device);
        if (rc || (rc = t->tm_sp.resolve())) return rc;
        if (t->tm_nx.pending) {
            u32 left = 0;   // the list's length: the spans the lane form left to the wave form
            if (t->nx_lanes) {
                SA_HIP_CHECK(hipMemcpyAsync(&left, t->s_list.p, sizeof left, hipMemcpyDeviceToHost, t->stream));
                SA_HIP_CHECK(hipStreamSynchronize(t->stream));
            }
            if ((rc = t->tm_nx.resolve())) return rc;
            t->nx_wave_spans = t->nx_lanes ? (u64)left : t->tm_nx.q;
            t->nx_lane_spans = t->tm_nx.q - t->nx_wave_spans;
        }
    }
    memset(out, 0, sizeof *out);
    out->q = t->s_last;
    out->spans_ms = t->tm_sp.ms;
    out->next_ms = t->tm_nx.ms;
    out->lane_spans = t->nx_lane_spans;
    out->wave_spans = t->nx_wave_spans;
    return 0;
}

}  // extern "C"
