// capi_token.hpp -- the C ABI of the token index (include/sa_hip.h section 6), included by sa_capi.hip (same translation unit).
// The kernels and the search structures are csrc/token_query.hpp; the suffix array of sa_hip_token_index_build comes from
// the build behind sa_hip_libsais_int_device (capi_dropins.hpp: int_device).
#pragma once
#include "token_query.hpp"

struct sa_hip_token_index {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    tq::Index x;
    DevBuf q_pat, q_off, q_out;          // staging of the host-pointer query
    hipEvent_t q_ev[2] = {};             // the last search launch
    bool q_pending = false;              // recorded, not yet resolved
    u64 q_last = 0;
    double q_ms = 0.0;
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
    hipError_t e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&t->q_ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&t->q_ev[1]);
    if (e != hipSuccess) {
        sa_hip_token_index_destroy(t);
        return fail(e == hipErrorOutOfMemory ? SA_HIP_ENOMEM : SA_HIP_EHIP, who, hipGetErrorString(e));
    }
    *out = t;
    return 0;
}

int token_launch(sa_hip_token_index* t, const int32_t* pat, const u64* off, u64 Q, sa_hip_pair_u32* out) {
    SA_HIP_CHECK(hipEventRecord(t->q_ev[0], t->stream));
    const int rc = t->x.search(t->stream, pat, off, Q, out);
    if (rc) return rc;
    SA_HIP_CHECK(hipEventRecord(t->q_ev[1], t->stream));
    t->q_pending = true;
    t->q_last = Q;
    return 0;
}

}  // namespace

extern "C" {

void sa_hip_token_index_destroy(sa_hip_token_index* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    t->x.release();
    t->q_pat.release(); t->q_off.release(); t->q_out.release();
    for (int j = 0; j < 2; ++j) if (t->q_ev[j]) (void)hipEventDestroy(t->q_ev[j]);
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
    for (u64 i = 0; i < Q; ++i) if (offsets[i + 1] < offsets[i]) return fail(SA_HIP_EINVAL, who, "offsets descend");
    const u64 total = offsets[Q];   // symbols [0, offsets[Q]) are staged, nothing beyond them is read
    if (!patterns && total) return fail(SA_HIP_EINVAL, who, "NULL patterns");
    std::lock_guard<std::mutex> g(t->mu);
    int rc = set_device(t->device);
    if (rc) return rc;
    if ((rc = t->q_pat.ensure((size_t)total * 4 + 64)) || (rc = t->q_off.ensure((size_t)(Q + 1) * 8)) || (rc = t->q_out.ensure((size_t)Q * 8))) return rc;
    if (total) SA_HIP_CHECK(hipMemcpyAsync(t->q_pat.p, patterns, (size_t)total * 4, hipMemcpyHostToDevice, t->stream));
    SA_HIP_CHECK(hipMemcpyAsync(t->q_off.p, offsets, (size_t)(Q + 1) * 8, hipMemcpyHostToDevice, t->stream));
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

int sa_hip_token_index_info(const sa_hip_token_index* ct, sa_hip_token_info* out) {
    if (!ct || !out) return fail(SA_HIP_EINVAL, "sa_hip_token_index_info", "NULL argument");
    sa_hip_token_index* t = const_cast<sa_hip_token_index*>(ct);
    std::lock_guard<std::mutex> g(t->mu);
    if (t->q_pending) {
        int rc = set_device(t->device);
        if (rc) return rc;
        float ms = 0.f;
        SA_HIP_CHECK(hipEventSynchronize(t->q_ev[1]));
        SA_HIP_CHECK(hipEventElapsedTime(&ms, t->q_ev[0], t->q_ev[1]));
        t->q_ms = ms;
        t->q_pending = false;
    }
    memset(out, 0, sizeof *out);
    out->n = t->x.n;
    out->min_symbol = t->x.mn;
    out->max_symbol = t->x.mx;
    out->dir_entries = t->x.dir_entries;
    out->key_bytes = t->x.key_bytes;
    out->last_rank = t->x.last_rank;
    out->prepare_ms = t->x.prepare_ms;
    out->q = t->q_last;
    out->kernel_ms = t->q_ms;
    return 0;
}

}  // extern "C"
