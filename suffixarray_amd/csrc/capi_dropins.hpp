// capi_dropins.hpp -- the call-compatible entry points of libsa_hip.so: libsais / libsais64 (suffix array, PLCP / LCP, BWT and its
// inverse, integer alphabets), their device forms, and the engine.c-compatible wrappers with the stand-alone helpers that go with
// them (sa_hip_sort_pairs, the CSV column extractor, the synthetic inputs).  Part of sa_capi.hip's translation unit: included
// there once, after struct sa_hip_index and set_device(), before the handle API (whose batched record retrieval borrows the ring
// of g_oneshot).
//
// Two procedures are written once here and used by every entry point below:
//   HostCall    a host drop-in call (host pointers in, host result out): the lock of the process-level workspace, the call
//               breakdown and its clock, the cached index handle, the drop-ins' own stream and the ring of pinned slabs
//   DeviceCall  a per-call device form: the device, a stream of its own, and the release of the call's buffers on every way out
#pragma once
#include <functional>
#include <type_traits>

namespace {

// one-shot helper for the libsais-/engine-compatible wrappers
struct TempIndex {
    sa_hip_index* idx = nullptr;
    ~TempIndex() { if (idx) sa_hip_index_destroy(idx); }
};

// The process-level workspace of the host drop-ins: a cached index handle whose device buffers are allocated once and grow on
// demand, and the ring of pinned slabs for both legs over PCIe (host_io.hpp).  sa_hip_release_workspace() gives the memory back;
// sa_hip_last_call_breakdown() tells where the time of the last call went.  The ring also carries the large host legs of
// sa_hip_index_query_rows_batch (under `mu`; lock order: a caller's own idx->mu first, then g_oneshot.mu -- the drop-ins take
// g_oneshot.mu and then the mutex of the CACHED handle, which no caller ever holds: HostCall::attach_index).
struct OneShot {
    std::mutex mu;
    sa_hip_index* idx = nullptr;
    PinnedRing ring;
    sa_hip_call_breakdown last{};
    // the LCP drop-ins (sa_hip_libsais[64]_plcp / _lcp): their own device buffers beside the cached index, same ring
    lcp::Workspace lcp;
    DevBuf l_text, l_sa, l_in, l_out;
    hipStream_t l_stream = nullptr;
    int l_device = -1;
    // the BWT drop-ins (sa_hip_libsais[64]_bwt / _unbwt): U / I on the device, the inverse's scratch; same stream
    bwt::Workspace bwt;
    DevBuf b_u, b_aux;
    // the integer-alphabet drop-ins (sa_hip_libsais_int, sa_hip_libsais64_long): the text (4 or 8 bytes per symbol), the alphabet
    // tables; the 64-bit build's buffers are given back after every call.  Same stream.
    ints::Workspace ints;
    DevBuf i_text;
    // everything above but the cached index and the ring: the stream and the device buffers of the LCP, BWT and integer drop-ins
    void release_device_buffers() {
        if (l_device >= 0) (void)hipSetDevice(l_device);
        if (l_stream) (void)hipStreamDestroy(l_stream);
        l_stream = nullptr;
        lcp.release(); l_text.release(); l_sa.release(); l_in.release(); l_out.release();
        bwt.release(); b_u.release(); b_aux.release();
        ints.release(); i_text.release();
        l_device = -1;
    }
} g_oneshot;

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// One host drop-in call.  Holds g_oneshot.mu from construction to return.  The breakdown's phases (workspace, upload, build,
// download) are closed one after the other with phase(); commit() ends the call on its success path and is the only place that
// writes g_oneshot.last -- a call that fails, or that is served by the opt-in host path, leaves the last breakdown alone.
struct HostCall {
    OneShot& g = g_oneshot;
    std::lock_guard<std::mutex> lock{g.mu};
    std::unique_lock<std::mutex> ilock;   // the cached handle's mutex (attach_index)
    const Clock::time_point t_all = Clock::now();
    Clock::time_point t0 = t_all;         // start of the open phase
    sa_hip_call_breakdown bd{};
    sa_hip_index* idx = nullptr;          // set by attach_index
    int device = 0;                       // set by attach_stream / attach_index

    explicit HostCall(u64 n) { bd.n = n; }
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;

    void phase(double* ms) { *ms = ms_since(t0); t0 = Clock::now(); }
    double phase_ms() const { return ms_since(t0); }   // of the open phase, so far
    int commit() { bd.total_ms = ms_since(t_all); g.last = bd; return 0; }

    // The cached index handle, with room for n characters, locked and its device current.  Lock order: g.mu (held since the
    // constructor), then idx->mu.
    int attach_index(u64 n) {
        int rc;
        if (g.idx && g.idx->b.n_max < n) { sa_hip_index_destroy(g.idx); g.idx = nullptr; }
        if (!g.idx && (rc = sa_hip_index_create(&g.idx, n ? n : 1, device))) return rc;
        idx = g.idx;
        ilock = std::unique_lock<std::mutex>(idx->mu);
        device = idx->device;
        if ((rc = set_device(device))) return rc;
        return ring_here();
    }

    // The drop-ins' own stream and buffers on the cached handle's device (device 0 without one).  reused(): the family's own
    // "nothing has to be allocated" condition, asked after the buffers of another device are gone and before the stream is made.
    template <class Reused>
    int attach_stream(Reused reused) {
        device = g.idx ? g.idx->device : 0;
        const int rc = set_device(device);
        if (rc) return rc;
        own_buffers();
        bd.workspace_reused = reused() ? 1u : 0u;
        if (!g.l_stream) SA_HIP_CHECK(hipStreamCreateWithFlags(&g.l_stream, hipStreamNonBlocking));
        return ring_here();
    }

    // the drop-ins' own device buffers live on one device at a time
    void own_buffers() {
        if (g.l_device >= 0 && g.l_device != device) g.release_device_buffers();
        g.l_device = device;
    }

private:
    int ring_here() {
        if (g.ring.ready && g.ring.device != device) g.ring.destroy();   // (its copy stream belongs to another device: a rows batch made it there)
        return g.ring.init();
    }
};

// One per-call device form: the device made current and a non-blocking stream of the call's own.  On every way out of the caller
// the destructor waits for the stream, gives back what was registered with it -- nothing else -- and destroys the stream.  The
// registered objects are declared before the DeviceCall (they must outlive it).
struct DeviceCall {
    hipStream_t stream = nullptr;
    std::vector<std::function<void()>> cleanup;

    DeviceCall() = default;
    DeviceCall(const DeviceCall&) = delete;
    DeviceCall& operator=(const DeviceCall&) = delete;

    int open(int device, bool with_stream = true) {
        const int rc = set_device(device);
        if (rc) return rc;
        if (with_stream) SA_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return 0;
    }
    template <class... T>
    void releases(T&... bufs) { (cleanup.push_back([&bufs] { bufs.release(); }), ...); }   // DevBufs, lcp:: / bwt:: / ints::Workspace
    void at_close(std::function<void()> fn) { cleanup.push_back(std::move(fn)); }
    ~DeviceCall() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto& fn : cleanup) fn();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// (libsais.h:84: the byte histogram, when asked for)
template <class FREQ>
void byte_histogram(const uint8_t* T, uint64_t n, FREQ* freq) {
    for (int c = 0; c < 256; ++c) freq[c] = 0;
    for (uint64_t i = 0; i < n; ++i) ++freq[T[i]];
}

// ---- libsais / engine.c suffix arrays: sa_hip_libsais[64][_omp], sa_hip_construct_truncated_suffix_array -------------------

// OUT = uint32_t / int32_t (libsais layout) or int64_t (libsais64 layout)
template <typename OUT, typename FREQ>
int oneshot_build(const uint8_t* T, uint64_t n, uint32_t L, OUT* out, FREQ* freq) {
    HostCall hc(n);
    OneShot& g = hc.g;
    sa_hip_call_breakdown& bd = hc.bd;
    if (!g.idx && host_path_allowed() && sa_hip_device_count() <= 0) {   // opt-in no-GPU path (host_index.hpp)
        if (n > HOST_MAX_N) return fail(SA_HIP_EINVAL, "the host path (no HIP device) holds at most 2^24 bytes");
        try {
            HostIndex h;
            h.set_text(T, n);
            h.build(L);
            for (u64 i = 0; i < n; ++i) out[i] = (OUT)h.sa[i];
            if (freq) for (int c = 0; c < 256; ++c) freq[c] = (FREQ)h.freq[c];
        } catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, "out of host memory"); }
        return 0;
    }
    int rc;
    // workspace: reuse the cached handle when it is large enough
    bd.workspace_reused = (g.idx && g.idx->b.n_max >= n && g.ring.ready) ? 1u : 0u;
    if ((rc = hc.attach_index(n))) return rc;
    sa_hip_index* idx = hc.idx;
    hc.phase(&bd.workspace_ms);
    if ((rc = ring_upload(g.ring, idx->stream, idx->device, idx->b.text.p, T, (size_t)n))) return rc;
    hc.phase(&bd.upload_ms);
    if ((rc = rebuild(idx, n, L))) return rc;
    SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
    hc.phase(&bd.build_ms);
    bd.build_device_ms = idx->b.stats.total_ms;
    if ((rc = ring_download(g.ring, idx->device, (const u32*)idx->b.sa, out, (size_t)n))) return rc;
    hc.phase(&bd.download_ms);
    if (freq) for (int c = 0; c < 256; ++c) freq[c] = (FREQ)idx->b.freq[c];
    return hc.commit();
}

}  // namespace

extern "C" {

int sa_hip_last_call_breakdown(sa_hip_call_breakdown* out) {
    if (!out) return fail(SA_HIP_EINVAL, "sa_hip_last_call_breakdown: NULL argument");
    std::lock_guard<std::mutex> lock(g_oneshot.mu);
    *out = g_oneshot.last;
    return 0;
}

void sa_hip_release_workspace(void) {
    std::lock_guard<std::mutex> lock(g_oneshot.mu);
    if (g_oneshot.idx) { (void)hipSetDevice(g_oneshot.idx->device); sa_hip_index_destroy(g_oneshot.idx); g_oneshot.idx = nullptr; }
    g_oneshot.release_device_buffers();
    g_oneshot.ring.destroy();
}

int32_t sa_hip_libsais_omp(const uint8_t* T, int32_t* SA, int32_t n, int32_t fs, int32_t* freq, int32_t threads) {
    if (T == nullptr || SA == nullptr || n < 0 || fs < 0 || threads < 0) return fail(SA_HIP_EINVAL, "sa_hip_libsais: invalid arguments");
    return oneshot_build<int32_t, int32_t>(T, (uint64_t)n, 0, SA, freq);
}

int32_t sa_hip_libsais(const uint8_t* T, int32_t* SA, int32_t n, int32_t fs, int32_t* freq) {
    return sa_hip_libsais_omp(T, SA, n, fs, freq, 0);
}

}  // extern "C"

// ---- texts beyond 2^32 - 2 bytes: 64-bit suffix indices (big_build.hpp; libsais64.c:6684 -> libsais64_main) ----------------

extern "C" int sa_hip_libsais64_device(const void* text_dev, int64_t* sa_dev, int64_t n, int device, sa_hip_big_stats* stats_out) {
    if ((!text_dev || !sa_dev) && n) return fail(SA_HIP_EINVAL, "sa_hip_libsais64_device: NULL argument");
    if (n < 0) return fail(SA_HIP_EINVAL, "sa_hip_libsais64_device: negative length");
    big::BigBuilder b;
    DeviceCall dc;
    int rc = dc.open(device);
    if (rc) return rc;
    dc.at_close([&b] { b.destroy(); });
    b.stream = dc.stream;
    rc = b.build(static_cast<const u8*>(text_dev), (u64)n, reinterpret_cast<u64*>(sa_dev));
    if (stats_out) {
        stats_out->sigma = b.stats.sigma; stats_out->bits_per_symbol = b.stats.bits_per_symbol; stats_out->initial_chars = b.stats.initial_chars;
        stats_out->sort_passes = b.stats.sort_passes; stats_out->rounds = b.stats.rounds; stats_out->pad_ = 0;
        stats_out->tied_after_sort = b.stats.tied_after_sort; stats_out->tied_total = b.stats.tied_total; stats_out->total_ms = b.stats.total_ms;
    }
    return rc;
}

namespace {

// S = u8 (sa_hip_sufcheck64_device) or int64_t (sa_hip_sufcheck_long_device)
template <class S>
int sufcheck_device(const S* text_dev, const int64_t* sa_dev, int64_t n, int device, uint64_t* violations, const char* name) {
    if (!violations || ((!text_dev || !sa_dev) && n) || n < 0) return fail(SA_HIP_EINVAL, name, "invalid arguments");
    big::BigBuilder b;
    DeviceCall dc;
    int rc = dc.open(device);
    if (rc) return rc;
    dc.at_close([&b] { b.destroy(); });
    b.stream = dc.stream;
    u64 v = 0;
    rc = b.verify<S>(text_dev, reinterpret_cast<const u64*>(sa_dev), (u64)n, &v);
    *violations = v;
    return rc;
}

// The plain-buffer path of a host text of this size (a call is dominated by its bytes over PCIe): the text up into `text`, its
// suffix array with 64-bit indices into `sa`.  Both buffers are the caller's to release.
int big_build_plain(const uint8_t* T, uint64_t n, DevBuf& text, DevBuf& sa) {
    int rc;
    if ((rc = text.ensure(n + 64)) || (rc = sa.ensure(n * 8 + 64))) return rc;
    SA_HIP_CHECK(hipMemcpy(text.p, T, n, hipMemcpyHostToDevice));
    return sa_hip_libsais64_device(text.p, sa.as<int64_t>(), (int64_t)n, 0, nullptr);
}

// host text in, host suffix array out
int big_oneshot(const uint8_t* T, uint64_t n, int64_t* SA, int64_t* freq) {
    {
        DevBuf text, sa;
        DeviceCall dc;
        int rc = dc.open(0, false);
        if (rc) return rc;
        dc.releases(text, sa);
        if ((rc = big_build_plain(T, n, text, sa))) return rc;
        SA_HIP_CHECK(hipMemcpy(SA, sa.p, n * 8, hipMemcpyDeviceToHost));
    }
    if (freq) byte_histogram(T, n, freq);
    return 0;
}

}  // namespace

extern "C" {

int sa_hip_sufcheck64_device(const void* text_dev, const int64_t* sa_dev, int64_t n, int device, uint64_t* violations) {
    return sufcheck_device(static_cast<const u8*>(text_dev), sa_dev, n, device, violations, "sa_hip_sufcheck64_device");
}
int sa_hip_sufcheck_long_device(const int64_t* T_dev, const int64_t* SA_dev, int64_t n, int device, uint64_t* violations) {
    return sufcheck_device(T_dev, SA_dev, n, device, violations, "sa_hip_sufcheck_long_device");
}

int64_t sa_hip_libsais64_omp(const uint8_t* T, int64_t* SA, int64_t n, int64_t fs, int64_t* freq, int64_t threads) {
    if (T == nullptr || SA == nullptr || n < 0 || fs < 0 || threads < 0) return fail(SA_HIP_EINVAL, "sa_hip_libsais64: invalid arguments");
    if ((uint64_t)n > 0xFFFFFFFEull) return big_oneshot(T, (uint64_t)n, SA, freq);   // 64-bit suffix indices (big_build.hpp)
    return oneshot_build<int64_t, int64_t>(T, (uint64_t)n, 0, SA, freq);
}

int64_t sa_hip_libsais64(const uint8_t* T, int64_t* SA, int64_t n, int64_t fs, int64_t* freq) {
    return sa_hip_libsais64_omp(T, SA, n, fs, freq, 0);
}

// ---- engine.c-call-compatible wrappers ---------------------------------------------------------------

int sa_hip_construct_truncated_suffix_array(const char* text, sa_hip_SuffixArray_struct* s) {
    if (!text || !s || (!s->suffix_array && s->n)) return fail(SA_HIP_EINVAL, "sa_hip_construct_truncated_suffix_array: NULL argument");
    // engine.c:841: depth = min(max_suffix_length, n); 0 would mean "no order at all" there,
    // which the device build expresses as L >= 1 only, so L == 0 degenerates to identity order.
    if (s->max_suffix_length == 0) {
        for (uint32_t i = 0; i < s->n; ++i) s->suffix_array[i] = i;
        return 0;
    }
    return oneshot_build<uint32_t, uint64_t>(reinterpret_cast<const uint8_t*>(text), s->n, s->max_suffix_length, s->suffix_array, nullptr);
}

sa_hip_pair_u32 sa_hip_get_substring_positions(const char* str, const sa_hip_SuffixArray_struct* s, const char* substring) {
    sa_hip_pair_u32 r = {0xFFFFFFFFu, 0xFFFFFFFFu};
    if (!str || !s || !substring || (!s->suffix_array && s->n)) { fail(SA_HIP_EINVAL, "sa_hip_get_substring_positions: NULL argument"); return r; }
    TempIndex t;
    if (sa_hip_index_create(&t.idx, s->n, 0)) return r;
    // max_suffix_length == 0 in the reference means cmp_length 0 (everything matches); the handle
    // API uses 0 for "unlimited", so pass the pattern truncated accordingly.
    const uint64_t m = strlen(substring);
    const uint32_t L = s->max_suffix_length;
    if (sa_hip_index_load(t.idx, reinterpret_cast<const uint8_t*>(str), s->suffix_array, s->n, L ? L : 1)) return r;
    const uint64_t off[2] = {0, L ? m : 0};
    if (sa_hip_query_batch(t.idx, reinterpret_cast<const uint8_t*>(substring), off, 1, &r)) {
        r.first = r.second = 0xFFFFFFFFu;
    }
    return r;
}

int sa_hip_sort_pairs(uint64_t* keys, uint32_t* values, uint64_t n, int begin_bit, int end_bit, int device) {
    if ((!keys && n) || begin_bit < 0 || end_bit > 64 || begin_bit > end_bit || n > 0xFFFFFFFEull)
        return fail(SA_HIP_EINVAL, "sa_hip_sort_pairs: invalid arguments");
    if (n == 0 || begin_bit == end_bit) return 0;
    RadixWorkspace ws;
    DevBuf k0, k1, v0, v1;
    int sort_block = 512;
    if (const char* e = diag_env("SA_HIP_SORT_BLOCK")) sort_block = (atoi(e) == 256) ? 256 : 512;
    DeviceCall dc;
    int rc = dc.open(device);
    if (rc) return rc;
    dc.releases(k0, k1, v0, v1);
    dc.at_close([&ws] { ws.destroy(); });
    hipStream_t stream = dc.stream;
    if ((rc = ws.init(n, sort_block)) || (rc = k0.ensure(n * 8)) || (rc = k1.ensure(n * 8)) || (rc = v0.ensure(n * 4)) || (rc = v1.ensure(n * 4)))
        return rc;
    u64* kr = nullptr; u32* vr = nullptr;
    SA_HIP_CHECK(hipMemcpyAsync(k0.p, keys, n * 8, hipMemcpyHostToDevice, stream));
    if (values) SA_HIP_CHECK(hipMemcpyAsync(v0.p, values, n * 4, hipMemcpyHostToDevice, stream));
    if ((rc = radix_sort_pairs(ws, stream, k0.as<u64>(), v0.as<u32>(), k1.as<u64>(), v1.as<u32>(), (u32)n, begin_bit, end_bit,
                               values == nullptr, false, &kr, &vr))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(keys, kr, n * 8, hipMemcpyDeviceToHost, stream));
    if (values) SA_HIP_CHECK(hipMemcpyAsync(values, vr, n * 4, hipMemcpyDeviceToHost, stream));
    DeviceStatus st;
    SA_HIP_CHECK(hipMemcpyAsync(&st, ws.dstat, sizeof st, hipMemcpyDeviceToHost, stream));
    SA_HIP_CHECK(hipStreamSynchronize(stream));
    if (st.error) return fail(SA_HIP_EINTERNAL, "device look-back spin limit expired");
    return ws.timer.flush();
}

int sa_hip_csv_extract_column(const char* path, const char* column, sa_hip_csv_column* out) {
    if (!path || !column || !out) return fail(SA_HIP_EINVAL, "sa_hip_csv_extract_column: NULL argument");
    // nothing may unwind through the C ABI: allocation failures and thread-creation failures become codes
    try {
        return csv_extract_column(path, column, out);
    } catch (const std::bad_alloc&) {
        csv_free(out);
        return fail(SA_HIP_ENOMEM, "sa_hip_csv_extract_column: out of host memory");
    } catch (const std::exception& e) {
        csv_free(out);
        return fail(SA_HIP_EINVAL, "sa_hip_csv_extract_column", e.what());
    }
}
void sa_hip_csv_free(sa_hip_csv_column* col) { csv_free(col); }
int sa_hip_synth_csv(const char* path, uint64_t rows, uint64_t seed) {
    if (!path) return fail(SA_HIP_EINVAL, "sa_hip_synth_csv: NULL path");
    try {
        return synth_csv(path, rows, seed);
    } catch (const std::bad_alloc&) {
        return fail(SA_HIP_ENOMEM, "sa_hip_synth_csv: out of host memory");
    } catch (const std::exception& e) {
        return fail(SA_HIP_EINVAL, "sa_hip_synth_csv", e.what());
    }
}

void sa_hip_synth_uniform27(uint8_t* out, uint64_t n, uint64_t seed) {
    // xorshift64 (13,7,17), symbol = (s >> 33) % 27, 26 -> '\n'
    uint64_t s = seed ? seed : 88172645463325252ull;
    for (uint64_t i = 0; i < n; ++i) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        const uint32_t v = (uint32_t)((s >> 33) % 27u);
        out[i] = (uint8_t)(v == 26 ? '\n' : 'a' + v);
    }
}

}  // extern "C"

// ---- LCP arrays (lcp.hpp) ---------------------------------------------------------------------------------------------

namespace {

// Host drop-ins: Idx = u32 (libsais layout, int32 on the host) or u64 (libsais64 layout); S = the symbol type of T (u8, or u32
// for sa_hip_libsais_plcp_int).  PLCP_IN == nullptr: PLCP of (T, SA) into out; else LCP = gather of PLCP_IN by SA into out.
// n >= 2, arguments checked by the caller.
template <class Idx, class S = u8>
int oneshot_lcp(const void* T, const void* plcp_in, const void* SA, void* out, uint64_t n) {
    HostCall hc(n);
    OneShot& g = hc.g;
    sa_hip_call_breakdown& bd = hc.bd;
    const size_t bytes = (size_t)n * sizeof(Idx), tbytes = (size_t)n * sizeof(S);
    int rc = hc.attach_stream([&] {
        return g.l_stream && g.ring.ready && g.l_sa.cap >= bytes && g.l_out.cap >= bytes &&
               (plcp_in ? g.l_in.cap >= bytes : (g.l_text.cap >= tbytes + 64 && g.lcp.w.cap >= bytes));
    });
    if (rc || (rc = g.l_sa.ensure(bytes + 64)) || (rc = g.l_out.ensure(bytes + 64))) return rc;
    if (plcp_in) { if ((rc = g.l_in.ensure(bytes + 64))) return rc; }
    else if ((rc = g.l_text.ensure(tbytes + 64)) || (rc = g.lcp.ensure(n, sizeof(Idx)))) return rc;
    hc.phase(&bd.workspace_ms);
    if ((rc = ring_upload(g.ring, g.l_stream, hc.device, g.l_sa.p, static_cast<const u8*>(SA), bytes))) return rc;
    if (plcp_in) rc = ring_upload(g.ring, g.l_stream, hc.device, g.l_in.p, static_cast<const u8*>(plcp_in), bytes);
    else rc = ring_upload(g.ring, g.l_stream, hc.device, g.l_text.p, static_cast<const u8*>(T), tbytes);
    if (rc) return rc;
    hc.phase(&bd.upload_ms);
    u32 error = 0;
    if (plcp_in) {
        if ((rc = lcp::gather_only<Idx>(g.lcp, g.l_stream, g.l_in.as<Idx>(), g.l_sa.as<Idx>(), n, g.l_out.as<Idx>(), &error))) return rc;
        bd.build_device_ms = hc.phase_ms();
    } else {
        lcp::Counters ctr{};
        sa_hip_lcp_stats st{};
        if ((rc = lcp::run<Idx, S>(g.lcp, g.l_stream, g.l_text.as<u8>(), g.l_sa.as<Idx>(), n, g.l_out.as<Idx>(), lcp::Out::PLCP, nullptr,
                                lcp::Knobs::read(), &ctr, &st))) return rc;
        error = ctr.error;
        bd.build_device_ms = st.total_ms;
    }
    hc.phase(&bd.build_ms);
    if (error) return fail(SA_HIP_EINVAL, "suffix array entry out of range [0, n)");
    if ((rc = ring_download(g.ring, hc.device, g.l_out.as<u8>(), static_cast<u8*>(out), bytes))) return rc;
    hc.phase(&bd.download_ms);
    return hc.commit();
}

// argument checks and n <= 1 of libsais_plcp (libsais.c:7763-7774); IO = int32_t / int64_t host entries, S as oneshot_lcp
template <class IO, class S = u8>
IO plcp_dropin(const void* T, const IO* SA, IO* PLCP, IO n, IO threads, const char* name) {
    if (T == nullptr || SA == nullptr || PLCP == nullptr || n < 0 || threads < 0) return fail(SA_HIP_EINVAL, name, "invalid arguments");
    if (n <= 1) { if (n == 1) PLCP[0] = 0; return 0; }
    return oneshot_lcp<std::make_unsigned_t<IO>, S>(T, nullptr, SA, PLCP, (uint64_t)n);
}

// ... of libsais_lcp (libsais.c:7812-7823)
template <class IO>
IO lcp_dropin(const IO* PLCP, const IO* SA, IO* LCP, IO n, IO threads, const char* name) {
    if (PLCP == nullptr || SA == nullptr || LCP == nullptr || n < 0 || threads < 0) return fail(SA_HIP_EINVAL, name, "invalid arguments");
    if (n <= 1) {
        if (n == 1) {
            if (SA[0] != 0) return fail(SA_HIP_EINVAL, name, "suffix array entry out of range [0, n)");
            LCP[0] = PLCP[0];
        }
        return 0;
    }
    return oneshot_lcp<std::make_unsigned_t<IO>>(nullptr, PLCP, SA, LCP, (uint64_t)n);
}

int index_lcp(sa_hip_index* idx, void* out_dev, sa_hip_lcp_stats* stats, lcp::Out what, const char* name) {
    if (!idx) return fail(SA_HIP_EINVAL, name, "NULL index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->host) return fail(SA_HIP_EINVAL, name, "the host path (no HIP device) has no device buffers");
    if (!idx->has_index) return fail(SA_HIP_EINVAL, name, "no index (build or load one first)");
    if (idx->b.max_suffix_length > 0)
        return fail(SA_HIP_EINVAL, name, "truncated index (max_suffix_length > 0): its order is not the suffix order LCP needs");
    const u64 n = idx->b.n;
    if (!out_dev && n) return fail(SA_HIP_EINVAL, name, "NULL output");
    int rc = set_device(idx->device);
    if (rc) return rc;
    if (n <= 1) {
        if (n == 1) SA_HIP_CHECK(hipMemsetAsync(out_dev, 0, 4, idx->stream));
        if (stats) { memset(stats, 0, sizeof *stats); stats->n = n; SA_HIP_CHECK(hipStreamSynchronize(idx->stream)); }
        return 0;
    }
    const lcp::Knobs kn = lcp::Knobs::read();
    const Builder& b = idx->b;
    lcp::KeyView kv{};
    const bool keys = kn.keys && (b.qkeys || (b.qkeys32 && b.q_bstart)) && b.q_b > 0 && b.q_k0 > 0;
    if (keys) { kv.keys = b.qkeys; kv.keys32 = b.qkeys ? nullptr : b.qkeys32; kv.bstart = b.q_bstart; kv.lo_shift = b.q_lo_shift; kv.b = b.q_b; kv.k0 = b.q_k0; }
    return lcp::run<u32>(idx->lcp_ws, idx->stream, b.text.as<u8>(), b.sa, n, static_cast<u32*>(out_dev), what, keys ? &kv : nullptr,
                         kn, nullptr, stats);
}

int lcp64_device(const void* text_dev, const int64_t* sa_dev, int64_t* out_dev, int64_t n, int device, sa_hip_lcp_stats* stats,
                 lcp::Out what, const char* name) {
    if (n < 0) return fail(SA_HIP_EINVAL, name, "negative length");
    if ((!text_dev || !sa_dev || !out_dev) && n) return fail(SA_HIP_EINVAL, name, "NULL argument");
    if (((uintptr_t)text_dev & 7u) != 0) return fail(SA_HIP_EINVAL, name, "text_dev must be 8-byte aligned");
    if (stats) { memset(stats, 0, sizeof *stats); stats->n = (u64)n; }
    if (n == 0) return 0;
    lcp::Workspace ws;
    DeviceCall dc;
    int rc = dc.open(device);
    if (rc) return rc;
    dc.releases(ws);
    hipStream_t stream = dc.stream;
    if (n == 1) {   // PLCP[0] = 0; LCP[0] = PLCP[SA[0]] with SA[0] range-checked
        int64_t s0 = 0;
        SA_HIP_CHECK(hipMemcpyAsync(&s0, sa_dev, 8, hipMemcpyDeviceToHost, stream));
        SA_HIP_CHECK(hipStreamSynchronize(stream));
        if (what == lcp::Out::LCP && s0 != 0) return fail(SA_HIP_EINVAL, name, "suffix array entry out of range [0, n)");
        SA_HIP_CHECK(hipMemsetAsync(out_dev, 0, 8, stream));
        SA_HIP_CHECK(hipStreamSynchronize(stream));
        return 0;
    }
    lcp::Counters ctr{};
    if ((rc = lcp::run<u64>(ws, stream, static_cast<const u8*>(text_dev), reinterpret_cast<const u64*>(sa_dev), (u64)n,
                            reinterpret_cast<u64*>(out_dev), what, nullptr, lcp::Knobs::read(), &ctr, stats))) return rc;
    if (ctr.error) return fail(SA_HIP_EINVAL, name, "suffix array entry out of range [0, n)");
    return 0;
}

}  // namespace

extern "C" {

int32_t sa_hip_libsais_plcp_omp(const uint8_t* T, const int32_t* SA, int32_t* PLCP, int32_t n, int32_t threads) {
    return plcp_dropin<int32_t>(T, SA, PLCP, n, threads, "sa_hip_libsais_plcp");
}
int32_t sa_hip_libsais_plcp(const uint8_t* T, const int32_t* SA, int32_t* PLCP, int32_t n) {
    return sa_hip_libsais_plcp_omp(T, SA, PLCP, n, 0);
}
int32_t sa_hip_libsais_lcp_omp(const int32_t* PLCP, const int32_t* SA, int32_t* LCP, int32_t n, int32_t threads) {
    return lcp_dropin<int32_t>(PLCP, SA, LCP, n, threads, "sa_hip_libsais_lcp");
}
int32_t sa_hip_libsais_lcp(const int32_t* PLCP, const int32_t* SA, int32_t* LCP, int32_t n) {
    return sa_hip_libsais_lcp_omp(PLCP, SA, LCP, n, 0);
}
int64_t sa_hip_libsais64_plcp_omp(const uint8_t* T, const int64_t* SA, int64_t* PLCP, int64_t n, int64_t threads) {
    return plcp_dropin<int64_t>(T, SA, PLCP, n, threads, "sa_hip_libsais64_plcp");
}
int64_t sa_hip_libsais64_plcp(const uint8_t* T, const int64_t* SA, int64_t* PLCP, int64_t n) {
    return sa_hip_libsais64_plcp_omp(T, SA, PLCP, n, 0);
}
int64_t sa_hip_libsais64_lcp_omp(const int64_t* PLCP, const int64_t* SA, int64_t* LCP, int64_t n, int64_t threads) {
    return lcp_dropin<int64_t>(PLCP, SA, LCP, n, threads, "sa_hip_libsais64_lcp");
}
int64_t sa_hip_libsais64_lcp(const int64_t* PLCP, const int64_t* SA, int64_t* LCP, int64_t n) {
    return sa_hip_libsais64_lcp_omp(PLCP, SA, LCP, n, 0);
}
int32_t sa_hip_libsais_plcp_int_omp(const int32_t* T, const int32_t* SA, int32_t* PLCP, int32_t n, int32_t threads) {
    return plcp_dropin<int32_t, u32>(T, SA, PLCP, n, threads, "sa_hip_libsais_plcp_int");
}
int32_t sa_hip_libsais_plcp_int(const int32_t* T, const int32_t* SA, int32_t* PLCP, int32_t n) {
    return sa_hip_libsais_plcp_int_omp(T, SA, PLCP, n, 0);
}

int sa_hip_index_plcp_device(sa_hip_index* idx, void* out_dev, sa_hip_lcp_stats* stats) {
    return index_lcp(idx, out_dev, stats, lcp::Out::PLCP, "sa_hip_index_plcp_device");
}
int sa_hip_index_lcp_device(sa_hip_index* idx, void* out_dev, sa_hip_lcp_stats* stats) {
    return index_lcp(idx, out_dev, stats, lcp::Out::LCP, "sa_hip_index_lcp_device");
}
int sa_hip_plcp64_device(const void* text_dev, const int64_t* sa_dev, int64_t* out_dev, int64_t n, int device, sa_hip_lcp_stats* stats) {
    return lcp64_device(text_dev, sa_dev, out_dev, n, device, stats, lcp::Out::PLCP, "sa_hip_plcp64_device");
}
int sa_hip_lcp64_device(const void* text_dev, const int64_t* sa_dev, int64_t* out_dev, int64_t n, int device, sa_hip_lcp_stats* stats) {
    return lcp64_device(text_dev, sa_dev, out_dev, n, device, stats, lcp::Out::LCP, "sa_hip_lcp64_device");
}

int sa_hip_plcp_int_device(const int32_t* T_dev, const int32_t* SA_dev, int32_t* PLCP_dev, int32_t n, int device, sa_hip_lcp_stats* stats) {
    const char* name = "sa_hip_plcp_int_device";
    if (n < 0) return fail(SA_HIP_EINVAL, name, "negative length");
    if ((!T_dev || !SA_dev || !PLCP_dev) && n) return fail(SA_HIP_EINVAL, name, "NULL argument");
    if (stats) { memset(stats, 0, sizeof *stats); stats->n = (u64)n; }
    if (n == 0) return 0;
    lcp::Workspace ws;
    DevBuf pad;
    DeviceCall dc;
    int rc = dc.open(device);
    if (rc) return rc;
    dc.releases(ws, pad);
    if (n == 1) { SA_HIP_CHECK(hipMemset(PLCP_dev, 0, 4)); SA_HIP_CHECK(hipDeviceSynchronize()); return 0; }
    // the kernels read the text as aligned 8-byte words up to the one that holds its last byte: a text that is not 8-byte
    // aligned or ends inside a word is copied into a padded buffer first
    const u8* t = reinterpret_cast<const u8*>(T_dev);
    if (((uintptr_t)t & 7u) != 0 || (n & 1) != 0) {
        if ((rc = pad.ensure((size_t)n * 4 + 64))) return rc;
        SA_HIP_CHECK(hipMemcpyAsync(pad.p, T_dev, (size_t)n * 4, hipMemcpyDeviceToDevice, dc.stream));
        t = pad.as<u8>();
    }
    lcp::Counters ctr{};
    if ((rc = lcp::run<u32, u32>(ws, dc.stream, t, reinterpret_cast<const u32*>(SA_dev), (u64)n, reinterpret_cast<u32*>(PLCP_dev), lcp::Out::PLCP,
                                 nullptr, lcp::Knobs::read(), &ctr, stats))) return rc;
    if (ctr.error) return fail(SA_HIP_EINVAL, name, "suffix array entry out of range [0, n)");
    return 0;
}

}  // extern "C"

// ---- BWT / inverse BWT (bwt.hpp) ----------------------------------------------------------------------------------------

namespace {

inline bool pow2_ge2(int64_t r) { return r >= 2 && (r & (r - 1)) == 0; }

// Host drop-in, forward: the suffix array is built on the device (the cached index for n <= 2^32 - 2, big_build.hpp
// beyond) and only U and I come back.  IO = int32_t / int64_t host entries of I and freq.  n >= 2, arguments checked.
template <class IO>
int oneshot_bwt(const uint8_t* T, uint8_t* U, uint64_t n, uint64_t r_aux, IO* I, IO* freq, uint64_t* primary) {
    const uint64_t m = r_aux ? (n - 1) / r_aux + 1 : 0;
    if (n > 0xFFFFFFFEull) {   // 64-bit suffix indices: plain device buffers, as sa_hip_libsais64 there
        if (freq) byte_histogram(T, n, freq);   // before U is written: U may be T
        DevBuf text, sa, u, aux;
        bwt::Workspace ws;
        DeviceCall dc;
        int rc = dc.open(0);
        if (rc) return rc;
        dc.releases(ws, text, sa, u, aux);
        if ((rc = u.ensure(n + 64)) || (m && (rc = aux.ensure(m * 8 + 64))) || (rc = big_build_plain(T, n, text, sa))) return rc;
        if ((rc = bwt::run_bwt<u64>(ws, dc.stream, text.as<u8>(), sa.as<u64>(), n, r_aux, m ? aux.as<u64>() : nullptr, u.as<u8>(), primary, nullptr))) return rc;
        SA_HIP_CHECK(hipMemcpy(U, u.p, n, hipMemcpyDeviceToHost));
        if (m) SA_HIP_CHECK(hipMemcpy(I, aux.p, m * 8, hipMemcpyDeviceToHost));   // IO = int64_t here
        return 0;
    }
    HostCall hc(n);
    OneShot& g = hc.g;
    sa_hip_call_breakdown& bd = hc.bd;
    int rc;
    bd.workspace_reused = (g.idx && g.idx->b.n_max >= n && g.ring.ready && g.b_u.cap >= n + 64) ? 1u : 0u;
    if ((rc = hc.attach_index(n))) return rc;
    hc.own_buffers();
    sa_hip_index* idx = hc.idx;
    if ((rc = g.b_u.ensure(n + 64)) || (m && (rc = g.b_aux.ensure(m * 4 + 64)))) return rc;
    hc.phase(&bd.workspace_ms);
    if ((rc = ring_upload(g.ring, idx->stream, idx->device, idx->b.text.p, T, (size_t)n))) return rc;
    hc.phase(&bd.upload_ms);
    if ((rc = rebuild(idx, n, 0))) return rc;
    sa_hip_bwt_stats st{};
    if ((rc = bwt::run_bwt<u32>(g.bwt, idx->stream, idx->b.text.as<u8>(), idx->b.sa, n, r_aux, m ? g.b_aux.as<u32>() : nullptr,
                                g.b_u.as<u8>(), primary, &st))) return rc;
    hc.phase(&bd.build_ms);
    bd.build_device_ms = idx->b.stats.total_ms + st.total_ms;
    if (freq) for (int c = 0; c < 256; ++c) freq[c] = (IO)idx->b.freq[c];   // before U is written: U may be T
    if ((rc = ring_download(g.ring, idx->device, g.b_u.as<u8>(), U, (size_t)n))) return rc;
    if (m) {
        std::vector<u32> h(m);
        SA_HIP_CHECK(hipMemcpy(h.data(), g.b_aux.p, m * 4, hipMemcpyDeviceToHost));
        for (uint64_t t = 0; t < m; ++t) I[t] = (IO)h[t];
    }
    hc.phase(&bd.download_ms);
    return hc.commit();
}

// Host drop-in, inverse: T = the BWT (input), U = the text (output; may be T).  n >= 2, I checked on the host.
template <class Idx, class IO>
int oneshot_unbwt_idx(const uint8_t* T, uint8_t* U, uint64_t n, uint64_t r_aux, const IO* I) {
    HostCall hc(n);
    OneShot& g = hc.g;
    sa_hip_call_breakdown& bd = hc.bd;
    const uint64_t m = (n - 1) / r_aux + 1;
    int rc = hc.attach_stream([&] {
        return g.l_stream && g.ring.ready && g.b_u.cap >= n + 64 && g.bwt.tmp.cap >= n + 64 && g.bwt.psi.cap >= n * sizeof(Idx) + 64;
    });
    if (rc || (rc = g.b_u.ensure(n + 64)) || (rc = g.bwt.tmp.ensure(n + 64)) || (rc = g.b_aux.ensure(m * sizeof(Idx) + 64))) return rc;
    hc.phase(&bd.workspace_ms);
    std::vector<Idx> h(m);
    for (uint64_t t = 0; t < m; ++t) h[t] = (Idx)I[t];
    SA_HIP_CHECK(hipMemcpy(g.b_aux.p, h.data(), m * sizeof(Idx), hipMemcpyHostToDevice));
    if ((rc = ring_upload(g.ring, g.l_stream, hc.device, g.b_u.p, T, (size_t)n))) return rc;
    hc.phase(&bd.upload_ms);
    sa_hip_bwt_stats st{};
    if ((rc = bwt::run_unbwt<Idx>(g.bwt, g.l_stream, g.b_u.as<u8>(), n, g.b_aux.as<Idx>(), r_aux, g.bwt.tmp.as<u8>(), bwt::Knobs::read(), &st)))
        return rc;
    hc.phase(&bd.build_ms);
    bd.build_device_ms = st.total_ms;
    if ((rc = ring_download(g.ring, hc.device, g.bwt.tmp.as<u8>(), U, (size_t)n))) return rc;
    hc.phase(&bd.download_ms);
    return hc.commit();
}

// argument checks of libsais_unbwt_aux (libsais.c:7600-7614), then the device
template <class IO>
IO unbwt_dropin(const uint8_t* T, uint8_t* U, const IO* A, IO n, IO r, const IO* I, IO threads, const char* name) {
    if (T == nullptr || U == nullptr || A == nullptr || n < 0 || (r != n && !pow2_ge2((int64_t)r)) || I == nullptr || threads < 0)
        return (IO)fail(SA_HIP_EINVAL, name, "invalid arguments");
    if (n <= 1) {
        if (I[0] != n) return (IO)fail(SA_HIP_EINVAL, name, "n <= 1 needs I[0] == n");
        if (n == 1) U[0] = T[0];
        return 0;
    }
    for (IO t = 0; t <= (n - 1) / r; ++t)
        if (I[t] <= 0 || I[t] > n) return (IO)fail(SA_HIP_EINVAL, name, "an aux index is outside (0, n]");
    if ((uint64_t)n > 0xFFFFFFFEull) return (IO)oneshot_unbwt_idx<u64, IO>(T, U, (uint64_t)n, (uint64_t)r, I);
    return (IO)oneshot_unbwt_idx<u32, IO>(T, U, (uint64_t)n, (uint64_t)r, I);
}

// argument checks and n <= 1 of libsais_bwt / libsais_bwt_aux (libsais.c:6665-6714); r == 0: the plain form
template <class IO>
IO bwt_dropin(const uint8_t* T, uint8_t* U, IO* A, IO n, IO fs, IO* freq, IO r, IO* I, IO threads, bool aux, const char* name) {
    if (T == nullptr || U == nullptr || A == nullptr || n < 0 || fs < 0 || threads < 0 || (aux && (!pow2_ge2((int64_t)r) || I == nullptr)))
        return (IO)fail(SA_HIP_EINVAL, name, "invalid arguments");
    if (n <= 1) {
        if (freq) byte_histogram(T, (uint64_t)n, freq);
        if (n == 1) U[0] = T[0];
        if (aux) { I[0] = n; return 0; }
        return n;
    }
    uint64_t p = 0;
    const int rc = oneshot_bwt<IO>(T, U, (uint64_t)n, aux ? (uint64_t)r : 0, aux ? I : nullptr, freq, &p);
    if (rc) return (IO)rc;
    return aux ? (IO)0 : (IO)p;
}

}  // namespace

extern "C" {

int32_t sa_hip_libsais_bwt_omp(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, int32_t fs, int32_t* freq, int32_t threads) {
    return bwt_dropin<int32_t>(T, U, A, n, fs, freq, 0, nullptr, threads, false, "sa_hip_libsais_bwt");
}
int32_t sa_hip_libsais_bwt(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, int32_t fs, int32_t* freq) {
    return sa_hip_libsais_bwt_omp(T, U, A, n, fs, freq, 0);
}
int32_t sa_hip_libsais_bwt_aux_omp(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, int32_t fs, int32_t* freq, int32_t r, int32_t* I, int32_t threads) {
    return bwt_dropin<int32_t>(T, U, A, n, fs, freq, r, I, threads, true, "sa_hip_libsais_bwt_aux");
}
int32_t sa_hip_libsais_bwt_aux(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, int32_t fs, int32_t* freq, int32_t r, int32_t* I) {
    return sa_hip_libsais_bwt_aux_omp(T, U, A, n, fs, freq, r, I, 0);
}
int32_t sa_hip_libsais_unbwt_aux_omp(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, const int32_t* freq, int32_t r, const int32_t* I, int32_t threads) {
    (void)freq;   // never read: the device computes the histogram itself
    return unbwt_dropin<int32_t>(T, U, A, n, r, I, threads, "sa_hip_libsais_unbwt_aux");
}
int32_t sa_hip_libsais_unbwt_aux(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, const int32_t* freq, int32_t r, const int32_t* I) {
    return sa_hip_libsais_unbwt_aux_omp(T, U, A, n, freq, r, I, 0);
}
int32_t sa_hip_libsais_unbwt_omp(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, const int32_t* freq, int32_t i, int32_t threads) {
    return sa_hip_libsais_unbwt_aux_omp(T, U, A, n, freq, n, &i, threads);
}
int32_t sa_hip_libsais_unbwt(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, const int32_t* freq, int32_t i) {
    return sa_hip_libsais_unbwt_aux_omp(T, U, A, n, freq, n, &i, 0);
}
int64_t sa_hip_libsais64_bwt_omp(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, int64_t fs, int64_t* freq, int64_t threads) {
    return bwt_dropin<int64_t>(T, U, A, n, fs, freq, 0, nullptr, threads, false, "sa_hip_libsais64_bwt");
}
int64_t sa_hip_libsais64_bwt(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, int64_t fs, int64_t* freq) {
    return sa_hip_libsais64_bwt_omp(T, U, A, n, fs, freq, 0);
}
int64_t sa_hip_libsais64_bwt_aux_omp(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, int64_t fs, int64_t* freq, int64_t r, int64_t* I, int64_t threads) {
    return bwt_dropin<int64_t>(T, U, A, n, fs, freq, r, I, threads, true, "sa_hip_libsais64_bwt_aux");
}
int64_t sa_hip_libsais64_bwt_aux(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, int64_t fs, int64_t* freq, int64_t r, int64_t* I) {
    return sa_hip_libsais64_bwt_aux_omp(T, U, A, n, fs, freq, r, I, 0);
}
int64_t sa_hip_libsais64_unbwt_aux_omp(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, const int64_t* freq, int64_t r, const int64_t* I, int64_t threads) {
    (void)freq;
    return unbwt_dropin<int64_t>(T, U, A, n, r, I, threads, "sa_hip_libsais64_unbwt_aux");
}
int64_t sa_hip_libsais64_unbwt_aux(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, const int64_t* freq, int64_t r, const int64_t* I) {
    return sa_hip_libsais64_unbwt_aux_omp(T, U, A, n, freq, r, I, 0);
}
int64_t sa_hip_libsais64_unbwt_omp(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, const int64_t* freq, int64_t i, int64_t threads) {
    return sa_hip_libsais64_unbwt_aux_omp(T, U, A, n, freq, n, &i, threads);
}
int64_t sa_hip_libsais64_unbwt(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, const int64_t* freq, int64_t i) {
    return sa_hip_libsais64_unbwt_aux_omp(T, U, A, n, freq, n, &i, 0);
}

int sa_hip_index_bwt_device(sa_hip_index* idx, void* U_dev, int64_t r, void* I_dev, int64_t* primary, sa_hip_bwt_stats* stats) {
    const char* name = "sa_hip_index_bwt_device";
    if (!idx) return fail(SA_HIP_EINVAL, name, "NULL index");
    if (!primary) return fail(SA_HIP_EINVAL, name, "NULL primary");
    if (I_dev && !pow2_ge2(r)) return fail(SA_HIP_EINVAL, name, "r must be a power of two >= 2");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->host) return fail(SA_HIP_EINVAL, name, "the host path (no HIP device) has no device buffers");
    if (!idx->has_index) return fail(SA_HIP_EINVAL, name, "no index (build or load one first)");
    if (idx->b.max_suffix_length > 0)
        return fail(SA_HIP_EINVAL, name, "truncated index (max_suffix_length > 0): its order is not the suffix order the BWT needs");
    const u64 n = idx->b.n;
    if (!U_dev && n) return fail(SA_HIP_EINVAL, name, "NULL output");
    int rc = set_device(idx->device);
    if (rc) return rc;
    if (n <= 1) {
        if (n == 1) SA_HIP_CHECK(hipMemcpyAsync(U_dev, idx->b.text.p, 1, hipMemcpyDeviceToDevice, idx->stream));
        if (I_dev) { const u32 v = (u32)n; SA_HIP_CHECK(hipMemcpyAsync(I_dev, &v, 4, hipMemcpyHostToDevice, idx->stream)); }
        SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
        if (stats) { memset(stats, 0, sizeof *stats); stats->n = n; }
        *primary = (int64_t)n;
        return 0;
    }
    u64 p = 0;
    rc = bwt::run_bwt<u32>(idx->bwt_ws, idx->stream, idx->b.text.as<u8>(), idx->b.sa, n, I_dev ? (u64)r : 0ull, static_cast<u32*>(I_dev),
                           static_cast<u8*>(U_dev), &p, stats);
    if (rc) return rc;
    *primary = (int64_t)p;
    return 0;
}

int64_t sa_hip_bwt64_device(const void* text_dev, const int64_t* sa_dev, void* U_dev, int64_t n, int64_t r, int64_t* I_dev, int device,
                            sa_hip_bwt_stats* stats) {
    const char* name = "sa_hip_bwt64_device";
    if (n < 0) return fail(SA_HIP_EINVAL, name, "negative length");
    if ((!text_dev || !sa_dev || !U_dev) && n) return fail(SA_HIP_EINVAL, name, "NULL argument");
    if (I_dev && !pow2_ge2(r)) return fail(SA_HIP_EINVAL, name, "r must be a power of two >= 2");
    if (stats) { memset(stats, 0, sizeof *stats); stats->n = (u64)n; }
    bwt::Workspace ws;
    DeviceCall dc;
    int rc = dc.open(device);
    if (rc) return rc;
    dc.releases(ws);
    if (n <= 1) {
        if (n == 1 && U_dev != text_dev) SA_HIP_CHECK(hipMemcpy(U_dev, text_dev, 1, hipMemcpyDeviceToDevice));
        if (I_dev) { const int64_t v = n; SA_HIP_CHECK(hipMemcpy(I_dev, &v, 8, hipMemcpyHostToDevice)); return 0; }
        return n;
    }
    u64 p = 0;
    const u8* t = static_cast<const u8*>(text_dev);
    u8* u = static_cast<u8*>(U_dev);
    const bool overlap = u < t + n && t < u + n;   // U over the text: gather into scratch, then copy
    u8* dst = u;
    if (overlap) { if ((rc = ws.tmp.ensure((size_t)n + 64))) return rc; dst = ws.tmp.as<u8>(); }
    if ((rc = bwt::run_bwt<u64>(ws, dc.stream, t, reinterpret_cast<const u64*>(sa_dev), (u64)n, I_dev ? (u64)r : 0ull,
                                reinterpret_cast<u64*>(I_dev), dst, &p, stats))) return rc;
    if (overlap) { SA_HIP_CHECK(hipMemcpyAsync(u, dst, (size_t)n, hipMemcpyDeviceToDevice, dc.stream)); SA_HIP_CHECK(hipStreamSynchronize(dc.stream)); }
    return I_dev ? 0 : (int64_t)p;
}

int sa_hip_unbwt64_device(const void* U_dev, void* out_dev, int64_t n, int64_t r, const int64_t* I_dev, int device, sa_hip_bwt_stats* stats) {
    const char* name = "sa_hip_unbwt64_device";
    if (n < 0) return fail(SA_HIP_EINVAL, name, "negative length");
    if (!I_dev || ((!U_dev || !out_dev) && n)) return fail(SA_HIP_EINVAL, name, "NULL argument");
    if (r != n && !pow2_ge2(r)) return fail(SA_HIP_EINVAL, name, "r must be n or a power of two >= 2");
    if (stats) { memset(stats, 0, sizeof *stats); stats->n = (u64)n; }
    bwt::Workspace ws;
    DeviceCall dc;
    int rc = dc.open(device);
    if (rc) return rc;
    dc.releases(ws);
    if (n <= 1) {
        int64_t i0 = -1;
        SA_HIP_CHECK(hipMemcpy(&i0, I_dev, 8, hipMemcpyDeviceToHost));
        if (i0 != n) return fail(SA_HIP_EINVAL, name, "n <= 1 needs I[0] == n");
        if (n == 1 && out_dev != U_dev) SA_HIP_CHECK(hipMemcpy(out_dev, U_dev, 1, hipMemcpyDeviceToDevice));
        return 0;
    }
    // out may be U: U is read only while psi is built, before the walks write
    return bwt::run_unbwt<u64>(ws, dc.stream, static_cast<const u8*>(U_dev), (u64)n, reinterpret_cast<const u64*>(I_dev), (u64)r,
                               static_cast<u8*>(out_dev), bwt::Knobs::read(), stats);
}

}  // extern "C"

// ---- integer alphabets (int_build.hpp) -----------------------------------------------------------------------------------

namespace {

// Where a finished integer build left its suffix array.
enum class IntRes { INDEX_U32, DEV_I32, DEV_U64 };

// The build of T[0..n) (n >= 2, on the device, k >= 1) on `stream`, synchronous.  get_idx(n, &idx) hands route A an index
// handle with n_max >= n (locked for the caller).  out32 / out64: where the caller wants the result on the device (at most one);
// to_index: route A may leave it in idx->b.sa (the host drop-ins download from there).  *res / *res_ptr: where it is.
template <class S, class GetIdx>
int int_core(ints::Workspace& ws, hipStream_t stream, const S* T, u64 n, int64_t k, GetIdx&& get_idx, int32_t* out32, int64_t* out64,
             bool to_index, sa_hip_int_stats* st, IntRes* res, const void** res_ptr, sa_hip_index** idx_used) {
    const ints::Knobs kn = ints::Knobs::read();
    ints::Alphabet a;
    float alpha_ms = 0.f, route_ms = 0.f;
    int rc = ints::alphabet<S>(ws, stream, T, n, k, kn, &a, &alpha_ms);
    if (rc) return rc;
    sa_hip_int_stats t{};
    t.n = n;
    t.sigma = a.sigma;
    t.compacted = a.dense ? 1u : 0u;
    t.min_symbol = a.min;
    t.max_symbol = a.max;
    t.alphabet_ms = alpha_ms;
    if (ints::route_bytes(a, n, kn)) {   // route A: rank bytes into an index's text, the product's byte build
        sa_hip_index* idx = nullptr;
        if ((rc = get_idx(n, &idx))) return rc;
        *idx_used = idx;
        t.plan = 0;
        idx->has_index = false;   // its text buffer is overwritten from here on
        SA_HIP_CHECK(hipEventRecord(ws.ev[0], idx->stream));
        if ((rc = ints::map_bytes<S>(ws, idx->stream, T, n, idx->b.text.as<u8>()))) return rc;
        if ((rc = rebuild(idx, n, 0))) return rc;
        *res = IntRes::INDEX_U32; *res_ptr = idx->b.sa;
        if (out32 && !to_index) {
            SA_HIP_CHECK(hipMemcpyAsync(out32, idx->b.sa, n * 4, hipMemcpyDeviceToDevice, idx->stream));
            *res = IntRes::DEV_I32; *res_ptr = out32;
        } else if (out64 && !to_index) {
            if ((rc = ints::widen(idx->stream, idx->b.sa, n, out64))) return rc;
            *res = IntRes::DEV_U64; *res_ptr = out64;
        }
        SA_HIP_CHECK(hipEventRecord(ws.ev[1], idx->stream));
        SA_HIP_CHECK(hipEventSynchronize(ws.ev[1]));
        SA_HIP_CHECK(hipEventElapsedTime(&route_ms, ws.ev[0], ws.ev[1]));
        const sa_hip_build_stats& bs = idx->b.stats;
        t.bits_per_symbol = bs.bits_per_symbol;
        t.symbols_per_key = bs.initial_chars;
        t.sort_passes = bs.radix_passes;
        t.rounds = bs.rounds;
        t.tied_total = bs.active_total;
    } else {                             // route B: integer keys, the 64-bit build's sort and doubling
        t.plan = 1;
        u64* sa64 = reinterpret_cast<u64*>(out64);
        if (!sa64) { if ((rc = ws.sa64.ensure(n * 8 + 64))) return rc; sa64 = ws.sa64.as<u64>(); }
        rc = ints::build_keys<S>(ws, stream, T, n, a, sa64);
        if (rc) return rc;
        float narrow_ms = 0.f;
        *res = IntRes::DEV_U64; *res_ptr = sa64;
        if (out32) {
            SA_HIP_CHECK(hipEventRecord(ws.ev[0], stream));
            if ((rc = ints::narrow(stream, sa64, n, out32))) return rc;
            SA_HIP_CHECK(hipEventRecord(ws.ev[1], stream));
            SA_HIP_CHECK(hipEventSynchronize(ws.ev[1]));
            SA_HIP_CHECK(hipEventElapsedTime(&narrow_ms, ws.ev[0], ws.ev[1]));
            *res = IntRes::DEV_I32; *res_ptr = out32;
        }
        SA_HIP_CHECK(hipStreamSynchronize(stream));
        const big::BigStats& bs = ws.big.stats;
        t.bits_per_symbol = bs.bits_per_symbol;
        t.symbols_per_key = bs.initial_chars;
        t.sort_passes = bs.sort_passes;
        t.rounds = bs.rounds;
        t.tied_after_sort = bs.tied_after_sort;
        t.tied_total = bs.tied_total;
        route_ms = bs.total_ms + narrow_ms;
    }
    t.total_ms = (double)alpha_ms + (double)route_ms;
    if (st) *st = t;
    return 0;
}

// Host drop-ins: T (n >= 2 symbols of S) up through the shared ring into a scratch buffer, the build, SA down.  OUT = int32_t or
// int64_t.  Arguments checked by the caller.
template <class S, class OUT>
int oneshot_int(const S* T, OUT* SA, uint64_t n, int64_t k) {
    HostCall hc(n);
    OneShot& g = hc.g;
    sa_hip_call_breakdown& bd = hc.bd;
    const size_t tbytes = (size_t)n * sizeof(S);
    int rc = hc.attach_stream([&] { return g.l_stream && g.ring.ready && g.i_text.cap >= tbytes + 64; });
    if (rc || (rc = g.i_text.ensure(tbytes + 64))) return rc;
    hc.phase(&bd.workspace_ms);
    if ((rc = ring_upload(g.ring, g.l_stream, hc.device, g.i_text.p, reinterpret_cast<const u8*>(T), tbytes))) return rc;
    hc.phase(&bd.upload_ms);
    auto get_idx = [&](u64 need, sa_hip_index** out) -> int {   // the cached index handle of sa_hip_libsais
        const int r2 = hc.attach_index(need);
        *out = hc.idx;
        return r2;
    };
    // route B narrows an int32 result into the text's own buffer (the text is not read after the keys are built)
    int32_t* out32 = sizeof(OUT) == 4 ? g.i_text.as<int32_t>() : nullptr;
    IntRes res;
    const void* res_ptr = nullptr;
    sa_hip_index* idx = nullptr;
    sa_hip_int_stats st{};
    rc = int_core<S>(g.ints, g.l_stream, g.i_text.as<S>(), n, k, get_idx, out32, nullptr, true, &st, &res, &res_ptr, &idx);
    g.ints.big.destroy();
    if (rc) { g.ints.sa64.release(); return rc; }
    hc.phase(&bd.build_ms);
    bd.build_device_ms = st.total_ms;
    if (res == IntRes::DEV_U64) rc = ring_download(g.ring, hc.device, static_cast<const u64*>(res_ptr), SA, (size_t)n);
    else rc = ring_download(g.ring, hc.device, static_cast<const u32*>(res_ptr), SA, (size_t)n);
    g.ints.sa64.release();
    if (rc) return rc;
    hc.phase(&bd.download_ms);
    return hc.commit();
}

template <class S, class OUT>
OUT int_dropin(const S* T, OUT* SA, OUT n, OUT k, OUT fs, OUT threads, const char* name) {
    if (T == nullptr || SA == nullptr || n < 0 || fs < 0 || threads < 0) return fail(SA_HIP_EINVAL, name, "invalid arguments");
    if (n < 2) { if (n == 1) SA[0] = 0; return 0; }   // libsais.c:6640-6644: T[0] not looked at
    if (k < 1) return fail(SA_HIP_EINVAL, name, "k < 1");
    return (OUT)oneshot_int<S, OUT>(T, SA, (uint64_t)n, (int64_t)k);
}

// Device forms: one stream, one workspace and (route A) one index handle per call.
template <class S, class OUT>
int int_device(const S* T_dev, OUT* SA_dev, int64_t n, int64_t k, int device, sa_hip_int_stats* stats, const char* name) {
    if (n < 0) return fail(SA_HIP_EINVAL, name, "negative length");
    if ((!T_dev || !SA_dev) && n) return fail(SA_HIP_EINVAL, name, "NULL argument");
    if (stats) { memset(stats, 0, sizeof *stats); stats->n = (u64)n; }
    if (n >= 2 && k < 1) return fail(SA_HIP_EINVAL, name, "k < 1");
    if (n == 0) return 0;
    ints::Workspace ws;
    TempIndex tmp;
    DeviceCall dc;
    int rc = dc.open(device);
    if (rc) return rc;
    dc.releases(ws);
    if (n == 1) { SA_HIP_CHECK(hipMemset(SA_dev, 0, sizeof(OUT))); SA_HIP_CHECK(hipDeviceSynchronize()); return 0; }
    auto get_idx = [&](u64 need, sa_hip_index** out) -> int {
        int r2 = sa_hip_index_create(&tmp.idx, need, device);
        if (r2) return r2;
        *out = tmp.idx;
        return 0;
    };
    IntRes res;
    const void* res_ptr = nullptr;
    sa_hip_index* idx = nullptr;
    int32_t* out32 = nullptr;
    int64_t* out64 = nullptr;
    if constexpr (sizeof(OUT) == 4) out32 = reinterpret_cast<int32_t*>(SA_dev); else out64 = reinterpret_cast<int64_t*>(SA_dev);
    return int_core<S>(ws, dc.stream, T_dev, (u64)n, k, get_idx, out32, out64, false, stats, &res, &res_ptr, &idx);
}

}  // namespace

extern "C" {

int32_t sa_hip_libsais_int_omp(int32_t* T, int32_t* SA, int32_t n, int32_t k, int32_t fs, int32_t threads) {
    return int_dropin<int32_t, int32_t>(T, SA, n, k, fs, threads, "sa_hip_libsais_int");
}
int32_t sa_hip_libsais_int(int32_t* T, int32_t* SA, int32_t n, int32_t k, int32_t fs) {
    return sa_hip_libsais_int_omp(T, SA, n, k, fs, 0);
}
int64_t sa_hip_libsais64_long_omp(int64_t* T, int64_t* SA, int64_t n, int64_t k, int64_t fs, int64_t threads) {
    return int_dropin<int64_t, int64_t>(T, SA, n, k, fs, threads, "sa_hip_libsais64_long");
}
int64_t sa_hip_libsais64_long(int64_t* T, int64_t* SA, int64_t n, int64_t k, int64_t fs) {
    return sa_hip_libsais64_long_omp(T, SA, n, k, fs, 0);
}
int sa_hip_libsais_int_device(const int32_t* T_dev, int32_t* SA_dev, int32_t n, int32_t k, int device, sa_hip_int_stats* stats) {
    return int_device<int32_t, int32_t>(T_dev, SA_dev, n, k, device, stats, "sa_hip_libsais_int_device");
}
int sa_hip_libsais64_long_device(const int64_t* T_dev, int64_t* SA_dev, int64_t n, int64_t k, int device, sa_hip_int_stats* stats) {
    return int_device<int64_t, int64_t>(T_dev, SA_dev, n, k, device, stats, "sa_hip_libsais64_long_device");
}

}  // extern "C"
