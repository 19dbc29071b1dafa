// sa_capi.hip -- the C ABI of libsa_hip.so (include/sa_hip.h).  Single translation unit for
// gfx950: hipcc --offload-arch=gfx950 -shared -fPIC.  No CPU fallback: every entry point needs
// a HIP device and fails with SA_HIP_EHIP when there is none.
//
// This file: the index handle with its build, query, record-retrieval, replica, multi-GPU, CSV and on-disk entry points.
// capi_dropins.hpp (included below, same translation unit): the libsais- / engine-call-compatible entry points, their device
// forms and the process-level workspace they share.  capi_token.hpp, capi_token_docs.hpp, capi_token_all.hpp, capi_token_cnf.hpp,
// capi_token_match.hpp and capi_token_shards.hpp with capi_token_shard_match.hpp, capi_token_shard_score.hpp,
// capi_token_shard_docs.hpp and capi_token_shard_all.hpp (included at the end): the token index, its documents, per-document counts,
// AND groups and CNF queries, matching statistics, and sets of token indexes with their matching statistics, infinity-gram scores,
// documents, per-document counts and AND groups.
#include <array>
#include <exception>
#include <mutex>
#include <new>
#include <vector>

#include "common.hpp"
#include "radix_sort.hpp"
#include "sa_build.hpp"
#include "sa_query.hpp"
#include "big_build.hpp"
#include "csv_ingest.hpp"
#include "records.hpp"
#include "host_io.hpp"
#include "rows_device.hpp"
#include "host_index.hpp"
#include "comm_rccl.hpp"
#include "lcp.hpp"
#include "bwt.hpp"
#include "int_build.hpp"
#include <memory>
#include <chrono>

using namespace sa;

// The mapped pinned block of the per-call paths (sa_hip_index_query_hits, _query_rows, a small sa_hip_query_batch) as one side sees
// it, host or device.  One query: [0,8) range, [8,12) hit count, [64, 64 + 4*MAX_HITS) hits or rows, 16 bytes of offsets {0, len},
// the pattern up to BYTES - 64 (zero padded).  A small batch lays its ranges, offsets and patterns over the same bytes.
struct QueryBlock {
    static constexpr u32 MAX_HITS = 4096;
    static constexpr size_t BYTES = 64 * 1024, OFF_HITS = 64, OFF_OFFSETS = OFF_HITS + 4 * MAX_HITS, OFF_PATTERN = OFF_OFFSETS + 64;
    static constexpr u64 MAX_PATTERN = BYTES - 64 - OFF_PATTERN;
    static constexpr u64 SMALL_Q = 448, SMALL_BYTES = 16384;
    static constexpr size_t SB_OUT = 0, SB_OFF = 4096, SB_PAT = 8192;
    static_assert(SMALL_Q * 8 <= SB_OFF && (SMALL_Q + 1) * 8 <= SB_PAT - SB_OFF && SB_PAT + SMALL_BYTES + 64 <= BYTES, "small-batch layout");
    u8* base = nullptr;
    sa_hip_pair_u32* range() const { return reinterpret_cast<sa_hip_pair_u32*>(base); }
    u32* nhits() const { return reinterpret_cast<u32*>(base + 8); }
    u32* hits() const { return reinterpret_cast<u32*>(base + OFF_HITS); }
    u64* offsets() const { return reinterpret_cast<u64*>(base + OFF_OFFSETS); }
    u8* pattern() const { return base + OFF_PATTERN; }
    sa_hip_pair_u32* sb_out() const { return reinterpret_cast<sa_hip_pair_u32*>(base + SB_OUT); }
    u64* sb_off() const { return reinterpret_cast<u64*>(base + SB_OFF); }
    u8* sb_pat() const { return base + SB_PAT; }
};

struct sa_hip_index {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    Builder b;
    bool has_index = false;
    // query staging (host-pointer API)
    DevBuf q_pat, q_off, q_out;
    DevBuf widen;
    QueryBlock qh_host, qh_dev;   // the pinned, device-mapped block (made on first use: query_block) and the same block as the device sees it
    // HIP events of the last QRING search launches: a pipelined caller (distributed.py: search chunk k+1 while chunk k is
    // gathered) asks for the statistics once per step, and every launch since the previous call is resolved then
    static constexpr int QRING = 32;
    hipEvent_t q_ev[QRING][2] = {};
    int q_head = 0, q_pending = 0;
    double q_sum_ms = 0.0;       // resolved launches since the last sa_hip_index_query_stats
    double q_last_ms = 0.0;
    u32 q_launches = 0;
    hipEvent_t w_begin = nullptr, w_end = nullptr;   // sa_hip_index_widen_device
    double widen_ms = 0.0;                           // < 0: recorded, not yet resolved
    sa_hip_query_stats qstats{};
    HostU64Array row_starts;   // sa_hip_index_set_rows: offset of every row (document, CSV field) in the indexed text
    DevBuf rows_dev;               // the same table in HBM (rows_device.hpp)
    DevBuf rows_coarse;            // every 256th entry of it (stays cached)
    u64 rows_coarse_n = 0;
    DevBuf r_rows, r_counts;       // results of the rows kernel (batched form)
    DevBuf r_pending;              // ... and the list of the queries its lane kernel leaves to the workgroup form (+ its length)
    std::unique_ptr<HostIndex> host;   // set: the opt-in no-GPU path of config 1 (host_index.hpp); nothing below touches HIP then
    bool receiving = false;        // sa_hip_index_replica_reserve .. _commit: the buffers are being filled by the caller
    bool k2_auto = true;           // sa_hip_index_deep_keys: large batches build the second-level keys on their way
    DevBuf qc_hist, qc_off, qc_part, qc_tmp;   // clustering of a large batch over a wide-key index (sa_query.hpp: qcluster_*)
    sa_hip_replica_layout pending{};
    lcp::Workspace lcp_ws;         // sa_hip_index_[p]lcp_device (lcp.hpp)
    bwt::Workspace bwt_ws;         // sa_hip_index_bwt_device (bwt.hpp)
    auto buffers() {               // every DevBuf member above (b and the two workspaces release their own)
        return std::array{&q_pat, &q_off, &q_out, &widen, &rows_dev, &rows_coarse, &r_rows, &r_counts, &r_pending, &qc_hist, &qc_off, &qc_part, &qc_tmp};
    }
    auto events() {                // every event above
        std::array<hipEvent_t*, 2 * QRING + 2> e{&w_begin, &w_end};
        for (int i = 0; i < 2 * QRING; ++i) e[2 + i] = &q_ev[i / 2][i % 2];
        return e;
    }
};

// multi-GPU lifecycle (comm_rccl.hpp): one communicator per process / GPU
struct sa_hip_comm {
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0, device = 0;
    hipStream_t stream = nullptr;   // replication runs here; the range gather runs on the searching index's stream
};

// CSV-mode index (SuffixArrayIndex of the reference, engine.h:163-172): the device index over one column + the row
// tables + the memory-mapped file the rows are copied out of
struct sa_hip_csv_index {
    sa_hip_index* idx = nullptr;
    HostU64Array row_file_offsets;   // num_rows + 1
    std::vector<std::string> columns;
    u32 column_index = 0;
    std::string path;
    const u8* map = nullptr;
    u64 map_len = 0;
};

namespace {

int set_device(int device) {
    SA_HIP_CHECK(hipSetDevice(device));
    return 0;
}

// One call on an index handle: what nearly every entry point below opens with, as steps.  An entry point takes the steps it needs
// in ITS order -- which refusal wins when two apply is part of the interface and differs between entry points -- and keeps its
// own checks (NULL outputs, ranges, an empty batch) between them.  The helpers that run under a lock already held (*_locked) take
// the steps without lock().
// Every step returns 0 or the error code, which stays in `rc`: if (c.lock() || c.device_form() || c.has_index()) return c.rc;
struct IndexCall {   // (not copyable: the lock)
    sa_hip_index* const idx;
    const char* const who;
    std::unique_lock<std::mutex> held;
    int rc = 0;

    IndexCall(sa_hip_index* idx, const char* who) : idx(idx), who(who) {}
    // refuses a NULL handle -- together with the NULL arguments of an entry point that names them in one text -- then locks
    int lock(const char* null_text = "NULL index", bool args = true) {
        if (!idx || !args) return rc = fail(SA_HIP_EINVAL, who, null_text);
        held = std::unique_lock<std::mutex>(idx->mu);
        return 0;
    }
    int device_form() { return rc = idx->host ? fail(SA_HIP_EHIP, who, "the host path (no HIP device) has no device buffers") : 0; }
    int has_index() { return rc = idx->has_index ? 0 : fail(SA_HIP_EINVAL, who, "no index"); }
    int current() { return rc = set_device(idx->device); }
};

// A build over the text in idx's own buffer (the caller holds idx->mu): the handle has no index while it runs or after it failed.
int rebuild(sa_hip_index* idx, u64 n, u32 L, int64_t* sa64_dev = nullptr) {
    idx->has_index = false;
    idx->widen_ms = 0.0;
    const int rc = idx->b.build(n, L, sa64_dev);
    idx->has_index = (rc == 0);
    return rc;
}

// idx->b.sa[first .. first + count) or the text, to the host (the caller holds idx->mu and has checked the index and `out`)
int copy_to_host(IndexCall& c, void* out, const void* src_dev, size_t bytes) {
    if (c.current()) return c.rc;
    if (bytes) SA_HIP_CHECK(hipMemcpyAsync(out, src_dev, bytes, hipMemcpyDeviceToHost, c.idx->stream));
    SA_HIP_CHECK(hipStreamSynchronize(c.idx->stream));
    return 0;
}

// an SA entry >= n would send the query kernel's text reads out of bounds: counts them into *bad_host, which is valid after the
// stream's next synchronisation
int check_sa_entries(sa_hip_index* idx, const u32* sa, u64 n, u64* bad_host) {
    u64* bad = reinterpret_cast<u64*>(idx->b.small.as<u8>() + 3072);
    SA_HIP_CHECK(hipMemsetAsync(bad, 0, 8, idx->stream));
    hipLaunchKernelGGL(sa_range_check_kernel, dim3(stream_grid(n, 1024)), dim3(256), 0, idx->stream, sa, n, bad);
    SA_HIP_CHECK(hipMemcpyAsync(bad_host, bad, 8, hipMemcpyDeviceToHost, idx->stream));
    return 0;
}

// resolves the `count` oldest pending launches of the event ring (blocks until they have finished)
int resolve_query_events(sa_hip_index* idx, int count) {
    for (; count > 0 && idx->q_pending > 0; --count) {
        const int slot = (idx->q_head - idx->q_pending + 2 * sa_hip_index::QRING) % sa_hip_index::QRING;
        SA_HIP_CHECK(hipEventSynchronize(idx->q_ev[slot][1]));
        float ms = 0.f;
        SA_HIP_CHECK(hipEventElapsedTime(&ms, idx->q_ev[slot][0], idx->q_ev[slot][1]));
        idx->q_sum_ms += ms;
        idx->q_last_ms = ms;
        --idx->q_pending;
    }
    return 0;
}

// second-level keys of a wide-key index (sa_query.hpp: k2_build_kernel), built once per index state; the caller holds idx->mu
// and has set the device.  Without memory for them (8 n bytes) the text search stays: not an error.
constexpr u64 K2_AUTO_BATCH = 32768;   // a batch of at least this many patterns builds them on its way (one gather over the tied slots)
int ensure_k2(sa_hip_index* idx) {
    Builder& b = idx->b;
    if (b.k2_ready || !b.qkeys || b.n < 2 || !idx->has_index) return 0;
    static const bool off = [] { const char* e = diag_env("SA_HIP_K2"); return e && atoi(e) == 0; }();
    if (off) return 0;
    int k2n = 64 / (b.q_b > 0 ? b.q_b : 1);
    if (k2n > 16) k2n = 16;
    if (b.qkeys2.ensure((size_t)b.n * 8 + 64)) return 0;
    if (b.qskeys.ensure(((size_t)b.n / SKEY_STRIDE + 2) * 8 + 64)) return 0;
    hipLaunchKernelGGL(skeys_kernel, dim3(stream_grid(b.n / SKEY_STRIDE + 1, 256)), dim3(256), 0, idx->stream, b.qkeys, b.n, b.qskeys.as<u64>());
    hipLaunchKernelGGL(k2_build_kernel, dim3(stream_grid(b.n, 256)), dim3(256), 0, idx->stream, b.qkeys, (const u32*)b.sa, (const u8*)b.text.as<u8>(), b.n,
                       b.qmap, b.q_b, b.q_k0, k2n, b.max_suffix_length, b.qkeys2.as<u64>());
    SA_HIP_CHECK(hipGetLastError());
    b.q_k2n = k2n;
    b.k2_ready = true;
    return 0;
}

QueryArgs query_args(sa_hip_index* idx, const u8* pat_dev, const u64* off_dev, u64 Q, sa_hip_pair_u32* out_dev, u64 fixed_len) {
    QueryArgs a;
    a.keys2 = idx->b.k2_ready ? idx->b.qkeys2.as<u64>() : nullptr;
    a.skeys = idx->b.k2_ready ? idx->b.qskeys.as<u64>() : nullptr;
    a.perm = nullptr;
    a.k2n = idx->b.q_k2n;
    a.fixed_len = fixed_len;
    a.text = idx->b.text.as<u8>();
    a.sa = idx->b.sa;
    a.n = idx->b.n;
    a.max_suffix_length = idx->b.max_suffix_length;
    a.patterns = pat_dev;
    a.offsets = off_dev;
    a.q = Q;
    a.out = out_dev;
    a.keys = idx->b.qkeys;
    a.keys32 = idx->b.qkeys32;
    a.lo_shift = idx->b.q_lo_shift;
    a.sector_search = idx->b.sector_search;
    a.dir = idx->b.qdir.as<u32>();
    a.b = idx->b.q_b; a.k0 = idx->b.q_k0; a.dbits = idx->b.q_dbits;
    return a;
}

// The search's switches (under SA_HIP_DIAG=1 only), read once at the top of every launch: the tests flip them on a live handle.
// SA_HIP_QCLUSTER_MIN lowers the clustering threshold for the tests, SA_HIP_QCLUSTER=0 switches the clustering off.
struct QuerySwitches {
    u64 cluster_min = 1ull << 20;
    QuerySwitches() {
        if (const char* e = diag_env("SA_HIP_QCLUSTER_MIN")) cluster_min = strtoull(e, nullptr, 10);
        if (const char* e = diag_env("SA_HIP_QCLUSTER")) { if (atoi(e) == 0) cluster_min = ~0ull; }
    }
};

// A large batch over a wide-key index is answered in the order of its patterns' first characters (qcluster_*).
// (from 2^20 patterns on: its ten small launches cost ~0.11 ms -- 1e6 names 0.324 vs 0.331 ms, 8e6 names 1.75 vs 2.40 ms)
struct ClusterShape {
    u32 qtiles;
    u64 hlen, nparts;
    explicit ClusterShape(u64 Q) : qtiles((u32)((Q + QC_TILE - 1) / QC_TILE)), hlen((u64)QC_BINS * qtiles), nparts((hlen + big::SC_TILE - 1) / big::SC_TILE) {}
};

// whether this batch is clustered, with the buffers for it (no memory: the plain order); before the launch's timed region
bool cluster_buffers(sa_hip_index* idx, const QuerySwitches& sw, const QueryArgs& a) {
    const u64 Q = a.q, cluster_min = sw.cluster_min;
    const bool cluster = Q >= cluster_min && Q >= QC_TILE && Q < 0xFFFFFFFFull && a.keys && idx->k2_auto;
    const ClusterShape s(Q);
    return cluster && !(idx->qc_hist.ensure(s.hlen * 4 + 64) || idx->qc_off.ensure(s.hlen * 8 + 64) || idx->qc_part.ensure((s.nparts + 1) * 8 + 64) ||
             idx->qc_tmp.ensure((size_t)Q * 16 + 64));
}

// the two passes of five small launches each, inside the timed region; returns the permutation
const u32* cluster_batch(sa_hip_index* idx, const QueryArgs& a) {
    const u64 Q = a.q;
    const ClusterShape s(Q);
    u32* qkey = idx->qc_tmp.as<u32>();
    u32* tmp = qkey + Q;
    u32* perm0 = tmp + Q;
    u32* perm1 = perm0 + Q;
    const u32 g = stream_grid(Q, 256);
    for (int pass = 0; pass < 2; ++pass) {
        const u32* order = pass ? perm0 : nullptr;
        hipLaunchKernelGGL(qcluster_rank_kernel, dim3(s.qtiles), dim3(256), 0, idx->stream, a, idx->b.qmap, pass, order, qkey, tmp, idx->qc_hist.as<u32>(), s.qtiles);
        hipLaunchKernelGGL(big::bg_scan_reduce_kernel, dim3((u32)s.nparts), dim3(big::SC_BLOCK), 0, idx->stream, (const u32*)idx->qc_hist.as<u32>(), s.hlen,
                           idx->qc_part.as<u64>());
        hipLaunchKernelGGL(big::bg_scan_parts_kernel, dim3(1), dim3(big::SC_BLOCK), 0, idx->stream, idx->qc_part.as<u64>(), s.nparts);
        hipLaunchKernelGGL(big::bg_scan_apply_kernel, dim3((u32)s.nparts), dim3(big::SC_BLOCK), 0, idx->stream, (const u32*)idx->qc_hist.as<u32>(), s.hlen,
                           (const u64*)idx->qc_part.as<u64>(), idx->qc_off.as<u64>());
        hipLaunchKernelGGL(qcluster_place_kernel, dim3(g), dim3(256), 0, idx->stream, Q, (const u64*)idx->qc_off.as<u64>(), (const u32*)tmp, order, s.qtiles,
                           pass ? perm1 : perm0);
    }
    return perm1;
}

// query_kernel<NARROW, SECTOR>: wide keys or narrow ones, the index's sector form (anything but 1 and 2: the plain bisection)
void launch_query_kernel(sa_hip_index* idx, const QueryArgs& a) {
    using Kernel = void (*)(QueryArgs, CodeMap);
    static constexpr Kernel form[2][3] = {{query_kernel<false, 0>, query_kernel<false, 1>, query_kernel<false, 2>},
                                          {query_kernel<true, 0>, query_kernel<true, 1>, query_kernel<true, 2>}};
    if (!a.q) return;
    u64 g = (a.q + 255) / 256;
    if (g > 256u * 16u) g = 256u * 16u;
    const int sector = (a.sector_search == 1 || a.sector_search == 2) ? a.sector_search : 0;
    hipLaunchKernelGGL(form[a.keys32 ? 1 : 0][sector], dim3((u32)g), dim3(256), 0, idx->stream, a, idx->b.qmap);
}

// the event ring: the slot of the next launch (the oldest pending launch is resolved first when all are taken) ...
int claim_query_slot(sa_hip_index* idx, hipEvent_t** ev) {
    if (idx->q_pending == sa_hip_index::QRING) { int rc = resolve_query_events(idx, 1); if (rc) return rc; }
    *ev = idx->q_ev[idx->q_head];
    return 0;
}
// ... and the launch entered into it
void advance_query_slot(sa_hip_index* idx, u64 Q) {
    idx->q_head = (idx->q_head + 1) % sa_hip_index::QRING;
    ++idx->q_pending;
    ++idx->q_launches;
    idx->qstats.q = Q;   // the times are resolved lazily by sa_hip_index_query_stats
}

int launch_query(sa_hip_index* idx, const u8* pat_dev, const u64* off_dev, u64 Q, sa_hip_pair_u32* out_dev, u64 fixed_len = 0) {
    const QuerySwitches sw;
    hipEvent_t* ev;
    if (int rc = claim_query_slot(idx, &ev)) return rc;
    if (Q >= K2_AUTO_BATCH && idx->k2_auto) { int rc = ensure_k2(idx); if (rc) return rc; }
    QueryArgs a = query_args(idx, pat_dev, off_dev, Q, out_dev, fixed_len);
    const bool cluster = cluster_buffers(idx, sw, a);
    SA_HIP_CHECK(hipEventRecord(ev[0], idx->stream));
    if (cluster) a.perm = cluster_batch(idx, a);
    launch_query_kernel(idx, a);
    SA_HIP_CHECK(hipEventRecord(ev[1], idx->stream));
    SA_HIP_CHECK(hipGetLastError());
    advance_query_slot(idx, Q);
    return 0;
}

// the pinned block, made on first use (the caller holds idx->mu and has set the device)
int query_block(sa_hip_index* idx) {
    if (idx->qh_host.base) return 0;
    SA_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&idx->qh_host.base), QueryBlock::BYTES, hipHostMallocMapped));
    SA_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&idx->qh_dev.base), idx->qh_host.base, 0));
    return 0;
}

// ONE pattern for the per-call paths: the bound the block sets on it, checked where the entry point checks its arguments ...
int one_pattern_fits(const char* who, u64 len) {
    return len > QueryBlock::MAX_PATTERN ? fail(SA_HIP_EINVAL, who, "pattern longer than 47 KB") : 0;
}
// ... and the pattern staged in the block: offsets {0, len}, the pattern, 64 zero bytes
int stage_one_pattern(sa_hip_index* idx, const u8* pattern, u64 len) {
    int rc = query_block(idx);
    if (rc) return rc;
    const QueryBlock& h = idx->qh_host;
    h.offsets()[0] = 0; h.offsets()[1] = len;
    if (len) memcpy(h.pattern(), pattern, len);
    memset(h.pattern() + len, 0, 64);
    return 0;
}
// QueryArgs of that one pattern, its range into the block
QueryArgs one_pattern_args(sa_hip_index* idx) {
    const QueryBlock& d = idx->qh_dev;
    return query_args(idx, d.pattern(), d.offsets(), 1, d.range(), 0);
}

// A host batch in q_pat / q_off (q_out sized for its ranges): patterns, offsets, the 64-byte pad, through the ring of pinned slabs
// when given one (host_io.hpp), by plain copies otherwise
int stage_batch(sa_hip_index* idx, PinnedRing* ring, const u8* patterns, const u64* offsets, u64 Q) {
    const u64 total = offsets[Q];
    int rc;
    if ((rc = idx->q_pat.ensure((size_t)total + 64))) return rc;
    if ((rc = idx->q_off.ensure((size_t)(Q + 1) * 8))) return rc;
    if ((rc = idx->q_out.ensure((size_t)Q * sizeof(sa_hip_pair_u32)))) return rc;
    if (ring) {
        if ((rc = ring_upload(*ring, idx->stream, idx->device, idx->q_pat.p, patterns, (size_t)total))) return rc;
        if ((rc = ring_upload(*ring, idx->stream, idx->device, idx->q_off.p, reinterpret_cast<const u8*>(offsets), (size_t)(Q + 1) * 8))) return rc;
    } else {
        if (total) SA_HIP_CHECK(hipMemcpyAsync(idx->q_pat.p, patterns, total, hipMemcpyHostToDevice, idx->stream));
        SA_HIP_CHECK(hipMemcpyAsync(idx->q_off.p, offsets, (size_t)(Q + 1) * 8, hipMemcpyHostToDevice, idx->stream));
    }
    SA_HIP_CHECK(hipMemsetAsync(idx->q_pat.as<u8>() + total, 0, 64, idx->stream));
    return 0;
}

// the first hits of a range into hits[], their number into *nhits (one workgroup)
__device__ __forceinline__ void copy_hits(const u32* __restrict__ sa, const sa_hip_pair_u32 rg, const u32 max_hits, u32* __restrict__ hits,
                                          u32* __restrict__ nhits) {
    u32 count = hits_of_range(rg);
    if (count > max_hits) count = max_hits;
    for (u32 i = threadIdx.x; i < count; i += blockDim.x) hits[i] = sa[(u64)rg.first + i];
    if (threadIdx.x == 0) *nhits = count;
}

__global__ __launch_bounds__(256) void hits_copy_kernel(const u32* __restrict__ sa, const sa_hip_pair_u32* __restrict__ range,
                                                        u32 max_hits, u32* __restrict__ hits, u32* __restrict__ nhits) {
    copy_hits(sa, *range, max_hits, hits, nhits);
}

// ONE query + its first hits in one launch (sa_hip_index_query_hits, sa_hip_get_substring_positions[_file]): thread 0 searches,
// the workgroup copies the hits -- launch_query + hits_copy_kernel without the launch (and the two events) in between
template <bool NARROW>
__global__ __launch_bounds__(256) void query_hits_one_kernel(QueryArgs qa, CodeMap map, const u32* __restrict__ sa, u32 max_hits,
                                                             u32* __restrict__ hits, u32* __restrict__ nhits) {
    __shared__ u16 s_map[256];
    __shared__ sa_hip_pair_u32 s_rg;
    s_map[threadIdx.x] = map.code[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        const sa_hip_pair_u32 rg = query_one<NARROW, 2>(qa, s_map, 0);
        qa.out[0] = rg;
        s_rg = rg;
    }
    __syncthreads();
    copy_hits(sa, s_rg, max_hits, hits, nhits);
}

}  // namespace

// The libsais- / engine-call-compatible entry points and the process-level workspace they share (g_oneshot: its ring of pinned
// slabs also carries the large host legs of sa_hip_index_query_rows_batch below)
#include "capi_dropins.hpp"

extern "C" {

const char* sa_hip_last_error(void) { return last_error().c_str(); }
const char* sa_hip_version(void) { return "suffixarray_amd 0.1 (gfx950)"; }

int sa_hip_device_count(void) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) return fail(SA_HIP_EHIP, "hipGetDeviceCount", hipGetErrorString(e));
    return c;
}

int sa_hip_index_create(sa_hip_index** out, uint64_t n_max, int device) {
    if (!out) return fail(SA_HIP_EINVAL, "sa_hip_index_create: out == NULL");
    *out = nullptr;
    if (n_max > 0xFFFFFFFEull) return fail(SA_HIP_EINVAL, "sa_hip_index_create: n_max exceeds 2^32 - 2");
    int cnt = sa_hip_device_count();
    if (cnt <= 0 && host_path_allowed()) {
        // no usable HIP device and the caller opted in (SA_HIP_ALLOW_HOST=1): the small host implementation of config 1
        if (n_max > HOST_MAX_N) return fail(SA_HIP_EINVAL, "sa_hip_index_create: the host path (no HIP device) holds at most 2^24 bytes");
        sa_hip_index* h = new (std::nothrow) sa_hip_index();
        if (!h) return fail(SA_HIP_ENOMEM, "sa_hip_index_create: host allocation");
        try { h->host.reset(new HostIndex()); } catch (const std::bad_alloc&) { delete h; return fail(SA_HIP_ENOMEM, "sa_hip_index_create: host allocation"); }
        h->host->n_max = n_max;
        h->device = -1;
        *out = h;
        return 0;
    }
    if (cnt < 0) return cnt;
    if (device < 0 || device >= cnt) return fail(SA_HIP_EHIP, "sa_hip_index_create: no such HIP device");
    int rc = set_device(device);
    if (rc) return rc;
    sa_hip_index* idx = new (std::nothrow) sa_hip_index();
    if (!idx) return fail(SA_HIP_ENOMEM, "sa_hip_index_create: host allocation");
    idx->device = device;
    hipError_t e = hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete idx; return fail(SA_HIP_EHIP, "hipStreamCreate", hipGetErrorString(e)); }
    rc = idx->b.init(n_max, idx->stream);
    for (hipEvent_t* ev : idx->events())
        if (!rc && hipEventCreate(ev) != hipSuccess) rc = fail(SA_HIP_EHIP, "hipEventCreate");
    if (rc) { sa_hip_index_destroy(idx); return rc; }
    *out = idx;
    return 0;
}

void sa_hip_index_destroy(sa_hip_index* idx) {
    if (!idx) return;
    if (idx->host) { delete idx; return; }
    (void)hipSetDevice(idx->device);
    if (idx->stream) (void)hipStreamSynchronize(idx->stream);
    idx->b.destroy();
    for (DevBuf* b : idx->buffers()) b->release();
    idx->lcp_ws.release();
    idx->bwt_ws.release();
    if (idx->qh_host.base) (void)hipHostFree(idx->qh_host.base);
    for (hipEvent_t* ev : idx->events()) if (*ev) (void)hipEventDestroy(*ev);
    if (idx->stream) (void)hipStreamDestroy(idx->stream);
    delete idx;
}

// the device leg of the three builds: the text into the handle's own buffer (unless it is that buffer), then the build
static int build_from(IndexCall& c, const void* T, uint64_t n, uint32_t L, hipMemcpyKind kind, void* sa64_dev = nullptr) {
    sa_hip_index* idx = c.idx;
    if (c.current()) return c.rc;
    if (n > idx->b.n_max) return fail(SA_HIP_EINVAL, c.who, "n exceeds the index capacity");
    if (n && T != idx->b.text.p) SA_HIP_CHECK(hipMemcpyAsync(idx->b.text.p, T, n, kind, idx->stream));
    return rebuild(idx, n, L, static_cast<int64_t*>(sa64_dev));
}

int sa_hip_index_build(sa_hip_index* idx, const uint8_t* T_host, uint64_t n, uint32_t max_suffix_length) {
    IndexCall c(idx, "sa_hip_index_build");
    if (c.lock("NULL argument", T_host || !n)) return c.rc;
    if (idx->host) {
        HostIndex& h = *idx->host;
        if (n > h.n_max) return fail(SA_HIP_EINVAL, c.who, "n exceeds the index capacity");
        try { h.set_text(T_host, n); h.build(max_suffix_length); }
        catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, c.who, "out of host memory"); }
        idx->has_index = true;
        return 0;
    }
    return build_from(c, T_host, n, max_suffix_length, hipMemcpyHostToDevice);
}

int sa_hip_index_build_device(sa_hip_index* idx, const void* T_dev, uint64_t n, uint32_t max_suffix_length) {
    IndexCall c(idx, "sa_hip_index_build_device");
    if (c.lock("NULL argument", T_dev || !n) || c.device_form()) return c.rc;
    return build_from(c, T_dev, n, max_suffix_length, hipMemcpyDeviceToDevice);
}

int sa_hip_index_build_device64(sa_hip_index* idx, const void* T_dev, uint64_t n, uint32_t max_suffix_length, void* sa64_dev) {
    IndexCall c(idx, "sa_hip_index_build_device64");
    if (c.lock("NULL argument", (T_dev && sa64_dev) || !n) || c.device_form()) return c.rc;
    return build_from(c, T_dev, n, max_suffix_length, hipMemcpyDeviceToDevice, sa64_dev);
}

static int load_common(sa_hip_index* idx, const void* T, const void* SA, uint64_t n, uint32_t L, hipMemcpyKind kind) {
    IndexCall c(idx, "sa_hip_index_load_device");
    c.lock();
    if (idx->host) {
        if (kind != hipMemcpyHostToDevice) return c.device_form();
        HostIndex& h = *idx->host;
        if (n > h.n_max) return fail(SA_HIP_EINVAL, "sa_hip_index_load: n exceeds the index capacity");
        const u32* s32 = static_cast<const u32*>(SA);
        for (u64 i = 0; i < n; ++i) if (s32[i] >= n) return fail(SA_HIP_EINVAL, "sa_hip_index_load: suffix array holds entries >= n");
        try { h.set_text(static_cast<const u8*>(T), n); h.sa.assign(s32, s32 + n); }
        catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, "sa_hip_index_load: out of host memory"); }
        h.L = L; h.ready = true;
        idx->has_index = true;
        return 0;
    }
    int rc = c.current();
    if (rc) return rc;
    if (n > idx->b.n_max) return fail(SA_HIP_EINVAL, "sa_hip_index_load: n exceeds the index capacity");
    Builder& b = idx->b;
    if ((rc = b.sa_own.ensure((size_t)(n ? n : 1) * 4))) return rc;
    idx->has_index = false;
    u64 bad_host = 0;
    if (n) {
        SA_HIP_CHECK(hipMemcpyAsync(b.text.p, T, n, kind, idx->stream));
        SA_HIP_CHECK(hipMemcpyAsync(b.sa_own.p, SA, (size_t)n * 4, kind, idx->stream));
        // refuse an array with entries >= n (the copy of the count rides on the synchronisation prepare_text() does anyway)
        if ((rc = check_sa_entries(idx, b.sa_own.as<u32>(), n, &bad_host))) return rc;
    }
    CodeMap map; u32 sigma; int bits;
    if ((rc = b.prepare_text(n, map, sigma, bits))) return rc;
    if (bad_host) return fail(SA_HIP_EINVAL, "sa_hip_index_load: suffix array holds entries >= n");
    b.sa = b.sa_own.as<u32>();
    b.max_suffix_length = L;
    if ((rc = b.prepare_query_from_sa(map, bits, L))) return rc;
    SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
    idx->has_index = true;
    return 0;
}

int sa_hip_index_load(sa_hip_index* idx, const uint8_t* T_host, const uint32_t* SA_host, uint64_t n,
                      uint32_t max_suffix_length) {
    if (!idx || ((!T_host || !SA_host) && n)) return fail(SA_HIP_EINVAL, "sa_hip_index_load: NULL argument");
    return load_common(idx, T_host, SA_host, n, max_suffix_length, hipMemcpyHostToDevice);
}

int sa_hip_index_load_device(sa_hip_index* idx, const void* T_dev, const void* SA_dev, uint64_t n,
                             uint32_t max_suffix_length) {
    if (!idx || ((!T_dev || !SA_dev) && n)) return fail(SA_HIP_EINVAL, "sa_hip_index_load_device: NULL argument");
    return load_common(idx, T_dev, SA_dev, n, max_suffix_length, hipMemcpyDeviceToDevice);
}

// ---- replicas: the query structures travel as they are -----------------------------------------------
// A replica used to receive text + SA and rebuild the key array by a random gather over the text and the directory by
// binary search (sa_hip_index_load_device: 115 ms at n = 1e9, 5x a build).  The building index already holds all of it:
// the replica reserves buffers of the same layout, the caller fills them (RCCL broadcast straight into them), commit
// range-checks the suffix array.

static void fill_layout(const sa_hip_index* idx, sa_hip_replica_layout* out) {
    const Builder& b = idx->b;
    memset(out, 0, sizeof *out);
    out->n = b.n;
    out->max_suffix_length = b.max_suffix_length;
    out->key_bytes = b.qkeys32 ? 4u : (b.qkeys ? 8u : 0u);
    out->bits_per_symbol = (uint32_t)b.q_b;
    out->initial_chars = (uint32_t)b.q_k0;
    out->dir_bits = out->key_bytes ? (uint32_t)b.q_dbits : 0u;
    out->lo_shift = b.q_lo_shift;
    out->dir_entries = out->key_bytes ? (1ull << b.q_dbits) + 1 : 0;
    memcpy(out->code, b.qmap.code, sizeof out->code);
    memcpy(out->freq, b.freq, sizeof out->freq);
}

int sa_hip_index_replica_layout(sa_hip_index* idx, sa_hip_replica_layout* out) {
    IndexCall c(idx, "sa_hip_index_replica_layout");
    if (c.lock("NULL argument", out) || c.device_form() || c.has_index()) return c.rc;
    fill_layout(idx, out);
    return 0;
}

// (keys: the key array of the layout's width -- the index's own, or the one a replica receives into)
static void fill_buffers(const sa_hip_index* idx, const sa_hip_replica_layout& l, void* keys, sa_hip_replica_buffers* out) {
    const Builder& b = idx->b;
    memset(out, 0, sizeof *out);
    out->text = b.text.p;                       out->text_bytes = l.n;
    out->sa = b.sa;                             out->sa_bytes = l.n * 4;
    out->keys = keys;                           out->keys_bytes = l.n * l.key_bytes;
    out->dir = l.key_bytes ? b.qdir.p : nullptr; out->dir_bytes = l.dir_entries * 4;
}

int sa_hip_index_replica_buffers(sa_hip_index* idx, sa_hip_replica_buffers* out) {
    IndexCall c(idx, "sa_hip_index_replica_buffers");
    if (c.lock("NULL argument", out) || c.device_form() || c.has_index() || c.current()) return c.rc;
    SA_HIP_CHECK(hipStreamSynchronize(idx->stream));   // whoever reads the buffers next runs on another stream
    sa_hip_replica_layout l;
    fill_layout(idx, &l);
    fill_buffers(idx, l, l.key_bytes == 4 ? (void*)idx->b.qkeys32 : (void*)idx->b.qkeys, out);
    return 0;
}

int sa_hip_index_replica_reserve(sa_hip_index* idx, const sa_hip_replica_layout* l, sa_hip_replica_buffers* out) {
    IndexCall c(idx, "sa_hip_index_replica_reserve");
    if (c.lock("NULL argument", l && out) || c.device_form()) return c.rc;
    if (l->n > idx->b.n_max) return fail(SA_HIP_EINVAL, c.who, "n exceeds the index capacity");
    if (l->key_bytes != 0 && l->key_bytes != 4 && l->key_bytes != 8) return fail(SA_HIP_EINVAL, c.who, "bad key width");
    if (l->key_bytes && (l->dir_bits < 8 || l->dir_bits > 28 || l->dir_entries != (1ull << l->dir_bits) + 1 || l->bits_per_symbol < 1 ||
                         l->bits_per_symbol > 16 || l->initial_chars < 1 || l->initial_chars * l->bits_per_symbol > 64 ||
                         l->lo_shift < 0 || l->lo_shift > 63))
        return fail(SA_HIP_EINVAL, c.who, "inconsistent layout");
    int rc;
    if (c.current()) return c.rc;
    Builder& b = idx->b;
    idx->has_index = false;
    if ((rc = b.sa_own.ensure((size_t)(l->n ? l->n : 1) * 4))) return rc;
    if (l->key_bytes) {
        if ((rc = b.keys0.ensure((size_t)l->n * l->key_bytes + 64))) return rc;
        if ((rc = b.qdir.ensure((size_t)l->dir_entries * 4))) return rc;
    }
    SA_HIP_CHECK(hipMemsetAsync(b.text.as<u8>() + l->n, 0, TEXT_PAD + 16, idx->stream));
    SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
    b.n = l->n;
    b.sa = b.sa_own.as<u32>();
    b.qkeys = nullptr; b.qkeys32 = nullptr; b.dir_ready = false; b.k2_ready = false;
    idx->pending = *l;
    idx->receiving = true;
    fill_buffers(idx, *l, l->key_bytes ? b.keys0.p : nullptr, out);
    return 0;
}

int sa_hip_index_replica_commit(sa_hip_index* idx) {
    IndexCall c(idx, "sa_hip_index_replica_commit");
    if (c.lock() || c.device_form()) return c.rc;
    if (!idx->receiving) return fail(SA_HIP_EINVAL, c.who, "nothing reserved");
    int rc;
    if (c.current()) return c.rc;
    Builder& b = idx->b;
    const sa_hip_replica_layout& l = idx->pending;
    idx->receiving = false;
    // what arrived is checked as far as it can send the search out of bounds: SA entries < n, the directory's ends
    u64 bad_host = 0;
    u32 dir_ends[2] = {0, (u32)l.n};
    if (l.n) {
        if ((rc = check_sa_entries(idx, b.sa_own.as<u32>(), l.n, &bad_host))) return rc;
        if (l.key_bytes) {
            SA_HIP_CHECK(hipMemcpyAsync(&dir_ends[0], b.qdir.as<u32>(), 4, hipMemcpyDeviceToHost, idx->stream));
            SA_HIP_CHECK(hipMemcpyAsync(&dir_ends[1], b.qdir.as<u32>() + (l.dir_entries - 1), 4, hipMemcpyDeviceToHost, idx->stream));
        }
        SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
    }
    if (bad_host) return fail(SA_HIP_EINVAL, "sa_hip_index_replica_commit: suffix array holds entries >= n");
    if (dir_ends[0] != 0 || dir_ends[1] != (u32)l.n) return fail(SA_HIP_EINVAL, "sa_hip_index_replica_commit: directory does not span the suffix array");
    b.max_suffix_length = l.max_suffix_length;
    memcpy(b.freq, l.freq, sizeof b.freq);
    memcpy(b.qmap.code, l.code, sizeof l.code);
    b.q_b = (int)l.bits_per_symbol; b.q_k0 = (int)l.initial_chars; b.q_dbits = (int)l.dir_bits; b.q_lo_shift = l.lo_shift;
    b.qkeys = l.key_bytes == 8 ? b.keys0.as<u64>() : nullptr;
    b.qkeys32 = l.key_bytes == 4 ? b.keys0.as<u32>() : nullptr;
    b.k2_ready = false;
    b.dir_ready = l.key_bytes != 0;
    idx->has_index = true;
    return 0;
}

// ---- multi-GPU lifecycle without PyTorch -----------------------------------------------------

int sa_hip_comm_unique_id(void* id128) {
    if (!id128) return fail(SA_HIP_EINVAL, "sa_hip_comm_unique_id: NULL argument");
    RcclApi& r = rccl_api();
    if (!r.ok) return fail(SA_HIP_EHIP, "sa_hip_comm: librccl.so could not be loaded");
    static_assert(sizeof(ncclUniqueId) == SA_HIP_COMM_ID_BYTES, "unique id size");
    ncclUniqueId id;
    SA_RCCL_CHECK(r.GetUniqueId(&id));
    memcpy(id128, &id, sizeof id);
    return 0;
}

int sa_hip_comm_create(sa_hip_comm** out, const void* id128, int nranks, int rank, int device) {
    if (!out || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(SA_HIP_EINVAL, "sa_hip_comm_create: invalid arguments");
    *out = nullptr;
    RcclApi& r = rccl_api();
    if (!r.ok) return fail(SA_HIP_EHIP, "sa_hip_comm: librccl.so could not be loaded");
    int rc = set_device(device);
    if (rc) return rc;
    sa_hip_comm* c = new (std::nothrow) sa_hip_comm();
    if (!c) return fail(SA_HIP_ENOMEM, "sa_hip_comm_create: host allocation");
    c->nranks = nranks; c->rank = rank; c->device = device;
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    ncclResult_t nr = r.CommInitRank(&c->comm, nranks, id, rank);
    if (nr != ncclSuccess) { delete c; return fail(SA_HIP_EHIP, "ncclCommInitRank", r.GetErrorString(nr)); }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { (void)r.CommDestroy(c->comm); delete c; return fail(SA_HIP_EHIP, "hipStreamCreate"); }
    *out = c;
    return 0;
}

void sa_hip_comm_destroy(sa_hip_comm* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    if (c->comm) (void)rccl_api().CommDestroy(c->comm);
    delete c;
}

int sa_hip_comm_rank(const sa_hip_comm* c) { return c ? c->rank : -1; }
int sa_hip_comm_size(const sa_hip_comm* c) { return c ? c->nranks : 0; }

int sa_hip_comm_replicate_index(sa_hip_comm* c, sa_hip_index* idx, int root, uint64_t* bytes_out) {
    if (!c || !idx || root < 0 || root >= c->nranks) return fail(SA_HIP_EINVAL, "sa_hip_comm_replicate_index: invalid arguments");
    if (idx->host) return fail(SA_HIP_EHIP, "sa_hip_comm_replicate_index: the host path (no HIP device) has no device buffers");
    RcclApi& r = rccl_api();
    int rc = set_device(c->device);
    if (rc) return rc;
    // Every fallible LOCAL step comes before a collective and its outcome travels with it, so that all ranks either run all
    // four buffer broadcasts or all return: (1) the root's layout goes out together with the root's status -- a root without
    // an index still broadcasts, with the error set; (2) after every rank has reserved (n > capacity, out of memory) the
    // ranks agree on the worst status by one all-reduce.  A rank that returned early would leave its peers inside
    // ncclBroadcast for good.
    struct Wire { int32_t status; int32_t pad; sa_hip_replica_layout lay; } w;
    memset(&w, 0, sizeof w);
    int rc_local = 0;
    if (c->rank == root) { rc_local = sa_hip_index_replica_layout(idx, &w.lay); w.status = rc_local; }
    void* bounce = nullptr;
    if (hipMalloc(&bounce, sizeof w + 16) != hipSuccess) {
        // (no device memory for ~5 KB: the peers cannot be told either; they fail in the broadcast's own error path)
        return fail(SA_HIP_ENOMEM, "sa_hip_comm_replicate_index: hipMalloc of the bounce buffer");
    }
    int32_t* agree = reinterpret_cast<int32_t*>(static_cast<u8*>(bounce) + sizeof w);
    auto body = [&]() -> int {
        SA_HIP_CHECK(hipMemcpyAsync(bounce, &w, sizeof w, hipMemcpyHostToDevice, c->stream));
        SA_RCCL_CHECK(r.Broadcast(bounce, bounce, sizeof w, ncclUint8, root, c->comm, c->stream));
        SA_HIP_CHECK(hipMemcpyAsync(&w, bounce, sizeof w, hipMemcpyDeviceToHost, c->stream));
        SA_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (w.status != 0)   // the same decision on every rank: nobody enters the buffer broadcasts
            return (c->rank == root) ? rc_local : fail(w.status, "sa_hip_comm_replicate_index: the root has no index to replicate");
        sa_hip_replica_buffers b;
        memset(&b, 0, sizeof b);
        rc_local = (c->rank == root) ? sa_hip_index_replica_buffers(idx, &b) : sa_hip_index_replica_reserve(idx, &w.lay, &b);
        int32_t mine = rc_local, worst = 0;   // error codes are negative: the minimum is the worst
        SA_HIP_CHECK(hipMemcpyAsync(agree, &mine, 4, hipMemcpyHostToDevice, c->stream));
        SA_RCCL_CHECK(r.AllReduce(agree, agree, 1, ncclInt32, ncclMin, c->comm, c->stream));
        SA_HIP_CHECK(hipMemcpyAsync(&worst, agree, 4, hipMemcpyDeviceToHost, c->stream));
        SA_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (worst != 0)
            return rc_local ? rc_local : fail(worst, "sa_hip_comm_replicate_index: another rank could not provide / reserve its buffers");
        void* ptr[4] = {b.text, b.sa, b.keys, b.dir};
        const u64 len[4] = {b.text_bytes, b.sa_bytes, b.keys_bytes, b.dir_bytes};
        u64 total = 0;
        for (int i = 0; i < 4; ++i) {
            if (!len[i]) continue;
            SA_RCCL_CHECK(r.Broadcast(ptr[i], ptr[i], (size_t)len[i], ncclUint8, root, c->comm, c->stream));
            total += len[i];
        }
        SA_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (bytes_out) *bytes_out = total;
        return (c->rank == root) ? 0 : sa_hip_index_replica_commit(idx);   // local, after the last collective
    };
    rc = body();
    (void)hipFree(bounce);
    return rc;
}

int sa_hip_comm_allgather_ranges(sa_hip_comm* c, sa_hip_index* idx, const void* send_dev, uint64_t pairs_per_rank, void* recv_dev) {
    if (!c || !idx || ((!send_dev || !recv_dev) && pairs_per_rank)) return fail(SA_HIP_EINVAL, "sa_hip_comm_allgather_ranges: NULL argument");
    if (idx->host) return fail(SA_HIP_EHIP, "sa_hip_comm_allgather_ranges: the host path (no HIP device) has no device buffers");
    if (pairs_per_rank == 0) return 0;
    int rc = set_device(c->device);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(idx->mu);
    // on the index's own stream: ordered after the search that produced send_dev, no host synchronisation in between
    SA_RCCL_CHECK(rccl_api().AllGather(send_dev, recv_dev, (size_t)pairs_per_rank * sizeof(sa_hip_pair_u32), ncclUint8, c->comm, idx->stream));
    return 0;
}

uint64_t sa_hip_index_n(const sa_hip_index* idx) { return idx ? (idx->host ? idx->host->n : idx->b.n) : 0; }
uint32_t sa_hip_index_max_suffix_length(const sa_hip_index* idx) { return idx ? (idx->host ? idx->host->L : idx->b.max_suffix_length) : 0; }
const void* sa_hip_index_text_dev(const sa_hip_index* idx) { return (idx && !idx->host) ? idx->b.text.p : nullptr; }
const void* sa_hip_index_sa_dev(const sa_hip_index* idx) { return (idx && idx->has_index && !idx->host) ? idx->b.sa : nullptr; }
void* sa_hip_index_stream(const sa_hip_index* idx) { return idx ? (void*)idx->stream : nullptr; }

int sa_hip_index_deep_keys(sa_hip_index* idx, int mode) {
    IndexCall c(idx, "sa_hip_index_deep_keys");
    if (!idx || mode < 0 || mode > 2) return fail(SA_HIP_EINVAL, c.who, "invalid arguments");
    if (idx->host) return 0;
    if (c.lock() || c.current()) return c.rc;
    if (mode == 0) {   // never: drop them (8 n bytes back), large batches do not build them
        SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
        idx->k2_auto = false;
        idx->b.k2_ready = false;
        idx->b.qkeys2.release();
        idx->b.qskeys.release();
        return 0;
    }
    idx->k2_auto = true;
    if (mode == 2) {
        if (c.has_index() || (c.rc = ensure_k2(idx))) return c.rc;
        SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
    }
    return idx->b.k2_ready ? 1 : 0;
}

int sa_hip_index_sync(sa_hip_index* idx) {
    if (!idx) return fail(SA_HIP_EINVAL, "sa_hip_index_sync: NULL index");
    if (idx->host) return 0;
    int rc = set_device(idx->device);
    if (rc) return rc;
    SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
    return 0;
}

int sa_hip_index_verify(sa_hip_index* idx, uint64_t* violations) {
    IndexCall c(idx, "sa_hip_index_verify");
    if (c.lock("NULL argument", violations) || c.has_index()) return c.rc;   // has_index / n are only read under the lock (a concurrent build rewrites them)
    if (idx->host) { *violations = idx->host->verify(); return 0; }
    if (c.current()) return c.rc;
    return idx->b.verify(violations);
}

int sa_hip_index_get_sa_u32(sa_hip_index* idx, uint32_t* out_host) {
    IndexCall c(idx, "sa_hip_index_get_sa_u32");
    if (c.lock() || c.has_index()) return c.rc;
    if (!out_host && sa_hip_index_n(idx)) return fail(SA_HIP_EINVAL, c.who, "NULL output");
    if (idx->host) { if (idx->host->n) memcpy(out_host, idx->host->sa.data(), (size_t)idx->host->n * 4); return 0; }
    return copy_to_host(c, out_host, idx->b.sa, (size_t)idx->b.n * 4);
}

int sa_hip_index_get_sa_i64(sa_hip_index* idx, int64_t* out_host) {
    IndexCall c(idx, "sa_hip_index_get_sa_i64");
    if (c.lock() || c.has_index()) return c.rc;
    if (!out_host && sa_hip_index_n(idx)) return fail(SA_HIP_EINVAL, c.who, "NULL output");
    if (idx->host) { for (u64 i = 0; i < idx->host->n; ++i) out_host[i] = (int64_t)idx->host->sa[i]; return 0; }
    int rc;
    if (c.current()) return c.rc;
    const u64 n = idx->b.n;
    if (n) {
        // widen on the device in slabs (libsais64.c:6248-6259 does this on the CPU, in place)
        const u64 slab = 64ull << 20;
        if ((rc = idx->widen.ensure((size_t)(n < slab ? n : slab) * 8))) return rc;
        for (u64 o = 0; o < n; o += slab) {
            const u64 cnt = (n - o) < slab ? (n - o) : slab;
            hipLaunchKernelGGL(widen_kernel, dim3(stream_grid(cnt, 1024)), dim3(256), 0, idx->stream, idx->b.sa + o, cnt,
                               idx->widen.as<int64_t>());
            SA_HIP_CHECK(hipMemcpyAsync(out_host + o, idx->widen.p, (size_t)cnt * 8, hipMemcpyDeviceToHost, idx->stream));
            SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
        }
    }
    return 0;
}

int sa_hip_index_widen_device(sa_hip_index* idx, void* out_dev) {
    IndexCall c(idx, "sa_hip_index_widen_device");
    if (c.lock() || c.device_form() || c.has_index()) return c.rc;
    const u64 n = idx->b.n;
    if (!out_dev && n) return fail(SA_HIP_EINVAL, c.who, "NULL output");
    if (c.current()) return c.rc;
    SA_HIP_CHECK(hipEventRecord(idx->w_begin, idx->stream));
    if (n) hipLaunchKernelGGL(widen_kernel, dim3(stream_grid(n / 4 + 1, 256)), dim3(256), 0, idx->stream, (const u32*)idx->b.sa, n,
                              static_cast<int64_t*>(out_dev));
    SA_HIP_CHECK(hipEventRecord(idx->w_end, idx->stream));
    SA_HIP_CHECK(hipGetLastError());
    idx->widen_ms = -1.0;   // resolved by sa_hip_index_build_stats
    return 0;
}

// (idx->mu held)
static int get_sa_range_locked(IndexCall& c, uint64_t first, uint64_t count, uint32_t* out_host) {
    sa_hip_index* idx = c.idx;
    if (c.has_index()) return c.rc;
    const u64 n_idx = sa_hip_index_n(idx);
    if (first > n_idx || count > n_idx - first) return fail(SA_HIP_EINVAL, c.who, "out of range");
    if (!out_host && count) return fail(SA_HIP_EINVAL, c.who, "NULL output");
    if (idx->host) { if (count) memcpy(out_host, idx->host->sa.data() + first, (size_t)count * 4); return 0; }
    return copy_to_host(c, out_host, idx->b.sa + first, (size_t)count * 4);
}

int sa_hip_index_get_sa_range(sa_hip_index* idx, uint64_t first, uint64_t count, uint32_t* out_host) {
    IndexCall c(idx, "sa_hip_index_get_sa_range");
    if (c.lock()) return c.rc;
    return get_sa_range_locked(c, first, count, out_host);
}

int sa_hip_index_get_freq(sa_hip_index* idx, uint64_t* freq256) {
    if (!idx || !freq256) return fail(SA_HIP_EINVAL, "sa_hip_index_get_freq: NULL argument");
    memcpy(freq256, idx->host ? idx->host->freq : idx->b.freq, sizeof idx->b.freq);
    return 0;
}

int sa_hip_query_batch(sa_hip_index* idx, const uint8_t* patterns, const uint64_t* offsets, uint64_t Q,
                       sa_hip_pair_u32* out) {
    IndexCall c(idx, "sa_hip_query_batch");
    if (c.lock() || c.has_index()) return c.rc;
    if (Q == 0) return 0;
    if (!offsets || !out) return fail(SA_HIP_EINVAL, c.who, "NULL argument");
    const u64 total = offsets[Q];
    if (!patterns && total) return fail(SA_HIP_EINVAL, c.who, "NULL patterns");
    if (idx->host) {
        for (u64 i = 0; i < Q; ++i) out[i] = idx->host->query(patterns + offsets[i], offsets[i + 1] - offsets[i]);
        return 0;
    }
    int rc;
    if (c.current()) return c.rc;
    // a small batch (a handful of patterns: what a caller of the single-query interfaces sends) goes through the mapped pinned block
    // -- no staged copies, one launch, one synchronisation: 55 -> ~28 us for one pattern
    if (Q <= QueryBlock::SMALL_Q && total <= QueryBlock::SMALL_BYTES) {
        if ((rc = query_block(idx))) return rc;
        const QueryBlock &h = idx->qh_host, &d = idx->qh_dev;
        memcpy(h.sb_off(), offsets, (size_t)(Q + 1) * 8);
        if (total) memcpy(h.sb_pat(), patterns, (size_t)total);
        memset(h.sb_pat() + total, 0, 64);
        if ((rc = launch_query(idx, d.sb_pat(), d.sb_off(), Q, d.sb_out()))) return rc;
        SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
        memcpy(out, h.sb_out(), (size_t)Q * sizeof(sa_hip_pair_u32));
        return 0;
    }
    if ((rc = stage_batch(idx, nullptr, patterns, offsets, Q))) return rc;
    if ((rc = launch_query(idx, idx->q_pat.as<u8>(), idx->q_off.as<u64>(), Q, idx->q_out.as<sa_hip_pair_u32>()))) return rc;
    SA_HIP_CHECK(hipMemcpyAsync(out, idx->q_out.p, (size_t)Q * sizeof(sa_hip_pair_u32), hipMemcpyDeviceToHost, idx->stream));
    SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
    return 0;
}

// (idx->mu held)
static int query_hits_locked(sa_hip_index* idx, const uint8_t* pattern, uint64_t len, uint32_t max_hits,
                             sa_hip_pair_u32* range, uint32_t* hits, uint32_t* nhits) {
    IndexCall c(idx, "sa_hip_index_query_hits");
    int rc;
    if (!range || !nhits || (!pattern && len) || (!hits && max_hits)) return fail(SA_HIP_EINVAL, c.who, "NULL argument");
    if ((rc = one_pattern_fits(c.who, len))) return rc;
    if (max_hits > QueryBlock::MAX_HITS) max_hits = QueryBlock::MAX_HITS;
    if (c.has_index()) return c.rc;
    if (idx->host) {
        const HostIndex& h = *idx->host;
        *range = h.query(pattern, len);
        const u32 count = std::min(hits_of_range(*range), max_hits);
        for (u32 i = 0; i < count; ++i) hits[i] = h.sa[(u64)range->first + i];
        *nhits = count;
        return 0;
    }
    if (c.current() || (c.rc = stage_one_pattern(idx, pattern, len))) return c.rc;
    const QueryBlock &h = idx->qh_host, &d = idx->qh_dev;
    if (idx->b.sector_search == 2) {   // the product configuration: one launch
        const QueryArgs qa = one_pattern_args(idx);
        if (qa.keys32) hipLaunchKernelGGL(query_hits_one_kernel<true>, dim3(1), dim3(256), 0, idx->stream, qa, idx->b.qmap, (const u32*)idx->b.sa,
                                          max_hits, d.hits(), d.nhits());
        else hipLaunchKernelGGL(query_hits_one_kernel<false>, dim3(1), dim3(256), 0, idx->stream, qa, idx->b.qmap, (const u32*)idx->b.sa,
                                max_hits, d.hits(), d.nhits());
    } else {
        if ((rc = launch_query(idx, d.pattern(), d.offsets(), 1, d.range()))) return rc;
        hipLaunchKernelGGL(hits_copy_kernel, dim3(1), dim3(256), 0, idx->stream, (const u32*)idx->b.sa, (const sa_hip_pair_u32*)d.range(), max_hits,
                           d.hits(), d.nhits());
    }
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
    *range = *h.range();
    *nhits = *h.nhits();
    if (*nhits) memcpy(hits, h.hits(), (size_t)*nhits * 4);
    return 0;
}

int sa_hip_index_query_hits(sa_hip_index* idx, const uint8_t* pattern, uint64_t len, uint32_t max_hits,
                            sa_hip_pair_u32* range, uint32_t* hits, uint32_t* nhits) {
    IndexCall c(idx, "sa_hip_index_query_hits");
    if (c.lock()) return c.rc;
    return query_hits_locked(idx, pattern, len, max_hits, range, hits, nhits);
}

int sa_hip_query_batch_device(sa_hip_index* idx, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                              void* out_dev) {
    IndexCall c(idx, "sa_hip_query_batch_device");
    if (c.lock() || c.device_form() || c.has_index()) return c.rc;
    if (Q == 0) return 0;
    if (!patterns_dev || !offsets_dev || !out_dev) return fail(SA_HIP_EINVAL, c.who, "NULL argument");
    if (c.current()) return c.rc;
    return launch_query(idx, (const u8*)patterns_dev, (const u64*)offsets_dev, Q, (sa_hip_pair_u32*)out_dev);
}

int sa_hip_query_batch_device_fixed(sa_hip_index* idx, const void* patterns_dev, uint64_t pattern_len, uint64_t Q, void* out_dev) {
    IndexCall c(idx, "sa_hip_query_batch_device_fixed");
    if (c.lock() || c.device_form() || c.has_index()) return c.rc;
    if (Q == 0) return 0;
    if ((!patterns_dev && pattern_len) || !out_dev) return fail(SA_HIP_EINVAL, c.who, "NULL argument");
    if (c.current()) return c.rc;
    return launch_query(idx, (const u8*)patterns_dev, nullptr, Q, (sa_hip_pair_u32*)out_dev, pattern_len);
}

int sa_hip_index_build_stats(const sa_hip_index* idx_c, sa_hip_build_stats* out) {
    sa_hip_index* idx = const_cast<sa_hip_index*>(idx_c);
    IndexCall c(idx, "sa_hip_index_build_stats");
    if (c.lock("NULL argument", out)) return c.rc;
    if (idx->host) { memset(out, 0, sizeof *out); out->n = idx->host->n; return 0; }
    if (idx->widen_ms < 0.0) {
        if (c.current()) return c.rc;
        SA_HIP_CHECK(hipEventSynchronize(idx->w_end));
        float ms = 0.f;
        SA_HIP_CHECK(hipEventElapsedTime(&ms, idx->w_begin, idx->w_end));
        idx->widen_ms = ms;
    }
    *out = idx->b.stats;
    out->widen_ms = idx->widen_ms;
    return 0;
}

int sa_hip_index_query_stats(const sa_hip_index* idx_c, sa_hip_query_stats* out) {
    sa_hip_index* idx = const_cast<sa_hip_index*>(idx_c);
    IndexCall c(idx, "sa_hip_index_query_stats");
    if (c.lock("NULL argument", out)) return c.rc;
    if (idx->host) { memset(out, 0, sizeof *out); return 0; }
    if (c.current() || (c.rc = resolve_query_events(idx, sa_hip_index::QRING))) return c.rc;
    idx->qstats.kernel_ms = idx->q_last_ms;
    idx->qstats.kernel_ms_sum = idx->q_sum_ms;
    idx->qstats.launches = idx->q_launches;
    *out = idx->qstats;
    idx->q_sum_ms = 0.0;
    idx->q_launches = 0;
    return 0;
}

// ---- record retrieval (engine.c:920-999, 1168-1215, 1326-1390; pyx:87-101) -----------------------

static int set_rows_locked_tail(sa_hip_index* idx);

// the row table of the library's own CSV extractor: a malloc'ed array that is ascending by construction -- adopted, not copied
static int set_rows_adopt(sa_hip_index* idx, uint64_t* malloced_starts, uint64_t num_rows) {
    std::lock_guard<std::mutex> g(idx->mu);
    idx->row_starts.adopt(malloced_starts, (size_t)num_rows);
    return set_rows_locked_tail(idx);
}

int sa_hip_index_set_rows(sa_hip_index* idx, const uint64_t* row_text_starts, uint64_t num_rows) {
    if (!idx || (!row_text_starts && num_rows)) return fail(SA_HIP_EINVAL, "sa_hip_index_set_rows: NULL argument");
    if (num_rows && row_text_starts[0] != 0) return fail(SA_HIP_EINVAL, "sa_hip_index_set_rows: the first row must start at offset 0");
    for (uint64_t r = 1; r < num_rows; ++r)
        if (row_text_starts[r] < row_text_starts[r - 1]) return fail(SA_HIP_EINVAL, "sa_hip_index_set_rows: offsets must ascend");
    std::lock_guard<std::mutex> g(idx->mu);
    try { idx->row_starts.assign(row_text_starts, row_text_starts + num_rows); }
    catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, "sa_hip_index_set_rows: out of host memory"); }
    return set_rows_locked_tail(idx);
}

static int set_rows_locked_tail(sa_hip_index* idx) {   // (idx->mu held) the table in HBM for the rows kernel
    const u64* row_text_starts = idx->row_starts.data();
    const u64 num_rows = idx->row_starts.size();
    if (idx->host) return 0;
    // ... and in HBM for the rows kernel
    int rc = set_device(idx->device);
    if (rc) return rc;
    if ((rc = idx->rows_dev.ensure((size_t)(num_rows ? num_rows : 1) * 8))) return rc;
    if (num_rows) SA_HIP_CHECK(hipMemcpyAsync(idx->rows_dev.p, row_text_starts, (size_t)num_rows * 8, hipMemcpyHostToDevice, idx->stream));
    // every 256th start as a table of its own: the rows kernel's search runs through it first
    std::vector<u64> coarse;
    try {
        for (u64 r = 0; r < num_rows; r += (1ull << ROWS_COARSE_SHIFT)) coarse.push_back(row_text_starts[r]);
    } catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, "sa_hip_index_set_rows: out of host memory"); }
    idx->rows_coarse_n = coarse.size();
    if ((rc = idx->rows_coarse.ensure((coarse.size() ? coarse.size() : 1) * 8))) return rc;
    if (!coarse.empty()) SA_HIP_CHECK(hipMemcpyAsync(idx->rows_coarse.p, coarse.data(), coarse.size() * 8, hipMemcpyHostToDevice, idx->stream));
    SA_HIP_CHECK(hipStreamSynchronize(idx->stream));   // (the staging vector lives until here)
    return 0;
}

int sa_hip_index_get_text(sa_hip_index* idx, uint8_t* out_host) {
    IndexCall c(idx, "sa_hip_index_get_text");
    if (c.lock() || c.has_index()) return c.rc;
    if (!out_host && sa_hip_index_n(idx)) return fail(SA_HIP_EINVAL, c.who, "NULL output");
    if (idx->host) { if (idx->host->n) memcpy(out_host, idx->host->text.data(), (size_t)idx->host->n); return 0; }
    return copy_to_host(c, out_host, idx->b.text.p, (size_t)idx->b.n);
}

// The record retrieval's switches (under SA_HIP_DIAG=1 only), read once at the top of every call.  SA_HIP_HOST_ROWS=1 sends every
// k through the host path (records.hpp), which otherwise serves k beyond ROWS_K_MAX ("all rows"): the tests compare the two paths
// row for row.  (The per-call form reads only that one.)
static bool host_rows_forced() {
    const char* e = diag_env("SA_HIP_HOST_ROWS");
    return e && atoi(e) != 0;
}
struct RowsSwitches {
    static bool is(const char* e, char c) { return e && e[0] == c; }
    static u32 groups(const char* e) { const int v = e ? atoi(e) : 0; return v >= 1 && v <= 256 ? (u32)v : 8u; }
    const bool host_rows = host_rows_forced();
    const bool waves = !is(diag_env("SA_HIP_ROWS_WAVES"), '0');           // =0: no wave-per-range form (A/B, tests)
    const u32 wave_groups = groups(diag_env("SA_HIP_ROWS_WAVE_GROUPS"));  // workgroups of the wave form per CU (A/B)
    const bool lanes = !is(diag_env("SA_HIP_ROWS_LANES"), '0');           // =0: every query through the workgroup form (A/B, tests)
    const bool trace = is(diag_env("SA_HIP_ROWS_TRACE"), '1');            // =1: one stderr line per large batch, where its time went
    const bool ring = !is(diag_env("SA_HIP_ROWS_RING"), '0');             // =0: every batch down by plain copies (A/B, tests)
};

// rows need the table of sa_hip_index_set_rows; more rows than it holds cannot come back (k = 10^9, "all", must not size anything)
static int rows_table(const sa_hip_index* idx, const char* who, u32* k) {
    if (*k && idx->row_starts.empty()) return fail(SA_HIP_EINVAL, who, "no row table (sa_hip_index_set_rows)");
    if ((u64)*k > idx->row_starts.size()) *k = (u32)idx->row_starts.size();
    return 0;
}

static RowsArgs rows_args(const sa_hip_index* idx, const sa_hip_pair_u32* ranges, u64 q, u32 k, u32* out_rows, u32* out_counts) {
    RowsArgs a;
    a.sa = idx->b.sa; a.ranges = ranges; a.q = q;
    a.row_starts = idx->rows_dev.as<u64>(); a.num_rows = idx->row_starts.size(); a.k = k;
    a.coarse = (idx->rows_coarse_n > 1) ? idx->rows_coarse.as<u64>() : nullptr; a.coarse_n = idx->rows_coarse_n;
    a.out_rows = out_rows; a.out_counts = out_counts;
    return a;
}

// (idx->mu held) the distinct rows of a range on the host (records.hpp), the hits beyond first_hits fetched slab by slab
static int host_rows_of_range(sa_hip_index* idx, const char* who, sa_hip_pair_u32 range, u32 k, const u32* first_hits, u32 n_first,
                              uint64_t* row_ids, uint32_t* count) {
    IndexCall sa_of(idx, "sa_hip_index_get_sa_range");
    try {
        std::vector<u64> rows;
        const int rc = distinct_rows(idx->row_starts, range, k, first_hits, n_first,
                                     [&](u64 pos, u64 n, u32* out) { return get_sa_range_locked(sa_of, pos, n, out); }, rows);
        if (rc) return rc;
        for (size_t i = 0; i < rows.size(); ++i) row_ids[i] = rows[i];
        *count = (uint32_t)rows.size();
    } catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, who, "out of host memory"); }
    return 0;
}

// (idx->mu held) ONE query: search + rows kernel through the pinned block, one synchronisation
static int query_rows_device_locked(sa_hip_index* idx, const uint8_t* pattern, uint64_t len, uint32_t k, uint64_t* row_ids,
                                    uint32_t* num_rows, sa_hip_pair_u32* range) {
    IndexCall c(idx, "sa_hip_index_query_rows");
    if ((c.rc = one_pattern_fits(c.who, len)) || c.has_index() || c.current() || (c.rc = stage_one_pattern(idx, pattern, len))) return c.rc;
    const QueryBlock &h = idx->qh_host, &d = idx->qh_dev;
    const RowsArgs a = rows_args(idx, d.range(), 1, k, d.hits(), d.nhits());
    if (idx->b.sector_search == 2 && k <= ROWS_K_SMALL) {
        // the product configuration: search + rows in ONE launch (no events: this path is not part of the query statistics)
        const QueryArgs qa = one_pattern_args(idx);
        if (qa.keys32) hipLaunchKernelGGL((query_rows_one_kernel<true, ROWS_SLOTS_SMALL>), dim3(1), dim3(256), 0, idx->stream, qa, idx->b.qmap, a);
        else hipLaunchKernelGGL((query_rows_one_kernel<false, ROWS_SLOTS_SMALL>), dim3(1), dim3(256), 0, idx->stream, qa, idx->b.qmap, a);
    } else {
        if (int rc = launch_query(idx, d.pattern(), d.offsets(), 1, d.range())) return rc;
        launch_rows(idx->stream, a);
    }
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
    if (range) *range = *h.range();
    const u32 n = *h.nhits();
    for (u32 i = 0; i < n; ++i) row_ids[i] = h.hits()[i];
    *num_rows = n;
    return 0;
}

int sa_hip_index_query_rows(sa_hip_index* idx, const uint8_t* pattern, uint64_t len, uint32_t k, uint64_t* row_ids,
                            uint32_t* num_rows, sa_hip_pair_u32* range) {
    IndexCall c(idx, "sa_hip_index_query_rows");
    if (!idx || !num_rows || (!row_ids && k) || (!pattern && len)) return fail(SA_HIP_EINVAL, c.who, "NULL argument");
    *num_rows = 0;
    c.lock();   // the search, the slabs of hits and the row table under ONE acquisition
    if ((c.rc = rows_table(idx, c.who, &k))) return c.rc;
    if (k && k <= ROWS_K_MAX && !host_rows_forced() && !idx->host) return query_rows_device_locked(idx, pattern, len, k, row_ids, num_rows, range);
    const u32 cap = k ? std::min<u32>(std::max<u32>(4u * k, 1024u), QueryBlock::MAX_HITS) : 0u;
    sa_hip_pair_u32 rg;
    u32 nh = 0;
    try {
        std::vector<u32> first(cap ? cap : 1);
        if ((c.rc = query_hits_locked(idx, pattern, len, cap, &rg, first.data(), &nh))) return c.rc;
        if (range) *range = rg;
        return host_rows_of_range(idx, c.who, rg, k, first.data(), nh, row_ids, num_rows);
    } catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, c.who, "out of host memory"); }
}

// ---- the batched form: one search launch for all the ranges, one rows launch for all the hits -> rows ------------------------
// A large batch moves its host legs through the process's ring of pinned slabs (host_io.hpp): patterns and offsets up, counts,
// ranges and the Q x k row ids down as u32, widened into the caller's uint64[Q][k] by the ring's worker threads while the
// next slabs arrive -- instead of one pageable copy into a Q x k vector (allocated and page-faulted per call) and one
// thread widening it (1e7 patterns, k = 16: 353 -> see profiles/r04_n_rows_batch.log).  Same bytes, same results.
// (batches whose Q x k row ids take less than this go down by one plain copy)
static constexpr size_t ROWS_RING_MIN_BYTES = 32u << 20;

struct RowsBatch {   // the caller's arrays; k clamped to the row table, k_in the stride of row_ids
    u64 Q; u32 k, k_in;
    uint64_t* row_ids; uint32_t* counts; sa_hip_pair_u32* ranges;
};

// where the time of a batch through the ring went, lap by lap, for its trace line (SA_HIP_ROWS_TRACE=1)
struct RowsTrace {
    const bool on;
    Clock::time_point mark = Clock::now();
    double up = 0, kern = 0, small = 0, rows = 0;
    void lap(double& ms) { if (on) { ms += ms_since(mark); mark = Clock::now(); } }
};

// the ring for this batch, held under g_oneshot.mu through `lock`; nullptr: the plain copies
static int rows_batch_ring(const sa_hip_index* idx, std::unique_lock<std::mutex>& lock, PinnedRing** ring) {
    lock = std::unique_lock<std::mutex>(g_oneshot.mu);
    if (!g_oneshot.ring.ready) { if (int rc = g_oneshot.ring.init()) return rc; }
    if (g_oneshot.ring.device == idx->device) *ring = &g_oneshot.ring;
    else lock.unlock();   // (the ring's copy stream lives on another device)
    return 0;
}

// device rows: ONE rows launch over q_out into r_rows / r_counts, no per-query synchronisation ...
static int rows_batch_launch(sa_hip_index* idx, const RowsSwitches& sw, const RowsBatch& o) {
    int rc;
    if ((rc = idx->r_rows.ensure((size_t)o.Q * o.k * 4)) || (rc = idx->r_counts.ensure((size_t)o.Q * 4))) return rc;
    const bool lanes = o.Q >= ROWS_LANE_MIN_BATCH && sw.lanes;
    if (lanes && (rc = idx->r_pending.ensure((2 * (size_t)o.Q + 2) * 4))) return rc;
    launch_rows(idx->stream, rows_args(idx, idx->q_out.as<sa_hip_pair_u32>(), o.Q, o.k, idx->r_rows.as<u32>(), idx->r_counts.as<u32>()),
                lanes ? idx->r_pending.as<u32>() : nullptr, sw.waves, sw.wave_groups);
    SA_HIP_CHECK(hipGetLastError());
    return 0;
}

// ... their download through the ring: counts and ranges, then the row ids in pieces of whole queries, widened by the workers ...
static int rows_batch_down_ring(sa_hip_index* idx, PinnedRing& ring, const RowsBatch& o, RowsTrace& t) {
    int rc;
    SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
    t.lap(t.kern);
    if ((rc = ring_download<u32>(ring, idx->device, idx->r_counts.as<u32>(), o.counts, (size_t)o.Q))) return rc;
    if (o.ranges && (rc = ring_download<u32>(ring, idx->device, idx->q_out.as<u32>(), reinterpret_cast<u32*>(o.ranges), (size_t)o.Q * 2))) return rc;
    t.lap(t.small);
    const size_t per_q = (size_t)o.k * 4;                                        // k <= ROWS_K_MAX: at most 16 KB
    // whole queries per piece; about 32 pieces (1 MB .. one slab) so that a mid-size batch still spreads over all workers
    const size_t target = std::min<size_t>(PinnedRing::SLAB_BYTES, std::max<size_t>((size_t)1 << 20, (size_t)o.Q * per_q / 32));
    const size_t piece = std::max<size_t>(per_q, (target / per_q) * per_q);
    const u32 k = o.k, k_in = o.k_in;
    const u32* counts = o.counts;
    u64* row_ids = o.row_ids;
    rc = ring_download_pieces(ring, idx->device, idx->r_rows.as<u8>(), (size_t)o.Q * per_q, piece,
                              [=](const u8* p, size_t off, size_t len) {
                                  const u32* in = reinterpret_cast<const u32*>(p);
                                  const u64 q0 = off / per_q, nq = len / per_q;
                                  for (u64 j = 0; j < nq; ++j) {
                                      const u32 c = counts[q0 + j];
                                      u64* out = row_ids + (q0 + j) * k_in;
                                      const u32* r = in + j * k;
                                      for (u32 i = 0; i < c; ++i) out[i] = r[i];
                                  }
                              });
    t.lap(t.rows);
    if (t.on) fprintf(stderr, "[sa_hip rows batch] Q=%llu k=%u: patterns+offsets up %.2f ms, search+rows kernels %.2f, counts+ranges down %.2f, row ids down+widened %.2f (pieces of %zu bytes)\n",
                      (unsigned long long)o.Q, o.k, t.up, t.kern, t.small, t.rows, piece);
    return rc;
}

// ... or by plain copies (the ranges are already on their way down)
static int rows_batch_down_plain(sa_hip_index* idx, const RowsBatch& o) {
    std::vector<u32> rows32((size_t)o.Q * o.k);
    SA_HIP_CHECK(hipMemcpyAsync(o.counts, idx->r_counts.p, (size_t)o.Q * 4, hipMemcpyDeviceToHost, idx->stream));
    SA_HIP_CHECK(hipMemcpyAsync(rows32.data(), idx->r_rows.p, (size_t)o.Q * o.k * 4, hipMemcpyDeviceToHost, idx->stream));
    SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
    for (u64 q = 0; q < o.Q; ++q)
        for (u32 i = 0; i < o.counts[q]; ++i) o.row_ids[q * o.k_in + i] = rows32[q * o.k + i];
    return 0;
}

// host rows (the host path; k beyond ROWS_K_MAX; SA_HIP_HOST_ROWS=1): every range resolved on the host
static int rows_batch_host_rows(sa_hip_index* idx, const char* who, const RowsBatch& o, const sa_hip_pair_u32* rg_host) {
    for (u64 q = 0; o.k && q < o.Q; ++q)
        if (int rc = host_rows_of_range(idx, who, rg_host[q], o.k, nullptr, 0, o.row_ids + q * o.k_in, &o.counts[q])) return rc;
    return 0;
}

int sa_hip_index_query_rows_batch(sa_hip_index* idx, const uint8_t* patterns, const uint64_t* offsets, uint64_t Q, uint32_t k,
                                  uint64_t* row_ids, uint32_t* counts, sa_hip_pair_u32* ranges) {
    IndexCall c(idx, "sa_hip_index_query_rows_batch");
    if (!idx || (Q && (!offsets || !counts || (!row_ids && k)))) return fail(SA_HIP_EINVAL, c.who, "NULL argument");
    if (Q == 0) return 0;
    const RowsSwitches sw;
    if (c.lock() || c.has_index()) return c.rc;
    if (!patterns && offsets[Q]) return fail(SA_HIP_EINVAL, c.who, "NULL patterns");
    const u32 k_in = k;
    if ((c.rc = rows_table(idx, c.who, &k))) return c.rc;
    const RowsBatch o{Q, k, k_in, row_ids, counts, ranges};
    for (u64 i = 0; i < Q; ++i) counts[i] = 0;
    try {
        std::vector<sa_hip_pair_u32> rg_host;
        if (idx->host) {   // host path: the search by the host index
            rg_host.resize(Q);
            for (u64 q = 0; q < Q; ++q) rg_host[q] = idx->host->query(patterns + offsets[q], offsets[q + 1] - offsets[q]);
            c.rc = rows_batch_host_rows(idx, c.who, o, rg_host.data());
        } else {           // stage, search, then the rows on the device (down by ring or by plain copies) or on the host
            if (c.current()) return c.rc;
            const bool device_rows = k && k <= ROWS_K_MAX && !sw.host_rows;
            std::unique_lock<std::mutex> ring_lock;
            PinnedRing* ring = nullptr;
            if (device_rows && (size_t)Q * k * 4 >= ROWS_RING_MIN_BYTES && sw.ring && (c.rc = rows_batch_ring(idx, ring_lock, &ring))) return c.rc;
            RowsTrace t{ring && sw.trace};
            if ((c.rc = stage_batch(idx, ring, patterns, offsets, Q))) return c.rc;
            t.lap(t.up);
            if ((c.rc = launch_query(idx, idx->q_pat.as<u8>(), idx->q_off.as<u64>(), Q, idx->q_out.as<sa_hip_pair_u32>()))) return c.rc;
            if (!ring && (ranges || !device_rows)) {
                rg_host.resize(Q);
                SA_HIP_CHECK(hipMemcpyAsync(rg_host.data(), idx->q_out.p, (size_t)Q * sizeof(sa_hip_pair_u32), hipMemcpyDeviceToHost, idx->stream));
            }
            if (device_rows) {
                if ((c.rc = rows_batch_launch(idx, sw, o))) return c.rc;
                if (ring) return rows_batch_down_ring(idx, *ring, o, t);
                c.rc = rows_batch_down_plain(idx, o);
            } else {
                SA_HIP_CHECK(hipStreamSynchronize(idx->stream));
                c.rc = rows_batch_host_rows(idx, c.who, o, rg_host.data());
            }
        }
        if (!c.rc && ranges) memcpy(ranges, rg_host.data(), (size_t)Q * sizeof(sa_hip_pair_u32));
    } catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, c.who, "out of host memory"); }
    return c.rc;
}

int sa_hip_index_rows_for_range(sa_hip_index* idx, sa_hip_pair_u32 range, uint32_t k, uint64_t* row_ids, uint32_t* num_rows) {
    IndexCall c(idx, "sa_hip_index_rows_for_range");
    if (!idx || !num_rows || (!row_ids && k)) return fail(SA_HIP_EINVAL, c.who, "NULL argument");
    *num_rows = 0;
    if (c.lock() || c.has_index()) return c.rc;
    if (hits_of_range(range) && ((u64)range.second >= sa_hip_index_n(idx) || range.first > range.second))
        return fail(SA_HIP_EINVAL, c.who, "range outside the suffix array");
    if ((c.rc = rows_table(idx, c.who, &k))) return c.rc;
    return host_rows_of_range(idx, c.who, range, k, nullptr, 0, row_ids, num_rows);
}

static int csv_index_finish(sa_hip_csv_index* c) {
    const int fd = open(c->path.c_str(), O_RDONLY);
    if (fd < 0) return fail(SA_HIP_EINVAL, "sa_hip_csv_index: cannot open file", c->path.c_str());
    struct stat sb;
    if (fstat(fd, &sb) != 0) { close(fd); return fail(SA_HIP_EINVAL, "sa_hip_csv_index: fstat failed", c->path.c_str()); }
    c->map_len = (u64)sb.st_size;
    if (!c->row_file_offsets.empty() && c->row_file_offsets.back() > c->map_len) { close(fd); return fail(SA_HIP_EINVAL, "sa_hip_csv_index: row table exceeds the file"); }
    void* m = c->map_len ? mmap(nullptr, c->map_len, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
    close(fd);
    if (c->map_len && m == MAP_FAILED) return fail(SA_HIP_ENOMEM, "sa_hip_csv_index: mmap failed", c->path.c_str());
    c->map = static_cast<const u8*>(m);
    return 0;
}

void sa_hip_csv_index_destroy(sa_hip_csv_index* c) {
    if (!c) return;
    if (c->map) munmap(const_cast<u8*>(c->map), c->map_len);
    if (c->idx) sa_hip_index_destroy(c->idx);
    delete c;
}

int sa_hip_csv_index_create(sa_hip_csv_index** out, const char* csv_file, const char* search_column, uint32_t max_suffix_length,
                            int device) {
    if (!out || !csv_file || !search_column) return fail(SA_HIP_EINVAL, "sa_hip_csv_index_create: NULL argument");
    *out = nullptr;
    if (max_suffix_length == 0) return fail(SA_HIP_EINVAL, "sa_hip_csv_index_create: max_suffix_length must be >= 1");
    sa_hip_csv_column col;
    // the HIP runtime of this process (context, code object: ~0.2 s the first time) comes up while the host parses
    std::thread warm;
    try { warm = std::thread([device]() { if (hipSetDevice(device) == hipSuccess) (void)hipFree(nullptr); }); } catch (...) {}
    int rc = sa_hip_csv_extract_column(csv_file, search_column, &col);
    if (warm.joinable()) warm.join();
    if (rc) return rc;
    sa_hip_csv_index* c = nullptr;
    try {
        c = new sa_hip_csv_index();
        c->path = csv_file;
        c->column_index = col.column_index;
        const char* p = col.column_names;
        for (u32 i = 0; i < col.num_columns; ++i) { c->columns.emplace_back(p); p += c->columns.back().size() + 1; }
        c->row_file_offsets.assign(col.row_file_offsets, col.row_file_offsets + col.num_rows + 1);
    } catch (const std::bad_alloc&) {
        delete c; sa_hip_csv_free(&col);
        return fail(SA_HIP_ENOMEM, "sa_hip_csv_index_create: out of host memory");
    }
    if (col.text_len > 0xFFFFFFFEull) rc = fail(SA_HIP_EINVAL, "sa_hip_csv_index_create: the column exceeds 2^32 - 2 bytes (one index per device)");
    if (!rc) rc = sa_hip_index_create(&c->idx, col.text_len ? col.text_len : 1, device);
    if (!rc) rc = sa_hip_index_build(c->idx, col.text, col.text_len, max_suffix_length);
    if (!rc) rc = sa_hip_index_set_rows(c->idx, col.row_text_starts, col.num_rows);
    sa_hip_csv_free(&col);
    if (!rc) rc = csv_index_finish(c);
    if (rc) { sa_hip_csv_index_destroy(c); return rc; }
    *out = c;
    return 0;
}

// one helper thread at a time gives large host buffers back (joined before the next one starts and when the library is unloaded:
// never detached)
namespace {
struct BackgroundFree {
    std::thread t;
    std::mutex m;
    void run(sa_hip_csv_column col) {
        std::lock_guard<std::mutex> g(m);
        if (t.joinable()) t.join();
        try { t = std::thread([col]() mutable { csv_free(&col); }); } catch (...) { csv_free(&col); }
    }
    ~BackgroundFree() { if (t.joinable()) t.join(); }
};
BackgroundFree g_bgfree;
}  // namespace

// The reference cuts a CSV file into 2 GiB partitions, one suffix array each (engine.c:1437-1481), and answers a query from
// the partitions one after the other (suffix_array.pyx:221-247).  Here one index holds up to 2^32 - 2 COLUMN bytes whatever
// the file's size; a column beyond `partition_bytes` is cut at ROW boundaries (no match is lost at a cut) into several
// independent sa_hip_csv_index objects over the same mapped file -- every entry point works on a part as on a whole index.
int sa_hip_csv_index_create_partitioned(sa_hip_csv_index*** out_parts, uint32_t* num_parts, const char* csv_file, const char* search_column,
                                        uint32_t max_suffix_length, int device, uint64_t partition_bytes) {
    if (!out_parts || !num_parts || !csv_file || !search_column) return fail(SA_HIP_EINVAL, "sa_hip_csv_index_create_partitioned: NULL argument");
    *out_parts = nullptr; *num_parts = 0;
    if (max_suffix_length == 0) return fail(SA_HIP_EINVAL, "sa_hip_csv_index_create_partitioned: max_suffix_length must be >= 1");
    if (partition_bytes == 0 || partition_bytes > 0xFFFFFFFEull) partition_bytes = 0xFFFFFFFEull;
    sa_hip_csv_column col;
    std::thread warm;
    try { warm = std::thread([device]() { if (hipSetDevice(device) == hipSuccess) (void)hipFree(nullptr); }); } catch (...) {}
    const bool timing = diag_env("SA_HIP_CSV_TIMING") && atoi(diag_env("SA_HIP_CSV_TIMING")) != 0;
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[sa_hip csv] %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
        t_prev = now;
    };
    int rc = sa_hip_csv_extract_column(csv_file, search_column, &col);
    if (warm.joinable()) warm.join();
    if (rc) return rc;
    lap("extract (all of the above)");
    // rows [cut[p], cut[p + 1]) form part p: as many whole rows as fit partition_bytes (a row's text includes its separator)
    std::vector<u64> cut;
    std::vector<sa_hip_csv_index*> parts;
    try {
        cut.push_back(0);
        u64 begin_text = 0;
        // (the usual case -- the whole column fits one index -- needs no walk over the rows)
        for (u64 r = 0; col.text_len > partition_bytes && r < col.num_rows; ++r) {
            const u64 row_end = (r + 1 < col.num_rows) ? col.row_text_starts[r + 1] : col.text_len;
            if (row_end - col.row_text_starts[r] > partition_bytes) {
                sa_hip_csv_free(&col);
                return fail(SA_HIP_EINVAL, "sa_hip_csv_index_create_partitioned: one row's column text exceeds partition_bytes");
            }
            if (row_end - begin_text > partition_bytes) { cut.push_back(r); begin_text = col.row_text_starts[r]; }
        }
        cut.push_back(col.num_rows);
        if (cut.size() == 2 && col.num_rows == 0) cut.assign({0, 0});
        for (size_t p = 0; p + 1 < cut.size() && !rc; ++p) {
            const u64 r0 = cut[p], r1 = cut[p + 1];
            const u64 t0 = (r0 < col.num_rows) ? col.row_text_starts[r0] : col.text_len;
            const u64 t1 = (r1 < col.num_rows) ? col.row_text_starts[r1] : col.text_len;
            sa_hip_csv_index* c = new sa_hip_csv_index();
            parts.push_back(c);
            c->path = csv_file;
            c->column_index = col.column_index;
            const char* q = col.column_names;
            for (u32 i = 0; i < col.num_columns; ++i) { c->columns.emplace_back(q); q += c->columns.back().size() + 1; }
            const bool whole = (r0 == 0 && r1 == col.num_rows);   // one part: the extractor's tables are adopted as they are
            std::vector<u64> starts;
            if (whole) {
                c->row_file_offsets.adopt(col.row_file_offsets, (size_t)col.num_rows + 1);
                col.row_file_offsets = nullptr;
            } else {
                c->row_file_offsets.assign(col.row_file_offsets + r0, col.row_file_offsets + r1 + 1);
                starts.resize(r1 - r0);
                for (u64 r = r0; r < r1; ++r) starts[r - r0] = col.row_text_starts[r] - t0;
            }
            const u64 len = t1 - t0;
            lap("cuts, row tables");
            rc = sa_hip_index_create(&c->idx, len ? len : 1, device);
            lap("index create (buffers)");
            if (!rc) rc = sa_hip_index_build(c->idx, col.text + t0, len, max_suffix_length);
            lap("upload + build");
            if (!rc) {
                if (whole) { u64* own = col.row_text_starts; col.row_text_starts = nullptr; rc = set_rows_adopt(c->idx, own, col.num_rows); }
                else rc = sa_hip_index_set_rows(c->idx, starts.data(), r1 - r0);
            }
            lap("row table to the device");
            if (!rc) rc = csv_index_finish(c);
            lap("file mapping");
        }
    } catch (const std::bad_alloc&) {
        rc = fail(SA_HIP_ENOMEM, "sa_hip_csv_index_create_partitioned: out of host memory");
    }
    // the extracted column (0.9 GB of touched pages at 50M rows) is given back on a thread of its own: unmapping it takes 0.2 s
    g_bgfree.run(col);
    memset(&col, 0, sizeof col);
    lap("free the extracted column");
    sa_hip_csv_index** arr = rc ? nullptr : static_cast<sa_hip_csv_index**>(malloc((parts.size() ? parts.size() : 1) * sizeof(sa_hip_csv_index*)));
    if (!rc && !arr) rc = fail(SA_HIP_ENOMEM, "sa_hip_csv_index_create_partitioned: out of host memory");
    if (rc) { for (sa_hip_csv_index* c : parts) sa_hip_csv_index_destroy(c); return rc; }
    for (size_t p = 0; p < parts.size(); ++p) arr[p] = parts[p];
    *out_parts = arr;
    *num_parts = (uint32_t)parts.size();
    return 0;
}
void sa_hip_csv_index_free_parts(sa_hip_csv_index** parts) { free(parts); }

int sa_hip_csv_index_adopt(sa_hip_csv_index** out, const char* csv_file, const uint8_t* text, const uint32_t* SA, uint64_t n,
                           const uint64_t* row_text_starts, const uint64_t* row_file_offsets, uint64_t num_rows,
                           const char* column_names, uint32_t num_columns, uint32_t column_index, uint32_t max_suffix_length, int device) {
    if (!out || !csv_file || (!text && n) || (!SA && n) || (num_rows && (!row_text_starts || !row_file_offsets)) || (!column_names && num_columns))
        return fail(SA_HIP_EINVAL, "sa_hip_csv_index_adopt: NULL argument");
    *out = nullptr;
    sa_hip_csv_index* c = nullptr;
    try {
        c = new sa_hip_csv_index();
        c->path = csv_file;
        c->column_index = column_index;
        const char* p = column_names;
        for (u32 i = 0; i < num_columns; ++i) { c->columns.emplace_back(p); p += c->columns.back().size() + 1; }
        if (num_rows) c->row_file_offsets.assign(row_file_offsets, row_file_offsets + num_rows + 1);
    } catch (const std::bad_alloc&) { delete c; return fail(SA_HIP_ENOMEM, "sa_hip_csv_index_adopt: out of host memory"); }
    // the tables come from a file: a row is copied out of the mapping by [row_file_offsets[r], row_file_offsets[r + 1]) and found
    // by row_text_starts -- both must ascend and stay inside what they index (csv_index_finish checks the last offset
    // against the file's size)
    for (u64 r = 0; r < num_rows; ++r) {
        if (row_file_offsets[r] > row_file_offsets[r + 1]) { delete c; return fail(SA_HIP_EINVAL, "sa_hip_csv_index_adopt: row_file_offsets must ascend"); }
        if (row_text_starts[r] > n) { delete c; return fail(SA_HIP_EINVAL, "sa_hip_csv_index_adopt: row_text_starts beyond the text"); }
    }
    if (column_index >= num_columns && num_columns) { delete c; return fail(SA_HIP_EINVAL, "sa_hip_csv_index_adopt: column_index out of range"); }
    int rc = sa_hip_index_create(&c->idx, n ? n : 1, device);
    if (!rc) rc = sa_hip_index_load(c->idx, text, SA, n, max_suffix_length);
    if (!rc) rc = sa_hip_index_set_rows(c->idx, row_text_starts, num_rows);
    if (!rc) rc = csv_index_finish(c);
    if (rc) { sa_hip_csv_index_destroy(c); return rc; }
    *out = c;
    return 0;
}

sa_hip_index* sa_hip_csv_index_handle(sa_hip_csv_index* c) { return c ? c->idx : nullptr; }
uint64_t sa_hip_csv_index_num_rows(const sa_hip_csv_index* c) { return (c && !c->row_file_offsets.empty()) ? c->row_file_offsets.size() - 1 : 0; }
uint32_t sa_hip_csv_index_num_columns(const sa_hip_csv_index* c) { return c ? (uint32_t)c->columns.size() : 0; }
uint32_t sa_hip_csv_index_column_index(const sa_hip_csv_index* c) { return c ? c->column_index : 0; }
const char* sa_hip_csv_index_column_name(const sa_hip_csv_index* c, uint32_t i) { return (c && i < c->columns.size()) ? c->columns[i].c_str() : nullptr; }
int sa_hip_csv_index_row_tables(const sa_hip_csv_index* c, const uint64_t** row_text_starts, const uint64_t** row_file_offsets) {
    if (!c || !c->idx) return fail(SA_HIP_EINVAL, "sa_hip_csv_index_row_tables: NULL index");
    if (row_text_starts) *row_text_starts = c->idx->row_starts.data();
    if (row_file_offsets) *row_file_offsets = c->row_file_offsets.data();
    return 0;
}

int sa_hip_csv_index_copy_rows(sa_hip_csv_index* c, const uint64_t* row_ids, uint32_t n, char** records) {
    if (!c || (n && (!row_ids || !records))) return fail(SA_HIP_EINVAL, "sa_hip_csv_index_copy_rows: NULL argument");
    const u64 rows = sa_hip_csv_index_num_rows(c);
    for (u32 i = 0; i < n; ++i) records[i] = nullptr;
    for (u32 i = 0; i < n; ++i) {
        if (row_ids[i] >= rows) { sa_hip_free_records(records, i); return fail(SA_HIP_EINVAL, "sa_hip_csv_index_copy_rows: no such row"); }
        records[i] = dup_row(c->map, c->row_file_offsets[row_ids[i]], c->row_file_offsets[row_ids[i] + 1]);
        if (!records[i]) { sa_hip_free_records(records, i); return fail(SA_HIP_ENOMEM, "sa_hip_csv_index_copy_rows: out of host memory"); }
    }
    return 0;
}

sa_hip_pair_u32 sa_hip_get_substring_positions_file(sa_hip_csv_index* c, const char* substring) {
    sa_hip_pair_u32 r = {0xFFFFFFFFu, 0xFFFFFFFFu};
    if (!c || !c->idx || !substring) { fail(SA_HIP_EINVAL, "sa_hip_get_substring_positions_file: NULL argument"); return r; }
    u32 nh = 0;
    sa_hip_pair_u32 q;
    if (sa_hip_index_query_hits(c->idx, reinterpret_cast<const uint8_t*>(substring), strlen(substring), 0, &q, nullptr, &nh)) return r;
    // engine.c:962-965: start / end are only ever set on an exact match, so ANY miss is {UINT32_MAX, UINT32_MAX}
    if (hits_of_range(q) == 0) return r;
    return q;
}

int sa_hip_get_matching_records_file(sa_hip_csv_index* c, const char* substring, uint32_t k, char** matching_records,
                                     uint32_t* num_matches) {
    if (!c || !c->idx || !substring || !num_matches || (!matching_records && k)) return fail(SA_HIP_EINVAL, "sa_hip_get_matching_records_file: NULL argument");
    if (*num_matches >= k) return 0;   // engine.c:1356: at most k - *num_matches more
    // never more than the file has rows: k = 10^9 ("all") must not size a 8 GB table
    const u32 want = (u32)std::min<u64>(k - *num_matches, sa_hip_csv_index_num_rows(c));
    if (want == 0) return 0;
    try {
        std::vector<u64> rows((size_t)want);
        u32 n = 0;
        int rc = sa_hip_index_query_rows(c->idx, reinterpret_cast<const uint8_t*>(substring), strlen(substring), want, rows.data(), &n, nullptr);
        if (rc) return rc;
        for (u32 i = 0; i < n; ++i) {
            const u64 r = rows[i];
            char* s = dup_row(c->map, c->row_file_offsets[r], c->row_file_offsets[r + 1]);
            if (!s) return fail(SA_HIP_ENOMEM, "sa_hip_get_matching_records_file: out of host memory");
            matching_records[(*num_matches)++] = s;
        }
    } catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, "sa_hip_get_matching_records_file: out of host memory"); }
    return 0;
}

int sa_hip_get_matching_row_spans_file(sa_hip_csv_index* c, const char* substring, uint32_t k, const char** row_ptrs,
                                       uint32_t* row_lens, uint32_t* num_matches) {
    if (!c || !c->idx || !substring || !num_matches || (k && (!row_ptrs || !row_lens))) return fail(SA_HIP_EINVAL, "sa_hip_get_matching_row_spans_file: NULL argument");
    *num_matches = 0;
    const u32 want = (u32)std::min<u64>(k, sa_hip_csv_index_num_rows(c));
    if (want == 0) return 0;
    try {
        std::vector<u64> rows((size_t)want);
        u32 n = 0;
        int rc = sa_hip_index_query_rows(c->idx, reinterpret_cast<const uint8_t*>(substring), strlen(substring), want, rows.data(), &n, nullptr);
        if (rc) return rc;
        for (u32 i = 0; i < n; ++i) {
            const u64 r = rows[i];
            u64 b = c->row_file_offsets[r], e = c->row_file_offsets[r + 1];
            while (e > b && (c->map[e - 1] == '\n' || c->map[e - 1] == '\r')) --e;
            row_ptrs[i] = reinterpret_cast<const char*>(c->map + b);
            row_lens[i] = (u32)std::min<u64>(e - b, 0xFFFFFFFFull);
        }
        *num_matches = n;
    } catch (const std::bad_alloc&) { return fail(SA_HIP_ENOMEM, "sa_hip_get_matching_row_spans_file: out of host memory"); }
    return 0;
}

uint32_t sa_hip_get_matching_records(const char* str, const sa_hip_SuffixArray_struct* s, const char* substring, uint32_t k,
                                     char** matching_records) {
    if (!str || !s || !substring || (!matching_records && k) || (!s->suffix_array && s->n)) { fail(SA_HIP_EINVAL, "sa_hip_get_matching_records: NULL argument"); return 0; }
    const sa_hip_pair_u32 rg = sa_hip_get_substring_positions(str, s, substring);
    if (hits_of_range(rg) == 0) return 0;   // engine.c:1181-1185
    const u64 n = s->n;
    u32 made = 0;
    try {
        std::unordered_set<u64> seen;
        for (u64 i = rg.first; i <= (u64)rg.second && made < k; ++i) {
            const u64 p = s->suffix_array[i];
            // the record = the text between the newlines around the hit (what engine.c:1187-1211 means to copy)
            u64 b = p, e = p;
            while (b > 0 && str[b - 1] != '\n') --b;
            while (e < n && str[e] != '\n') ++e;
            if (!seen.insert(b).second) continue;
            char* r = static_cast<char*>(malloc((size_t)(e - b) + 1));
            if (!r) { fail(SA_HIP_ENOMEM, "sa_hip_get_matching_records: out of host memory"); return made; }
            memcpy(r, str + b, (size_t)(e - b));
            r[e - b] = '\0';
            matching_records[made++] = r;
        }
    } catch (const std::bad_alloc&) { fail(SA_HIP_ENOMEM, "sa_hip_get_matching_records: out of host memory"); }
    return made;
}

void sa_hip_free_records(char** records, uint32_t n) {
    if (!records) return;
    for (uint32_t i = 0; i < n; ++i) { free(records[i]); records[i] = nullptr; }
}

// ---- lifecycle mirrors of the seam (engine.c:326-349; pyx:68-74) -------------------------------------------------------

int sa_hip_init_suffix_array_byte_idxs(sa_hip_SuffixArray_struct* s, uint32_t max_suffix_length, uint64_t global_byte_start_idx,
                                       uint64_t global_byte_end_idx, uint32_t n) {
    if (!s) return fail(SA_HIP_EINVAL, "sa_hip_init_suffix_array_byte_idxs: NULL argument");
    s->max_suffix_length = max_suffix_length;
    s->n = n;
    s->suffix_array = static_cast<uint32_t*>(malloc((size_t)(n ? n : 1) * sizeof(uint32_t)));
    s->is_quoted_bitflag = nullptr;   // the row table of sa_hip_csv_index replaces the reference's per-character quoted bits
    s->global_byte_start_idx = global_byte_start_idx;
    s->global_byte_end_idx = global_byte_end_idx;
    if (!s->suffix_array) return fail(SA_HIP_ENOMEM, "sa_hip_init_suffix_array_byte_idxs: out of host memory");
    return 0;
}

void sa_hip_free_suffix_array(sa_hip_SuffixArray_struct* s) {
    if (!s) return;
    free(s->suffix_array);
    s->suffix_array = nullptr;
}

// ---- the reference's on-disk layout (engine.c:1098-1165) ----------------------------------------------------------------

int sa_hip_write_suffix_array(const sa_hip_SuffixArray_struct* s, const char* sa_filename, const char* is_quoted_filename) {
    if (!s || !sa_filename || (!s->suffix_array && s->n)) return fail(SA_HIP_EINVAL, "sa_hip_write_suffix_array: NULL argument");
    FILE* f = fopen(sa_filename, "wb");
    if (!f) return fail(SA_HIP_EINVAL, "sa_hip_write_suffix_array: cannot open file", sa_filename);
    // engine.c:1123-1128: {u64 global_byte_start_idx, u64 global_byte_end_idx, u32 max_suffix_length, u32 n, u32 suffix_array[n]}
    bool ok = fwrite(&s->global_byte_start_idx, 8, 1, f) == 1 && fwrite(&s->global_byte_end_idx, 8, 1, f) == 1 &&
              fwrite(&s->max_suffix_length, 4, 1, f) == 1 && fwrite(&s->n, 4, 1, f) == 1 &&
              (s->n == 0 || fwrite(s->suffix_array, 4, s->n, f) == s->n);
    ok = (fclose(f) == 0) && ok;
    if (!ok) return fail(SA_HIP_EINVAL, "sa_hip_write_suffix_array: short write", sa_filename);
    if (is_quoted_filename) {
        // engine.c:1098-1101 write_buffer_bit: {u32 capacity, bytes}; this library keeps no quoted bits (sa_hip.h): capacity 0
        FILE* q = fopen(is_quoted_filename, "wb");
        if (!q) return fail(SA_HIP_EINVAL, "sa_hip_write_suffix_array: cannot open file", is_quoted_filename);
        const uint32_t cap = 0;
        ok = fwrite(&cap, 4, 1, q) == 1;
        ok = (fclose(q) == 0) && ok;
        if (!ok) return fail(SA_HIP_EINVAL, "sa_hip_write_suffix_array: short write", is_quoted_filename);
    }
    return 0;
}

int sa_hip_read_suffix_array(sa_hip_SuffixArray_struct* s, const char* sa_filename) {
    if (!s || !sa_filename) return fail(SA_HIP_EINVAL, "sa_hip_read_suffix_array: NULL argument");
    memset(s, 0, sizeof *s);
    FILE* f = fopen(sa_filename, "rb");
    if (!f) return fail(SA_HIP_EINVAL, "sa_hip_read_suffix_array: cannot open file", sa_filename);
    int rc = 0;
    if (fread(&s->global_byte_start_idx, 8, 1, f) != 1 || fread(&s->global_byte_end_idx, 8, 1, f) != 1 ||
        fread(&s->max_suffix_length, 4, 1, f) != 1 || fread(&s->n, 4, 1, f) != 1)
        rc = fail(SA_HIP_EINVAL, "sa_hip_read_suffix_array: truncated header", sa_filename);
    if (!rc) {
        s->suffix_array = static_cast<uint32_t*>(malloc((size_t)(s->n ? s->n : 1) * 4));
        if (!s->suffix_array) rc = fail(SA_HIP_ENOMEM, "sa_hip_read_suffix_array: out of host memory");
        else if (s->n && fread(s->suffix_array, 4, s->n, f) != s->n) rc = fail(SA_HIP_EINVAL, "sa_hip_read_suffix_array: truncated array", sa_filename);
        if (!rc) for (uint32_t i = 0; i < s->n; ++i) if (s->suffix_array[i] >= s->n) { rc = fail(SA_HIP_EINVAL, "sa_hip_read_suffix_array: entry >= n", sa_filename); break; }
    }
    fclose(f);
    if (rc) { free(s->suffix_array); memset(s, 0, sizeof *s); }
    return rc;
}

}  // extern "C"

// The token index (batched n-gram ranges over an int32 text): a handle and kernels of its own
#include "capi_token.hpp"
#include "capi_token_docs.hpp"
#include "capi_token_all.hpp"
#include "capi_token_cnf.hpp"
#include "capi_token_match.hpp"
#include "capi_token_score.hpp"
#include "capi_token_top.hpp"
#include "capi_token_shards.hpp"
#include "capi_token_shard_top.hpp"
#include "capi_token_shard_match.hpp"
#include "capi_token_shard_score.hpp"
#include "capi_token_shard_docs.hpp"
#include "capi_token_shard_all.hpp"
