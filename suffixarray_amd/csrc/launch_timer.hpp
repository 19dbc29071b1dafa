// launch_timer.hpp -- the stopwatches of a handle's stream (capi_token*.hpp), resolved when an *_info call asks for the figures.
// LaunchTimer: one kind of launch, an event either side of the last one.  ChunkTimer: a call that runs in chunks of several stages
// (the next symbols, documents and AND groups of a shard set), every stage summed over the chunks of the last call.
// The caller has set the device and holds the handle's mutex.
#pragma once
#include "common.hpp"
#include <vector>

namespace sa {

struct LaunchTimer {
    hipEvent_t ev[2] = {};
    bool pending = false;   // recorded, not yet resolved
    double ms = 0.0;
    u64 q = 0;              // what the last launch answered (contexts, spans, groups)

    hipError_t create() {   // (the handle's constructor words the failure)
        hipError_t e = hipEventCreate(&ev[0]);
        return e == hipSuccess ? hipEventCreate(&ev[1]) : e;
    }
    void destroy() {        // (also of a timer whose create never ran, or failed half-way)
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
    int begin(hipStream_t stream) {
        SA_HIP_CHECK(hipEventRecord(ev[0], stream));
        return 0;
    }
    // behind the launch; after a launch that failed it is not called, and pending, q and ms stay as they were
    int end(hipStream_t stream, u64 Q) {
        SA_HIP_CHECK(hipEventRecord(ev[1], stream));
        pending = true;
        q = Q;
        return 0;
    }
    int resolve() {
        if (!pending) return 0;
        float f = 0.f;
        SA_HIP_CHECK(hipEventSynchronize(ev[1]));
        SA_HIP_CHECK(hipEventElapsedTime(&f, ev[0], ev[1]));
        ms = f;
        pending = false;
        return 0;
    }
};

// STAGES + 1 events per chunk: in front of the first stage, behind every stage.  The events are created on demand and reused by the
// next call; only chunks whose events are all recorded are published, so after a call that failed midway the chunks it completed
// are what resolve() sums.  A new call clears what the last one published, since it records over the same events; when it fails
// before its first chunk is published, ms keeps what was last resolved while q and chunk are those of the last call that ran to its
// end, and whatever else the owner reset for the new call (the streamed-ranks counter of a shard set) no longer belongs to them.
template <u32 STAGES>
struct ChunkTimer {
    std::vector<hipEvent_t> ev;
    size_t next = 0;        // the event the next mark() records
    size_t used = 0;        // events of the published chunks of the last call
    bool pending = false;   // published, not yet resolved
    double ms[STAGES] = {};
    u64 q = 0;              // what the last call that ran to its end answered (contexts, groups), and in chunks of how many
    u32 chunk = 0;

    void destroy() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear();
    }
    void restart() {                         // a new call records from the first event on: what the last one published is gone
        next = used = 0;
        pending = false;
    }
    int mark(hipStream_t stream) {           // the next stage boundary
        if (ev.size() <= next) {
            hipEvent_t e = nullptr;
            SA_HIP_CHECK(hipEventCreate(&e));
            ev.push_back(e);
        }
        SA_HIP_CHECK(hipEventRecord(ev[next++], stream));
        return 0;
    }
    void publish() {                         // behind the last mark of a chunk
        used = next;
        pending = true;
    }
    void finish(u64 Q, u32 chunk_) {         // behind the last chunk of a call
        q = Q;
        chunk = chunk_;
    }
    int resolve() {
        if (!pending) return 0;
        double sum[STAGES] = {};
        float f = 0.f;
        SA_HIP_CHECK(hipEventSynchronize(ev[used - 1]));
        for (size_t k = 0; k + STAGES < used; k += STAGES + 1)
            for (u32 s = 0; s < STAGES; ++s) {
                SA_HIP_CHECK(hipEventElapsedTime(&f, ev[k + s], ev[k + s + 1]));
                sum[s] += f;
            }
        for (u32 s = 0; s < STAGES; ++s) ms[s] = sum[s];
        pending = false;
        return 0;
    }
};

}  // namespace sa
