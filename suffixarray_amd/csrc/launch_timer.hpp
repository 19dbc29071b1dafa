// launch_timer.hpp -- the stopwatch of one kind of launch on a handle's stream (capi_token*.hpp): an event either side of the last
// launch, resolved when an *_info call asks for the figure.  The caller has set the device and holds the handle's mutex.
#pragma once
#include "common.hpp"

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

}  // namespace sa
