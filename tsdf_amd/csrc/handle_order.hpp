// The stream order of a handle ("scratch arrays"): the device it was created on, the event recorded behind what was last
// enqueued on it, and whether anybody has waited for that yet.  Every handle that lives beside a volume begins with one: tsdf_mesh
// (mesh_handle.hpp), VoxelSet (voxel_set.hpp: tsdf_explorer, tsdf_objects, tsdf_frame_diff), tsdf_reach, tsdf_esdf, tsdf_snapshot,
// tsdf_columns and tsdf_render.  A plain struct: all zero is "not created", like every handle here.  The texts of the failures are the caller's, so each handle reports under its own
// name.  Like device_buffer.hpp this includes only the HIP runtime and the public header.
#pragma once

#include <hip/hip_runtime.h>

#include "tsdf_amd.h"

namespace tsdf {

int hip_fail(hipError_t e, const char *what);

struct HandleOrder {
    int device;
    hipEvent_t done;        // recorded behind the last call's launches
    mutable int pending;    // ... and not waited for yet (a reader of a const handle orders itself on it too)

    hipError_t create() {
        const hipError_t e = hipGetDevice(&device);
        return e == hipSuccess ? hipEventCreateWithFlags(&done, hipEventDisableTiming) : e;
    }

    // waits for what is in flight, then lets the event go: before the handle's arrays are freed.  Fine on a handle whose create()
    // failed or never ran.
    void destroy() {
        if (!done) return;
        (void)hipEventSynchronize(done);
        (void)hipEventDestroy(done);
        done = nullptr;
        pending = 0;
    }

    // the stream waits for what is in flight on the handle
    int join(hipStream_t stream, const char *what) const {
        if (!pending) return TSDF_OK;
        const hipError_t e = hipStreamWaitEvent(stream, done, 0);
        return e == hipSuccess ? TSDF_OK : hip_fail(e, what);
    }

    // what has just been enqueued on the stream is in flight on the handle
    int leave(hipStream_t stream, const char *what) const {
        const hipError_t e = hipEventRecord(done, stream);
        if (e != hipSuccess) return hip_fail(e, what);
        pending = 1;
        return TSDF_OK;
    }

    // the host waits for it
    int wait(const char *what) const {
        if (!pending) return TSDF_OK;
        const hipError_t e = hipEventSynchronize(done);
        if (e != hipSuccess) return hip_fail(e, what);
        pending = 0;
        return TSDF_OK;
    }
};

}  // namespace tsdf
