// The device memory of a handle ("scratch arrays"): the grow-only array, its release, the destroy functions' free-all, and
// the frame of a one-shot host variant.  Handles stay plain structs that are memset to zero: a null pointer with a capacity of 0 is an
// empty array, and nothing here owns memory.
#pragma once

#include <hip/hip_runtime.h>

#include "tsdf_amd.h"

namespace tsdf {

void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what);

// free p, leave an empty array
template <typename T>
void device_release(T *&p, size_t &cap) {
    (void)hipFree(p);   // (a null pointer is fine)
    p = nullptr;
    cap = 0;
}

// every pointer freed and nulled, for the destroy functions (capacities are the dying handle's)
template <typename... T>
void device_free_all(T *&...p) {
    ((void)hipFree(p), ...);
    ((p = nullptr), ...);
}

// At least `want` units of `unit_bytes` each behind p, `cap` counting in those units.  Arrays only grow; what they held is not kept.
// A failure leaves the array empty (p null, cap 0), so the next call tries again.
template <typename T>
hipError_t device_reserve_units(T *&p, size_t &cap, size_t want, size_t unit_bytes) {
    if (want <= cap) return hipSuccess;
    device_release(p, cap);
    const hipError_t e = hipMalloc((void **)&p, want * unit_bytes);
    if (e == hipSuccess) cap = want;
    else p = nullptr;
    return e;
}

// ... cap in elements of the array
template <typename T>
hipError_t device_reserve(T *&p, size_t &cap, size_t want) {
    return device_reserve_units(p, cap, want, sizeof(T));
}

// ... cap in bytes (the void * members, and typed ones whose capacity word counts bytes)
template <typename T>
hipError_t device_reserve_bytes(T *&p, size_t &cap, size_t want_bytes) {
    return device_reserve_units(p, cap, want_bytes, 1);
}

// The frame of a one-shot host variant: one device buffer for the call's inputs and outputs, uploads, the device call, downloads, and
// the stream synchronised before the buffer goes, whatever happened.  Where the arrays lie inside the buffer is the caller's.
//     HostStage st;
//     int rc = st.begin(stream, bytes, "...: couldn't allocate %zu bytes ...");
//     if (rc != TSDF_OK) return rc;
//     st.up(...);  if (st.ok()) rc = the device call;  if (rc == TSDF_OK) st.down(...);
//     return st.finish(rc, "... failed");
struct HostStage {
    hipStream_t stream;
    void *buf;
    hipError_t e;   // the first copy that failed

    // nomem_format takes the byte count (%zu): the text of the TSDF_ERR_NOMEM this returns when the allocation fails
    int begin(hipStream_t s, size_t bytes, const char *nomem_format) {
        stream = s;
        buf = nullptr;
        e = hipSuccess;
        if (hipMalloc(&buf, bytes) != hipSuccess) {
            (void)hipGetLastError();
            buf = nullptr;
            set_error(nomem_format, bytes);
            return TSDF_ERR_NOMEM;
        }
        return TSDF_OK;
    }
    bool ok() const { return e == hipSuccess; }
    // host -> device and device -> host on the stream; nothing once a copy has failed
    void up(void *dst, const void *src, size_t bytes) {
        if (ok()) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
    }
    void down(void *dst, const void *src, size_t bytes) {
        if (ok()) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream);
    }
    // the call's own refusal first, then the first copy failure, then the synchronisation's
    int finish(int rc, const char *what) {
        const hipError_t es = hipStreamSynchronize(stream);
        (void)hipFree(buf);
        buf = nullptr;
        if (rc != TSDF_OK) return rc;
        if (e != hipSuccess) return hip_fail(e, what);
        if (es != hipSuccess) return hip_fail(es, what);
        return TSDF_OK;
    }
};

}  // namespace tsdf
