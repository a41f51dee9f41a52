// An opt-in channel of one dword per resident voxel beside the distances (colour.hip, classes.hip): enabling and disabling it, asking
// for it, its device pointer and whole-array download / upload, once.  A channel is the handle's member that holds the array plus the
// texts of its user; `who` is the public function's name.
#pragma once

#include "common.hpp"

namespace tsdf {

struct VoxelWords {
    uint32_t *tsdf_volume::*words;    // null while the channel is off
    const char *not_enabled, *slab;   // formats taking `who`
    const char *free_sync, *alloc, *clear, *to_device, *from_device;
};

inline int voxel_words_require(const tsdf_volume *v, const VoxelWords &c, const char *who) {
    TSDF_REQUIRE(v, "%s: null volume", who);
    TSDF_REQUIRE(v->*c.words, c.not_enabled, who);
    return TSDF_OK;
}

inline int voxel_words_enable(tsdf_volume *v, const VoxelWords &c, const char *who, int enabled) {
    TSDF_REQUIRE(v, "%s: null volume", who);
    uint32_t *&words = v->*c.words;
    if (!enabled) {
        if (words) {
            TSDF_HIP(hipStreamSynchronize(v->stream), c.free_sync);
            (void)hipFree(words);
            words = nullptr;
        }
        return TSDF_OK;
    }
    TSDF_REQUIRE(!v->slab, c.slab, who);
    if (words) return TSDF_OK;
    const size_t bytes = v->resident_voxels() * sizeof(uint32_t);
    TSDF_HIP(hipMalloc((void **)&words, bytes), c.alloc);
    const hipError_t e = hipMemsetAsync(words, 0, bytes, v->stream);
    if (e != hipSuccess) {
        (void)hipFree(words);
        words = nullptr;
        return hip_fail(e, c.clear);
    }
    return TSDF_OK;
}

inline int voxel_words_enabled(const tsdf_volume *v, const VoxelWords &c, const char *who, int *enabled) {
    TSDF_REQUIRE(v && enabled, "%s: null argument", who);
    *enabled = v->*c.words ? 1 : 0;
    return TSDF_OK;
}

inline int voxel_words_pointer(const tsdf_volume *v, const VoxelWords &c, const char *who, uint32_t **device_ptr) {
    TSDF_REQUIRE(device_ptr, "%s: null argument", who);
    const int rc = voxel_words_require(v, c, who);
    if (rc != TSDF_OK) return rc;
    *device_ptr = v->*c.words;
    return TSDF_OK;
}

// download (host_out) or upload (host_in) of the whole array, blocking; exactly one of the two is given
inline int voxel_words_copy(const tsdf_volume *v, const VoxelWords &c, const char *who, uint32_t *host_out, const uint32_t *host_in) {
    TSDF_REQUIRE(host_out || host_in, "%s: null argument", who);
    const int rc = voxel_words_require(v, c, who);
    if (rc != TSDF_OK) return rc;
    const size_t bytes = v->resident_voxels() * sizeof(uint32_t);
    const char *what = host_out ? c.from_device : c.to_device;
    if (host_out)
        TSDF_HIP(hipMemcpyAsync(host_out, v->*c.words, bytes, hipMemcpyDeviceToHost, v->stream), what);
    else
        TSDF_HIP(hipMemcpyAsync(v->*c.words, host_in, bytes, hipMemcpyHostToDevice, v->stream), what);
    TSDF_HIP(hipStreamSynchronize(v->stream), what);
    return TSDF_OK;
}

}  // namespace tsdf
