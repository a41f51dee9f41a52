// The voxel a world point lies in, in the frame the class words are sampled in (include/tsdf_amd.h, "class fusion", Sampling):
// i = (int)floorf(((p - offset) - offset_at_clear) / voxel_size) per axis.  class_sample_kernel (classes.hip) and objects_lookup_kernel
// (objects.hip) both read the voxel this names, so a lookup's object is the object of the voxel whose class the sampler reports.
#pragma once

#include "common.hpp"

namespace tsdf {

// false for a NaN coordinate or an index off the resident grid; otherwise `at` is the voxel's place in the resident arrays (its voxel
// id on a volume that holds every plane).  p: the point's three floats.
__device__ inline bool class_voxel_at(const Geom &g, const float *__restrict__ p, size_t &at) {
    const float fx = floorf(((p[0] - g.offset.x) - g.offset_clear.x) / g.vs.x);
    const float fy = floorf(((p[1] - g.offset.y) - g.offset_clear.y) / g.vs.y);
    const float fz = floorf(((p[2] - g.offset.z) - g.offset_clear.z) / g.vs.z);
    // (false for NaN; the grid's sides are below 2^16, so the bounds are exact floats)
    if (!(fx >= 0.0f && fx < (float)g.X && fy >= 0.0f && fy < (float)g.Y && fz >= (float)g.z_store_begin && fz < (float)g.z_store_end)) return false;
    at = ((size_t)((uint32_t)fz - g.z_store_begin) * g.Y + (uint32_t)fy) * g.X + (uint32_t)fx;
    return true;
}

}  // namespace tsdf
