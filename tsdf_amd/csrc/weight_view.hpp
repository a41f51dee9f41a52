// Where a volume's weights are, as a kernel that only reads them needs it (weights.hip's three layouts), shared by field.hip (the
// field queries) and fuse.hip (volume fusion).  Reading through a view never converts the storage.
#pragma once

#include "common.hpp"

namespace tsdf {

struct WeightView {
    const float *f32;          // wmode 0
    const uint32_t *packed;    // wmode 8 / 16
    int mode;
};

// the weight of voxel (in_plane = x + X y, z) of a whole volume as a float, xy = X * Y (the branch on the mode is wave-uniform)
__device__ inline float weight_at(const WeightView &wv, size_t xy, size_t in_plane, uint32_t z) {
    if (wv.mode == 0) return wv.f32[xy * z + in_plane];
    if (wv.mode == 8) return (float)((wv.packed[xy * (z >> 2) + in_plane] >> (8u * (z & 3u))) & 0xffu);
    return (float)((wv.packed[xy * (z >> 1) + in_plane] >> (16u * (z & 1u))) & 0xffffu);
}

}  // namespace tsdf
