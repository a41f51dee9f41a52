// Voxel ids and the per-chunk masks over them, shared by voxel_set.hpp (the list and the clusters of a voxel set), explore.hip (its
// flag kernel marks the frontier voxels) and objects.hip (its flag kernel marks the labelled voxels, its lookup reads the masks): voxel
// (x, y, z) of an X x Y x Z grid has id (z * Y + y) * X + x, 64 consecutive ids are a chunk, and a chunk's 64-bit mask says which of its
// voxels are listed (store_keep_mask and compact_index, mesh_device.hpp, write the masks and turn an id into a list index).
// And the voxel a world point lies in, which the samplers of the per-voxel words (colour.hip, classes.hip) and objects.hip's lookup share.
#pragma once

#include "common.hpp"

namespace tsdf {

struct VoxelGrid {
    uint32_t X, Y, Z, n;   // n = X * Y * Z <= 2^32 - 1
    __device__ void split(uint32_t id, uint32_t &x, uint32_t &y, uint32_t &z) const {
        const uint32_t xy = X * Y;
        z = id / xy;
        const uint32_t ip = id - z * xy;
        y = ip / X;
        x = ip - y * X;
    }
};

__device__ inline bool mask_bit(const uint64_t *__restrict__ mask, uint32_t id) { return (mask[id >> 6] >> (id & 63u)) & 1u; }

inline VoxelGrid voxel_grid(const Geom &g) { return {g.X, g.Y, g.Z, (uint32_t)((uint64_t)g.X * g.Y * g.Z)}; }

// The voxel a world point lies in, in the frame colour and class words are sampled in (include/tsdf_amd.h, "class fusion", Sampling):
// i = (int)floorf(((p - offset) - offset_at_clear) / voxel_size) per axis, the cell whose centre, as integrate forms it, is nearest.
// colour_sample_kernel, class_sample_kernel and objects_lookup_kernel all read the voxel this names, so a lookup's object is the object
// of the voxel whose class the sampler reports.  false for a NaN coordinate or an index off the resident grid; otherwise `at` is the
// voxel's place in the resident arrays (its voxel id on a volume that holds every plane).  p: the point's three floats.
__device__ inline bool point_voxel_at(const Geom &g, const float *__restrict__ p, size_t &at) {
    const float fx = floorf(((p[0] - g.offset.x) - g.offset_clear.x) / g.vs.x);
    const float fy = floorf(((p[1] - g.offset.y) - g.offset_clear.y) / g.vs.y);
    const float fz = floorf(((p[2] - g.offset.z) - g.offset_clear.z) / g.vs.z);
    // (false for NaN; the grid's sides are below 2^16, so the bounds are exact floats)
    if (!(fx >= 0.0f && fx < (float)g.X && fy >= 0.0f && fy < (float)g.Y && fz >= (float)g.z_store_begin && fz < (float)g.z_store_end)) return false;
    at = ((size_t)((uint32_t)fz - g.z_store_begin) * g.Y + (uint32_t)fy) * g.X + (uint32_t)fx;
    return true;
}

}  // namespace tsdf
