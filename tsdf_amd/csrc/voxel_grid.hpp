// Voxel ids and the per-chunk masks over them, shared by voxel_set.hpp (the list and the clusters of a voxel set), explore.hip (its
// flag kernel marks the frontier voxels) and objects.hip (its flag kernel marks the labelled voxels, its lookup reads the masks): voxel
// (x, y, z) of an X x Y x Z grid has id (z * Y + y) * X + x, 64 consecutive ids are a chunk, and a chunk's 64-bit mask says which of its
// voxels are listed (store_keep_mask and compact_index, mesh_device.hpp, write the masks and turn an id into a list index).
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

}  // namespace tsdf
