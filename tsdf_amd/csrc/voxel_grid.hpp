// Voxel ids and the per-chunk masks over them, shared by voxel_set.hpp (the flag walk, the list and the clusters of a voxel set) and
// its users explore.hip (frontier voxels), objects.hip (labelled voxels; its lookup reads the masks) and reach.hip (traversable voxels;
// its seeds, tiles and paths read the mask): voxel (x, y, z) of an X x Y x Z grid has id (z * Y + y) * X + x, 64 consecutive ids are a
// chunk, and a chunk's 64-bit mask says which of its voxels are listed (compact_index, mesh_device.hpp, turns an id into a list index).
// The host side of the handles that walk a volume by voxel id, esdf.hip included: which volumes and ESDFs they refuse (whole_volume_checked, esdf_array_checked) and
// the geometry they hold and report (geometry_into, geometry_of, same_geometry).
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

// ---- the host side: which volumes a handle takes, and whose geometry it holds ------------------------------------------------------
// What an entry point that walks a volume's voxels by id refuses, under its own name `who`: a Z-slab (why_not_slab, if given, says
// what of the caller's lies in other slabs), a materialised deformation-node array, more voxels than 32-bit ids hold, and a handle
// of another device.  v is not null.  `accepts`: what this caller has always taken -- objects.hip reads only the class words, so the
// nodes do not matter to it; esdf.hip indexes with size_t.
enum : unsigned { kAcceptsNodes = 1u, kAcceptsWideIds = 2u };
inline int whole_volume_checked(const char *who, const tsdf_volume *v, int handle_device, const char *why_not_slab, unsigned accepts = 0u) {
    const Geom &g = v->g;
    TSDF_REQUIRE(!v->slab && g.z_store_begin == 0 && g.z_store_end == g.Z, "%s: a Z-slab volume (tsdf_volume_create_slab) is not supported%s%s", who,
                 why_not_slab ? ": " : "", why_not_slab ? why_not_slab : "");
    TSDF_REQUIRE((accepts & kAcceptsNodes) || !v->nodes,
                 "%s: the volume has a materialised deformation-node array: voxel centres must be the implicit grid", who);
    TSDF_REQUIRE((accepts & kAcceptsWideIds) || (uint64_t)g.X * g.Y * g.Z <= 0xffffffffull, "%s: %u x %u x %u voxels do not fit 32-bit voxel ids", who,
                 g.X, g.Y, g.Z);
    TSDF_REQUIRE(v->device == handle_device, "%s: the handle was created on device %d, the volume on device %d", who, handle_device, v->device);
    return TSDF_OK;
}

// the geometry as every info struct reports it, and back (the fields no info carries stay zero)
template <class Info>
void geometry_into(Info &info, const Geom &g) {
    info.size[0] = g.X; info.size[1] = g.Y; info.size[2] = g.Z;
    info.voxel_size[0] = g.vs.x; info.voxel_size[1] = g.vs.y; info.voxel_size[2] = g.vs.z;
    info.offset[0] = g.offset.x; info.offset[1] = g.offset.y; info.offset[2] = g.offset.z;
}
template <class Info>
Geom geometry_of(const Info &info) {
    Geom g = {};
    g.X = info.size[0]; g.Y = info.size[1]; g.Z = info.size[2];
    g.vs = {info.voxel_size[0], info.voxel_size[1], info.voxel_size[2]};
    g.offset = {info.offset[0], info.offset[1], info.offset[2]};
    return g;
}

// the same grid, voxel sizes and offset: what a handle's arrays and another's can be read together for
inline bool same_geometry(const Geom &a, const Geom &b) {
    return a.X == b.X && a.Y == b.Y && a.Z == b.Z && a.vs.x == b.vs.x && a.vs.y == b.vs.y && a.vs.z == b.vs.z && a.offset.x == b.offset.x &&
           a.offset.y == b.offset.y && a.offset.z == b.offset.z;
}

// What an entry point that reads an optional ESDF beside the volume (reach.hip, columns.hip) refuses, under its own name: a handle that
// has never been computed, or one computed for another geometry than `g`.  *array: the ESDF's device array, null without a handle.
inline int esdf_array_checked(const char *who, const tsdf_esdf *esdf, const Geom &g, const float **array) {
    *array = nullptr;
    if (!esdf) return TSDF_OK;
    tsdf_esdf_info ei;
    int rc = tsdf_esdf_get_info(esdf, &ei);   // (waits for a computation in flight; it is on the volume's stream anyway)
    if (rc == TSDF_OK) rc = tsdf_esdf_buffer(esdf, array);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(*array, "%s: the ESDF handle has never been computed (tsdf_volume_compute_esdf)", who);
    TSDF_REQUIRE(same_geometry(geometry_of(ei), g), "%s: the ESDF was computed for another geometry (%u x %u x %u, or other voxel sizes or offset) than the volume's",
                 who, ei.size[0], ei.size[1], ei.size[2]);
    return TSDF_OK;
}

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
