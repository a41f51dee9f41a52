// Reading the fused field at a point, for the kernels that write nothing of the volume they read: field.hip (the field queries),
// align.hip (field alignment) and fuse.hip (the source side of volume fusion).  Each rule is here once: where the weights are, which
// points are valid, which voxel a valid point lies in and its weight, the distance sample (the ray cast's own trilinear(),
// raycast_sample.hpp, so that a read agrees bit for bit with what the cast saw) and the central-difference gradient.  Points are in
// the frame of the grid's lower corner (world - offset).  Contraction is off: every expression rounds as written.
#pragma once

#include "raycast_sample.hpp"

namespace tsdf {

// Where a volume's weights are (weights.hip's three layouts).  Reading through a view never converts the storage.
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

// What a read-only kernel needs of a whole (not Z-slab) volume; travels as one kernel argument.
struct FieldView {
    const float *dist;
    WeightView wv;
    Geom g;
    TriConst tc;
};

inline FieldView make_field_view(const tsdf_volume *v) {
    return {v->dist, {v->weight, v->wpacked, v->wmode}, v->g, make_tri_const(v->g)};
}

// field.hip: the field queries' launch on a view -- distance (n), gradient (3 n), weight (n) at n device points, any output may be
// null but not all, n > 0; flags as tsdf_volume_sample_field_device.  fast_div: the volume's verified division (tsdf_volume::fast_div).
int sample_field_view(const FieldView &f, bool fast_div, uint64_t n, const float *points, float *d, float *grad, float *w, int flags,
                      hipStream_t stream);

// The taps of a sample cross slab boundaries: every caller refuses a Z-slab volume, under its own name.
inline int field_refuse_slab(const tsdf_volume *v, const char *what) {
    TSDF_REQUIRE(!v->slab && v->g.z_store_begin == 0 && v->g.z_store_end == v->g.Z,
                 "%s: not supported on a Z-slab volume (tsdf_volume_create_slab): the taps of a sample cross slab boundaries", what);
    return TSDF_OK;
}

// valid(q): finite, >= 0 and below the fp32 product the cast forms as max_x / y / z (false for NaN; -0.0 is valid)
__device__ inline bool field_valid(const FieldView &f, float x, float y, float z) {
    return x >= 0.0f && x < f.tc.max_x && y >= 0.0f && y < f.tc.max_y && z >= 0.0f && z < f.tc.max_z;
}

// The voxel a valid point lies in: trilinear's voxel_for_point (same quotient, FASTDIV or not; no clamping applies to a valid point).
// False where a quotient reaches `size` itself, as it can for a point within rounding of the upper bound: no such voxel.
template <bool FASTDIV>
__device__ inline bool field_voxel(const FieldView &f, float x, float y, float z, int &vx, int &vy, int &vz) {
    vx = f2i_sat(floorf(div_by<FASTDIV>(x, f.tc.dx)));
    vy = f2i_sat(floorf(div_by<FASTDIV>(y, f.tc.dy)));
    vz = f2i_sat(floorf(div_by<FASTDIV>(z, f.tc.dz)));
    return (uint32_t)vx < f.g.X && (uint32_t)vy < f.g.Y && (uint32_t)vz < f.g.Z;
}

__device__ inline float field_voxel_weight(const FieldView &f, int vx, int vy, int vz) {
    return weight_at(f.wv, f.tc.plane, (size_t)f.tc.row * (uint32_t)vy + (uint32_t)vx, (uint32_t)vz);
}

// the weight of the voxel a valid point lies in, 0 where there is none
template <bool FASTDIV>
__device__ inline float field_weight(const FieldView &f, float x, float y, float z) {
    int vx, vy, vz;
    return field_voxel<FASTDIV>(f, x, y, z, vx, vy, vz) ? field_voxel_weight(f, vx, vy, vz) : 0.0f;
}

// the distance at a valid point (NaN where field_voxel is false)
template <bool FASTDIV>
__device__ inline float field_distance(const FieldView &f, float x, float y, float z) {
    bool owned;
    return trilinear<false, false, FASTDIV>(x, y, z, f.dist, f.g, f.tc, 0u, 0u, owned, nullptr);
}

// The points of the central difference: q and q -+ voxel_size along each axis.  Each of the seven is sampled as a point of its own
// (its own cell: at a cell face rounding decides), and a caller may read anything else of the field at the same seven.
struct FieldStencil {
    float x, y, z;
    float xp, xm, yp, ym, zp, zm;
};

__device__ inline FieldStencil field_stencil(const FieldView &f, float x, float y, float z) {
    return {x, y, z, x + f.g.vs.x, x - f.g.vs.x, y + f.g.vs.y, y - f.g.vs.y, z + f.g.vs.z, z - f.g.vs.z};
}

// the gradient is defined where all seven points are valid
__device__ inline bool field_stencil_valid(const FieldView &f, const FieldStencil &s) {
    return field_valid(f, s.x, s.y, s.z) && field_valid(f, s.xp, s.y, s.z) && field_valid(f, s.xm, s.y, s.z) &&
           field_valid(f, s.x, s.yp, s.z) && field_valid(f, s.x, s.ym, s.z) && field_valid(f, s.x, s.y, s.zp) &&
           field_valid(f, s.x, s.y, s.zm);
}

// the raw gradient at a stencil that is valid: six samples
template <bool FASTDIV>
__device__ inline void field_gradient(const FieldView &f, const FieldStencil &s, float &gx, float &gy, float &gz) {
    const float sxp = field_distance<FASTDIV>(f, s.xp, s.y, s.z), sxm = field_distance<FASTDIV>(f, s.xm, s.y, s.z);
    const float syp = field_distance<FASTDIV>(f, s.x, s.yp, s.z), sym = field_distance<FASTDIV>(f, s.x, s.ym, s.z);
    const float szp = field_distance<FASTDIV>(f, s.x, s.y, s.zp), szm = field_distance<FASTDIV>(f, s.x, s.y, s.zm);
    gx = (sxp - sxm) / (f.g.vs.x + f.g.vs.x);
    gy = (syp - sym) / (f.g.vs.y + f.g.vs.y);
    gz = (szp - szm) / (f.g.vs.z + f.g.vs.z);
}

}  // namespace tsdf
