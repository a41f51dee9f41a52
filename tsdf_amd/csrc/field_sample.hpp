// Reading the fused field at a point, for the kernels that write nothing of the volume they read: field.hip (the field queries),
// align.hip (field alignment) and fuse.hip (the source side of volume fusion).  Each rule is here once: where the weights are, which
// points are valid, which voxel a valid point lies in and its weight, the distance sample (the ray cast's own trilinear(),
// raycast_sample.hpp, so that a read agrees bit for bit with what the cast saw) and the central-difference gradient.  Points are in
// the frame of the grid's lower corner (world - offset).  Contraction is off: every expression rounds as written.  At the end: the
// intensity of the fused colours in the cell of the distance sample, for align.hip's colour term.
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

// The state of a voxel, for everything that asks what has been seen (explore.hip, reach.hip, esdf.hip).  Observed: weight > 0, false
// for a NaN weight, so such a voxel is unknown.  The distance is read only where the voxel is observed; occupied is the mesh's sign
// test, dist < 0: NaN and both zeros are not negative, so they are free.  voxel_state is the whole rule; a caller that does something
// between its two halves (marks an unknown voxel, compares two observed ones) asks voxel_observed, then voxel_occupied.
enum : int { kVoxelUnknown = 0, kVoxelFree = 1, kVoxelOccupied = 2 };

__device__ inline bool voxel_observed(const WeightView &wv, size_t xy, size_t in_plane, uint32_t z) {
    return weight_at(wv, xy, in_plane, z) > 0.0f;
}

// of an OBSERVED voxel, `at` its place in the distance array
__device__ inline bool voxel_occupied(const float *__restrict__ dist, size_t at) { return dist[at] < 0.0f; }

__device__ inline int voxel_state(const float *__restrict__ dist, const WeightView &wv, size_t xy, size_t in_plane, uint32_t z) {
    if (!voxel_observed(wv, xy, in_plane, z)) return kVoxelUnknown;
    return voxel_occupied(dist, xy * z + in_plane) ? kVoxelOccupied : kVoxelFree;
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

// ---- the intensity of the fused colour field (include/tsdf_amd.h, "colour alignment") ------------------------------------------

// Y = (77 r + 150 g + 29 b) / 256 of a colour word {r, g, b, n}: an integer <= 65280 times a power of two, exact in fp32
__device__ inline float colour_intensity(uint32_t c) {
    return (float)(77u * (c & 0xFFu) + 150u * ((c >> 8) & 0xFFu) + 29u * ((c >> 16) & 0xFFu)) * 0x1p-8f;
}

// The trilinear cell of the distance sample at a valid point: trilinear()'s lower voxel, u, v, w and clamped tap offsets, by its
// expressions (a valid point is never clamped).  False where trilinear() finds no voxel (the distance there is NaN).
struct FieldCell {
    size_t base;            // index of tap 000, x fastest
    uint32_t ox, oy, oz;    // offsets of the upper taps; 0 where the tap is clamped onto the lower one
    float u, v, w;
};

template <bool FASTDIV>
__device__ inline bool field_cell(const FieldView &f, float px, float py, float pz, FieldCell &c) {
    int vx, vy, vz;
    if (!field_voxel<FASTDIV>(f, px, py, pz, vx, vy, vz)) return false;
    const float ccx = (vx + 0.5f) * f.g.vs.x + 0.0f;
    const float ccy = (vy + 0.5f) * f.g.vs.y + 0.0f;
    const float ccz = (vz + 0.5f) * f.g.vs.z + 0.0f;
    const int lx = max((px < ccx) ? vx - 1 : vx, 0);
    const int ly = max((py < ccy) ? vy - 1 : vy, 0);
    const int lz = max((pz < ccz) ? vz - 1 : vz, 0);
    const float lcx = (lx + 0.5f) * f.g.vs.x + 0.0f;
    const float lcy = (ly + 0.5f) * f.g.vs.y + 0.0f;
    const float lcz = (lz + 0.5f) * f.g.vs.z + 0.0f;
    c.u = div_by<FASTDIV>(px - lcx, f.tc.dx);
    c.v = div_by<FASTDIV>(py - lcy, f.tc.dy);
    c.w = div_by<FASTDIV>(pz - lcz, f.tc.dz);
    c.ox = ((uint32_t)lx + 1 < f.g.X) ? 1u : 0u;
    c.oy = ((uint32_t)ly + 1 < f.g.Y) ? f.tc.row : 0u;
    c.oz = ((uint32_t)lz + 1 < f.g.Z) ? f.tc.plane : 0u;
    c.base = (size_t)f.tc.plane * (uint32_t)lz + ((size_t)f.tc.row * (uint32_t)ly + (uint32_t)lx);
    return true;
}

// The intensity at a cell and the exact derivative of the interpolant inside it: eight colour dwords.  False (outputs untouched)
// where a tap was never observed (n == 0).  VALUE / GRAD: an instance asked for one of the two has none of the other's code.
template <bool FASTDIV, bool VALUE, bool GRAD>
__device__ inline bool field_intensity(const FieldView &f, const uint32_t *__restrict__ colour, const FieldCell &c, float &value, float &gx,
                                       float &gy, float &gz) {
    const uint32_t *b000 = colour + c.base;
    const uint32_t k000 = b000[0], k001 = b000[c.oz], k010 = b000[c.oy], k011 = b000[c.oy + c.oz];
    const uint32_t k100 = b000[c.ox], k101 = b000[c.ox + c.oz], k110 = b000[c.ox + c.oy], k111 = b000[c.ox + c.oy + c.oz];
    // (n > 0 in all eight: the smallest of the eight counts is not zero)
    if (min(min(min(k000, k001), min(k010, k011)), min(min(k100, k101), min(k110, k111))) < (1u << 24)) return false;
    const float i000 = colour_intensity(k000), i001 = colour_intensity(k001), i010 = colour_intensity(k010), i011 = colour_intensity(k011);
    const float i100 = colour_intensity(k100), i101 = colour_intensity(k101), i110 = colour_intensity(k110), i111 = colour_intensity(k111);
    const float u = c.u, v = c.v, w = c.w;
    if (VALUE) {
        value = i000 * (1 - u) * (1 - v) * (1 - w) +
                i001 * (1 - u) * (1 - v) * w +
                i010 * (1 - u) * v * (1 - w) +
                i011 * (1 - u) * v * w +
                i100 * u * (1 - v) * (1 - w) +
                i101 * u * (1 - v) * w +
                i110 * u * v * (1 - w) +
                i111 * u * v * w;
    }
    if (GRAD) {
        gx = div_by<FASTDIV>((i100 - i000) * (1 - v) * (1 - w) + (i101 - i001) * (1 - v) * w + (i110 - i010) * v * (1 - w) + (i111 - i011) * v * w, f.tc.dx);
        gy = div_by<FASTDIV>((i010 - i000) * (1 - u) * (1 - w) + (i011 - i001) * (1 - u) * w + (i110 - i100) * u * (1 - w) + (i111 - i101) * u * w, f.tc.dy);
        gz = div_by<FASTDIV>((i001 - i000) * (1 - u) * (1 - v) + (i011 - i010) * (1 - u) * v + (i101 - i100) * u * (1 - v) + (i111 - i110) * u * v, f.tc.dz);
    }
    return true;
}

}  // namespace tsdf
