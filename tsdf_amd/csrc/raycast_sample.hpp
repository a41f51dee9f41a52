// The ray cast's trilinear sample and what it needs: the loop-invariant constants, the division by a voxel edge, RayParams and
// trilinear() itself.  Shared by raycast.hip (the march, the cell-parallel cast) and, through field_sample.hpp, by field.hip,
// align.hip and fuse.hip, so that every translation unit samples with the very same expressions.
#pragma once

#include "common.hpp"

namespace tsdf {

struct InvDiv {
    float b, y;
};

// Loop-invariant pieces of trilinearly_interpolate (:60-71) and of tsdf_value_at, same float expressions.
struct TriConst {
    float max_x, max_y, max_z;        // voxel_grid_size * voxel_size
    float clamp_x, clamp_y, clamp_z;  // max - voxel_size / 10
    InvDiv dx, dy, dz;
    uint32_t row, plane;              // X, X*Y
};
__host__ __device__ inline TriConst make_tri_const(const Geom &g) {
    TriConst c;
    c.max_x = g.X * g.vs.x;
    c.max_y = g.Y * g.vs.y;
    c.max_z = g.Z * g.vs.z;
    c.clamp_x = c.max_x - (g.vs.x / 10.0f);
    c.clamp_y = c.max_y - (g.vs.y / 10.0f);
    c.clamp_z = c.max_z - (g.vs.z / 10.0f);
    c.dx = {g.vs.x, 1.0f / g.vs.x};
    c.dy = {g.vs.y, 1.0f / g.vs.y};
    c.dz = {g.vs.z, 1.0f / g.vs.z};
    c.row = g.X;
    c.plane = g.X * g.Y;  // X, Y <= 65535
    return c;
}

struct RayParams {
    F3 origin;
    Mat33 rot;
    Mat33 kinv;
    F3 space_min;
    F3 space_max;
    uint32_t width, height;
    uint32_t own_lo, own_hi;  // slab ownership (planes of the lower trilinear tap)
    uint32_t seg_len;         // > 0: blockIdx.z handles samples [z*seg_len, (z+1)*seg_len) and writes records
    uint32_t slab_ranges;     // > 0 (slabs): blockIdx.z handles that part of each ray's own stretch through the slab
    uint32_t tile_map;        // which image tiles an XCD gets (see process_ray_kernel): 0 every eighth tile, 1 one contiguous eighth of the image, 2 one 5x5-tile block per block row
    uint32_t range_order;     // order in which the sample ranges are dispatched (see process_ray_kernel): 0 ascending, 1 descending (default), 2 last, first, then descending
    TriConst tc;              // loop-invariant pieces of the interpolation, formed once on the host (same IEEE operations)
    // entry bound of this view (EntryParams, common.hpp): one word per 16 x 16 tile + the on/off word at [ztile_count]; nullptr = none
    const uint32_t *ztile;
    uint32_t ztile_pitch, ztile_count;
};

// Division by a loop-invariant voxel edge.  The reference divides (IEEE, correctly rounded); when FASTDIV is
// set the quotient is formed as q0 = a*y, r = fma(-b, q0, a), q = fma(r, y, q0) with y = RN(1/b).  That
// sequence is used ONLY after volume.hip has checked it against the IEEE quotient for EVERY finite fp32
// numerator with |a| >= kFastDivMin for this very b (verify_fast_division, ~2^32 cases per voxel
// edge, a few ms once per volume), so on that domain it is the same function in three instructions instead
// of the ~14 of a full fp32 division; numerators outside the domain take the IEEE division.
template <bool FASTDIV>
__device__ inline float div_by(float a, const InvDiv &d) {
    if (FASTDIV) {
        const float mag = fabsf(a);
        const bool verified = mag >= kFastDivMin && mag < INFINITY;  // the verified domain
        const float q0 = a * d.y;
        const float r = __builtin_fmaf(-d.b, q0, a);
        float q = __builtin_fmaf(r, d.y, q0);
        // the IEEE sequence sits behind a wave-uniform branch: left to itself the compiler computes both and selects
        if (__builtin_expect(__ballot(!verified) != 0ull, 0)) {
            if (!verified) q = a / d.b;
        }
        return q;
    }
    return a / d.b;
}

// trilinearly_interpolate (src/RayCaster/GPURaycaster.cu:53-124) with voxel_for_point, centre_of_voxel_at and
// tsdf_value_at (src/TSDF/TSDF_utilities.cu:10-53) inlined.  For SLAB, samples whose lower tap plane is not
// owned (outside [own_lo, own_hi), RayParams' words) are not evaluated (owned=false, result NaN); otherwise the two are not read.
template <bool SLAB, bool STATS, bool FASTDIV>
__device__ inline float trilinear(float px, float py, float pz, const float *__restrict__ dist, const Geom &g,
                                  const TriConst &tc, uint32_t own_lo, uint32_t own_hi, bool &owned,
                                  unsigned int *__restrict__ touched) {
    float ax = px, ay = py, az = pz;
    if (px >= tc.max_x) ax = tc.clamp_x;
    if (py >= tc.max_y) ay = tc.clamp_y;
    if (pz >= tc.max_z) az = tc.clamp_z;
    if (px < 0.0f) ax = 0.0f;
    if (py < 0.0f) ay = 0.0f;
    if (pz < 0.0f) az = 0.0f;

    // voxel_for_point (src/TSDF/TSDF_utilities.cu:45-53)
    int vx = f2i_sat(floorf(div_by<FASTDIV>(ax, tc.dx)));
    int vy = f2i_sat(floorf(div_by<FASTDIV>(ay, tc.dy)));
    int vz = f2i_sat(floorf(div_by<FASTDIV>(az, tc.dz)));

    owned = true;
    if (vx < 0 || vy < 0 || vz < 0 || (uint32_t)vx >= g.X || (uint32_t)vy >= g.Y || (uint32_t)vz >= g.Z) {
        return NAN;  // the reference also printf's here (:78)
    }

    // centre_of_voxel_at with its default zero offset (src/TSDF/TSDF_utilities.cu:10-17)
    float ccx = (vx + 0.5f) * g.vs.x + 0.0f;
    float ccy = (vy + 0.5f) * g.vs.y + 0.0f;
    float ccz = (vz + 0.5f) * g.vs.z + 0.0f;

    int lx = (px < ccx) ? vx - 1 : vx;
    int ly = (py < ccy) ? vy - 1 : vy;
    int lz = (pz < ccz) ? vz - 1 : vz;
    lx = max(lx, 0);
    ly = max(ly, 0);
    lz = max(lz, 0);

    if (SLAB) {
        if (!((uint32_t)lz >= own_lo && (uint32_t)lz < own_hi)) {
            owned = false;
            return NAN;
        }
    }

    float lcx = (lx + 0.5f) * g.vs.x + 0.0f;
    float lcy = (ly + 0.5f) * g.vs.y + 0.0f;
    float lcz = (lz + 0.5f) * g.vs.z + 0.0f;
    float u = div_by<FASTDIV>(px - lcx, tc.dx);
    float v = div_by<FASTDIV>(py - lcy, tc.dy);
    float w = div_by<FASTDIV>(pz - lcz, tc.dz);

    // tsdf_value_at clamps each tap to the grid (:31-33): lower is in range, so only lower+1 can be
    // clamped, to lower itself (0 <= lower <= size-1 <= 65534: the uint16_t parameters never wrap).
    const uint32_t ox = ((uint32_t)lx + 1 < g.X) ? 1u : 0u;
    const uint32_t oy = ((uint32_t)ly + 1 < g.Y) ? tc.row : 0u;
    const uint32_t oz = ((uint32_t)lz + 1 < g.Z) ? tc.plane : 0u;
    const float *b000 = dist + ((size_t)tc.plane * ((uint32_t)lz - g.z_store_begin) + (__umul24(tc.row, (uint32_t)ly) + (uint32_t)lx));   // (X, Y < 2^16: 24-bit multiply, X * Y < 2^32)
    if (STATS) {
        const size_t gi = (size_t)tc.plane * (uint32_t)lz + (size_t)tc.row * (uint32_t)ly + (uint32_t)lx;
        const uint32_t offs[8] = {0, oz, oy, oy + oz, ox, ox + oz, ox + oy, ox + oy + oz};
        for (int i = 0; i < 8; i++) {
            size_t q = gi + offs[i];
            atomicOr(&touched[q >> 5], 1u << (q & 31));
        }
    }
    float c000 = b000[0];
    float c001 = b000[oz];
    float c010 = b000[oy];
    float c011 = b000[oy + oz];
    float c100 = b000[ox];
    float c101 = b000[ox + oz];
    float c110 = b000[ox + oy];
    float c111 = b000[ox + oy + oz];

    float interpolated = c000 * (1 - u) * (1 - v) * (1 - w) +
                         c001 * (1 - u) * (1 - v) * w +
                         c010 * (1 - u) * v * (1 - w) +
                         c011 * (1 - u) * v * w +
                         c100 * u * (1 - v) * (1 - w) +
                         c101 * u * (1 - v) * w +
                         c110 * u * v * (1 - w) +
                         c111 * u * v * w;
    return interpolated;
}

}  // namespace tsdf
