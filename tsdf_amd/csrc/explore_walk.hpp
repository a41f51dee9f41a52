// Rules 1 - 5 of view gain (include/tsdf_amd.h, "exploration") for one ray: the decreed skips, the clip to the grid, the drift-free
// voxel walk of rays_walk.hpp (the same clip, start cell, boundary expression and tie order) and per visited voxel the state handed
// back by `visit(ix, iy, iz)`.  Host and device: view_gain_kernel (explore.hip) runs it a lane per ray; compiled for the host it is the
// same arithmetic, every fp32 operation rounded on its own (-ffp-contract=off).
#pragma once

#include "field_sample.hpp"   // kVoxelUnknown / kVoxelFree / kVoxelOccupied
#include "rays_walk.hpp"

namespace tsdf {

enum : uint8_t { kGainSkipped = 0, kGainEnded = 1, kGainBlocked = 2 };

// The stop code of the ray; n_unknown / n_free count the voxels visited in either state.  t_max: +inf for "no limit".
// `visit` returns kVoxelUnknown / kVoxelFree / kVoxelOccupied for a voxel inside the grid (and marks an unknown one, if it wants to).
template <class Visit>
__host__ __device__ inline uint8_t gain_walk(const Geom &g, const float ox, const float oy, const float oz, const float dx, const float dy,
                                             const float dz, const float t_max, uint32_t &n_unknown, uint32_t &n_free, Visit &&visit) {
    n_unknown = 0;
    n_free = 0;
    // rule 1
    if (!(rays_finite(ox) && rays_finite(oy) && rays_finite(oz) && rays_finite(dx) && rays_finite(dy) && rays_finite(dz))) return kGainSkipped;
    if (dx == 0.0f && dy == 0.0f && dz == 0.0f) return kGainSkipped;
    if (!(t_max > 0.0f)) return kGainSkipped;   // (NaN included)
    // rule 2
    const float ax = (ox - g.offset.x) / g.vs.x, ay = (oy - g.offset.y) / g.vs.y, az = (oz - g.offset.z) / g.vs.z;
    const float sx = dx / g.vs.x, sy = dy / g.vs.y, sz = dz / g.vs.z;
    if (!(rays_finite(ax) && rays_finite(ay) && rays_finite(az) && rays_finite(sx) && rays_finite(sy) && rays_finite(sz))) return kGainSkipped;
    // rule 3
    float t0 = 0.0f, t1 = t_max;
    if (!rays_clip_axis(ax, sx, g.X, t0, t1)) return kGainSkipped;
    if (!rays_clip_axis(ay, sy, g.Y, t0, t1)) return kGainSkipped;
    if (!rays_clip_axis(az, sz, g.Z, t0, t1)) return kGainSkipped;
    if (!(t0 < t1)) return kGainSkipped;
    // rule 4
    int ix = rays_start_cell(ax, t0, sx, g.X), iy = rays_start_cell(ay, t0, sy, g.Y), iz = rays_start_cell(az, t0, sz, g.Z);
    const int stepx = sx > 0.0f ? 1 : -1, stepy = sy > 0.0f ? 1 : -1, stepz = sz > 0.0f ? 1 : -1;
    const int aheadx = sx > 0.0f ? 1 : 0, aheady = sy > 0.0f ? 1 : 0, aheadz = sz > 0.0f ? 1 : 0;
    const uint32_t limit = g.X + g.Y + g.Z;   // the bound of the loop: every trip moves one voxel along one axis, never back
    for (uint32_t visited = 0; visited < limit; visited++) {
        // rule 5 ((ix, iy, iz) is inside the grid: the start cell is clamped, and a step that leaves the grid ends the walk below)
        const int state = visit(ix, iy, iz);
        if (state == kVoxelOccupied) return kGainBlocked;
        if (state == kVoxelUnknown) n_unknown++;
        else n_free++;
        int axis = -1;
        float best = 0.0f;
        if (sx != 0.0f) {
            best = ((float)(ix + aheadx) - ax) / sx;
            axis = 0;
        }
        if (sy != 0.0f) {
            const float tn = ((float)(iy + aheady) - ay) / sy;
            if (axis < 0 || tn < best) {
                best = tn;
                axis = 1;
            }
        }
        if (sz != 0.0f) {
            const float tn = ((float)(iz + aheadz) - az) / sz;
            if (axis < 0 || tn < best) {
                best = tn;
                axis = 2;
            }
        }
        if (axis < 0 || best > t1) break;
        if (axis == 0) {
            ix += stepx;
            if (ix < 0 || ix >= (int)g.X) break;
        } else if (axis == 1) {
            iy += stepy;
            if (iy < 0 || iy >= (int)g.Y) break;
        } else {
            iz += stepz;
            if (iz < 0 || iz >= (int)g.Z) break;
        }
    }
    return kGainEnded;
}

}  // namespace tsdf
