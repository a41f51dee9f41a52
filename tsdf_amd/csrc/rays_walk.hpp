// Rules 1 - 6 of ray integration (include/tsdf_amd.h, "ray integration") for one ray: the decreed skips, the stretch, the clip to the grid,
// the drift-free Amanatides-Woo walk, and per visited voxel the quantised observation handed to `observe(ix, iy, iz, q)`.  Host and
// device: rays_scatter_kernel (integrate_rays.hip) runs it a lane per ray; compiled for the host it is the same arithmetic, every
// fp32 operation rounded on its own (-ffp-contract=off).  rays_walk_sdf is the same walk handing `observe(ix, iy, iz, q, sdf)` the
// unclamped sdf of rule 6 as well: the band test of rule 9 (rays_scatter_colour_kernel) is on it, not on q.
#pragma once

#include "common.hpp"

namespace tsdf {

__host__ __device__ inline bool rays_finite(float x) { return x - x == 0.0f; }

// rule 4 for one axis: false = the ray is skipped
__host__ __device__ inline bool rays_clip_axis(float a, float s, uint32_t n, float &t0, float &t1) {
    if (s == 0.0f) return a >= 0.0f && a < (float)n;
    const float ta = (0.0f - a) / s, tb = ((float)n - a) / s;
    t0 = fmaxf(t0, fminf(ta, tb));
    t1 = fminf(t1, fmaxf(ta, tb));
    return true;
}

__host__ __device__ inline int rays_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__host__ __device__ inline int rays_start_cell(float a, float t0, float s, uint32_t n) {
    return rays_clampi(f2i_sat(floorf(a + t0 * s)), 0, (int)n - 1);
}

template <class Observe>
__host__ __device__ inline void rays_walk_sdf(const Geom &g, const float ox, const float oy, const float oz, const float px, const float py,
                                              const float pz, const float min_range, const float max_range, const int band_only,
                                              Observe &&observe) {
    // rule 1
    if (!(rays_finite(ox) && rays_finite(oy) && rays_finite(oz) && rays_finite(px) && rays_finite(py) && rays_finite(pz))) return;
    const float dx = px - ox, dy = py - oy, dz = pz - oz;
    const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
    if (!(r > 0.0f) || !rays_finite(r)) return;
    if (min_range != min_range || max_range != max_range) return;
    if (r < min_range || r > max_range) return;
    const float ux = dx / r, uy = dy / r, uz = dz / r;
    // rule 2
    const float trunc = g.trunc;
    float t1 = r + trunc;
    float t0 = band_only ? fmaxf(r - trunc, 0.0f) : 0.0f;
    // rule 3
    const float ax = (ox - g.offset.x) / g.vs.x, ay = (oy - g.offset.y) / g.vs.y, az = (oz - g.offset.z) / g.vs.z;
    const float sx = ux / g.vs.x, sy = uy / g.vs.y, sz = uz / g.vs.z;
    // rule 4
    if (!rays_clip_axis(ax, sx, g.X, t0, t1)) return;
    if (!rays_clip_axis(ay, sy, g.Y, t0, t1)) return;
    if (!rays_clip_axis(az, sz, g.Z, t0, t1)) return;
    if (!(t0 < t1)) return;
    // rule 5
    int ix = rays_start_cell(ax, t0, sx, g.X), iy = rays_start_cell(ay, t0, sy, g.Y), iz = rays_start_cell(az, t0, sz, g.Z);
    const int stepx = sx > 0.0f ? 1 : -1, stepy = sy > 0.0f ? 1 : -1, stepz = sz > 0.0f ? 1 : -1;
    const int aheadx = sx > 0.0f ? 1 : 0, aheady = sy > 0.0f ? 1 : 0, aheadz = sz > 0.0f ? 1 : 0;
    const uint32_t limit = g.X + g.Y + g.Z;
    for (uint32_t visit = 0; visit < limit; visit++) {
        // rule 6
        const float cx = ((ix + 0.5f) * g.vs.x) + g.offset.x, cy = ((iy + 0.5f) * g.vs.y) + g.offset.y, cz = ((iz + 0.5f) * g.vs.z) + g.offset.z;
        const float ex = cx - ox, ey = cy - oy, ez = cz - oz;
        const float sdf = r - ((ex * ux + ey * uy) + ez * uz);
        if (!(sdf < -trunc)) {
            const float tsdf = sdf > 0.0f ? fminf(sdf, trunc) : sdf;
            const int q = (int)rintf((tsdf / trunc) * 32768.0f);
            // (ix, iy, iz) is inside the grid: the start cell is clamped, and a step that leaves the grid ends the walk below
            observe(ix, iy, iz, q, sdf);
        }
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
}

template <class Observe>
__host__ __device__ inline void rays_walk(const Geom &g, const float ox, const float oy, const float oz, const float px, const float py,
                                          const float pz, const float min_range, const float max_range, const int band_only,
                                          Observe &&observe) {
    rays_walk_sdf(g, ox, oy, oz, px, py, pz, min_range, max_range, band_only, [&](int ix, int iy, int iz, int q, float) { observe(ix, iy, iz, q); });
}

}  // namespace tsdf
