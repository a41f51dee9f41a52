// The pixel boxes of the cell-parallel cast (raycast_cells.hpp): which pixels a box of the grid, or a mixed cell, can be seen by.
// Bounds, not results -- a box that is too wide costs pairs, one that is too narrow loses a hit -- so the arithmetic is chosen for
// its instruction count and its error is paid for in the margins, with the argument written beside each.  Plain C++ for both sides:
// cast_cells_kernel and cell_cast_prepare_kernel run it on the GPU, tsdf_selftest_cell_boxes runs the same expressions on the host
// (tests/test_cell_boxes.py compares them with the hull projected in double precision and needs no GPU).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TSDF_BOX_HD __host__ __device__
#else
#define TSDF_BOX_HD
#endif

namespace tsdf {

// 1 / x to an ulp or so (the hardware's reciprocal on the device)
TSDF_BOX_HD inline float box_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}

// guard band at the dual-cell faces, in voxels (SkipCtx::eps): the cells are projected grown by it
TSDF_BOX_HD inline float cell_guard_eps(uint32_t x, uint32_t y, uint32_t z) {
    const uint32_t m = x > y ? (x > z ? x : z) : (y > z ? y : z);
    return fmaxf(1.0e-3f, 2.0e-6f * (float)m);
}

// pixel box of the axis-aligned box [lo, hi] (grid millimetres) under the view's projection: false = no pixel can see it.
// (V: anything with EntryParams' r, k, offset, width, height, z_clip, z_near -- EntryParams itself, or the cells' block below.)
// A sample's camera depth is its ray parameter t >= z_clip >= 0 (the last row of kinv is (0, 0, 1): view_projection; z_clip > 0 when
// the camera is outside the volume, choose_cell_cast): only the part of the box with depth D >= z_clip can hold samples.
//   * wholly behind that plane: none;
//   * wholly in front of z_near > 0: the integers inside the hull of its 8 projected corners;
//   * otherwise (the box straddles the plane, or comes within a quarter voxel of the camera plane): u = N(P) / D(P), N and D affine in
//     P, so for any u*, u - u* = F(P) / D(P) with F = N - u* D affine too: over the box F lies in [F_c - h, F_c + h] (its value at the
//     centre -+ half the sum of its coefficients along the box's edges) and D in (max(z_min, z_clip), z_max].  F_c - h > 0: the box is
//     to the right of u* for every sample in it, by at least (F_c - h) / z_max; F_c + h < 0: to the left; the far side is bounded by
//     the nearest depth when that is positive, not at all otherwise (a box that holds the camera asks every pixel).  u* = the image's
//     centre: a box beside or behind the camera that reaches across the camera plane lies far off the image and is dropped here.
struct PixelBox {
    int u0, v0, w, h;
};
template <bool HULL = true, class V>   // (false: the bound from the centre only -- wider in front of z_near, where the cells' kernel has its own)
TSDF_BOX_HD inline bool project_box(const V &ep, float lox, float loy, float loz, float hix, float hiy, float hiz, PixelBox &pb) {
    const float mx = 0.5f * (lox + hix) + ep.offset.x, my = 0.5f * (loy + hiy) + ep.offset.y, mz = 0.5f * (loz + hiz) + ep.offset.z;
    const float ccx = ep.r[0][0] * mx + ep.r[0][1] * my + ep.r[0][2] * mz + ep.r[0][3];
    const float ccy = ep.r[1][0] * mx + ep.r[1][1] * my + ep.r[1][2] * mz + ep.r[1][3];
    const float ccz = ep.r[2][0] * mx + ep.r[2][1] * my + ep.r[2][2] * mz + ep.r[2][3];
    const float ext[3] = {hix - lox, hiy - loy, hiz - loz};
    const float hz = 0.5f * ((fabsf(ep.r[2][0] * ext[0]) + fabsf(ep.r[2][1] * ext[1])) + fabsf(ep.r[2][2] * ext[2]));
    // (the centre's coordinates are good to a few ulps of the largest term: 1e-5 of the camera's distance covers it with room)
    const float zslack = 1.0e-5f * (((fabsf(ep.r[2][0] * mx) + fabsf(ep.r[2][1] * my)) + fabsf(ep.r[2][2] * mz)) + fabsf(ep.r[2][3])) + 1.0e-5f * hz;
    const float zmin = ccz - hz - zslack, zmax = ccz + hz + zslack;
    if (!(ccx == ccx && ccy == ccy && zmin == zmin && zmax == zmax) || fabsf(ccx) == INFINITY || fabsf(ccy) == INFINITY || zmax == INFINITY || zmin == -INFINITY) {
        pb.u0 = 0; pb.v0 = 0; pb.w = (int)ep.width; pb.h = (int)ep.height;   // (something not finite: every pixel is asked)
        return true;
    }
    if (zmax < ep.z_clip) return false;
    float a0, a1, b0, b1;
    const float kMargin = 0.05f;   // (the projection is the double-precision inverse of the matrices the rays are formed with, evaluated in fp32: 1e-2 px at most)
    if (HULL && zmin > ep.z_near) {
        float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const float wx = ((c & 1) ? hix : lox) + ep.offset.x, wy = ((c & 2) ? hiy : loy) + ep.offset.y, wz = ((c & 4) ? hiz : loz) + ep.offset.z;
            const float cx = ep.r[0][0] * wx + ep.r[0][1] * wy + ep.r[0][2] * wz + ep.r[0][3];
            const float cy = ep.r[1][0] * wx + ep.r[1][1] * wy + ep.r[1][2] * wz + ep.r[1][3];
            const float cz = fmaxf(ep.r[2][0] * wx + ep.r[2][1] * wy + ep.r[2][2] * wz + ep.r[2][3], 0.5f * ep.z_near);
            const float rz = box_rcp(cz);   // (a bound, not a result: the margin below covers the last bits)
            const float u = (ep.k[0][0] * cx + ep.k[0][1] * cy + ep.k[0][2] * cz) * rz, w = (ep.k[1][0] * cx + ep.k[1][1] * cy + ep.k[1][2] * cz) * rz;
            umin = fminf(umin, u); umax = fmaxf(umax, u);
            vmin = fminf(vmin, w); vmax = fmaxf(vmax, w);
        }
        // a ray exists per INTEGER pixel: the integers inside the hull's box
        a0 = ceilf(umin - kMargin); a1 = floorf(umax + kMargin); b0 = ceilf(vmin - kMargin); b1 = floorf(vmax + kMargin);
    } else {
        const float us = 0.5f * (float)ep.width, vs_ = 0.5f * (float)ep.height;
        const float dlo = fmaxf(zmin, ep.z_clip), rhi = 1.0f / (zmax * 1.0001f), rlo = dlo > 0.0f ? 1.0001f / dlo : INFINITY;
        auto side = [&](const float *kr, float centre, float &lo_, float &hi_) {
            const float t0 = kr[0] * ccx, t1 = kr[1] * ccy, t2 = kr[2] * ccz, t3 = centre * ccz;
            const float fc = ((t0 + t1) + t2) - t3;
            float h = 0.0f;
#pragma unroll
            for (int a_ = 0; a_ < 3; a_++) {
                const float ex_ = ep.r[0][a_] * ext[a_], ey_ = ep.r[1][a_] * ext[a_], ez_ = ep.r[2][a_] * ext[a_];
                h += 0.5f * fabsf(((kr[0] * ex_ + kr[1] * ey_) + kr[2] * ez_) - centre * ez_);
            }
            const float slack = 1.0e-5f * ((((fabsf(t0) + fabsf(t1)) + fabsf(t2)) + fabsf(t3)) + h) + (fabsf(kr[0]) + fabsf(kr[1]) + fabsf(kr[2]) + centre) * zslack;
            const float fmin_ = fc - h - slack, fmax_ = fc + h + slack;
            lo_ = fmin_ > 0.0f ? fmin_ * rhi : (dlo > 0.0f ? fmin_ * rlo : -INFINITY);
            hi_ = fmax_ < 0.0f ? fmax_ * rhi : (dlo > 0.0f ? fmax_ * rlo : INFINITY);
        };
        float ul, uh, vl, vh;
        side(ep.k[0], us, ul, uh);
        side(ep.k[1], vs_, vl, vh);
        a0 = ceilf(us + ul - kMargin); a1 = floorf(us + uh + kMargin); b0 = ceilf(vs_ + vl - kMargin); b1 = floorf(vs_ + vh + kMargin);
    }
    const float wmax = (float)(ep.width - 1u), hmax = (float)(ep.height - 1u);
    if (!(a0 <= a1 && b0 <= b1) || a1 < 0.0f || b1 < 0.0f || a0 > wmax || b0 > hmax) return false;
    pb.u0 = (int)fmaxf(a0, 0.0f); pb.v0 = (int)fmaxf(b0, 0.0f);
    pb.w = (int)fminf(a1, wmax) - pb.u0 + 1; pb.h = (int)fminf(b1, hmax) - pb.v0 + 1;
    return true;
}

// ---- a mixed cell's box: what a brick's turn of cast_cells_kernel computes per lane ---------------------------------------------------
// The cell with lower voxel l = (lx, ly, lz) spans the voxel centres l + 1/2 .. l + 3/2, grown by eps: centre P_c = (l + 1) vs + offset,
// edges (1 + 2 eps) vs.  u = N(P) / D(P) with N = k0 . (R P + t) and D = the camera depth (R P + t).z, both affine in P: for P in the
// cell |u(P) - u_c| = |N(P) - u_c D(P)| / D(P) <= S / D_min, S = half the sum over the axes of |the coefficient of N - u_c D along the
// cell's edge| (any number may stand for u_c here: what the bound is centred on only has to be what S is formed with).
// Everything is affine in the INTEGERS l, so the numerators and the depth at the cell's centre are three fmas each on launch constants,
//     N_u = nu[0] + lx nu[1] + ly nu[2] + lz nu[3],   N_v likewise,   D = dz[0] + lx dz[1] + ly dz[2] + lz dz[3],
// and the edge coefficients are the same nu[1..3], nv[1..3], dz[1..3] (times 1 + 2 eps, which goes into `scale`).  Up to this round
// every lane built the centre's world coordinates, three rows of the pose and two of the intrinsics from 30 uniform values with
// separately rounded products, some 40 instructions a turn and 30 registers that a round never reads again.
//
// The constants are formed once per workgroup in double precision (cell_box_consts) and rounded once: each is good to 2^-24 of itself.
// Rounding, u = 2^-24: the three fmas and the four constants put N_u off by at most 5 u B_u, B_u = |nu[0]| + sum_a size_a |nu[a]| (the
// largest any partial sum gets over the grid), and D by 5 u B_z: N_u - u_c D, which is 0 at the true centre, by 5 u (B_u + |u_c| B_z).
// The same again for the order of roundings this form replaced -- the separately rounded chain through the world coordinates, 11 u of
// sum_j |k_j| A_j with A_j = sum_a |r[j][a]| (|offset_a| + (size_a + 1) vs_a) + |r[j][3]| -- and 8 u |u_c| for the reciprocal and the
// products from N_u to u_c in either form (in the numerator's units: times a depth, at most B_z), so that the box holds every pixel
// the earlier form's box held wherever both bounds hold.  That is `grow` = edge[0] + |u_c| lim[3]: added to S before the division by
// D_min, and as an absolute term to the half depth D_min is formed with.  For the bench view it is 4e-3 px at two metres; near the
// camera, where a constant margin was never an argument, it grows as 1 / D_min does.  On top of it the constant 0.05 px and the factor
// 1.0001 stay what they were: the reciprocals to an ulp, the products and sums from N_u to the box's edge (a dozen roundings of values
// below 2^16 px: 1e-2 px), and the projection itself, the double-precision inverse of the matrices the rays are formed with, in fp32.
struct CellBoxFast {          // five 16-byte rows: what a lane needs in front of z_near, read once per turn
    float nu[4], nv[4], dz[4];
    float lim[4];             // {half depth of the grown cell + its error term, z_near, scale = 0.5 (1 + 2 eps) 1.0001, grow per |u_c|}
    float edge[4];            // {grow of u, grow of v, width - 1, height - 1}  (the grow terms twice: they join S in front of scale)
};
struct CellBoxF3 {
    float x, y, z;
};
struct alignas(16) CellBoxConsts {
    CellBoxFast fast;
    // at or behind z_near: project_box<false> on the cell's corners, with the view's own matrices
    float r[3][4];
    float k[2][3];
    CellBoxF3 vs, offset;
    float e, z_clip, z_near;
    uint32_t width, height;
};
static_assert(sizeof(CellBoxFast) == 80 && sizeof(CellBoxConsts) % 16 == 0, "rows of 16 bytes");

template <class V>
TSDF_BOX_HD inline void cell_box_consts(CellBoxConsts &c, const V &ep, float vsx, float vsy, float vsz, uint32_t gx, uint32_t gy, uint32_t gz, float e) {
    // (one thread's work in front of a workgroup's first brick: fmas spelt out, no division)
    const double vs[3] = {vsx, vsy, vsz}, size[3] = {(double)gx, (double)gy, (double)gz};
    const double off[3] = {ep.offset.x, ep.offset.y, ep.offset.z};
    double t[3], m[3][3], a_[3], reach[3];   // camera coordinates of the cell l = 0's centre; per voxel along each axis; the bound A_j
#pragma unroll
    for (int a = 0; a < 3; a++) reach[a] = __builtin_fma(size[a] + 1.0, vs[a], fabs(off[a]));
#pragma unroll
    for (int j = 0; j < 3; j++) {
        t[j] = ep.r[j][3];
        a_[j] = fabs((double)ep.r[j][3]);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            m[j][a] = (double)ep.r[j][a] * vs[a];
            t[j] = __builtin_fma((double)ep.r[j][a], off[a] + vs[a], t[j]);
            a_[j] = __builtin_fma(fabs((double)ep.r[j][a]), reach[a], a_[j]);
        }
    }
    double b[3], old[2];   // B_u, B_v, B_z; the earlier form's sum_j |k_j| A_j
#pragma unroll
    for (int i = 0; i < 2; i++) {
        float *row = i == 0 ? c.fast.nu : c.fast.nv;
        const double k0 = ep.k[i][0], k1 = ep.k[i][1], k2 = ep.k[i][2];
        const double t_ = __builtin_fma(k2, t[2], __builtin_fma(k1, t[1], k0 * t[0]));
        row[0] = (float)t_;
        b[i] = fabs(t_);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double p = __builtin_fma(k2, m[2][a], __builtin_fma(k1, m[1][a], k0 * m[0][a]));
            row[1 + a] = (float)p;
            b[i] = __builtin_fma(size[a], fabs(p), b[i]);
        }
        old[i] = __builtin_fma(fabs(k2), a_[2], __builtin_fma(fabs(k1), a_[1], fabs(k0) * a_[0]));
    }
    c.fast.dz[0] = (float)t[2];
    b[2] = fabs(t[2]);
    double edges_z = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        c.fast.dz[1 + a] = (float)m[2][a];
        b[2] = __builtin_fma(size[a], fabs(m[2][a]), b[2]);
        edges_z += fabs(m[2][a]);
    }
    const double u = 1.0 / 16777216.0, up = 1.0 + 2.0 * u;   // (up: the conversions to float round either way)
    const double grown = 1.0 + 2.0 * (double)e, grow_z = u * __builtin_fma(5.0, b[2], 11.0 * a_[2]);
    c.fast.lim[0] = (float)(__builtin_fma(0.5 * grown, edges_z, grow_z) * up);
    c.fast.lim[1] = ep.z_near;
    c.fast.lim[2] = (float)(0.5 * grown * 1.0001);
    // (the grow terms join S in front of `scale`, which is above a half: twice them is at least them divided by it)
    c.fast.lim[3] = (float)(2.0 * up * u * __builtin_fma(13.0, b[2], 11.0 * a_[2]));
    c.fast.edge[0] = (float)(2.0 * up * u * __builtin_fma(5.0, b[0], 11.0 * old[0]));
    c.fast.edge[1] = (float)(2.0 * up * u * __builtin_fma(5.0, b[1], 11.0 * old[1]));
    c.fast.edge[2] = (float)(ep.width - 1u);
    c.fast.edge[3] = (float)(ep.height - 1u);
    for (int j = 0; j < 3; j++)
        for (int a = 0; a < 4; a++) c.r[j][a] = ep.r[j][a];
    for (int j = 0; j < 2; j++)
        for (int a = 0; a < 3; a++) c.k[j][a] = ep.k[j][a];
    c.vs = {vsx, vsy, vsz};
    c.offset = {ep.offset.x, ep.offset.y, ep.offset.z};
    c.e = e;
    c.z_clip = ep.z_clip;
    c.z_near = ep.z_near;
    c.width = ep.width;
    c.height = ep.height;
}

// the cell's box in front of z_near, from the five rows (in registers for the span of this call); false with `near` set: the cell
// comes within z_near of the camera plane and takes cell_box_near
TSDF_BOX_HD inline bool cell_box_front(const CellBoxFast &f, uint32_t lx, uint32_t ly, uint32_t lz, PixelBox &pb, bool &near) {
    const float fx = (float)lx, fy = (float)ly, fz = (float)lz;
    const float nu = __builtin_fmaf(fz, f.nu[3], __builtin_fmaf(fy, f.nu[2], __builtin_fmaf(fx, f.nu[1], f.nu[0])));
    const float nv = __builtin_fmaf(fz, f.nv[3], __builtin_fmaf(fy, f.nv[2], __builtin_fmaf(fx, f.nv[1], f.nv[0])));
    const float d = __builtin_fmaf(fz, f.dz[3], __builtin_fmaf(fy, f.dz[2], __builtin_fmaf(fx, f.dz[1], f.dz[0])));
    const float zmin = d - f.lim[0];
    near = !(zmin > f.lim[1]);
    if (near) return false;
    const float rz = box_rcp(d), rm = box_rcp(zmin) * f.lim[2];
    const float uc = nu * rz, vc = nv * rz;
    const float su = ((__builtin_fmaf(fabsf(uc), f.lim[3], f.edge[0]) + fabsf(__builtin_fmaf(-uc, f.dz[1], f.nu[1]))) + fabsf(__builtin_fmaf(-uc, f.dz[2], f.nu[2]))) + fabsf(__builtin_fmaf(-uc, f.dz[3], f.nu[3]));
    const float sv = ((__builtin_fmaf(fabsf(vc), f.lim[3], f.edge[1]) + fabsf(__builtin_fmaf(-vc, f.dz[1], f.nv[1]))) + fabsf(__builtin_fmaf(-vc, f.dz[2], f.nv[2]))) + fabsf(__builtin_fmaf(-vc, f.dz[3], f.nv[3]));
    // (a ray exists per INTEGER pixel)
    const float hu = __builtin_fmaf(su, rm, 0.05f), hv = __builtin_fmaf(sv, rm, 0.05f);
    const float a0 = fmaxf(ceilf(uc - hu), 0.0f), a1 = fminf(floorf(uc + hu), f.edge[2]);
    const float b0 = fmaxf(ceilf(vc - hv), 0.0f), b1 = fminf(floorf(vc + hv), f.edge[3]);
    if (!(a0 <= a1 && b0 <= b1)) return false;   // (also for anything not a number)
    pb.u0 = (int)a0; pb.v0 = (int)b0; pb.w = (int)a1 - (int)a0 + 1; pb.h = (int)b1 - (int)b0 + 1;
    return true;
}
// at or behind the plane in front of which the view's samples lie: the 8 corners, the part in front of the plane
TSDF_BOX_HD inline bool cell_box_near(const CellBoxConsts &c, uint32_t lx, uint32_t ly, uint32_t lz, PixelBox &pb) {
    const float e = c.e;
    const float clx = ((float)lx + 0.5f - e) * c.vs.x, chx = ((float)lx + 1.5f + e) * c.vs.x;
    const float cly = ((float)ly + 0.5f - e) * c.vs.y, chy = ((float)ly + 1.5f + e) * c.vs.y;
    const float clz = ((float)lz + 0.5f - e) * c.vs.z, chz = ((float)lz + 1.5f + e) * c.vs.z;
    return project_box<false>(c, clx, cly, clz, chx, chy, chz, pb);
}

}  // namespace tsdf
