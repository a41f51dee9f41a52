// The band pass: one read-modify-write of a dword per voxel (colour.hip: {r, g, b, n}; classes.hip: {class, votes}) behind the integrate
// kernel of the same frame, on the volume's stream, over the brick list brick_cull_kernel made for that frame (integrate.hip).  It visits
// the voxels the distance update touched -- in the frustum, depth > 0, sdf >= -trunc (src/TSDF/TSDFVolume.cu:337-366) -- whose sdf is
// <= +trunc, and hands each one's word and the pixel whose depth integrate used to an Update policy.  The projection is integrate_kernel's:
// the same fp32 expressions in the same order (fp contraction is off, Makefile), round_quotients for the pixel, and for the standard
// camera the same dropped `0 * x` terms, so (u, v) and the sdf are the bits integrate computed.  Words are read and written only in the
// band, and only by the policy.
//
// The pixel index is formed in size_t; ColourBlend narrows it to 32 bits for its 3 * pixel.  The two differ only for images of 2^32
// pixels or more, which nothing here produces.
#pragma once

#include "common.hpp"
#include "integrate_grid.hpp"

namespace tsdf {

// the running average of colour.hip on one word: old = {r, g, b, n}, one observation (c0, c1, c2); each channel rounds half up, n
// saturates at 255
__device__ __forceinline__ uint32_t colour_blend(uint32_t old, uint32_t c0, uint32_t c1, uint32_t c2) {
    const uint32_t n = old >> 24, n1 = n + 1u, half = n1 >> 1;
    const uint32_t r = ((old & 0xFFu) * n + c0 + half) / n1;
    const uint32_t gg = (((old >> 8) & 0xFFu) * n + c1 + half) / n1;
    const uint32_t bb = (((old >> 16) & 0xFFu) * n + c2 + half) / n1;
    return r | (gg << 8) | (bb << 16) | (min(n1, 255u) << 24);
}

constexpr uint32_t kClassVoid = TSDF_CLASS_VOID;

// the vote of include/tsdf_amd.h on one word: old = {c, n}, an observation of class k with strength s >= 1, k != VOID
__device__ __forceinline__ uint32_t class_vote(uint32_t old, uint32_t k, uint32_t s) {
    const uint32_t c = old & 0xFFFFu, n = old >> 16;
    if (n == 0) return k | (s << 16);
    if (c == k) return k | (min(n + s, 65535u) << 16);
    if (n > s) return c | ((n - s) << 16);
    if (n == s) return 0u;
    return k | ((s - n) << 16);
}

// tsdf_integrate_colour: rgb is the frame, three bytes a pixel
struct ColourBlend {
    const uint8_t *rgb;
    __device__ __forceinline__ void operator()(uint32_t *word, size_t pixel) const {
        const uint32_t old = *word;
        const uint8_t *c = rgb + 3u * (uint32_t)pixel;
        *word = colour_blend(old, c[0], c[1], c[2]);
    }
};

// tsdf_integrate_classes: a class id per pixel and, unless null, a strength per pixel
struct ClassVote {
    const uint16_t *classes;
    const uint8_t *confidence;
    __device__ __forceinline__ void operator()(uint32_t *word, size_t pixel) const {
        const uint32_t kk = classes[pixel];
        const uint32_t s = confidence ? confidence[pixel] : 1u;
        if (kk == kClassVoid || s == 0) return;   // the pixel says nothing: the word is not even read
        const uint32_t old = *word;
        const uint32_t now = class_vote(old, kk, s);
        if (now != old) *word = now;   // (a saturated count stays as it is)
    }
};

// One workgroup (64 x 4 lanes, one wave per row) per listed brick, walking its planes; a lane owns one (x, y) column.
template <bool STD, class Update>
__global__ __launch_bounds__(256) void band_pass_kernel(uint32_t *__restrict__ words, const Geom g, const BrickGrid bg, const Mat44 ip,
                                                        const Mat33 k, const Mat33 kinv, const uint32_t width, const uint32_t height,
                                                        const uint16_t *__restrict__ depth, const Update up,
                                                        const uint32_t *__restrict__ list, const uint32_t *__restrict__ count) {
    const uint32_t i = blockIdx.x;
    if (i >= *count) return;
    const uint32_t b = list[i];
    const uint32_t bx = b % bg.nx, by = (b / bg.nx) % bg.ny, bz = b / (bg.nx * bg.ny);
    const uint32_t vx = bx * kTileX + threadIdx.x, vy = by * kTileY + threadIdx.y;
    if (vx >= g.X || vy >= g.Y) return;
    const uint32_t z0 = g.z_store_begin + bz * kChunkZ;
    const uint32_t z1 = min(z0 + kChunkZ + (bz + 1 == bg.nz ? bg.z_extra : 0u), g.z_store_end);   // exclusive
    const float neg_trunc = -g.trunc;
    const float fwidth = (float)width, fheight = (float)height;
    const float round_near_half = __uint_as_float(__float_as_uint(0.5f - 4.0e-7f * ((float)max(width, height) + 2.0f)) - 1u);
    // voxel centre (initialise_deformation, :783-785, then integrate_kernel's offset, :343) and the x / y parts of the row sums,
    // as integrate_kernel forms them
    const float cx = ((((int)vx + 0.5f) * g.vs.x) + g.offset_clear.x) + g.offset.x;
    const float cy = ((((int)vy + 0.5f) * g.vs.y) + g.offset_clear.y) + g.offset.y;
    const float r1 = ip.m11 * cx + ip.m12 * cy;
    const float r2 = ip.m21 * cx + ip.m22 * cy;
    const float r3 = ip.m31 * cx + ip.m32 * cy;
    const float r4 = ip.m41 * cx + ip.m42 * cy;
    const size_t plane = (size_t)g.X * g.Y;
    size_t idx = plane * (z0 - g.z_store_begin) + (size_t)g.X * vy + vx;
    for (uint32_t vz = z0; vz < z1; vz++, idx += plane) {
        const float cz = ((((int)vz + 0.5f) * g.vs.z) + g.offset_clear.z) + g.offset.z;
        const float camx = (r1 + ip.m13 * cz) + ip.m14;
        const float camy = (r2 + ip.m23 * cz) + ip.m24;
        const float camz = (r3 + ip.m33 * cz) + ip.m34;
        const float imx = STD ? k.m11 * camx + k.m13 * camz : k.m11 * camx + k.m12 * camy + k.m13 * camz;
        const float imy = STD ? k.m22 * camy + k.m23 * camz : k.m21 * camx + k.m22 * camy + k.m23 * camz;
        const float imz = STD ? camz : k.m31 * camx + k.m32 * camy + k.m33 * camz;
        float rx, ry;
        round_quotients(imx, imy, imz, round_near_half, rx, ry);
        if (!(rx >= 0.0f && rx < fwidth && ry >= 0.0f && ry < fheight)) continue;   // the frustum test (:349)
        const uint32_t px = (uint32_t)cvt_i32_sat(rx), py = (uint32_t)cvt_i32_sat(ry);
        const size_t pixel = (size_t)py * width + px;
        const uint32_t d = depth[pixel];
        if (d == 0) continue;   // (:355)
        float surf_z, voxel_cam_z;
        if (STD) {
            surf_z = (float)d;
            voxel_cam_z = camz;
        } else {
            const float ipz = kinv.m31 * (int)px + kinv.m32 * (int)py + kinv.m33;
            const float scale = (float)d / ipz;
            surf_z = ipz * scale;
            const float w = (r4 + ip.m43 * cz) + ip.m44;
            voxel_cam_z = camz / w;
        }
        const float sdf = surf_z - voxel_cam_z;
        // the distance update's set (sdf >= -trunc, :366) without free space (sdf > +trunc)
        if (!(sdf >= neg_trunc && sdf <= g.trunc)) continue;
        up(words + idx, pixel);
    }
}

// integrate.hip's launch_integrate calls this through launch_colour_integrate / launch_class_integrate, behind the integrate kernel of
// the same frame.  One workgroup per brick of the grid, as integrate's launch: those beyond the list's length leave at once.
template <class Update>
int launch_band_pass(tsdf_volume *v, uint32_t *words, const BrickGrid &bg, const Mat44 &ip, const Mat33 &mk, const Mat33 &mkinv,
                     bool std_camera, uint32_t width, uint32_t height, const uint16_t *d_depth, const Update &up, const uint32_t *count,
                     const char *what) {
    const dim3 grid((unsigned)((size_t)bg.nx * bg.ny * bg.nz)), block(kTileX, kTileY, 1);
    if (std_camera)
        hipLaunchKernelGGL((band_pass_kernel<true, Update>), grid, block, 0, v->stream, words, v->g, bg, ip, mk, mkinv, width, height, d_depth,
                           up, v->brick_list, count);
    else
        hipLaunchKernelGGL((band_pass_kernel<false, Update>), grid, block, 0, v->stream, words, v->g, bg, ip, mk, mkinv, width, height, d_depth,
                           up, v->brick_list, count);
    TSDF_HIP(hipGetLastError(), what);
    return TSDF_OK;
}

}  // namespace tsdf
