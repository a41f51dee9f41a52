// Colour fusion for gfx950: a per-voxel RGB average beside the distances (include/tsdf_amd.h, "colour fusion").
//
// The reference's volume carries a uchar3 colour per voxel (src/include/TSDFVolume.hpp:290-293) that no kernel of it writes;
// here colour is opt-in per volume and stored as one dword per voxel, {r, g, b, n} (r in bits 0-7, n = observations, saturating
// at 255, in bits 24-31), x fastest like the distances.  A dword instead of three bytes keeps every update a whole-word
// read-modify-write by one lane.
//
// Two kernels:
//   colour_integrate_kernel  runs right behind the integrate kernel of a tsdf_integrate_colour call, on the volume's stream, over
//                            the brick list brick_cull_kernel made for that frame (integrate.hip).  A voxel the distance update
//                            touched -- in the frustum, depth > 0, sdf >= -trunc (src/TSDF/TSDFVolume.cu:337-366) -- and whose
//                            sdf is <= +trunc blends the colour of the very pixel whose depth integrate used.  The projection
//                            is integrate_kernel's: the same fp32 expressions in the same order (fp contraction is off, Makefile),
//                            round_quotients for the pixel, and for the standard camera the same dropped `0 * x` terms, so (u, v)
//                            and the sdf are the bits integrate computed.  Colour words are read and written only in the band.
//   colour_sample_kernel     one thread per point: the colour of the voxel the point lies in (tsdf_volume_sample_colours_device),
//                            what ray casts and meshes are coloured with.
#include <cstring>

#include "common.hpp"
#include "integrate_grid.hpp"

namespace tsdf {

// One workgroup (64 x 4 lanes, one wave per row) per listed brick, walking its planes; a lane owns one (x, y) column.
template <bool STD>
__global__ __launch_bounds__(256) void colour_integrate_kernel(uint32_t *__restrict__ colour, const Geom g, const BrickGrid bg,
                                                               const Mat44 ip, const Mat33 k, const Mat33 kinv, const uint32_t width,
                                                               const uint32_t height, const uint16_t *__restrict__ depth,
                                                               const uint8_t *__restrict__ rgb, const uint32_t *__restrict__ list,
                                                               const uint32_t *__restrict__ count) {
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
        const uint32_t pixel = py * width + px;
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
        const uint32_t old = colour[idx];
        const uint32_t n = old >> 24, n1 = n + 1u, half = n1 >> 1;
        const uint8_t *c = rgb + 3u * pixel;
        const uint32_t r = ((old & 0xFFu) * n + c[0] + half) / n1;
        const uint32_t gg = (((old >> 8) & 0xFFu) * n + c[1] + half) / n1;
        const uint32_t bb = (((old >> 16) & 0xFFu) * n + c[2] + half) / n1;
        colour[idx] = r | (gg << 8) | (bb << 16) | (min(n1, 255u) << 24);
    }
}

// One thread per point: the voxel i = (int)floorf(((p - offset) - offset_at_clear) / voxel_size) per axis (the cell whose
// centre, as integrate forms it, is nearest); (0, 0, 0) for NaN, off-grid or unobserved (n = 0) voxels.
__global__ __launch_bounds__(256) void colour_sample_kernel(const uint32_t *__restrict__ colour, const Geom g, const uint64_t n_points,
                                                            const float *__restrict__ points, uint8_t *__restrict__ rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_points) return;
    const float fx = floorf(((points[3 * i + 0] - g.offset.x) - g.offset_clear.x) / g.vs.x);
    const float fy = floorf(((points[3 * i + 1] - g.offset.y) - g.offset_clear.y) / g.vs.y);
    const float fz = floorf(((points[3 * i + 2] - g.offset.z) - g.offset_clear.z) / g.vs.z);
    uint32_t c = 0;
    // (false for NaN; the grid's sides are below 2^16, so the bounds are exact floats)
    if (fx >= 0.0f && fx < (float)g.X && fy >= 0.0f && fy < (float)g.Y && fz >= (float)g.z_store_begin && fz < (float)g.z_store_end) {
        const uint32_t w = colour[((size_t)((uint32_t)fz - g.z_store_begin) * g.Y + (uint32_t)fy) * g.X + (uint32_t)fx];
        if (w >> 24) c = w;
    }
    rgb[3 * i + 0] = (uint8_t)c;
    rgb[3 * i + 1] = (uint8_t)(c >> 8);
    rgb[3 * i + 2] = (uint8_t)(c >> 16);
}

int launch_colour_integrate(tsdf_volume *v, const BrickGrid &bg, const Mat44 &ip, const Mat33 &mk, const Mat33 &mkinv, bool std_camera,
                            uint32_t width, uint32_t height, const uint16_t *d_depth, const uint8_t *d_rgb, const uint32_t *count) {
    // one workgroup per brick of the grid, as integrate's launch: those beyond the list's length leave at once
    const dim3 grid((unsigned)((size_t)bg.nx * bg.ny * bg.nz)), block(kTileX, kTileY, 1);
    if (std_camera)
        hipLaunchKernelGGL(colour_integrate_kernel<true>, grid, block, 0, v->stream, v->colour, v->g, bg, ip, mk, mkinv, width, height,
                           d_depth, d_rgb, v->brick_list, count);
    else
        hipLaunchKernelGGL(colour_integrate_kernel<false>, grid, block, 0, v->stream, v->colour, v->g, bg, ip, mk, mkinv, width, height,
                           d_depth, d_rgb, v->brick_list, count);
    TSDF_HIP(hipGetLastError(), "Colour integrate kernel failed");
    return TSDF_OK;
}

int integrate_with_colour(tsdf_volume *v, const uint16_t *d_depth, const uint8_t *d_rgb, uint32_t width, uint32_t height,
                          const float inv_pose[16], const float k[9], const float kinv[9], const uint16_t *tile_max);   // integrate.hip

static int sample_colours(const tsdf_volume *v, uint64_t n, const float *d_points, uint8_t *d_rgb, hipStream_t stream) {
    if (n == 0) return TSDF_OK;
    const uint64_t blocks = (n + 255) / 256;
    TSDF_REQUIRE(blocks <= 0x7FFFFFFFull, "tsdf_volume_sample_colours: too many points");
    hipLaunchKernelGGL(colour_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, v->colour, v->g, n, d_points, d_rgb);
    TSDF_HIP(hipGetLastError(), "Colour sample kernel failed");
    return TSDF_OK;
}

static int require_colour(const tsdf_volume *v, const char *what) {
    TSDF_REQUIRE(v, "%s: null volume", what);
    TSDF_REQUIRE(v->colour, "%s: colour is not enabled on this volume (tsdf_volume_enable_colour)", what);
    return TSDF_OK;
}

}  // namespace tsdf

using namespace tsdf;

extern "C" {

int tsdf_volume_enable_colour(tsdf_volume *v, int enabled) {
    TSDF_REQUIRE(v, "tsdf_volume_enable_colour: null volume");
    if (!enabled) {
        if (v->colour) {
            TSDF_HIP(hipStreamSynchronize(v->stream), "colour free");
            (void)hipFree(v->colour);
            v->colour = nullptr;
        }
        return TSDF_OK;
    }
    TSDF_REQUIRE(!v->slab, "tsdf_volume_enable_colour: colour is not supported on a Z-slab volume (tsdf_volume_create_slab)");
    if (v->colour) return TSDF_OK;
    const size_t bytes = v->resident_voxels() * sizeof(uint32_t);
    TSDF_HIP(hipMalloc((void **)&v->colour, bytes), "Couldn't allocate space for colour data");
    const hipError_t e = hipMemsetAsync(v->colour, 0, bytes, v->stream);
    if (e != hipSuccess) {
        (void)hipFree(v->colour);
        v->colour = nullptr;
        return hip_fail(e, "Couldn't clear colour data");
    }
    return TSDF_OK;
}

int tsdf_volume_colour_enabled(const tsdf_volume *v, int *enabled) {
    TSDF_REQUIRE(v && enabled, "tsdf_volume_colour_enabled: null argument");
    *enabled = v->colour ? 1 : 0;
    return TSDF_OK;
}

int tsdf_volume_colours(const tsdf_volume *v, uint32_t **device_ptr) {
    TSDF_REQUIRE(device_ptr, "tsdf_volume_colours: null argument");
    const int rc = require_colour(v, "tsdf_volume_colours");
    if (rc != TSDF_OK) return rc;
    *device_ptr = v->colour;
    return TSDF_OK;
}

int tsdf_volume_get_colour_data(const tsdf_volume *v, uint32_t *host) {
    TSDF_REQUIRE(host, "tsdf_volume_get_colour_data: null argument");
    const int rc = require_colour(v, "tsdf_volume_get_colour_data");
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipMemcpyAsync(host, v->colour, v->resident_voxels() * sizeof(uint32_t), hipMemcpyDeviceToHost, v->stream),
             "Failed to copy colour data from device");
    TSDF_HIP(hipStreamSynchronize(v->stream), "Failed to copy colour data from device");
    return TSDF_OK;
}

int tsdf_volume_set_colour_data(tsdf_volume *v, const uint32_t *host) {
    TSDF_REQUIRE(host, "tsdf_volume_set_colour_data: null argument");
    const int rc = require_colour(v, "tsdf_volume_set_colour_data");
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipMemcpyAsync(v->colour, host, v->resident_voxels() * sizeof(uint32_t), hipMemcpyHostToDevice, v->stream),
             "Failed to copy colour data to device");
    TSDF_HIP(hipStreamSynchronize(v->stream), "Failed to copy colour data to device");
    return TSDF_OK;
}

int tsdf_integrate_colour_device(tsdf_volume *v, const uint16_t *device_depth, const uint8_t *device_rgb, uint32_t width,
                                 uint32_t height, const float pose[16], const float inv_pose[16], const float k[9],
                                 const float kinv[9]) {
    const int rc = require_colour(v, "tsdf_integrate_colour");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(device_depth && device_rgb && inv_pose && k && kinv, "tsdf_integrate_colour: null argument");
    TSDF_REQUIRE(width > 0 && height > 0, "tsdf_integrate_colour: empty depth map");
    TSDF_REQUIRE(!v->nodes, "tsdf_integrate_colour: not supported once the deformation nodes are explicit (deformation() / set_deformation())");
    (void)pose;   // (as tsdf_integrate: the reference never reads it)
    return integrate_with_colour(v, device_depth, device_rgb, width, height, inv_pose, k, kinv, nullptr);
}

int tsdf_integrate_colour(tsdf_volume *v, const uint16_t *host_depth, const uint8_t *host_rgb, uint32_t width, uint32_t height,
                          const float pose[16], const float inv_pose[16], const float k[9], const float kinv[9]) {
    const int rc0 = require_colour(v, "tsdf_integrate_colour");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(host_depth && host_rgb && inv_pose && k && kinv, "tsdf_integrate_colour: null argument");
    TSDF_REQUIRE(width > 0 && height > 0, "tsdf_integrate_colour: empty depth map");
    TSDF_REQUIRE(!v->nodes, "tsdf_integrate_colour: not supported once the deformation nodes are explicit (deformation() / set_deformation())");
    const size_t pixels = (size_t)width * height;
    TSDF_HIP(device_reserve_bytes(v->depth_buf, v->depth_cap, pixels * sizeof(uint16_t)), "Couldn't allocate storage for depth map");
    TSDF_HIP(device_reserve(v->rgb_buf, v->rgb_cap, pixels * 3), "Couldn't allocate storage for colour frame");
    TSDF_HIP(hipMemcpyAsync(v->depth_buf, host_depth, pixels * sizeof(uint16_t), hipMemcpyHostToDevice, v->stream),
             "Failed to copy depth map to GPU");
    TSDF_HIP(hipMemcpyAsync(v->rgb_buf, host_rgb, pixels * 3, hipMemcpyHostToDevice, v->stream), "Failed to copy colour frame to GPU");
    const int rc = tsdf_integrate_colour_device(v, v->depth_buf, v->rgb_buf, width, height, pose, inv_pose, k, kinv);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipStreamSynchronize(v->stream), "Colour integrate failed");
    return TSDF_OK;
}

int tsdf_volume_sample_colours_device(const tsdf_volume *v, uint64_t n, const float *device_points, uint8_t *device_rgb,
                                      void *hip_stream) {
    const int rc = require_colour(v, "tsdf_volume_sample_colours");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(n == 0 || (device_points && device_rgb), "tsdf_volume_sample_colours: null argument");
    return sample_colours(v, n, device_points, device_rgb, (hipStream_t)hip_stream);
}

int tsdf_raycast_colour_device(const tsdf_volume *v, uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                               float *device_vertices, float *device_normals, uint8_t *device_rgb) {
    const int rc0 = require_colour(v, "tsdf_raycast_colour");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(device_vertices && device_rgb, "tsdf_raycast_colour: null buffer");
    const int rc = tsdf_raycast_device(v, width, height, pose, kinv, device_vertices, device_normals);
    if (rc != TSDF_OK) return rc;
    return sample_colours(v, (uint64_t)width * height, device_vertices, device_rgb, v->stream);
}

int tsdf_raycast_colour(const tsdf_volume *cv, uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                        float *host_vertices, float *host_normals, uint8_t *host_rgb) {
    const int rc0 = require_colour(cv, "tsdf_raycast_colour");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(host_vertices && host_rgb, "tsdf_raycast_colour: null buffer");
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);   // per-call temporaries are cached in the handle
    const size_t pixels = (size_t)width * height;
    // tsdf_raycast leaves the vertex map in the handle's vertex buffer: the colours are sampled from there
    int rc = tsdf_raycast(v, width, height, pose, kinv, host_vertices, host_normals);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(device_reserve(v->rgb_buf, v->rgb_cap, pixels * 3), "Couldn't allocate storage for colour map");
    rc = sample_colours(v, pixels, v->vert_buf, v->rgb_buf, v->stream);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipMemcpyAsync(host_rgb, v->rgb_buf, pixels * 3, hipMemcpyDeviceToHost, v->stream), "Colours Memcpy failed");
    TSDF_HIP(hipStreamSynchronize(v->stream), "Colour sample failed");
    return TSDF_OK;
}

}  // extern "C"
