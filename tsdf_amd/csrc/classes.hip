// Class fusion for gfx950: a per-voxel class id with a vote count beside the distances (include/tsdf_amd.h, "class fusion").
//
// Opt-in per volume, one dword per voxel, {class: bits 0-15, votes: bits 16-31}, x fastest like the distances; a word without votes
// is 0x00000000.  Colour (colour.hip) is the template: the same opt-in dword, the same band pass behind the integrate kernel over the
// frame's brick list, the same nearest-voxel sample.  Where colour blends, this votes: the weighted Boyer-Moore majority vote keeps
// one candidate and its lead, which fits the dword and needs one writer per word and no atomics.
//
// Three kernels:
//   class_integrate_kernel  runs behind the integrate kernel (and the colour pass, when there is one) of a tsdf_integrate_classes
//                           call, on the volume's stream, over the brick list brick_cull_kernel made for that frame.  It visits the
//                           voxels colour_integrate_kernel visits, with that kernel's fp32 expressions in that kernel's order, so the
//                           pixel and the sdf are the bits integrate computed; class words are read and written only in the band, and
//                           only where the pixel has a class and a strength.
//   class_sample_kernel     one thread per point: class and votes of the voxel the point lies in (tsdf_volume_sample_classes_device).
//   class_counts_kernel     voxels per class: a histogram of the class words, per workgroup in LDS where the classes fit, else
//                           straight to global integer atomics (tsdf_volume_class_counts_device).
#include <algorithm>
#include <cstring>

#include "class_voxel.hpp"
#include "common.hpp"
#include "integrate_grid.hpp"

namespace tsdf {

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

// One workgroup (64 x 4 lanes, one wave per row) per listed brick, walking its planes; a lane owns one (x, y) column
// (colour_integrate_kernel's walk and projection, colour.hip).
template <bool STD>
__global__ __launch_bounds__(256) void class_integrate_kernel(uint32_t *__restrict__ cls, const Geom g, const BrickGrid bg, const Mat44 ip,
                                                              const Mat33 k, const Mat33 kinv, const uint32_t width, const uint32_t height,
                                                              const uint16_t *__restrict__ depth, const uint16_t *__restrict__ classes,
                                                              const uint8_t *__restrict__ confidence, const uint32_t *__restrict__ list,
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
        if (!(rx >= 0.0f && rx < fwidth && ry >= 0.0f && ry < fheight)) continue;   // the frustum test
        const uint32_t px = (uint32_t)cvt_i32_sat(rx), py = (uint32_t)cvt_i32_sat(ry);
        const size_t pixel = (size_t)py * width + px;
        const uint32_t d = depth[pixel];
        if (d == 0) continue;
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
        // the distance update's set (sdf >= -trunc) without free space (sdf > +trunc): the colour update's set
        if (!(sdf >= neg_trunc && sdf <= g.trunc)) continue;
        const uint32_t kk = classes[pixel];
        const uint32_t s = confidence ? confidence[pixel] : 1u;
        if (kk == kClassVoid || s == 0) continue;   // the pixel says nothing: the word is not even read
        const uint32_t old = cls[idx];
        const uint32_t now = class_vote(old, kk, s);
        if (now != old) cls[idx] = now;   // (a saturated count stays as it is)
    }
}

// One thread per point: the voxel colour_sample_kernel reads -- i = (int)floorf(((p - offset) - offset_at_clear) / voxel_size) per
// axis (class_voxel.hpp, shared with objects.hip's lookup); (VOID, 0) for NaN, off-grid or unclassified (votes = 0) voxels.  votes
// may be null.
__global__ __launch_bounds__(256) void class_sample_kernel(const uint32_t *__restrict__ cls, const Geom g, const uint64_t n_points,
                                                           const float *__restrict__ points, uint16_t *__restrict__ classes,
                                                           uint16_t *__restrict__ votes) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_points) return;
    size_t at;
    const uint32_t w = class_voxel_at(g, points + 3 * i, at) ? cls[at] : 0u;
    const uint32_t n = w >> 16;
    classes[i] = (uint16_t)(n ? (w & 0xFFFFu) : kClassVoid);
    if (votes) votes[i] = (uint16_t)n;
}

// Voxels per class.  A grid-stride walk of the class words, a wave on 64 consecutive words per step.  LDS = true: a histogram of
// n_classes 32-bit bins per workgroup in LDS (a workgroup sees far fewer than 2^32 voxels), its non-zero bins added to the 64-bit counts
// at the end; LDS = false: straight to the counts in global memory, one add per wave and distinct class among its 64 words -- a scene's
// band holds a handful of classes, and 64 lanes adding 1 to the same three addresses serialise in the L2 (2.5 ms at 256^3 before the
// lanes were grouped).  Integer atomics either way: the counts are unique.
//
// The threshold (kClassCountsLdsBins) is 4096 bins = 16 KiB a workgroup.  A compute unit has 160 KiB of LDS and room for 32 waves =
// 8 workgroups of 256 lanes: at 16 KiB each the 8 of them take 128 KiB, so the histogram never costs a resident wave, and one more
// doubling would (32 KiB x 8 > 160 KiB).  Label sets of segmentation networks (tens to a few thousand classes) all fit.
constexpr uint32_t kClassCountsLdsBins = 4096;
constexpr uint32_t kClassCountsGrid = 2048;   // workgroups at most: 8 per compute unit

template <bool LDS>
__global__ __launch_bounds__(256) void class_counts_kernel(const uint32_t *__restrict__ cls, const size_t n_voxels, const uint32_t n_classes,
                                                           const uint32_t min_votes, unsigned long long *__restrict__ counts) {
    extern __shared__ uint32_t bins[];
    if (LDS) {
        for (uint32_t j = threadIdx.x; j < n_classes; j += 256u) bins[j] = 0;
        __syncthreads();
    }
    const size_t stride = (size_t)gridDim.x * 256u;
    const uint32_t lane = threadIdx.x & 63u;
    // (the loop's bounds are the wave's, not the lane's: every lane of a wave makes the same trips, the ballots below need that)
    for (size_t base = (size_t)blockIdx.x * 256u + (threadIdx.x - lane); base < n_voxels; base += stride) {
        const size_t i = base + lane;
        const uint32_t w = i < n_voxels ? cls[i] : 0u;
        const uint32_t c = w & 0xFFFFu;
        bool counted = (w >> 16) >= min_votes && c < n_classes;   // (min_votes >= 1: an unclassified word, and the tail's 0, never counts)
        if (LDS) {
            if (counted) atomicAdd(&bins[c], 1u);
        } else {
            unsigned long long left = __ballot(counted);
            while (left) {
                const int leader = __ffsll((long long)left) - 1;
                const uint32_t lc = (uint32_t)__shfl((int)c, leader);
                const bool mine = counted && c == lc;
                const unsigned long long group = __ballot(mine);
                if ((int)lane == leader) atomicAdd(&counts[lc], (unsigned long long)__popcll(group));
                if (mine) counted = false;
                left &= ~group;
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < n_classes; j += 256u) {
            const uint32_t m = bins[j];
            if (m) atomicAdd(&counts[j], (unsigned long long)m);
        }
    }
}

// integrate.hip calls this behind the integrate kernel (and the colour update) of the same frame
int launch_class_integrate(tsdf_volume *v, const BrickGrid &bg, const Mat44 &ip, const Mat33 &mk, const Mat33 &mkinv, bool std_camera,
                           uint32_t width, uint32_t height, const uint16_t *d_depth, const uint16_t *d_classes, const uint8_t *d_confidence,
                           const uint32_t *count) {
    // one workgroup per brick of the grid, as integrate's launch: those beyond the list's length leave at once
    const dim3 grid((unsigned)((size_t)bg.nx * bg.ny * bg.nz)), block(kTileX, kTileY, 1);
    if (std_camera)
        hipLaunchKernelGGL(class_integrate_kernel<true>, grid, block, 0, v->stream, v->classes, v->g, bg, ip, mk, mkinv, width, height,
                           d_depth, d_classes, d_confidence, v->brick_list, count);
    else
        hipLaunchKernelGGL(class_integrate_kernel<false>, grid, block, 0, v->stream, v->classes, v->g, bg, ip, mk, mkinv, width, height,
                           d_depth, d_classes, d_confidence, v->brick_list, count);
    TSDF_HIP(hipGetLastError(), "Class integrate kernel failed");
    return TSDF_OK;
}

int integrate_with_classes(tsdf_volume *v, const uint16_t *d_depth, const uint8_t *d_rgb, const uint16_t *d_classes,
                           const uint8_t *d_confidence, uint32_t width, uint32_t height, const float inv_pose[16], const float k[9],
                           const float kinv[9]);   // integrate.hip

static int sample_classes(const tsdf_volume *v, uint64_t n, const float *d_points, uint16_t *d_classes, uint16_t *d_votes,
                          hipStream_t stream) {
    if (n == 0) return TSDF_OK;
    const uint64_t blocks = (n + 255) / 256;
    TSDF_REQUIRE(blocks <= 0x7FFFFFFFull, "tsdf_volume_sample_classes: too many points");
    hipLaunchKernelGGL(class_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, v->classes, v->g, n, d_points, d_classes, d_votes);
    TSDF_HIP(hipGetLastError(), "Class sample kernel failed");
    return TSDF_OK;
}

static int require_classes(const tsdf_volume *v, const char *what) {
    TSDF_REQUIRE(v, "%s: null volume", what);
    TSDF_REQUIRE(v->classes, "%s: classes are not enabled on this volume (tsdf_volume_enable_classes)", what);
    return TSDF_OK;
}

// everything tsdf_integrate_classes* refuses, before anything is written
static int check_class_integrate(const tsdf_volume *v, const void *depth, const void *rgb, const void *classes, uint32_t width,
                                 uint32_t height, const float *inv_pose, const float *k, const float *kinv) {
    const int rc = require_classes(v, "tsdf_integrate_classes");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(depth && classes && inv_pose && k && kinv, "tsdf_integrate_classes: null argument");
    TSDF_REQUIRE(width > 0 && height > 0, "tsdf_integrate_classes: empty depth map");
    TSDF_REQUIRE(!v->nodes, "tsdf_integrate_classes: not supported once the deformation nodes are explicit (deformation() / set_deformation())");
    TSDF_REQUIRE(!rgb || v->colour, "tsdf_integrate_classes: rgb given but colour is not enabled on this volume (tsdf_volume_enable_colour)");
    return TSDF_OK;
}

}  // namespace tsdf

using namespace tsdf;

extern "C" {

int tsdf_volume_enable_classes(tsdf_volume *v, int enabled) {
    TSDF_REQUIRE(v, "tsdf_volume_enable_classes: null volume");
    if (!enabled) {
        if (v->classes) {
            TSDF_HIP(hipStreamSynchronize(v->stream), "class free");
            (void)hipFree(v->classes);
            v->classes = nullptr;
        }
        return TSDF_OK;
    }
    TSDF_REQUIRE(!v->slab, "tsdf_volume_enable_classes: classes are not supported on a Z-slab volume (tsdf_volume_create_slab)");
    if (v->classes) return TSDF_OK;
    const size_t bytes = v->resident_voxels() * sizeof(uint32_t);
    TSDF_HIP(hipMalloc((void **)&v->classes, bytes), "Couldn't allocate space for class data");
    const hipError_t e = hipMemsetAsync(v->classes, 0, bytes, v->stream);
    if (e != hipSuccess) {
        (void)hipFree(v->classes);
        v->classes = nullptr;
        return hip_fail(e, "Couldn't clear class data");
    }
    return TSDF_OK;
}

int tsdf_volume_classes_enabled(const tsdf_volume *v, int *enabled) {
    TSDF_REQUIRE(v && enabled, "tsdf_volume_classes_enabled: null argument");
    *enabled = v->classes ? 1 : 0;
    return TSDF_OK;
}

int tsdf_volume_classes(const tsdf_volume *v, uint32_t **device_ptr) {
    TSDF_REQUIRE(device_ptr, "tsdf_volume_classes: null argument");
    const int rc = require_classes(v, "tsdf_volume_classes");
    if (rc != TSDF_OK) return rc;
    *device_ptr = v->classes;
    return TSDF_OK;
}

int tsdf_volume_get_class_data(const tsdf_volume *v, uint32_t *host) {
    TSDF_REQUIRE(host, "tsdf_volume_get_class_data: null argument");
    const int rc = require_classes(v, "tsdf_volume_get_class_data");
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipMemcpyAsync(host, v->classes, v->resident_voxels() * sizeof(uint32_t), hipMemcpyDeviceToHost, v->stream),
             "Failed to copy class data from device");
    TSDF_HIP(hipStreamSynchronize(v->stream), "Failed to copy class data from device");
    return TSDF_OK;
}

int tsdf_volume_set_class_data(tsdf_volume *v, const uint32_t *host) {
    TSDF_REQUIRE(host, "tsdf_volume_set_class_data: null argument");
    const int rc = require_classes(v, "tsdf_volume_set_class_data");
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipMemcpyAsync(v->classes, host, v->resident_voxels() * sizeof(uint32_t), hipMemcpyHostToDevice, v->stream),
             "Failed to copy class data to device");
    TSDF_HIP(hipStreamSynchronize(v->stream), "Failed to copy class data to device");
    return TSDF_OK;
}

int tsdf_integrate_classes_device(tsdf_volume *v, const uint16_t *device_depth, const uint8_t *device_rgb, const uint16_t *device_classes,
                                  const uint8_t *device_confidence, uint32_t width, uint32_t height, const float pose[16],
                                  const float inv_pose[16], const float k[9], const float kinv[9]) {
    const int rc = check_class_integrate(v, device_depth, device_rgb, device_classes, width, height, inv_pose, k, kinv);
    if (rc != TSDF_OK) return rc;
    (void)pose;   // (as tsdf_integrate: the reference never reads it)
    return integrate_with_classes(v, device_depth, device_rgb, device_classes, device_confidence, width, height, inv_pose, k, kinv);
}

int tsdf_integrate_classes(tsdf_volume *v, const uint16_t *host_depth, const uint8_t *host_rgb, const uint16_t *host_classes,
                           const uint8_t *host_confidence, uint32_t width, uint32_t height, const float pose[16], const float inv_pose[16],
                           const float k[9], const float kinv[9]) {
    const int rc0 = check_class_integrate(v, host_depth, host_rgb, host_classes, width, height, inv_pose, k, kinv);
    if (rc0 != TSDF_OK) return rc0;
    const size_t pixels = (size_t)width * height;
    TSDF_HIP(device_reserve_bytes(v->depth_buf, v->depth_cap, pixels * sizeof(uint16_t)), "Couldn't allocate storage for depth map");
    TSDF_HIP(device_reserve(v->class_buf, v->class_cap, pixels), "Couldn't allocate storage for class frame");
    if (host_rgb) TSDF_HIP(device_reserve(v->rgb_buf, v->rgb_cap, pixels * 3), "Couldn't allocate storage for colour frame");
    if (host_confidence) TSDF_HIP(device_reserve(v->conf_buf, v->conf_cap, pixels), "Couldn't allocate storage for confidence frame");
    TSDF_HIP(hipMemcpyAsync(v->depth_buf, host_depth, pixels * sizeof(uint16_t), hipMemcpyHostToDevice, v->stream),
             "Failed to copy depth map to GPU");
    TSDF_HIP(hipMemcpyAsync(v->class_buf, host_classes, pixels * sizeof(uint16_t), hipMemcpyHostToDevice, v->stream),
             "Failed to copy class frame to GPU");
    if (host_rgb)
        TSDF_HIP(hipMemcpyAsync(v->rgb_buf, host_rgb, pixels * 3, hipMemcpyHostToDevice, v->stream), "Failed to copy colour frame to GPU");
    if (host_confidence)
        TSDF_HIP(hipMemcpyAsync(v->conf_buf, host_confidence, pixels, hipMemcpyHostToDevice, v->stream),
                 "Failed to copy confidence frame to GPU");
    const int rc = tsdf_integrate_classes_device(v, v->depth_buf, host_rgb ? v->rgb_buf : nullptr, v->class_buf,
                                                 host_confidence ? v->conf_buf : nullptr, width, height, pose, inv_pose, k, kinv);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipStreamSynchronize(v->stream), "Class integrate failed");
    return TSDF_OK;
}

int tsdf_volume_sample_classes_device(const tsdf_volume *v, uint64_t n, const float *device_points, uint16_t *device_classes,
                                      uint16_t *device_votes, void *hip_stream) {
    const int rc = require_classes(v, "tsdf_volume_sample_classes");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(n == 0 || (device_points && device_classes), "tsdf_volume_sample_classes: null argument");
    return sample_classes(v, n, device_points, device_classes, device_votes, (hipStream_t)hip_stream);
}

int tsdf_raycast_classes_device(const tsdf_volume *v, uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                                float *device_vertices, float *device_normals, uint16_t *device_classes, uint16_t *device_votes) {
    const int rc0 = require_classes(v, "tsdf_raycast_classes");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(device_vertices && device_classes, "tsdf_raycast_classes: null buffer");
    const int rc = tsdf_raycast_device(v, width, height, pose, kinv, device_vertices, device_normals);
    if (rc != TSDF_OK) return rc;
    return sample_classes(v, (uint64_t)width * height, device_vertices, device_classes, device_votes, v->stream);
}

int tsdf_raycast_classes(const tsdf_volume *cv, uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                         float *host_vertices, float *host_normals, uint16_t *host_classes, uint16_t *host_votes) {
    const int rc0 = require_classes(cv, "tsdf_raycast_classes");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(host_vertices && host_classes, "tsdf_raycast_classes: null buffer");
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);   // per-call temporaries are cached in the handle
    const size_t pixels = (size_t)width * height;
    // tsdf_raycast leaves the vertex map in the handle's vertex buffer: the classes are sampled from there, {classes, votes} into the
    // class upload buffer
    int rc = tsdf_raycast(v, width, height, pose, kinv, host_vertices, host_normals);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(device_reserve(v->class_buf, v->class_cap, 2 * pixels), "Couldn't allocate storage for class map");
    rc = sample_classes(v, pixels, v->vert_buf, v->class_buf, v->class_buf + pixels, v->stream);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipMemcpyAsync(host_classes, v->class_buf, pixels * sizeof(uint16_t), hipMemcpyDeviceToHost, v->stream), "Classes Memcpy failed");
    if (host_votes)
        TSDF_HIP(hipMemcpyAsync(host_votes, v->class_buf + pixels, pixels * sizeof(uint16_t), hipMemcpyDeviceToHost, v->stream),
                 "Classes Memcpy failed");
    TSDF_HIP(hipStreamSynchronize(v->stream), "Class sample failed");
    return TSDF_OK;
}

int tsdf_volume_class_counts_device(const tsdf_volume *v, uint32_t n_classes, uint32_t min_votes, uint64_t *device_counts, void *hip_stream) {
    const int rc = require_classes(v, "tsdf_volume_class_counts");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(device_counts, "tsdf_volume_class_counts: null argument");
    TSDF_REQUIRE(n_classes >= 1 && n_classes <= 65535u, "tsdf_volume_class_counts: n_classes %u is not in 1..65535", n_classes);
    const hipStream_t stream = (hipStream_t)hip_stream;
    const size_t n = v->resident_voxels();
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(device_counts);
    TSDF_HIP(hipMemsetAsync(counts, 0, (size_t)n_classes * sizeof(uint64_t), stream), "Couldn't clear the class counts");
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, kClassCountsGrid);
    const uint32_t votes = std::max(min_votes, 1u);
    if (n_classes <= kClassCountsLdsBins)
        hipLaunchKernelGGL(class_counts_kernel<true>, dim3(grid), dim3(256), n_classes * sizeof(uint32_t), stream, v->classes, n, n_classes,
                           votes, counts);
    else
        hipLaunchKernelGGL(class_counts_kernel<false>, dim3(grid), dim3(256), 0, stream, v->classes, n, n_classes, votes, counts);
    TSDF_HIP(hipGetLastError(), "Class counts kernel failed");
    return TSDF_OK;
}

int tsdf_volume_class_counts(const tsdf_volume *v, uint32_t n_classes, uint32_t min_votes, uint64_t *host_counts) {
    const int rc0 = require_classes(v, "tsdf_volume_class_counts");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(host_counts, "tsdf_volume_class_counts: null argument");
    TSDF_REQUIRE(n_classes >= 1 && n_classes <= 65535u, "tsdf_volume_class_counts: n_classes %u is not in 1..65535", n_classes);
    HostStage st;
    const size_t bytes = (size_t)n_classes * sizeof(uint64_t);
    int rc = st.begin(v->stream, bytes, "tsdf_volume_class_counts: couldn't allocate %zu bytes for the counts");
    if (rc != TSDF_OK) return rc;
    rc = tsdf_volume_class_counts_device(v, n_classes, min_votes, (uint64_t *)st.buf, v->stream);
    if (rc == TSDF_OK) st.down(host_counts, st.buf, bytes);
    return st.finish(rc, "Class counts failed");
}

}  // extern "C"
