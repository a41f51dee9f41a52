// Colour fusion for gfx950: a per-voxel RGB average beside the distances (include/tsdf_amd.h, "colour fusion").
//
// The reference's volume carries a uchar3 colour per voxel (src/include/TSDFVolume.hpp:290-293) that no kernel of it writes;
// here colour is opt-in per volume and stored as one dword per voxel, {r, g, b, n} (r in bits 0-7, n = observations, saturating
// at 255, in bits 24-31), x fastest like the distances.  A dword instead of three bytes keeps every update a whole-word
// read-modify-write by one lane.
//
// The kernels:
//   band_pass_kernel<STD, ColourBlend>  (band_pass.hpp) runs right behind the integrate kernel of a tsdf_integrate_colour call: a voxel
//                            in the band blends the colour of the very pixel whose depth integrate used.
//   colour_sample_kernel     one thread per point: the colour of the voxel the point lies in (tsdf_volume_sample_colours_device),
//                            what ray casts and meshes are coloured with.
#include <cstring>

#include "band_pass.hpp"
#include "voxel_grid.hpp"
#include "voxel_words.hpp"

namespace tsdf {

// One thread per point: the voxel the point lies in (point_voxel_at, voxel_grid.hpp); (0, 0, 0) for NaN, off-grid or unobserved
// (n = 0) voxels.
__global__ __launch_bounds__(256) void colour_sample_kernel(const uint32_t *__restrict__ colour, const Geom g, const uint64_t n_points,
                                                            const float *__restrict__ points, uint8_t *__restrict__ rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_points) return;
    size_t at;
    uint32_t c = 0;
    if (point_voxel_at(g, points + 3 * i, at)) {
        const uint32_t w = colour[at];
        if (w >> 24) c = w;
    }
    rgb[3 * i + 0] = (uint8_t)c;
    rgb[3 * i + 1] = (uint8_t)(c >> 8);
    rgb[3 * i + 2] = (uint8_t)(c >> 16);
}

int launch_colour_integrate(tsdf_volume *v, const BrickGrid &bg, const Mat44 &ip, const Mat33 &mk, const Mat33 &mkinv, bool std_camera,
                            uint32_t width, uint32_t height, const uint16_t *d_depth, const uint8_t *d_rgb, const uint32_t *count) {
    return launch_band_pass(v, v->colour, bg, ip, mk, mkinv, std_camera, width, height, d_depth, ColourBlend{d_rgb}, count,
                            "Colour integrate kernel failed");
}

static int sample_colours(const tsdf_volume *v, uint64_t n, const float *d_points, uint8_t *d_rgb, hipStream_t stream) {
    if (n == 0) return TSDF_OK;
    const uint64_t blocks = (n + 255) / 256;
    TSDF_REQUIRE(blocks <= 0x7FFFFFFFull, "tsdf_volume_sample_colours: too many points");
    hipLaunchKernelGGL(colour_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, v->colour, v->g, n, d_points, d_rgb);
    TSDF_HIP(hipGetLastError(), "Colour sample kernel failed");
    return TSDF_OK;
}

constexpr VoxelWords kColourWords = {&tsdf_volume::colour,
                                     "%s: colour is not enabled on this volume (tsdf_volume_enable_colour)",
                                     "%s: colour is not supported on a Z-slab volume (tsdf_volume_create_slab)",
                                     "colour free", "Couldn't allocate space for colour data", "Couldn't clear colour data",
                                     "Failed to copy colour data to device", "Failed to copy colour data from device"};

}  // namespace tsdf

using namespace tsdf;

extern "C" {

int tsdf_volume_enable_colour(tsdf_volume *v, int enabled) { return voxel_words_enable(v, kColourWords, "tsdf_volume_enable_colour", enabled); }

int tsdf_volume_colour_enabled(const tsdf_volume *v, int *enabled) {
    return voxel_words_enabled(v, kColourWords, "tsdf_volume_colour_enabled", enabled);
}

int tsdf_volume_colours(const tsdf_volume *v, uint32_t **device_ptr) {
    return voxel_words_pointer(v, kColourWords, "tsdf_volume_colours", device_ptr);
}

int tsdf_volume_get_colour_data(const tsdf_volume *v, uint32_t *host) {
    return voxel_words_copy(v, kColourWords, "tsdf_volume_get_colour_data", host, nullptr);
}

int tsdf_volume_set_colour_data(tsdf_volume *v, const uint32_t *host) {
    return voxel_words_copy(v, kColourWords, "tsdf_volume_set_colour_data", nullptr, host);
}

int tsdf_integrate_colour_device(tsdf_volume *v, const uint16_t *device_depth, const uint8_t *device_rgb, uint32_t width,
                                 uint32_t height, const float pose[16], const float inv_pose[16], const float k[9],
                                 const float kinv[9]) {
    const int rc = voxel_words_require(v, kColourWords, "tsdf_integrate_colour");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(device_depth && device_rgb && inv_pose && k && kinv, "tsdf_integrate_colour: null argument");
    TSDF_REQUIRE(width > 0 && height > 0, "tsdf_integrate_colour: empty depth map");
    TSDF_REQUIRE(!v->nodes, "tsdf_integrate_colour: not supported once the deformation nodes are explicit (deformation() / set_deformation())");
    (void)pose;   // (as tsdf_integrate: the reference never reads it)
    IntegrateFrame f{device_depth, width, height, inv_pose, k, kinv};
    f.rgb = device_rgb;
    return launch_integrate(v, f);
}

int tsdf_integrate_colour(tsdf_volume *v, const uint16_t *host_depth, const uint8_t *host_rgb, uint32_t width, uint32_t height,
                          const float pose[16], const float inv_pose[16], const float k[9], const float kinv[9]) {
    const int rc0 = voxel_words_require(v, kColourWords, "tsdf_integrate_colour");
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
    const int rc = voxel_words_require(v, kColourWords, "tsdf_volume_sample_colours");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(n == 0 || (device_points && device_rgb), "tsdf_volume_sample_colours: null argument");
    return sample_colours(v, n, device_points, device_rgb, (hipStream_t)hip_stream);
}

int tsdf_raycast_colour_device(const tsdf_volume *v, uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                               float *device_vertices, float *device_normals, uint8_t *device_rgb) {
    const int rc0 = voxel_words_require(v, kColourWords, "tsdf_raycast_colour");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(device_vertices && device_rgb, "tsdf_raycast_colour: null buffer");
    const int rc = tsdf_raycast_device(v, width, height, pose, kinv, device_vertices, device_normals);
    if (rc != TSDF_OK) return rc;
    return sample_colours(v, (uint64_t)width * height, device_vertices, device_rgb, v->stream);
}

int tsdf_raycast_colour(const tsdf_volume *cv, uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                        float *host_vertices, float *host_normals, uint8_t *host_rgb) {
    const int rc0 = voxel_words_require(cv, kColourWords, "tsdf_raycast_colour");
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
