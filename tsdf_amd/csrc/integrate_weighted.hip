// Weighted integration for gfx950 (include/tsdf_amd.h, "weighted integration"; no reference counterpart: the reference's blend
// names current_weight and sets it to 1, src/TSDF/TSDFVolume.cu:375-381).
//
//   weight_mask_kernel    one lane per pixel: the frame's depth where the pixel's weight is finite and > 0, else 0, into scratch of the
//                         volume.  Everything behind it -- tile maxima, culling, the update test, the colour pass, the counters --
//                         then sees an invalid pixel exactly as a pixel without depth; the caller's arrays are only read.
//   depth_weights_kernel  one lane per pixel: the standard weight models (1 / z^2, cosine of the incidence angle) of a depth frame.
//   integrate_weighted_kernel lives in integrate.hip, beside the walk it shares (integrate_body.hpp).
#include <cmath>

#include "common.hpp"

namespace tsdf {

__global__ __launch_bounds__(256) void weight_mask_kernel(const uint16_t *__restrict__ depth, const float *__restrict__ pweight, const uint32_t n,
                                                          uint16_t *__restrict__ masked) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float p = pweight[i];
    masked[i] = (p > 0.0f && p < INFINITY) ? depth[i] : (uint16_t)0;   // (false for -0, negatives, NaN and both infinities)
}

// pixel_to_camera of pixel (px, py) at depth d, as depth_to_points_kernel (align.hip) forms it
__device__ inline F3 weights_point(const Mat33 &kinv, int px, int py, float d) {
    const float ipx = (kinv.m11 * px + kinv.m12 * py) + kinv.m13;
    const float ipy = (kinv.m21 * px + kinv.m22 * py) + kinv.m23;
    const float ipz = (kinv.m31 * px + kinv.m32 * py) + kinv.m33;
    const float scale = d / ipz;
    F3 r;
    r.x = ipx * scale;
    r.y = ipy * scale;
    r.z = ipz * scale;
    return r;
}

// The operation order is the header's (tsdf_depth_weights_device); tests/weighted_ref.py restates it in numpy.  A workgroup is four
// rows of 64 pixels: the five depth loads of a wave are three stretches of consecutive pixels of the rows y - 1, y, y + 1.
__global__ __launch_bounds__(256) void depth_weights_kernel(const uint16_t *__restrict__ depth, const uint32_t width, const uint32_t height,
                                                            const Mat33 kinv, const uint32_t flags, const float z_ref,
                                                            float *__restrict__ out) {
    const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= width || y >= height) return;
    const size_t i = (size_t)y * width + x;
    const uint32_t raw = depth[i];
    float w = raw != 0 ? 1.0f : 0.0f;
    if (raw != 0 && (flags & TSDF_WEIGHTS_INVERSE_SQUARE)) {
        const float r = z_ref / (float)raw;
        float f = r * r;
        f = f > 1.0f ? 1.0f : f;
        w = w * f;
    }
    if (raw != 0 && (flags & TSDF_WEIGHTS_COSINE)) {
        const bool inside = x > 0 && x + 1 < width && y > 0 && y + 1 < height;
        const uint32_t dl = inside ? depth[i - 1] : 0u, dr = inside ? depth[i + 1] : 0u;
        const uint32_t du = inside ? depth[i - width] : 0u, dd = inside ? depth[i + width] : 0u;
        float c = 0.0f;
        if (dl != 0 && dr != 0 && du != 0 && dd != 0) {
            const int px = (int)x, py = (int)y;
            const F3 P = weights_point(kinv, px, py, (float)raw);
            const F3 Pr = weights_point(kinv, px + 1, py, (float)dr), Pl = weights_point(kinv, px - 1, py, (float)dl);
            const F3 Pd = weights_point(kinv, px, py + 1, (float)dd), Pu = weights_point(kinv, px, py - 1, (float)du);
            const float ax = Pr.x - Pl.x, ay = Pr.y - Pl.y, az = Pr.z - Pl.z;
            const float bx = Pd.x - Pu.x, by = Pd.y - Pu.y, bz = Pd.z - Pu.z;
            const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
            const float np = (nx * P.x + ny * P.y) + nz * P.z;
            const float nn = (nx * nx + ny * ny) + nz * nz;
            const float pp = (P.x * P.x + P.y * P.y) + P.z * P.z;
            c = fabsf(np) / (sqrtf(nn) * sqrtf(pp));
            c = c > 1.0f ? 1.0f : c;
            if (!(c > 0.0f)) c = 0.0f;   // (a NaN too: a degenerate normal)
        }
        w = w * c;
    }
    out[i] = w;
}

static int weights_arguments(uint32_t width, uint32_t height, const void *depth, const float kinv[9], uint32_t flags, float z_ref, const void *weight) {
    TSDF_REQUIRE(depth && kinv && weight, "tsdf_depth_weights: null argument");
    TSDF_REQUIRE(width > 0 && height > 0 && width <= 65535 && height <= 65535, "tsdf_depth_weights: bad image size");
    TSDF_REQUIRE((flags & ~(uint32_t)(TSDF_WEIGHTS_INVERSE_SQUARE | TSDF_WEIGHTS_COSINE)) == 0, "tsdf_depth_weights: unknown flag bits %#x", flags);
    TSDF_REQUIRE(!(flags & TSDF_WEIGHTS_INVERSE_SQUARE) || (z_ref > 0.0f && z_ref < INFINITY),
                 "tsdf_depth_weights: z_ref must be finite and > 0 (depth units) for TSDF_WEIGHTS_INVERSE_SQUARE");
    return TSDF_OK;
}

}  // namespace tsdf

using namespace tsdf;

extern "C" {

int tsdf_depth_weights_device(uint32_t width, uint32_t height, const uint16_t *device_depth, const float kinv[9], uint32_t flags, float z_ref,
                              float *device_weight, void *hip_stream) {
    const int rc = weights_arguments(width, height, device_depth, kinv, flags, z_ref, device_weight);
    if (rc != TSDF_OK) return rc;
    Mat33 mkinv;
    memcpy(&mkinv, kinv, sizeof(mkinv));
    hipLaunchKernelGGL(depth_weights_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, (hipStream_t)hip_stream, device_depth, width,
                       height, mkinv, flags, z_ref, device_weight);
    TSDF_HIP(hipGetLastError(), "depth_weights kernel failed");
    return TSDF_OK;
}

int tsdf_depth_weights(uint32_t width, uint32_t height, const uint16_t *host_depth, const float kinv[9], uint32_t flags, float z_ref,
                       float *host_weight) {
    int rc = weights_arguments(width, height, host_depth, kinv, flags, z_ref, host_weight);
    if (rc != TSDF_OK) return rc;
    const size_t n = (size_t)width * height;
    HostStage st;
    rc = st.begin(nullptr, n * (sizeof(float) + sizeof(uint16_t)), "tsdf_depth_weights: couldn't allocate %zu bytes of device memory");
    if (rc != TSDF_OK) return rc;
    float *d_weight = static_cast<float *>(st.buf);
    uint16_t *d_depth = reinterpret_cast<uint16_t *>(d_weight + n);
    st.up(d_depth, host_depth, n * sizeof(uint16_t));
    if (st.ok()) rc = tsdf_depth_weights_device(width, height, d_depth, kinv, flags, z_ref, d_weight, nullptr);
    if (rc == TSDF_OK) st.down(host_weight, d_weight, n * sizeof(float));
    return st.finish(rc, "tsdf_depth_weights failed");
}

int tsdf_integrate_weighted_device(tsdf_volume *v, const uint16_t *device_depth, const float *device_pixel_weight, const uint8_t *device_rgb,
                                   uint32_t width, uint32_t height, const float pose[16], const float inv_pose[16], const float k[9],
                                   const float kinv[9]) {
    TSDF_REQUIRE(v && device_depth && device_pixel_weight && inv_pose && k && kinv, "tsdf_integrate_weighted: null argument");
    TSDF_REQUIRE(width > 0 && height > 0, "tsdf_integrate_weighted: empty depth map");
    TSDF_REQUIRE((uint64_t)width * height <= 0xFFFFFFFFull, "tsdf_integrate_weighted: the image has more than 2^32 - 1 pixels");
    if (device_rgb) {
        TSDF_REQUIRE(v->colour, "tsdf_integrate_weighted: colour is not enabled on this volume (tsdf_volume_enable_colour)");
        TSDF_REQUIRE(!v->nodes, "tsdf_integrate_weighted: colour is not supported once the deformation nodes are explicit (deformation() / set_deformation())");
    }
    (void)pose;   // (as tsdf_integrate: the reference never reads it)
    const uint32_t n = width * height;
    TSDF_HIP(device_reserve(v->wdepth_buf, v->wdepth_cap, (size_t)n), "Couldn't allocate storage for the masked depth map");
    hipLaunchKernelGGL(weight_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, v->stream, device_depth, device_pixel_weight, n, v->wdepth_buf);
    TSDF_HIP(hipGetLastError(), "weight mask kernel failed");
    // the volume goes to fp32 weights first (it stays there until clear(), as after any widening), then the usual culling,
    // integrate_weighted_kernel and -- with rgb -- the colour pass, all over the masked image
    const int rc = weights_require_f32(v);
    if (rc != TSDF_OK) return rc;
    IntegrateFrame f{v->wdepth_buf, width, height, inv_pose, k, kinv};
    f.pweight = device_pixel_weight;
    f.rgb = device_rgb;
    return launch_integrate(v, f);
}

int tsdf_integrate_weighted(tsdf_volume *v, const uint16_t *host_depth, const float *host_pixel_weight, const uint8_t *host_rgb, uint32_t width,
                            uint32_t height, const float pose[16], const float inv_pose[16], const float k[9], const float kinv[9]) {
    TSDF_REQUIRE(v && host_depth && host_pixel_weight && inv_pose && k && kinv, "tsdf_integrate_weighted: null argument");
    TSDF_REQUIRE(width > 0 && height > 0, "tsdf_integrate_weighted: empty depth map");
    TSDF_REQUIRE(!host_rgb || v->colour, "tsdf_integrate_weighted: colour is not enabled on this volume (tsdf_volume_enable_colour)");
    const size_t pixels = (size_t)width * height;
    TSDF_HIP(device_reserve_bytes(v->depth_buf, v->depth_cap, pixels * sizeof(uint16_t)), "Couldn't allocate storage for depth map");
    TSDF_HIP(device_reserve(v->pweight_buf, v->pweight_cap, pixels), "Couldn't allocate storage for the pixel weights");
    TSDF_HIP(hipMemcpyAsync(v->depth_buf, host_depth, pixels * sizeof(uint16_t), hipMemcpyHostToDevice, v->stream), "Failed to copy depth map to GPU");
    TSDF_HIP(hipMemcpyAsync(v->pweight_buf, host_pixel_weight, pixels * sizeof(float), hipMemcpyHostToDevice, v->stream),
             "Failed to copy the pixel weights to GPU");
    if (host_rgb) {
        TSDF_HIP(device_reserve(v->rgb_buf, v->rgb_cap, pixels * 3), "Couldn't allocate storage for colour frame");
        TSDF_HIP(hipMemcpyAsync(v->rgb_buf, host_rgb, pixels * 3, hipMemcpyHostToDevice, v->stream), "Failed to copy colour frame to GPU");
    }
    const int rc = tsdf_integrate_weighted_device(v, v->depth_buf, v->pweight_buf, host_rgb ? v->rgb_buf : nullptr, width, height, pose, inv_pose, k, kinv);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipStreamSynchronize(v->stream), "Weighted integrate failed");
    return TSDF_OK;
}

}  // extern "C"
