// ICP tracking for gfx950 (wave64): the replacement of the reference's third_party/ICP_CUDA --
// pyrDown / createVMap / createNMap (Cuda/pyrdown.cu), estimateStep (Cuda/estimate.cu) and
// ICPOdometry::getIncrementalTransformation (ICPOdometry.cpp:97-136).
//
// What is different from the reference's shape, and why:
//   * The reference runs 19 iterations (10/5/4 over three pyramid levels), each = reduction kernel, second reduction
//     kernel, device synchronise, 116-byte download, 6x6 LDLT + SE3 exponential on the host, next launch.  Here the
//     pose lives on the device: every workgroup of icp_reduce_kernel first finishes the step before it -- adds up the partial
//     sums, solves the 6x6 system in double and applies T <- exp(x) * T -- so a frame is 19 launches and a finishing one
//     queued back to back with no host round trip; the host reads the pose once at the end.  That chain is gn_solve.hpp's,
//     shared with align.hip: this file supplies the projective association that makes a point's row, and the maps.
//   * The reduction is deterministic: a fixed grid, per-thread fp32 partial sums (as in the reference), wave64 shuffle
//     tree, fixed-order cross-wave and cross-block sums (the last stage in double).  The reference's sums depend on the
//     threads x blocks the caller passes; those two arguments are accepted and ignored.
//   * Maps keep the reference's planar layout (component c of pixel (x,y) at [(y + c*rows)*cols + x], NaN pattern
//     0x7fffffff in component 0 of an invalid pixel); lane <-> x, so every plane access is coalesced.
// Per-pixel arithmetic follows the reference's operation order with fp contraction off.
#include <cmath>
#include <cstring>
#include <new>

#include "common.hpp"
#include "gn_solve.hpp"   // the chain: gn_step_begin, gn_add_row, gn_block_sums, gn_finish_kernel, GnChain

struct tsdf_icp {
    int width, height;
    float cx, cy, fx, fy;
    float dist_thresh, angle_thresh;
    int device;
    hipStream_t stream;
    uint16_t *depth[3];                      // pyramid scratch (used by both init calls)
    uint16_t *upload;                        // the host variants' image on the device
    float *vmap_prev[3], *nmap_prev[3];      // model
    float *vmap_curr[3], *nmap_curr[3];      // current frame
    tsdf::GnChain chain;                     // state, partial sums and the pinned in/out block (its result 18 doubles wide)
};

namespace tsdf {

constexpr int kIcpLevels = 3;

__device__ inline float nan_sentinel() { return __uint_as_float(0x7fffffffu); }

// pyrDownGaussKernel (Cuda/pyrdown.cu:41-78), sigma_color = 30 (:87).  (The weighted sums are exact in fp32: the
// weights are multiples of 1/256 and the values 16-bit, so the order of the additions does not matter.)
__global__ __launch_bounds__(256) void icp_pyr_down_kernel(const uint16_t *__restrict__ src, int src_rows, int src_cols,
                                                           uint16_t *__restrict__ dst) {
    const int rows = src_rows / 2, cols = src_cols / 2;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    const int D = 5;
    const float sigma_color = 30;
    const int center = src[(size_t)(2 * y) * src_cols + 2 * x];
    const int x_mi = max(0, 2 * x - D / 2) - 2 * x, y_mi = max(0, 2 * y - D / 2) - 2 * y;
    const int x_ma = min(src_cols, 2 * x - D / 2 + D) - 2 * x, y_ma = min(src_rows, 2 * y - D / 2 + D) - 2 * y;
    float sum = 0, wall = 0;
    const float weights[3] = {0.375f, 0.25f, 0.0625f};
    // All 25 taps are requested at once, at clamped coordinates, and the taps outside [y_mi, y_ma) x [x_mi, x_ma) are left out of the
    // sums afterwards (the loop over the per-lane range was one dependent memory round trip per tap: 7-9 us for this kernel).
    int val_[D][D];
#pragma unroll
    for (int j = 0; j < D; j++)
#pragma unroll
        for (int i = 0; i < D; i++) {
            const int yi = min(max(j - D / 2, y_mi), y_ma - 1), xi = min(max(i - D / 2, x_mi), x_ma - 1);
            val_[j][i] = src[(size_t)(2 * y + yi) * src_cols + (2 * x + xi)];
        }
#pragma unroll
    for (int j = 0; j < D; j++)
#pragma unroll
        for (int i = 0; i < D; i++) {
            const int yi = j - D / 2, xi = i - D / 2, val = val_[j][i];
            if (yi >= y_mi && yi < y_ma && xi >= x_mi && xi < x_ma && abs(val - center) < 3 * sigma_color) {
                sum += val * weights[abs(xi)] * weights[abs(yi)];
                wall += weights[abs(xi)] * weights[abs(yi)];
            }
        }
    dst[(size_t)y * cols + x] = (uint16_t)(int)(sum / wall);
}

// computeVmapKernel (Cuda/pyrdown.cu:93-117) + computeNmapKernel (:135-172; Eigen's normalized(): n / sqrt(n.n) when n.n > 0) for all
// pyramid levels in ONE launch (blockIdx.z = level): a thread forms its own vertex and the two neighbours' its normal needs from the depth
// images with the same expressions -- the bits the reference's two kernels exchange through the vertex map -- so initICP is the pyramid (two launches) + this instead of a copy and nine launches
// (on the tracked loop's critical path for the model image: 18 us of launch chain).  Level 0 reads the caller's image and leaves
// the copy the pyramid scratch used to get from a memcpy.
struct IcpLevelMaps {
    const uint16_t *depth[3];
    float *vmap[3], *nmap[3];
    uint16_t *depth0_copy;
    int rows0, cols0;
    float fx, fy, cx, cy, depth_cutoff;
};
__device__ inline bool icp_vertex(const uint16_t *__restrict__ depth, int cols, int u, int v, float fx_inv, float fy_inv, float cx, float cy,
                                  float depth_cutoff, float &x, float &y, float &z) {
    z = depth[(size_t)v * cols + u] / 1000.f;  // mm -> metres
    if (!(z != 0 && z < depth_cutoff)) return false;
    x = z * (u - cx) * fx_inv;
    y = z * (v - cy) * fy_inv;
    return true;
}
__global__ __launch_bounds__(256) void icp_maps_kernel(const IcpLevelMaps m) {
    const int level = blockIdx.z, rows = m.rows0 >> level, cols = m.cols0 >> level, div = 1 << level;
    const int u = blockIdx.x * 64 + (threadIdx.x & 63), v = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u >= cols || v >= rows) return;
    // Intr::operator()(level): every intrinsic divided by 2^level (Cuda/internal.h:63-67); 1.f / fx: createVMap (:131)
    const float fx_inv = 1.f / (m.fx / div), fy_inv = 1.f / (m.fy / div), cx = m.cx / div, cy = m.cy / div;
    const uint16_t *depth = m.depth[level];
    float *vmap = m.vmap[level], *nmap = m.nmap[level];
    if (level == 0) m.depth0_copy[(size_t)v * cols + u] = depth[(size_t)v * cols + u];
    float a0, a1, a2;
    const bool a_ok = icp_vertex(depth, cols, u, v, fx_inv, fy_inv, cx, cy, m.depth_cutoff, a0, a1, a2);
    if (a_ok) {
        vmap[(size_t)v * cols + u] = a0;
        vmap[(size_t)(v + rows) * cols + u] = a1;
        vmap[(size_t)(v + rows * 2) * cols + u] = a2;
    } else {
        vmap[(size_t)v * cols + u] = nan_sentinel();
    }
    if (u == cols - 1 || v == rows - 1) {
        nmap[(size_t)v * cols + u] = nan_sentinel();
        return;
    }
    float b0, b1, b2, c0, c1, c2;
    const bool b_ok = icp_vertex(depth, cols, u + 1, v, fx_inv, fy_inv, cx, cy, m.depth_cutoff, b0, b1, b2);
    const bool c_ok = icp_vertex(depth, cols, u, v + 1, fx_inv, fy_inv, cx, cy, m.depth_cutoff, c0, c1, c2);
    if (a_ok && b_ok && c_ok) {
        const float px = b0 - a0, py = b1 - a1, pz = b2 - a2;
        const float qx = c0 - a0, qy = c1 - a1, qz = c2 - a2;
        float rx = py * qz - pz * qy, ry = pz * qx - px * qz, rz = px * qy - py * qx;
        const float z = rx * rx + ry * ry + rz * rz;
        if (z > 0.0f) {
            const float l = sqrtf(z);
            rx = rx / l;
            ry = ry / l;
            rz = rz / l;
        }
        nmap[(size_t)v * cols + u] = rx;
        nmap[(size_t)(v + rows) * cols + u] = ry;
        nmap[(size_t)(v + 2 * rows) * cols + u] = rz;
    } else {
        nmap[(size_t)v * cols + u] = nan_sentinel();
    }
}

// __float2int_rn: to nearest even, saturating, NaN -> 0
__device__ inline int float2int_rn(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return (-2147483647 - 1);
    return (int)rintf(f);
}

// Reduction::operator() (Cuda/estimate.cu:139-209): projective association of the current frame's vertices into the
// model, distance / angle gates, the row (n, v x n, n.(v_prev - v)) of every inlier into the thread's 29 sums, over this
// workgroup's share of the pixels at the pose R, t.  Per-pixel arithmetic as the reference's.
__device__ __forceinline__ void icp_accumulate(const float *R, const float *t, const float *__restrict__ vmap_curr, const float *__restrict__ nmap_curr,
                                               const float *__restrict__ vmap_prev, const float *__restrict__ nmap_prev, int rows, int cols,
                                               float fx, float fy, float cx, float cy, float dist_thresh, float angle_thresh, float *sum) {
    const int N = rows * cols;
    for (int i = blockIdx.x * kIcpThreads + threadIdx.x; i < N; i += kIcpThreads * gridDim.x) {
        const int y = i / cols, x = i - y * cols;
        const float v0 = vmap_curr[(size_t)y * cols + x], v1 = vmap_curr[(size_t)(y + rows) * cols + x],
                    v2 = vmap_curr[(size_t)(y + 2 * rows) * cols + x];
        const float p0 = ((R[0] * v0 + R[3] * v1) + R[6] * v2) + t[0];
        const float p1 = ((R[1] * v0 + R[4] * v1) + R[7] * v2) + t[1];
        const float p2 = ((R[2] * v0 + R[5] * v1) + R[8] * v2) + t[2];
        const int px = float2int_rn(p0 * fx / p2 + cx);
        const int py = float2int_rn(p1 * fy / p2 + cy);
        if (px >= 0 && py >= 0 && px < cols && py < rows && v2 > 0 && p2 > 0) {
            const float w0 = vmap_prev[(size_t)py * cols + px], w1 = vmap_prev[(size_t)(py + rows) * cols + px],
                        w2 = vmap_prev[(size_t)(py + 2 * rows) * cols + px];
            const float n0 = nmap_curr[(size_t)y * cols + x], n1 = nmap_curr[(size_t)(y + rows) * cols + x],
                        n2 = nmap_curr[(size_t)(y + 2 * rows) * cols + x];
            const float m0 = (R[0] * n0 + R[3] * n1) + R[6] * n2;
            const float m1 = (R[1] * n0 + R[4] * n1) + R[7] * n2;
            const float m2 = (R[2] * n0 + R[5] * n1) + R[8] * n2;
            const float q0 = nmap_prev[(size_t)py * cols + px], q1 = nmap_prev[(size_t)(py + rows) * cols + px],
                        q2 = nmap_prev[(size_t)(py + 2 * rows) * cols + px];
            const float c0 = m1 * q2 - m2 * q1, c1 = m2 * q0 - m0 * q2, c2 = m0 * q1 - m1 * q0;
            const float sine = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
            const float d0 = w0 - p0, d1 = w1 - p1, d2 = w2 - p2;
            const float dist = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
            if (sine < angle_thresh && dist < dist_thresh && !(n0 != n0) && !(q0 != q0)) {
                float row[7];
                row[0] = q0;
                row[1] = q1;
                row[2] = q2;
                row[3] = p1 * q2 - p2 * q1;
                row[4] = p2 * q0 - p0 * q2;
                row[5] = p0 * q1 - p1 * q0;
                row[6] = (q0 * d0 + q1 * d1) + q2 * d2;
                gn_add_row(row, sum);
            }
        }
    }
}

// One Gauss-Newton step's sums: gn_step_begin (the step before is finished by every workgroup of this launch), the rows, the
// workgroup's sums to partial[29] of this workgroup.
__global__ __launch_bounds__(kIcpThreads) void icp_reduce_kernel(const double *__restrict__ state_in, double *__restrict__ state_out,
                                                                const float *__restrict__ partial_prev, int pending,
                                                                const float *__restrict__ vmap_curr,
                                                                const float *__restrict__ nmap_curr,
                                                                const float *__restrict__ vmap_prev,
                                                                const float *__restrict__ nmap_prev, int rows, int cols,
                                                                float fx, float fy, float cx, float cy, float dist_thresh,
                                                                float angle_thresh, float *__restrict__ partial) {
    __shared__ double pose[16];
    float R[9], t[3];
    gn_step_begin(state_in, state_out, partial_prev, pending, (int)gridDim.x, 0.0f, pose, R, t);
    float sum[29];
#pragma unroll
    for (int i = 0; i < 29; i++) sum[i] = 0.0f;
    icp_accumulate(R, t, vmap_curr, nmap_curr, vmap_prev, nmap_prev, rows, cols, fx, fy, cx, cy, dist_thresh, angle_thresh, sum);
    gn_block_sums(sum, nullptr, partial);
}

static void free_icp(tsdf_icp *f) {
    for (int i = 0; i < kIcpLevels; i++) device_free_all(f->depth[i], f->vmap_prev[i], f->nmap_prev[i], f->vmap_curr[i], f->nmap_curr[i]);
    device_free_all(f->upload);
    f->chain.free();
    delete f;
}

// pyramid + vertex / normal maps of one depth image (device pointer; f->depth[0] gets a copy as a by-product of the maps launch)
static int build_maps(tsdf_icp *f, const uint16_t *depth0, float **vmaps, float **nmaps, float depth_cutoff) {
    for (int i = 1; i < kIcpLevels; i++) {
        const int src_rows = f->height >> (i - 1), src_cols = f->width >> (i - 1);
        dim3 grid((src_cols / 2 + 63) / 64, (src_rows / 2 + 3) / 4);
        hipLaunchKernelGGL(icp_pyr_down_kernel, grid, dim3(256), 0, f->stream, i == 1 ? depth0 : (const uint16_t *)f->depth[i - 1], src_rows, src_cols,
                           f->depth[i]);
    }
    static_assert(kIcpLevels == 3, "icp_maps_kernel carries three levels");
    IcpLevelMaps m;
    m.depth[0] = depth0;
    for (int i = 1; i < kIcpLevels; i++) m.depth[i] = f->depth[i];
    for (int i = 0; i < kIcpLevels; i++) {
        m.vmap[i] = vmaps[i];
        m.nmap[i] = nmaps[i];
    }
    m.depth0_copy = f->depth[0];
    m.rows0 = f->height;
    m.cols0 = f->width;
    m.fx = f->fx; m.fy = f->fy; m.cx = f->cx; m.cy = f->cy;
    m.depth_cutoff = depth_cutoff;
    hipLaunchKernelGGL(icp_maps_kernel, dim3((f->width + 63) / 64, (f->height + 3) / 4, kIcpLevels), dim3(256), 0, f->stream, m);
    TSDF_HIP(hipGetLastError(), "ICP map kernels failed");
    return TSDF_OK;
}

// Launches the sums of one step at `level`, taken at the pose the pending step (if any) leads to.
// `start` (pending == 0 only): where the pose to start from lies, if not in the device state (the host's pinned copy).
static void launch_step(tsdf_icp *f, int level, int pending, const double *start = nullptr) {
    const int rows = f->height >> level, cols = f->width >> level, div = 1 << level;
    GnChain &c = f->chain;
    hipLaunchKernelGGL(icp_reduce_kernel, dim3(kIcpBlocks), dim3(kIcpThreads), 0, f->stream, start ? start : c.state_in(), c.state_out(),
                       c.partial_in(), pending, f->vmap_curr[level], f->nmap_curr[level], f->vmap_prev[level], f->nmap_prev[level], rows, cols,
                       f->fx / div, f->fy / div, f->cx / div, f->cy / div, f->dist_thresh, f->angle_thresh, c.partial_out());
    c.flip();
}

void launch_gn_finish(hipStream_t stream, const double *state_in, double *state_out, const float *partial_prev, int n_blocks, int update,
                      double *mirror, const float *colour_weight) {
    if (colour_weight)
        hipLaunchKernelGGL(gn_finish_kernel<true>, dim3(1), dim3(kIcpThreads), 0, stream, state_in, state_out, partial_prev, n_blocks, update, *colour_weight, mirror);
    else
        hipLaunchKernelGGL(gn_finish_kernel<false>, dim3(1), dim3(kIcpThreads), 0, stream, state_in, state_out, partial_prev, n_blocks, update, 0.0f, mirror);
}

}  // namespace tsdf

using namespace tsdf;

extern "C" {

int tsdf_icp_create(int width, int height, float cx, float cy, float fx, float fy, float dist_thresh, float angle_thresh,
                    tsdf_icp **out) {
    TSDF_REQUIRE(out, "tsdf_icp_create: null argument");
    *out = nullptr;
    TSDF_REQUIRE(width >= 4 && height >= 4 && width <= 65535 && height <= 65535, "tsdf_icp_create: bad image size");
    tsdf_icp *f = new (std::nothrow) tsdf_icp();
    TSDF_REQUIRE(f, "out of host memory");
    std::memset(f, 0, sizeof(*f));
    f->width = width; f->height = height;
    f->cx = cx; f->cy = cy; f->fx = fx; f->fy = fy;
    f->dist_thresh = dist_thresh; f->angle_thresh = angle_thresh;
    hipError_t e = hipGetDevice(&f->device);
    for (int i = 0; i < kIcpLevels && e == hipSuccess; i++) {
        const size_t px = (size_t)(height >> i) * (width >> i);
        e = hipMalloc((void **)&f->depth[i], px * sizeof(uint16_t));
        float **maps[4] = {&f->vmap_prev[i], &f->nmap_prev[i], &f->vmap_curr[i], &f->nmap_curr[i]};
        for (int m = 0; m < 4 && e == hipSuccess; m++) {
            e = hipMalloc((void **)maps[m], px * 3 * sizeof(float));
            // the reference's maps start uninitialised and invalid pixels only ever get component 0 written: define the rest
            if (e == hipSuccess) e = hipMemset(*maps[m], 0, px * 3 * sizeof(float));
        }
    }
    if (e == hipSuccess) e = f->chain.alloc(18);
    if (e != hipSuccess) {
        free_icp(f);
        return hip_fail(e, "ICP alloc failed");
    }
    *out = f;
    return TSDF_OK;
}

void tsdf_icp_destroy(tsdf_icp *f) {
    if (f) free_icp(f);
}

int tsdf_icp_stream(const tsdf_icp *f, void **hip_stream) {
    TSDF_REQUIRE(f && hip_stream, "null argument");
    *hip_stream = f->stream;
    return TSDF_OK;
}

int tsdf_icp_set_stream(tsdf_icp *f, void *hip_stream) {
    TSDF_REQUIRE(f, "null ICP handle");
    f->stream = (hipStream_t)hip_stream;
    return TSDF_OK;
}

int tsdf_icp_init_device(tsdf_icp *f, int model, const uint16_t *device_depth, float depth_cutoff) {
    TSDF_REQUIRE(f && device_depth, "tsdf_icp_init: null argument");
    TSDF_REQUIRE(device_depth != f->depth[0], "tsdf_icp_init: the image must not be the pyramid's own level 0");
    return model ? build_maps(f, device_depth, f->vmap_prev, f->nmap_prev, depth_cutoff) : build_maps(f, device_depth, f->vmap_curr, f->nmap_curr, depth_cutoff);
}

int tsdf_icp_init(tsdf_icp *f, int model, const uint16_t *host_depth, float depth_cutoff) {
    TSDF_REQUIRE(f && host_depth, "tsdf_icp_init: null argument");
    if (!f->upload) TSDF_HIP(hipMalloc((void **)&f->upload, (size_t)f->width * f->height * sizeof(uint16_t)), "ICP upload buffer");
    TSDF_HIP(hipMemcpyAsync(f->upload, host_depth, (size_t)f->width * f->height * sizeof(uint16_t), hipMemcpyHostToDevice,
                            f->stream), "ICP depth upload");
    int rc = model ? build_maps(f, f->upload, f->vmap_prev, f->nmap_prev, depth_cutoff) : build_maps(f, f->upload, f->vmap_curr, f->nmap_curr, depth_cutoff);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipStreamSynchronize(f->stream), "ICP init");  // (the reference synchronises here too)
    return TSDF_OK;
}

int tsdf_icp_get_map(const tsdf_icp *f, int which, int level, float *host_map) {
    TSDF_REQUIRE(f && host_map && level >= 0 && level < kIcpLevels && which >= 0 && which < 4, "tsdf_icp_get_map: bad argument");
    const float *src[4] = {f->vmap_prev[level], f->nmap_prev[level], f->vmap_curr[level], f->nmap_curr[level]};
    const size_t bytes = (size_t)(f->height >> level) * (f->width >> level) * 3 * sizeof(float);
    TSDF_HIP(hipMemcpyAsync(host_map, src[which], bytes, hipMemcpyDeviceToHost, f->stream), "ICP map download");
    TSDF_HIP(hipStreamSynchronize(f->stream), "ICP map download");
    return TSDF_OK;
}

int tsdf_icp_get_depth_level(const tsdf_icp *f, int level, uint16_t *host_depth) {
    TSDF_REQUIRE(f && host_depth && level >= 0 && level < kIcpLevels, "tsdf_icp_get_depth_level: bad argument");
    const size_t bytes = (size_t)(f->height >> level) * (f->width >> level) * sizeof(uint16_t);
    TSDF_HIP(hipMemcpyAsync(host_depth, f->depth[level], bytes, hipMemcpyDeviceToHost, f->stream), "ICP depth download");
    TSDF_HIP(hipStreamSynchronize(f->stream), "ICP depth download");
    return TSDF_OK;
}

int tsdf_icp_estimate_step(tsdf_icp *f, int level, const float R[9], const float t[3], float A[36], float b[6],
                           float residual_inliers[2]) {
    TSDF_REQUIRE(f && R && t && A && b && residual_inliers && level >= 0 && level < kIcpLevels, "tsdf_icp_estimate_step: bad argument");
    double T[16] = {0};
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) T[c * 4 + r] = R[c * 3 + r];
    for (int r = 0; r < 3; r++) T[12 + r] = t[r];
    T[15] = 1.0;
    TSDF_HIP(hipMemcpyAsync(f->chain.state_in(), T, sizeof(T), hipMemcpyHostToDevice, f->stream), "ICP pose upload");
    launch_step(f, level, 0);
    f->chain.finish(f->stream, kIcpBlocks, 0, nullptr);
    TSDF_HIP(hipGetLastError(), "ICP estimate kernels failed");
    return f->chain.download(f->stream, A, b, residual_inliers, 1, "ICP result download", "ICP estimate");
}

int tsdf_icp_get_incremental_transformation(tsdf_icp *f, double T_prev_curr[16], float *last_error, float *last_inliers) {
    TSDF_REQUIRE(f && T_prev_curr, "tsdf_icp_get_incremental_transformation: null argument");
    const int iterations[kIcpLevels] = {10, 5, 4};  // ICPOdometry.cpp:99-101
    // The pose goes to the device and the result comes back through pinned host memory that the first and the last launch of the chain
    // address directly (every call ends with the stream idle, so the host may write it here): the two 128-byte copies were launches of
    // their own on the stream, 4-5 us each plus their boundaries, on the path every tracked frame waits for.
    std::memcpy(f->chain.host_io, T_prev_curr, 16 * sizeof(double));
    int pending = 0;   // every launch finishes the step before it, the last step gets a launch of its own
    for (int i = kIcpLevels - 1; i >= 0; i--)
        for (int j = 0; j < iterations[i]; j++) {
            launch_step(f, i, pending, pending ? nullptr : f->chain.host_io_dev);
            pending = 1;
        }
    f->chain.finish(f->stream, kIcpBlocks, 1, f->chain.host_io_dev + 16);
    TSDF_HIP(hipGetLastError(), "ICP kernels failed");
    TSDF_HIP(hipStreamSynchronize(f->stream), "ICP");   // (polling a ticket in the pinned block instead: 0.5-1 %, not kept)
    double out[18];
    std::memcpy(out, f->chain.host_io + 16, sizeof(out));
    std::memcpy(T_prev_curr, out, 16 * sizeof(double));
    // lastError = sqrt(residual) / inliers, lastInliers = inliers of the last iteration (ICPOdometry.cpp:127-128)
    if (last_error) *last_error = sqrtf((float)out[16]) / (float)out[17];
    if (last_inliers) *last_inliers = (float)out[17];
    return TSDF_OK;
}

int tsdf_selftest_gn_finish(const float *partial, int n_blocks, const double T_in[16], int update, double state_out[64]) {
    TSDF_REQUIRE(partial && T_in && state_out && n_blocks >= 1 && n_blocks <= kIcpBlocks, "tsdf_selftest_gn_finish: 1 .. 256 blocks of sums");
    // the whole buffer a step leaves, the blocks nobody wrote poisoned: the kernel must not let them into the sums
    float sums[kIcpBlocks * 32];
    for (int i = 0; i < kIcpBlocks * 32; i++) sums[i] = i < n_blocks * 32 ? partial[i] : 1.0e30f;
    double state[kIcpStateDoubles] = {0};
    std::memcpy(state, T_in, 16 * sizeof(double));
    float *sums_dev = nullptr;
    double *state_dev = nullptr;   // [0, 64) in, [64, 128) out
    hipError_t e = hipMalloc((void **)&sums_dev, sizeof(sums));
    if (e == hipSuccess) e = hipMalloc((void **)&state_dev, 2 * sizeof(state));
    if (e == hipSuccess) e = hipMemset(state_dev, 0, 2 * sizeof(state));
    if (e == hipSuccess) e = hipMemcpy(sums_dev, sums, sizeof(sums), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(state_dev, state, sizeof(state), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_gn_finish(nullptr, state_dev, state_dev + kIcpStateDoubles, sums_dev, n_blocks, update, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) e = hipMemcpy(state_out, state_dev + kIcpStateDoubles, sizeof(state), hipMemcpyDeviceToHost);
    device_free_all(sums_dev, state_dev);
    if (e != hipSuccess) return hip_fail(e, "tsdf_selftest_gn_finish");
    return TSDF_OK;
}

}  // extern "C"
