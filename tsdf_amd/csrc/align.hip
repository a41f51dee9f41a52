// Field alignment for gfx950 (wave64): the rigid pose that puts a point set on the zero level of the fused field, by Gauss-Newton on
// sum S(T x)^2 (include/tsdf_amd.h, "field alignment"; Bylow et al. 2013, Canelhas' SDF tracker).  It is point-to-plane ICP with the
// association replaced by a trilinear sample: no ray cast, no model maps, no projective association.  No reference counterpart.
//
//   * One hot kernel, align_reduce_kernel: per point the pose product (ICP's expression), the field query of field.hip (the ray cast's
//     trilinear(), the central-difference gradient: seven samples), seven weight reads at the same points (field_sample.hpp), the row
//     (g, u x g, -d) and its 28 products + the inlier count, summed in icp_accumulate's order: per-thread fp32 over a strided share
//     of the points, the wave64 shuffle tree, the four waves in a fixed order.  B = min(256, ceil(n / 256)) workgroups.
//   * The chain is ICP's: every launch first finishes the step before it in every workgroup (icp_finish_step of gn_solve.hpp: second
//     reduction stage, 6 x 6 solve, T <- exp(x) T, the same bits in every workgroup), the last step gets icp_finish_kernel; the pose
//     goes in and comes out through a pinned coherent block, so a run is its launches and one synchronise.
//   * The pose is kept about the centre of the volume's box (the host shifts it in double both ways): the rotation columns of the
//     normal matrix are u x g, and with u measured from the world origin they would carry the distance to it.
// Nothing of the volume is written.  Per-point arithmetic is separately rounded fp32 (contraction is off).
#include <cmath>
#include <cstring>
#include <new>

#include "common.hpp"
#include "gn_solve.hpp"
#include "field_sample.hpp"

struct tsdf_aligner {
    int device;
    hipStream_t stream;
    float *partial;        // 2 x kIcpBlocks x 32 floats: per-workgroup sums of the 29 entries (two steps)
    double *state;         // device, 2 x kIcpStateDoubles, laid out as tsdf_icp's: [0..15] T_c, [16] residual, [17] inliers, [18..53] A, [54..59] b
    int side;              // which copy of state / partial holds the latest step
    double *host_io;       // pinned, coherent: [0..15] the pose a chain starts from, [16..33] its result (pose, residual, inliers)
    double *host_io_dev;
};

namespace tsdf {

constexpr int kAlignMaxStages = 8;

// the aligner's own constants of a call
struct AlignField {
    F3 h;          // the pivot: 0.5f * TriConst's max per axis
    float gate;
};

// The row of one point at the pose (R, t about the pivot); false for an outlier (row then undefined).
template <bool FASTDIV>
__device__ inline bool align_row(const float *R, const float *t, float x0, float x1, float x2, const FieldView &f, const AlignField &a,
                                 float *row) {
    const float u0 = ((R[0] * x0 + R[3] * x1) + R[6] * x2) + t[0];
    const float u1 = ((R[1] * x0 + R[4] * x1) + R[7] * x2) + t[1];
    const float u2 = ((R[2] * x0 + R[5] * x1) + R[8] * x2) + t[2];
    const FieldStencil s = field_stencil(f, u0 + a.h.x, u1 + a.h.y, u2 + a.h.z);
    if (!field_stencil_valid(f, s)) return false;
    // an unobserved neighbourhood holds the cleared distance, not a surface
    const float w0 = field_weight<FASTDIV>(f, s.x, s.y, s.z);
    const float w1 = field_weight<FASTDIV>(f, s.xp, s.y, s.z), w2 = field_weight<FASTDIV>(f, s.xm, s.y, s.z);
    const float w3 = field_weight<FASTDIV>(f, s.x, s.yp, s.z), w4 = field_weight<FASTDIV>(f, s.x, s.ym, s.z);
    const float w5 = field_weight<FASTDIV>(f, s.x, s.y, s.zp), w6 = field_weight<FASTDIV>(f, s.x, s.y, s.zm);
    if (!(w0 > 0.0f && w1 > 0.0f && w2 > 0.0f && w3 > 0.0f && w4 > 0.0f && w5 > 0.0f && w6 > 0.0f)) return false;
    const float d = field_distance<FASTDIV>(f, s.x, s.y, s.z);
    float gx, gy, gz;
    field_gradient<FASTDIV>(f, s, gx, gy, gz);
    const float inf = INFINITY;
    if (!(fabsf(d) < inf && fabsf(gx) < inf && fabsf(gy) < inf && fabsf(gz) < inf)) return false;   // (false for NaN)
    if (!(fabsf(d) < a.gate)) return false;
    if (!((gx * gx + gy * gy) + gz * gz > 0.0f)) return false;
    row[0] = gx;
    row[1] = gy;
    row[2] = gz;
    row[3] = u1 * gz - u2 * gy;
    row[4] = u2 * gx - u0 * gz;
    row[5] = u0 * gy - u1 * gx;
    row[6] = -d;
    return true;
}

// One Gauss-Newton step's sums over `n` points (3 floats each).  `pending` != 0: the launch before left the sums of its
// `prev_blocks` workgroups in partial_prev and the pose they were taken at in state_in; every workgroup finishes that step first
// (icp_reduce_kernel's prologue).  ROWS: also the row of every point (seven floats, the NaN row for an outlier) to `rows`: the
// tests' hook for the per-point arithmetic; the instance without it has none of that code.
template <bool FASTDIV, bool ROWS>
__global__ __launch_bounds__(kIcpThreads) void align_reduce_kernel(const double *__restrict__ state_in, double *__restrict__ state_out,
                                                                  const float *__restrict__ partial_prev, int pending, int prev_blocks,
                                                                  const FieldView f, const AlignField a, const uint32_t n,
                                                                  const float *__restrict__ points, float *__restrict__ rows,
                                                                  float *__restrict__ partial) {
    __shared__ double pose[16];
    if (pending) {
        icp_finish_step(partial_prev, prev_blocks, state_in, 1, pose, blockIdx.x == 0 ? state_out : nullptr);
    } else {
        if (threadIdx.x < 16) {
            pose[threadIdx.x] = state_in[threadIdx.x];
            if (blockIdx.x == 0) state_out[threadIdx.x] = state_in[threadIdx.x];
        }
    }
    __syncthreads();
    __shared__ float shared[4][32];
    float R[9], t[3];  // column-major
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) R[c * 3 + r] = (float)pose[c * 4 + r];
    for (int r = 0; r < 3; r++) t[r] = (float)pose[12 + r];

    float sum[29];
#pragma unroll
    for (int i = 0; i < 29; i++) sum[i] = 0.0f;
    const uint32_t stride = (uint32_t)kIcpThreads * gridDim.x;   // <= 65536
    for (uint64_t i = (uint64_t)blockIdx.x * kIcpThreads + threadIdx.x; i < n; i += stride) {
        float row[7];
        const bool in = align_row<FASTDIV>(R, t, points[3 * i + 0], points[3 * i + 1], points[3 * i + 2], f, a, row);
        if (ROWS) {
#pragma unroll
            for (int k = 0; k < 7; k++) rows[7 * i + k] = in ? row[k] : NAN;
        }
        if (in) {
            int s = 0;
#pragma unroll
            for (int o = 0; o < 7; o++)
#pragma unroll
                for (int k = o; k < 7; k++) sum[s++] += row[o] * row[k];
            sum[28] += 1.0f;
        }
    }
    // wave64 shuffle tree, then the four waves of the workgroup in a fixed order (icp_accumulate's)
#pragma unroll
    for (int i = 0; i < 29; i++) {
        float v = sum[i];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        sum[i] = v;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 29; i++) shared[wave][i] = sum[i];
    }
    __syncthreads();
    if (threadIdx.x < 29) {
        partial[blockIdx.x * 32 + threadIdx.x] =
            ((shared[0][threadIdx.x] + shared[1][threadIdx.x]) + shared[2][threadIdx.x]) + shared[3][threadIdx.x];
    }
}

// orc-style pixel_to_camera of every step-th pixel: (kinv * (x, y, 1)) * (depth / its z), the NaN triple for depth 0 or above the cutoff
__global__ __launch_bounds__(256) void depth_to_points_kernel(const uint16_t *__restrict__ depth, uint32_t width, uint32_t out_w,
                                                              uint32_t out_h, uint32_t step, const Mat33 kinv, float depth_cutoff,
                                                              float *__restrict__ points) {
    const uint32_t ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= out_w || oy >= out_h) return;
    const int px = (int)(ox * step), py = (int)(oy * step);
    const uint16_t raw = depth[(size_t)py * width + (uint32_t)px];
    const float d = (float)raw;
    float *out = points + 3 * ((size_t)oy * out_w + ox);
    if (raw == 0 || d > depth_cutoff) {
        out[0] = out[1] = out[2] = NAN;
        return;
    }
    const float ipx = (kinv.m11 * px + kinv.m12 * py) + kinv.m13;
    const float ipy = (kinv.m21 * px + kinv.m22 * py) + kinv.m23;
    const float ipz = (kinv.m31 * px + kinv.m32 * py) + kinv.m33;
    const float scale = d / ipz;
    out[0] = ipx * scale;
    out[1] = ipy * scale;
    out[2] = ipz * scale;
}

static void free_aligner(tsdf_aligner *a) {
    device_free_all(a->partial, a->state);
    (void)hipHostFree(a->host_io);
    delete a;
}

static int align_blocks(uint32_t n) {
    const uint32_t b = (n + (uint32_t)kIcpThreads - 1u) / (uint32_t)kIcpThreads;   // n <= 2^32 - 1: no overflow in uint64
    return (int)(b < (uint32_t)kIcpBlocks ? b : (uint32_t)kIcpBlocks);
}

// everything a launch needs of the volume, formed once per call
struct AlignSetup {
    FieldView f;
    AlignField a;
    double pivot[3];   // offset + h: subtracted from the caller's translation on the way in, added on the way out
    int fast_div;
};

static int align_setup(const tsdf_aligner *a, const tsdf_volume *v, const double *T, float gate, const char *what, AlignSetup &s) {
    TSDF_REQUIRE(a && v && T, "%s: null argument", what);
    const int rc = field_refuse_slab(v, what);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(v->device == a->device, "%s: the volume (device %d) and the aligner (device %d) are on different devices", what, v->device, a->device);
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 3; r++) TSDF_REQUIRE(std::isfinite(T[c * 4 + r]), "%s: T has a non-finite entry in its top three rows", what);
    TSDF_REQUIRE(gate > 0.0f, "%s: the gate must be > 0", what);   // (false for NaN)
    s.f = make_field_view(v);
    s.a.h = {0.5f * s.f.tc.max_x, 0.5f * s.f.tc.max_y, 0.5f * s.f.tc.max_z};
    s.a.gate = gate;
    s.pivot[0] = (double)v->g.offset.x + (double)s.a.h.x;
    s.pivot[1] = (double)v->g.offset.y + (double)s.a.h.y;
    s.pivot[2] = (double)v->g.offset.z + (double)s.a.h.z;
    s.fast_div = v->fast_div;
    return TSDF_OK;
}

// T (the caller's, points' frame -> the frame of the field queries) -> T_c about the pivot, into the pinned block
static void align_pose_in(tsdf_aligner *a, const AlignSetup &s, const double *T) {
    double *io = a->host_io;
    for (int c = 0; c < 4; c++) {
        for (int r = 0; r < 3; r++) io[c * 4 + r] = T[c * 4 + r];
        io[c * 4 + 3] = c == 3 ? 1.0 : 0.0;
    }
    for (int r = 0; r < 3; r++) io[12 + r] = T[12 + r] - s.pivot[r];
}

// The sums of one step over `n` > 0 points at the pose the pending step (if any) leads to.
static void launch_align_step(tsdf_aligner *a, const AlignSetup &s, uint32_t n, const float *points, float *rows, int pending, int prev_blocks,
                              const double *start) {
    const int in = a->side, out = 1 - a->side;
    const double *state_in = start ? start : a->state + in * kIcpStateDoubles;
    double *state_out = a->state + out * kIcpStateDoubles;
    const float *partial_prev = a->partial + (size_t)in * kIcpBlocks * 32;
    float *partial = a->partial + (size_t)out * kIcpBlocks * 32;
    const dim3 grid((unsigned)align_blocks(n)), block(kIcpThreads);
#define TSDF_ALIGN_LAUNCH(FD, RW) \
    hipLaunchKernelGGL((align_reduce_kernel<FD, RW>), grid, block, 0, a->stream, state_in, state_out, partial_prev, pending, prev_blocks, s.f, s.a, n, points, rows, partial)
    if (rows) {
        if (s.fast_div) TSDF_ALIGN_LAUNCH(true, true);
        else TSDF_ALIGN_LAUNCH(false, true);
    } else {
        if (s.fast_div) TSDF_ALIGN_LAUNCH(true, false);
        else TSDF_ALIGN_LAUNCH(false, false);
    }
#undef TSDF_ALIGN_LAUNCH
    a->side = out;
}

static void launch_align_finish(tsdf_aligner *a, int n_blocks, int update, double *mirror) {
    const int in = a->side, out = 1 - a->side;
    launch_gn_finish(a->stream, a->state + in * kIcpStateDoubles, a->state + out * kIcpStateDoubles, a->partial + (size_t)in * kIcpBlocks * 32,
                     n_blocks, update, mirror);
    a->side = out;
}

}  // namespace tsdf

using namespace tsdf;

extern "C" {

int tsdf_aligner_create(tsdf_aligner **out) {
    TSDF_REQUIRE(out, "tsdf_aligner_create: null argument");
    *out = nullptr;
    tsdf_aligner *a = new (std::nothrow) tsdf_aligner();
    if (!a) {
        set_error("out of host memory");
        return TSDF_ERR_NOMEM;
    }
    std::memset(a, 0, sizeof(*a));
    hipError_t e = hipGetDevice(&a->device);
    if (e == hipSuccess) e = hipMalloc((void **)&a->partial, (size_t)2 * kIcpBlocks * 32 * sizeof(float));
    if (e == hipSuccess) e = hipMemset(a->partial, 0, (size_t)2 * kIcpBlocks * 32 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&a->state, 2 * kIcpStateDoubles * sizeof(double));
    if (e == hipSuccess) e = hipMemset(a->state, 0, 2 * kIcpStateDoubles * sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc((void **)&a->host_io, (16 + 18) * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) std::memset(a->host_io, 0, (16 + 18) * sizeof(double));
    if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&a->host_io_dev, a->host_io, 0);
    if (e != hipSuccess) {
        free_aligner(a);
        return hip_fail(e, "aligner alloc failed");
    }
    *out = a;
    return TSDF_OK;
}

void tsdf_aligner_destroy(tsdf_aligner *a) {
    if (a) free_aligner(a);   // (every call ends with the stream idle: nothing of the aligner's is in flight)
}

int tsdf_aligner_set_stream(tsdf_aligner *a, void *hip_stream) {
    TSDF_REQUIRE(a, "null aligner");
    a->stream = (hipStream_t)hip_stream;
    return TSDF_OK;
}

int tsdf_aligner_stream(const tsdf_aligner *a, void **hip_stream) {
    TSDF_REQUIRE(a && hip_stream, "null argument");
    *hip_stream = a->stream;
    return TSDF_OK;
}

int tsdf_aligner_step(tsdf_aligner *a, const tsdf_volume *v, uint32_t n, const float *device_points, const double T[16], float gate,
                      float A[36], float b[6], float residual_inliers[2], float *device_rows) {
    TSDF_REQUIRE(A && b && residual_inliers, "tsdf_aligner_step: null argument");
    TSDF_REQUIRE(n == 0 || device_points, "tsdf_aligner_step: null points");
    AlignSetup s;
    const int rc = align_setup(a, v, T, gate, "tsdf_aligner_step", s);
    if (rc != TSDF_OK) return rc;
    if (n == 0) {
        std::memset(A, 0, 36 * sizeof(float));
        std::memset(b, 0, 6 * sizeof(float));
        residual_inliers[0] = residual_inliers[1] = 0.0f;
        return TSDF_OK;
    }
    align_pose_in(a, s, T);
    launch_align_step(a, s, n, device_points, device_rows, 0, 0, a->host_io_dev);
    launch_align_finish(a, align_blocks(n), 0, nullptr);
    TSDF_HIP(hipGetLastError(), "align kernels failed");
    double out[kIcpStateDoubles];
    TSDF_HIP(hipMemcpyAsync(out, a->state + a->side * kIcpStateDoubles, sizeof(out), hipMemcpyDeviceToHost, a->stream), "align result download");
    TSDF_HIP(hipStreamSynchronize(a->stream), "align step");
    residual_inliers[0] = (float)out[16];
    residual_inliers[1] = (float)out[17];
    for (int i = 0; i < 36; i++) A[i] = (float)out[18 + i];
    for (int i = 0; i < 6; i++) b[i] = (float)out[54 + i];
    return TSDF_OK;
}

int tsdf_aligner_run(tsdf_aligner *a, const tsdf_volume *v, uint32_t n_stages, const tsdf_align_stage *stages, float gate, double T[16],
                     float *residual, float *inliers) {
    TSDF_REQUIRE(n_stages <= (uint32_t)kAlignMaxStages, "tsdf_aligner_run: more than %d stages", kAlignMaxStages);
    TSDF_REQUIRE(n_stages == 0 || stages, "tsdf_aligner_run: null stages");
    for (uint32_t i = 0; i < n_stages; i++)
        TSDF_REQUIRE(stages[i].n == 0 || stages[i].iterations == 0 || stages[i].device_points, "tsdf_aligner_run: stage %u has null points", i);
    AlignSetup s;
    const int rc = align_setup(a, v, T, gate, "tsdf_aligner_run", s);
    if (rc != TSDF_OK) return rc;
    // The pose goes to the device and the result comes back through the pinned block (every call ends with the stream idle, so the
    // host may write it here), as tsdf_icp_get_incremental_transformation does.
    align_pose_in(a, s, T);
    int pending = 0, prev_blocks = 0;   // every launch finishes the step before it, the last step gets a launch of its own
    for (uint32_t i = 0; i < n_stages; i++) {
        if (stages[i].n == 0) continue;
        for (uint32_t j = 0; j < stages[i].iterations; j++) {
            launch_align_step(a, s, stages[i].n, stages[i].device_points, nullptr, pending, prev_blocks, pending ? nullptr : a->host_io_dev);
            pending = 1;
            prev_blocks = align_blocks(stages[i].n);
        }
    }
    if (!pending) {   // nothing to do: the pose stays as given
        if (residual) *residual = 0.0f;
        if (inliers) *inliers = 0.0f;
        return TSDF_OK;
    }
    launch_align_finish(a, prev_blocks, 1, a->host_io_dev + 16);
    TSDF_HIP(hipGetLastError(), "align kernels failed");
    TSDF_HIP(hipStreamSynchronize(a->stream), "align");
    double out[18];
    std::memcpy(out, a->host_io + 16, sizeof(out));
    // A chain that did not move the pose (no step had an inlier) hands the caller's matrix back as given, not through the two shifts.
    bool moved = false;
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 3; r++) moved = moved || out[c * 4 + r] != a->host_io[c * 4 + r];
    if (moved) {
        for (int c = 0; c < 4; c++) {
            for (int r = 0; r < 3; r++) T[c * 4 + r] = out[c * 4 + r];
            T[c * 4 + 3] = c == 3 ? 1.0 : 0.0;
        }
        for (int r = 0; r < 3; r++) T[12 + r] = out[12 + r] + s.pivot[r];
    }
    if (residual) *residual = (float)out[16];
    if (inliers) *inliers = (float)out[17];
    return TSDF_OK;
}

int tsdf_depth_to_points_device(uint32_t width, uint32_t height, const uint16_t *device_depth, const float kinv[9], uint32_t step,
                                float depth_cutoff, float *device_points, void *hip_stream) {
    TSDF_REQUIRE(device_depth && kinv && device_points, "tsdf_depth_to_points: null argument");
    TSDF_REQUIRE(step != 0, "tsdf_depth_to_points: step is 0");
    TSDF_REQUIRE(width > 0 && height > 0 && width <= 65535 && height <= 65535, "tsdf_depth_to_points: bad image size");
    const uint32_t out_w = (uint32_t)(((uint64_t)width + step - 1) / step), out_h = (uint32_t)(((uint64_t)height + step - 1) / step);
    Mat33 m;
    static_assert(sizeof(m) == 9 * sizeof(float), "Mat33 is nine floats");
    std::memcpy(&m, kinv, sizeof(m));
    hipLaunchKernelGGL(depth_to_points_kernel, dim3((out_w + 63) / 64, (out_h + 3) / 4), dim3(256), 0, (hipStream_t)hip_stream, device_depth, width,
                       out_w, out_h, step, m, depth_cutoff, device_points);
    TSDF_HIP(hipGetLastError(), "depth_to_points kernel failed");
    return TSDF_OK;
}

}  // extern "C"
