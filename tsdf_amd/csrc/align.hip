// Field alignment for gfx950 (wave64): the rigid pose that puts a point set on the zero level of the fused field, by Gauss-Newton on
// sum S(T x)^2 (include/tsdf_amd.h, "field alignment"; Bylow et al. 2013, Canelhas' SDF tracker).  It is point-to-plane ICP with the
// association replaced by a trilinear sample: no ray cast, no model maps, no projective association.  No reference counterpart.
//
//   * One hot kernel, align_reduce_kernel: per point the pose product (ICP's expression), the field query of field.hip (the ray cast's
//     trilinear(), the central-difference gradient: seven samples), seven weight reads at the same points (field_sample.hpp) and the row
//     (g, u x g, -d): align_row.  B = min(256, ceil(n / 256)) workgroups.
//   * The chain is gn_solve.hpp's, shared with icp.hip: gn_step_begin (every launch first finishes the step before it in every
//     workgroup: second reduction stage, 6 x 6 solve, T <- exp(x) T, the same bits in every workgroup; align_reduce_kernel alone has
//     it written out, for its speed), gn_add_row (the 28 products +
//     the inlier count, per-thread fp32 over a strided share of the points), gn_block_sums (the wave64 shuffle tree, the four waves in
//     a fixed order), gn_finish_kernel for the last step, and GnChain on the host: the pose goes in and comes out through its pinned
//     coherent block, so a run is its launches and one synchronise.
//   * The pose is kept about the centre of the volume's box (the host shifts it in double both ways): the rotation columns of the
//     normal matrix are u x g, and with u measured from the world origin they would carry the distance to it.
//   * The colour term (include/tsdf_amd.h, "colour alignment") is a kernel of its own, align_colour_reduce_kernel: align_row, then for a geometric inlier
//     the intensity of the fused colours in the cell of the distance sample and the exact derivative of that interpolant (eight colour
//     dwords), the photometric row against the point's observed intensity (align_colour_row) and a second block of 29 sums in the same
//     order; 64 floats a workgroup, combined by gn_step_begin<true> / gn_finish_kernel<true>.  58 accumulators and two rows: 141 - 148
//     VGPRs, no scratch.
// Nothing of the volume is written.  Per-point arithmetic is separately rounded fp32 (contraction is off).
#include <cmath>
#include <cstring>
#include <new>
#include <type_traits>

#include "common.hpp"
#include "gn_solve.hpp"
#include "field_sample.hpp"

struct tsdf_aligner {
    int device;
    hipStream_t stream;
    tsdf::GnChain chain;   // the pose is T_c; the pinned result is 20 doubles wide (the colour term's residual and inliers last)
};

namespace tsdf {

constexpr int kAlignMaxStages = 8;

// the aligner's own constants of a call
struct AlignField {
    F3 h;          // the pivot: 0.5f * TriConst's max per axis
    float gate;
};

// The row of point x at the pose (R, t about the pivot), and the point there, u; false for an outlier (row then undefined).
template <bool FASTDIV>
__device__ inline bool align_row(const float *R, const float *t, const float *x, const FieldView &f, const AlignField &a, float *row, float *u) {
    const float u0 = u[0] = ((R[0] * x[0] + R[3] * x[1]) + R[6] * x[2]) + t[0];
    const float u1 = u[1] = ((R[1] * x[0] + R[4] * x[1]) + R[7] * x[2]) + t[1];
    const float u2 = u[2] = ((R[2] * x[0] + R[5] * x[1]) + R[8] * x[2]) + t[2];
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

// One Gauss-Newton step's sums over `n` points (3 floats each), behind gn_step_begin's job: `pending` != 0 says that the launch before left
// the sums of its `prev_blocks` workgroups in partial_prev.  ROWS: also the row of every point (seven floats, the NaN row for an
// outlier) to `rows`: the tests' hook for the per-point arithmetic; the instance without it has none of that code.
template <bool FASTDIV, bool ROWS>
__global__ __launch_bounds__(kIcpThreads) void align_reduce_kernel(const double *__restrict__ state_in, double *__restrict__ state_out,
                                                                  const float *__restrict__ partial_prev, int pending, int prev_blocks,
                                                                  const FieldView f, const AlignField a, const uint32_t n,
                                                                  const float *__restrict__ points, float *__restrict__ rows,
                                                                  float *__restrict__ partial) {
    // gn_step_begin, written out: through the helper this kernel's code differs only before and behind the per-point loop, yet a step
    // over 300 000 points and more measured 0.7 % slower than before the helper existed, in three visits (LABNOTES.md)
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
    float R[9], t[3];  // column-major
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) R[c * 3 + r] = (float)pose[c * 4 + r];
    for (int r = 0; r < 3; r++) t[r] = (float)pose[12 + r];
    float sum[29];
#pragma unroll
    for (int i = 0; i < 29; i++) sum[i] = 0.0f;
    const uint32_t stride = (uint32_t)kIcpThreads * gridDim.x;   // <= 65536
    for (uint64_t i = (uint64_t)blockIdx.x * kIcpThreads + threadIdx.x; i < n; i += stride) {
        float row[7], u[3];
        const bool in = align_row<FASTDIV>(R, t, points + 3 * i, f, a, row, u);
        if (ROWS) {
#pragma unroll
            for (int k = 0; k < 7; k++) rows[7 * i + k] = in ? row[k] : NAN;
        }
        if (in) gn_add_row(row, sum);
    }
    gn_block_sums(sum, nullptr, partial);
}

// ---- the colour term (include/tsdf_amd.h, "colour alignment") ---------------------------------------------------------------------
// the colour term's constants of a call
struct AlignColour {
    const uint32_t *colour;   // the volume's colour words
    float gate;
    float weight;
};

// The photometric row of a geometric inlier with observed intensity y (u as align_row forms it); false for a colour outlier.
template <bool FASTDIV>
__device__ inline bool align_colour_row(float u0, float u1, float u2, float y, const FieldView &f, const AlignField &a, const AlignColour &ac,
                                        float *row) {
    FieldCell cell;
    if (!field_cell<FASTDIV>(f, u0 + a.h.x, u1 + a.h.y, u2 + a.h.z, cell)) return false;
    float c = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if (!field_intensity<FASTDIV, true, true>(f, ac.colour, cell, c, gx, gy, gz)) return false;
    const float e = c - y;
    if (!(fabsf(y) < INFINITY && fabsf(e) < ac.gate)) return false;   // (false for a NaN y: a point without colour)
    row[0] = gx;
    row[1] = gy;
    row[2] = gz;
    row[3] = u1 * gz - u2 * gy;
    row[4] = u2 * gx - u0 * gz;
    row[5] = u0 * gy - u1 * gx;
    row[6] = -e;
    return true;
}

// align_reduce_kernel with the photometric row beside the geometric one: a second block of 29 sums in the same order, 64 floats a
// workgroup (the geometric block at [0, 29), the colour block at [32, 61)).  The colour taps are read for geometric inliers only.  The
// prologue combines the two blocks of the step before (gn_step_begin<true>).  ROWS: 14 floats a point, both rows.
template <bool FASTDIV, bool ROWS>
__global__ __launch_bounds__(kIcpThreads) void align_colour_reduce_kernel(const double *__restrict__ state_in, double *__restrict__ state_out,
                                                                         const float *__restrict__ partial_prev, int pending, int prev_blocks,
                                                                         const FieldView f, const AlignField a, const AlignColour ac,
                                                                         const uint32_t n, const float *__restrict__ points,
                                                                         const float *__restrict__ intensity, float *__restrict__ rows,
                                                                         float *__restrict__ partial) {
    __shared__ double pose[16];
    float R[9], t[3];
    gn_step_begin<true>(state_in, state_out, partial_prev, pending, prev_blocks, ac.weight, pose, R, t);
    float sum[29], sum_c[29];
#pragma unroll
    for (int i = 0; i < 29; i++) sum[i] = sum_c[i] = 0.0f;
    const uint32_t stride = (uint32_t)kIcpThreads * gridDim.x;   // <= 65536
    for (uint64_t i = (uint64_t)blockIdx.x * kIcpThreads + threadIdx.x; i < n; i += stride) {
        float row[7], row_c[7], u[3];
        const bool in = align_row<FASTDIV>(R, t, points + 3 * i, f, a, row, u);
        const bool in_c = in && align_colour_row<FASTDIV>(u[0], u[1], u[2], intensity[i], f, a, ac, row_c);
        if (ROWS) {
#pragma unroll
            for (int k = 0; k < 7; k++) {
                rows[14 * i + k] = in ? row[k] : NAN;
                rows[14 * i + 7 + k] = in_c ? row_c[k] : NAN;
            }
        }
        if (in) gn_add_row(row, sum);
        if (in_c) gn_add_row(row_c, sum_c);
    }
    gn_block_sums<true>(sum, sum_c, partial);
}

// The intensity of the colour field and its gradient at world points, one thread per point (the frame of the field queries).
template <bool VALUE, bool GRAD, bool FASTDIV>
__global__ __launch_bounds__(256) void intensity_sample_kernel(const FieldView f, const uint32_t *__restrict__ colour, const uint64_t n_points,
                                                               const float *__restrict__ points, float *__restrict__ out_intensity,
                                                               float *__restrict__ out_gradient) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_points) return;
    const float qx = points[3 * i + 0] - f.g.offset.x;
    const float qy = points[3 * i + 1] - f.g.offset.y;
    const float qz = points[3 * i + 2] - f.g.offset.z;
    float c = NAN, gx = NAN, gy = NAN, gz = NAN;
    FieldCell cell;
    if (field_valid(f, qx, qy, qz) && field_cell<FASTDIV>(f, qx, qy, qz, cell)) (void)field_intensity<FASTDIV, VALUE, GRAD>(f, colour, cell, c, gx, gy, gz);
    if (VALUE) out_intensity[i] = c;
    if (GRAD) {
        out_gradient[3 * i + 0] = gx;
        out_gradient[3 * i + 1] = gy;
        out_gradient[3 * i + 2] = gz;
    }
}

// Y of every step-th pixel of an RGB frame (3 bytes a pixel), in the order and count of depth_to_points_kernel's points
__global__ __launch_bounds__(256) void rgb_to_intensity_kernel(const uint8_t *__restrict__ rgb, uint32_t width, uint32_t out_w, uint32_t out_h,
                                                               uint32_t step, float *__restrict__ intensity) {
    const uint32_t ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= out_w || oy >= out_h) return;
    const uint8_t *p = rgb + 3 * ((size_t)(oy * step) * width + ox * step);
    intensity[(size_t)oy * out_w + ox] = colour_intensity((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
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
    a->chain.free();
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

// `ac` (the colour calls; null without the term) comes with its gate and weight and leaves with the volume's colours; the chain's
// colour sums are made here, by the first such call.
static int align_setup(tsdf_aligner *a, const tsdf_volume *v, AlignColour *ac, const double *T, float gate, const char *what, AlignSetup &s) {
    TSDF_REQUIRE(a && v && T, "%s: null argument", what);
    const int rc = field_refuse_slab(v, what);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(v->device == a->device, "%s: the volume (device %d) and the aligner (device %d) are on different devices", what, v->device, a->device);
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 3; r++) TSDF_REQUIRE(std::isfinite(T[c * 4 + r]), "%s: T has a non-finite entry in its top three rows", what);
    TSDF_REQUIRE(gate > 0.0f, "%s: the gate must be > 0", what);   // (false for NaN)
    if (ac) {
        TSDF_REQUIRE(v->colour, "%s: colour is not enabled on this volume (tsdf_volume_enable_colour)", what);
        TSDF_REQUIRE(ac->gate > 0.0f, "%s: the colour gate must be > 0", what);   // (false for NaN)
        TSDF_REQUIRE(ac->weight >= 0.0f && ac->weight < INFINITY, "%s: the colour weight must be finite and >= 0", what);
        TSDF_HIP(a->chain.alloc_colour(), "aligner: the colour sums");
        ac->colour = v->colour;
    }
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
    double *io = a->chain.host_io;
    for (int c = 0; c < 4; c++) {
        for (int r = 0; r < 3; r++) io[c * 4 + r] = T[c * 4 + r];
        io[c * 4 + 3] = c == 3 ? 1.0 : 0.0;
    }
    for (int r = 0; r < 3; r++) io[12 + r] = T[12 + r] - s.pivot[r];
}

// T_c as a chain left it behind the pose it started from -> the caller's T.  A chain that did not move the pose (no step had an inlier)
// hands the caller's matrix back as given, not through the two shifts.
static void align_pose_out(const tsdf_aligner *a, const AlignSetup &s, const double *out, double *T) {
    bool moved = false;
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 3; r++) moved = moved || out[c * 4 + r] != a->chain.host_io[c * 4 + r];
    if (!moved) return;
    for (int c = 0; c < 4; c++) {
        for (int r = 0; r < 3; r++) T[c * 4 + r] = out[c * 4 + r];
        T[c * 4 + 3] = c == 3 ? 1.0 : 0.0;
    }
    for (int r = 0; r < 3; r++) T[12 + r] = out[12 + r] + s.pivot[r];
}

// launch(fd, rw) with the volume's division and the rows hook as compile-time constants
template <typename F>
static void align_dispatch(bool fast_div, bool rows, F launch) {
    if (rows) {
        if (fast_div) launch(std::true_type(), std::true_type());
        else launch(std::false_type(), std::true_type());
    } else {
        if (fast_div) launch(std::true_type(), std::false_type());
        else launch(std::false_type(), std::false_type());
    }
}

// The sums of one step over `n` > 0 points at the pose the pending step (if any) leads to; with `ac` both terms' (`intensity` is theirs).
static void launch_align_step(tsdf_aligner *a, const AlignSetup &s, const AlignColour *ac, uint32_t n, const float *points, const float *intensity,
                              float *rows, int pending, int prev_blocks, const double *start) {
    GnChain &c = a->chain;
    const double *state_in = start ? start : c.state_in();
    const dim3 grid((unsigned)align_blocks(n)), block(kIcpThreads);
    align_dispatch(s.fast_div != 0, rows != nullptr, [&](auto fd, auto rw) {
        constexpr bool FD = decltype(fd)::value, RW = decltype(rw)::value;
        if (ac)
            hipLaunchKernelGGL((align_colour_reduce_kernel<FD, RW>), grid, block, 0, a->stream, state_in, c.state_out(), c.partial_in(true), pending,
                               prev_blocks, s.f, s.a, *ac, n, points, intensity, rows, c.partial_out(true));
        else
            hipLaunchKernelGGL((align_reduce_kernel<FD, RW>), grid, block, 0, a->stream, state_in, c.state_out(), c.partial_in(), pending, prev_blocks,
                               s.f, s.a, n, points, rows, c.partial_out());
    });
    c.flip();
}

// tsdf_aligner_step[_colour] behind the caller's own refusals: `what` is its name, residual_inliers two floats a term
static int align_step(tsdf_aligner *a, const tsdf_volume *v, AlignColour *ac, uint32_t n, const float *points, const float *intensity,
                      const double *T, float gate, float *A, float *b, float *residual_inliers, float *rows, const char *what) {
    AlignSetup s;
    const int rc = align_setup(a, v, ac, T, gate, what, s);
    if (rc != TSDF_OK) return rc;
    const int terms = ac ? 2 : 1;
    if (n == 0) {
        std::memset(A, 0, 36 * sizeof(float));
        std::memset(b, 0, 6 * sizeof(float));
        std::memset(residual_inliers, 0, 2 * terms * sizeof(float));
        return TSDF_OK;
    }
    align_pose_in(a, s, T);
    launch_align_step(a, s, ac, n, points, intensity, rows, 0, 0, a->chain.host_io_dev);
    a->chain.finish(a->stream, align_blocks(n), 0, nullptr, ac ? &ac->weight : nullptr);
    TSDF_HIP(hipGetLastError(), "align kernels failed");
    return a->chain.download(a->stream, A, b, residual_inliers, terms, "align result download", "align step");
}

// a stage of either kind (intensity null without the colour term)
struct AlignStage {
    const float *points, *intensity;
    uint32_t n, iterations;
};

// tsdf_aligner_run[_colour] behind the caller's own refusals; residual / inliers (either may be null): one float a term
static int align_run(tsdf_aligner *a, const tsdf_volume *v, AlignColour *ac, uint32_t n_stages, const AlignStage *stages, float gate, double *T,
                     float *residual, float *inliers, const char *what) {
    AlignSetup s;
    const int rc = align_setup(a, v, ac, T, gate, what, s);
    if (rc != TSDF_OK) return rc;
    GnChain &c = a->chain;
    const int terms = ac ? 2 : 1;
    // The pose goes to the device and the result comes back through the pinned block (every call ends with the stream idle, so the
    // host may write it here), as tsdf_icp_get_incremental_transformation does.
    align_pose_in(a, s, T);
    int pending = 0, prev_blocks = 0;   // every launch finishes the step before it, the last step gets a launch of its own
    for (uint32_t i = 0; i < n_stages; i++) {
        if (stages[i].n == 0) continue;
        for (uint32_t j = 0; j < stages[i].iterations; j++) {
            launch_align_step(a, s, ac, stages[i].n, stages[i].points, stages[i].intensity, nullptr, pending, prev_blocks, pending ? nullptr : c.host_io_dev);
            pending = 1;
            prev_blocks = align_blocks(stages[i].n);
        }
    }
    double out[20] = {0};   // the pose, then residual and inliers of every term (zeros for a chain with nothing to do: the pose stays as given)
    if (pending) {
        c.finish(a->stream, prev_blocks, 1, c.host_io_dev + 16, ac ? &ac->weight : nullptr);
        TSDF_HIP(hipGetLastError(), "align kernels failed");
        TSDF_HIP(hipStreamSynchronize(a->stream), "align");
        std::memcpy(out, c.host_io + 16, (16 + 2 * terms) * sizeof(double));
        align_pose_out(a, s, out, T);
    }
    for (int k = 0; k < terms; k++) {
        if (residual) residual[k] = (float)out[16 + 2 * k];
        if (inliers) inliers[k] = (float)out[17 + 2 * k];
    }
    return TSDF_OK;
}

static int sample_intensity_check(const tsdf_volume *v, const char *what) {
    TSDF_REQUIRE(v, "%s: null volume", what);
    const int rc = field_refuse_slab(v, what);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(v->colour, "%s: colour is not enabled on this volume (tsdf_volume_enable_colour)", what);
    return TSDF_OK;
}

// the launch: at least one output, n > 0
static int sample_intensity(const tsdf_volume *v, uint64_t n, const float *points, float *intensity, float *gradient, hipStream_t stream) {
    TSDF_REQUIRE((n + 255) / 256 <= 0x7FFFFFFFull, "tsdf_volume_sample_intensity: too many points");
    const FieldView f = make_field_view(v);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
#define TSDF_INTENSITY_LAUNCH(VAL, GR) \
    do { \
        if (v->fast_div) hipLaunchKernelGGL((intensity_sample_kernel<VAL, GR, true>), grid, block, 0, stream, f, v->colour, n, points, intensity, gradient); \
        else hipLaunchKernelGGL((intensity_sample_kernel<VAL, GR, false>), grid, block, 0, stream, f, v->colour, n, points, intensity, gradient); \
    } while (0)
    if (intensity && gradient) TSDF_INTENSITY_LAUNCH(true, true);
    else if (intensity) TSDF_INTENSITY_LAUNCH(true, false);
    else TSDF_INTENSITY_LAUNCH(false, true);
#undef TSDF_INTENSITY_LAUNCH
    TSDF_HIP(hipGetLastError(), "Intensity sample kernel failed");
    return TSDF_OK;
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
    if (e == hipSuccess) e = a->chain.alloc(20);
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
    return align_step(a, v, nullptr, n, device_points, nullptr, T, gate, A, b, residual_inliers, device_rows, "tsdf_aligner_step");
}

int tsdf_aligner_run(tsdf_aligner *a, const tsdf_volume *v, uint32_t n_stages, const tsdf_align_stage *stages, float gate, double T[16],
                     float *residual, float *inliers) {
    TSDF_REQUIRE(n_stages <= (uint32_t)kAlignMaxStages, "tsdf_aligner_run: more than %d stages", kAlignMaxStages);
    TSDF_REQUIRE(n_stages == 0 || stages, "tsdf_aligner_run: null stages");
    AlignStage st[kAlignMaxStages];
    for (uint32_t i = 0; i < n_stages; i++) {
        TSDF_REQUIRE(stages[i].n == 0 || stages[i].iterations == 0 || stages[i].device_points, "tsdf_aligner_run: stage %u has null points", i);
        st[i] = {stages[i].device_points, nullptr, stages[i].n, stages[i].iterations};
    }
    return align_run(a, v, nullptr, n_stages, st, gate, T, residual, inliers, "tsdf_aligner_run");
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

// ---- colour alignment -----------------------------------------------------------------------------------------------------------
int tsdf_volume_sample_intensity_device(const tsdf_volume *v, uint64_t n, const float *device_points, float *device_intensity,
                                        float *device_gradient, void *hip_stream) {
    const int rc = sample_intensity_check(v, "tsdf_volume_sample_intensity");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(device_intensity || device_gradient, "tsdf_volume_sample_intensity: no output asked for (both are NULL)");
    TSDF_REQUIRE(n == 0 || device_points, "tsdf_volume_sample_intensity: null points");
    if (n == 0) return TSDF_OK;
    return sample_intensity(v, n, device_points, device_intensity, device_gradient, (hipStream_t)hip_stream);
}

int tsdf_volume_sample_intensity(const tsdf_volume *v, uint64_t n, const float *host_points, float *host_intensity, float *host_gradient) {
    const int rc0 = sample_intensity_check(v, "tsdf_volume_sample_intensity");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(host_intensity || host_gradient, "tsdf_volume_sample_intensity: no output asked for (both are NULL)");
    TSDF_REQUIRE(n == 0 || host_points, "tsdf_volume_sample_intensity: null points");
    if (n == 0) return TSDF_OK;
    TSDF_REQUIRE(n <= ((uint64_t)1 << 40), "tsdf_volume_sample_intensity: too many points");
    // one allocation: points (3n), then intensity (n) and gradient (3n) as far as asked for
    const size_t fn = (size_t)n;
    const size_t o_i = 3 * fn, o_g = o_i + (host_intensity ? fn : 0), total = o_g + (host_gradient ? 3 * fn : 0);
    HostStage st;
    int rc = st.begin(v->stream, total * sizeof(float), "tsdf_volume_sample_intensity: couldn't allocate %zu bytes for the points and results");
    if (rc != TSDF_OK) return rc;
    float *const buf = static_cast<float *>(st.buf);
    float *c = host_intensity ? buf + o_i : nullptr, *g = host_gradient ? buf + o_g : nullptr;
    st.up(buf, host_points, 3 * fn * sizeof(float));
    if (st.ok()) rc = sample_intensity(v, n, buf, c, g, v->stream);
    if (rc == TSDF_OK) {
        if (c) st.down(host_intensity, c, fn * sizeof(float));
        if (g) st.down(host_gradient, g, 3 * fn * sizeof(float));
    }
    return st.finish(rc, "Intensity sample failed");
}

int tsdf_rgb_to_intensity_device(uint32_t width, uint32_t height, const uint8_t *device_rgb, uint32_t step, float *device_intensity,
                                 void *hip_stream) {
    TSDF_REQUIRE(device_rgb && device_intensity, "tsdf_rgb_to_intensity: null argument");
    TSDF_REQUIRE(step != 0, "tsdf_rgb_to_intensity: step is 0");
    TSDF_REQUIRE(width > 0 && height > 0 && width <= 65535 && height <= 65535, "tsdf_rgb_to_intensity: bad image size");
    const uint32_t out_w = (uint32_t)(((uint64_t)width + step - 1) / step), out_h = (uint32_t)(((uint64_t)height + step - 1) / step);
    hipLaunchKernelGGL(rgb_to_intensity_kernel, dim3((out_w + 63) / 64, (out_h + 3) / 4), dim3(256), 0, (hipStream_t)hip_stream, device_rgb, width,
                       out_w, out_h, step, device_intensity);
    TSDF_HIP(hipGetLastError(), "rgb_to_intensity kernel failed");
    return TSDF_OK;
}

int tsdf_aligner_step_colour(tsdf_aligner *a, const tsdf_volume *v, uint32_t n, const float *device_points, const float *device_intensity,
                             const double T[16], float gate, float colour_gate, float colour_weight, float A[36], float b[6],
                             float residual_inliers[4], float *device_rows) {
    TSDF_REQUIRE(A && b && residual_inliers, "tsdf_aligner_step_colour: null argument");
    TSDF_REQUIRE(n == 0 || device_points, "tsdf_aligner_step_colour: null points");
    TSDF_REQUIRE(n == 0 || device_intensity, "tsdf_aligner_step_colour: null intensities");
    AlignColour ac = {nullptr, colour_gate, colour_weight};
    return align_step(a, v, &ac, n, device_points, device_intensity, T, gate, A, b, residual_inliers, device_rows, "tsdf_aligner_step_colour");
}

int tsdf_aligner_run_colour(tsdf_aligner *a, const tsdf_volume *v, uint32_t n_stages, const tsdf_align_colour_stage *stages, float gate,
                            float colour_gate, float colour_weight, double T[16], float residual[2], float inliers[2]) {
    TSDF_REQUIRE(n_stages <= (uint32_t)kAlignMaxStages, "tsdf_aligner_run_colour: more than %d stages", kAlignMaxStages);
    TSDF_REQUIRE(n_stages == 0 || stages, "tsdf_aligner_run_colour: null stages");
    AlignStage st[kAlignMaxStages];
    for (uint32_t i = 0; i < n_stages; i++) {
        const bool empty = stages[i].n == 0 || stages[i].iterations == 0;
        TSDF_REQUIRE(empty || stages[i].device_points, "tsdf_aligner_run_colour: stage %u has null points", i);
        TSDF_REQUIRE(empty || stages[i].device_intensity, "tsdf_aligner_run_colour: stage %u has null intensities", i);
        st[i] = {stages[i].device_points, stages[i].device_intensity, stages[i].n, stages[i].iterations};
    }
    AlignColour ac = {nullptr, colour_gate, colour_weight};
    return align_run(a, v, &ac, n_stages, st, gate, T, residual, inliers, "tsdf_aligner_run_colour");
}

}  // extern "C"
