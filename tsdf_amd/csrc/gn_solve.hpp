// One Gauss-Newton chain with the pose kept on the device, shared by icp.hip (frame-to-model ICP) and align.hip (field alignment and
// its colour term).  A feature supplies the row of a point; everything round it is here, once:
//   * the front end of a step: gn_step_begin (finish the pending step in every workgroup or copy the pose, the barrier, the pose
//     narrowed to R, t), gn_add_row (row -> 28 products + count) and gn_block_sums (wave64 shuffle tree, the four waves in a fixed
//     order) for one or two blocks of 29 sums;
//   * the back end: the second stage of the 29-entry reduction, the 6 x 6 LDL^T solvers, the SE3 exponential and T <- exp(x) * T
//     (icp_finish_step), and gn_finish_kernel for the last step of a chain, which has no next launch to finish it;
//   * the host's side: GnChain, the two-sided device state, the partial sums, the pinned in/out block and their slot arithmetic.
// The expressions and the order of the additions are those icp.hip had: every translation unit steps with the very same bits.
#pragma once

#include <cmath>
#include <cstring>

#include "common.hpp"

namespace tsdf {

constexpr int kIcpBlocks = 256;   // one workgroup per CU (icp_finish_step adds them as 8 groups of 32)
constexpr int kIcpThreads = 256;
constexpr int kIcpStateDoubles = 64;

// icp.hip: launches gn_finish_kernel (one workgroup: icp_finish_step of the sums in partial_prev, state_in -> state_out; `mirror`,
// pinned host memory or null, also gets pose, residual and inliers) on `stream`.  colour_weight null: one block of sums a workgroup and
// a mirror of 18 doubles; else two blocks combined with that weight and 20 doubles, the colour term's residual and count last.
void launch_gn_finish(hipStream_t stream, const double *state_in, double *state_out, const float *partial_prev, int n_blocks, int update,
                      double *mirror, const float *colour_weight = nullptr);

// x = A^-1 b, 6x6 symmetric positive (semi-)definite, LDL^T with diagonal pivoting in double -- the job of
// `A_icp.cast<double>().ldlt().solve(b_icp.cast<double>())` (ICPOdometry.cpp:131).  Zero pivots give zero components.
// One lane runs this, so latency is everything: all loops are fully unrolled and the pivot exchanges are predicated
// swaps at compile-time indices, which keeps the matrices in registers instead of scratch memory.
__device__ inline void swap_if(bool c, double &a, double &b) {
    const double t = a;
    a = c ? b : a;
    b = c ? t : b;
}
// The same factorisation without pivoting: for the positive definite, reasonably conditioned normal matrix of a
// healthy ICP step it needs no row exchanges; returns false (result unused) when a pivot is not safely positive, and the
// pivoted version above/below takes over.  ~250 dependent flops instead of ~4000 predicated moves.
__device__ inline bool ldlt_solve6_unpivoted(const float *A_in, const float *b_in, double *x) {
    double A[6][6], L[6][6], D[6], Dinv[6], y[6];
    double dmax = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        y[i] = b_in[i];
#pragma unroll
        for (int j = 0; j < 6; j++) A[i][j] = A_in[i * 6 + j];
        dmax = fmax(dmax, fabs(A[i][i]));
    }
    bool ok = dmax > 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        D[k] = A[k][k];
        ok = ok && D[k] > 1.0e-9 * dmax;
        const double inv = 1.0 / D[k];
        Dinv[k] = inv;
#pragma unroll
        for (int i = k + 1; i < 6; i++) L[i][k] = A[i][k] * inv;
#pragma unroll
        for (int i = k + 1; i < 6; i++)
#pragma unroll
            for (int j = k + 1; j <= i; j++) {
                A[i][j] -= L[i][k] * D[k] * L[j][k];
                A[j][i] = A[i][j];
            }
    }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < i; j++) y[i] -= L[i][j] * y[j];
#pragma unroll
    for (int i = 0; i < 6; i++) y[i] = y[i] * Dinv[i];   // (the pivots' reciprocals again: six divisions fewer on the critical path)
#pragma unroll
    for (int i = 5; i >= 0; i--) {
#pragma unroll
        for (int j = i + 1; j < 6; j++) y[i] -= L[j][i] * y[j];
        x[i] = y[i];
    }
    return ok;
}

__device__ inline void ldlt_solve6(const float *A_in, const float *b_in, double *x) {
    double A[6][6], L[6][6], D[6], y[6], z[6];
    int perm[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        perm[i] = i;
        y[i] = b_in[i];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            A[i][j] = A_in[i * 6 + j];
            L[i][j] = 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        // pivot: the largest remaining diagonal entry (first one on ties)
        int p = k;
        double best = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; i++) {
            const double v = fabs(A[i][i]);
            if (v > best) {
                best = v;
                p = i;
            }
        }
#pragma unroll
        for (int i = k + 1; i < 6; i++) {
            const bool sw = (p == i);  // exchange rows / columns k and i of A, rows of L, the permutation, the rhs
#pragma unroll
            for (int j = 0; j < 6; j++) swap_if(sw, A[k][j], A[i][j]);
#pragma unroll
            for (int r = 0; r < 6; r++) swap_if(sw, A[r][k], A[r][i]);
#pragma unroll
            for (int j = 0; j < k; j++) swap_if(sw, L[k][j], L[i][j]);
            const int tp = perm[k];
            perm[k] = sw ? perm[i] : perm[k];
            perm[i] = sw ? tp : perm[i];
            swap_if(sw, y[k], y[i]);
        }
        D[k] = A[k][k];
        L[k][k] = 1.0;
        const bool nz = D[k] != 0.0;
#pragma unroll
        for (int i = k + 1; i < 6; i++) L[i][k] = nz ? A[i][k] / D[k] : 0.0;
#pragma unroll
        for (int i = k + 1; i < 6; i++)
#pragma unroll
            for (int j = k + 1; j < 6; j++) A[i][j] -= L[i][k] * D[k] * L[j][k];
    }
    // (y was permuted along with the rows: y = P b)
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < i; j++) y[i] -= L[i][j] * y[j];
#pragma unroll
    for (int i = 0; i < 6; i++) z[i] = (D[i] != 0.0) ? y[i] / D[i] : 0.0;
#pragma unroll
    for (int i = 5; i >= 0; i--)
#pragma unroll
        for (int j = i + 1; j < 6; j++) z[i] -= L[j][i] * z[j];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++)
            if (perm[i] == j) x[j] = z[i];
}

// Sophus::SE3d::exp(a) for a = (upsilon, omega): R = exp(hat(omega)), translation = V * upsilon; E column-major 4x4.
__device__ inline void se3_exp(const double *a, double *E) {
    const double wx = a[3], wy = a[4], wz = a[5];
    const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
    const double W[3][3] = {{0, -wz, wy}, {wz, 0, -wx}, {-wy, wx, 0}};
    double W2[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            W2[i][j] = 0;
            for (int k = 0; k < 3; k++) W2[i][j] += W[i][k] * W[k][j];
        }
    double A, B, C;  // sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3
    if (th2 < 0.0625) {
        // |th| < 1/4 (every step of a converging ICP): the three entire functions by their power series in th^2, summed
        // from the smallest term (Horner, constant reciprocals: a double division costs this lane ~25 dependent instructions);
        // the first omitted terms are < 1e-19 relative.  One lane evaluates this on the
        // critical path of every iteration, and the library's double sin / cos cost several microseconds there.
        const double t = th2;
        A = 1.0 - t * (1.0 / 6.0) * (1.0 - t * (1.0 / 20.0) * (1.0 - t * (1.0 / 42.0) * (1.0 - t * (1.0 / 72.0) * (1.0 - t * (1.0 / 110.0) * (1.0 - t * (1.0 / 156.0) * (1.0 - t * (1.0 / 210.0)))))));
        B = 0.5 * (1.0 - t * (1.0 / 12.0) * (1.0 - t * (1.0 / 30.0) * (1.0 - t * (1.0 / 56.0) * (1.0 - t * (1.0 / 90.0) * (1.0 - t * (1.0 / 132.0) * (1.0 - t * (1.0 / 182.0) * (1.0 - t * (1.0 / 240.0))))))));
        C = 1.0 / 6.0 * (1.0 - t * (1.0 / 20.0) * (1.0 - t * (1.0 / 42.0) * (1.0 - t * (1.0 / 72.0) * (1.0 - t * (1.0 / 110.0) * (1.0 - t * (1.0 / 156.0) * (1.0 - t * (1.0 / 210.0) * (1.0 - t * (1.0 / 272.0))))))));
    } else {
        A = sin(th) / th;
        B = (1.0 - cos(th)) / th2;
        C = (th - sin(th)) / (th2 * th);
    }
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) E[c * 4 + r] = (r == c) ? 1.0 : 0.0;
    for (int i = 0; i < 3; i++) {
        double ti = 0;
        for (int j = 0; j < 3; j++) {
            const double I = (i == j) ? 1.0 : 0.0;
            E[j * 4 + i] = I + A * W[i][j] + B * W2[i][j];
            ti += (I + B * W[i][j] + C * W2[i][j]) * a[j];
        }
        E[12 + i] = ti;
    }
}

// Second stage of the reduction (reduceSum<29>, Cuda/estimate.cu:70-85) + the host part of estimateStep /
// getIncrementalTransformation: A, b, residual, inliers; when `update` != 0 also x = A^-1 b and T <- exp(x) * T.
// Run by all 256 threads of a workgroup; the pose after the step goes to pose_out (shared memory, for the caller's
// __syncthreads), the whole state to state_out when that is not null.  The sums were written by the previous launch.
// COLOUR (align.hip's colour term; the default is the function as it always was): a workgroup's sums are 64 floats, the geometric
// block at [0, 29) and the colour block at [32, 61); each block is added as above, then every entry of A and b handed to the solve is
// (float)((double)S_g + (double)colour_weight * (double)S_c); state_out[60], [61] get the colour block's residual and count.
template <bool COLOUR = false>
__device__ __forceinline__ void icp_finish_step(const float *partial, int n_blocks, const double *state_in, int update, double *pose_out,
                                       double *state_out, float colour_weight = 0.0f) {
    constexpr int kStride = COLOUR ? 64 : 32;   // floats a workgroup
    // 29 entries x 8 groups of blocks: thread (entry, group) adds its 32 blocks in order (loads issued together), then
    // one thread per entry adds the 8 group sums in order -- a fixed tree, in double
    __shared__ double group_sum[8][32];
    __shared__ float total[32];
    const int entry = threadIdx.x & 31, group = threadIdx.x >> 5;
    // (the pose the sums were taken at: requested now, with the sums, not after them -- one memory round trip less on the
    // path every iteration waits for)
    double T[16];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 16; i++) T[i] = state_in[i];
    }
    if (entry < 29) {
        // (The loads are unconditional -- a block past n_blocks re-reads block 0 and its value is replaced by 0 afterwards: with the
        // test in front of each load the compiler made 32 branches, each load waited for on its own: 32 dependent round trips, 8 of
        // the 9.5 us this step took, profiles/r04zz_icp_finish_phases.txt.)
        float v[32];
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const int b = group * 32 + i, bb = b < n_blocks ? b : 0;
            v[i] = partial[bb * kStride + entry];
        }
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 32; i++) s += (double)(group * 32 + i < n_blocks ? v[i] : 0.0f);
        group_sum[group][entry] = s;
    }
    __shared__ double group_sum_c[COLOUR ? 8 : 1][32];
    __shared__ float total_c[32];
    if (COLOUR && entry < 29) {
        float v[32];
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const int b = group * 32 + i, bb = b < n_blocks ? b : 0;
            v[i] = partial[bb * kStride + 32 + entry];
        }
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 32; i++) s += (double)(group * 32 + i < n_blocks ? v[i] : 0.0f);
        group_sum_c[group][entry] = s;
    }
    __syncthreads();
    if (threadIdx.x < 29) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < 8; g++) s += group_sum[g][threadIdx.x];
        total[threadIdx.x] = (float)s;  // the reference hands fp32 sums to the host
        if (COLOUR) {
            double c = 0.0;
#pragma unroll
            for (int g = 0; g < 8; g++) c += group_sum_c[g][threadIdx.x];
            total_c[threadIdx.x] = (float)c;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (COLOUR) {
        if (state_out) {
            state_out[60] = total_c[27];
            state_out[61] = total_c[28];
        }
        // (the residual and the count stay per term: entries 27 and 28 are not combined)
        for (int i = 0; i < 27; i++) total[i] = (float)((double)total[i] + (double)colour_weight * (double)total_c[i]);
    }
    float A[36], b[6];
    int shift = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 7; ++j) {
            const float value = total[shift++];
            if (j == 6) b[i] = value;
            else A[j * 6 + i] = A[i * 6 + j] = value;
        }
    if (state_out) {
        state_out[16] = total[27];
        state_out[17] = total[28];
        for (int i = 0; i < 36; i++) state_out[18 + i] = A[i];
        for (int i = 0; i < 6; i++) state_out[54 + i] = b[i];
    }
    double out[16];
    for (int i = 0; i < 16; i++) out[i] = T[i];
    if (update) {
        double x[6], E[16];
        if (!ldlt_solve6_unpivoted(A, b, x)) ldlt_solve6(A, b, x);
        se3_exp(x, E);
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 4; r++) {
                double s = 0;
                for (int k = 0; k < 4; k++) s += E[k * 4 + r] * T[c * 4 + k];
                out[c * 4 + r] = s;
            }
    }
    for (int i = 0; i < 16; i++) {
        pose_out[i] = out[i];
        if (state_out) state_out[i] = out[i];
    }
}

// The start of a step's launch.  `pending` != 0: the launch before left the sums of its `prev_blocks` workgroups in partial_prev and the
// pose they were taken at in state_in; EVERY workgroup finishes that step first (icp_finish_step, the same fixed-order arithmetic, so
// all arrive at the same pose) and workgroup 0 records it in state_out.  Else the pose is copied.  The kernel boundary orders the two
// launches -- no fence, no ticket, no workgroup waiting for the others across the chip's eight L2s (that hand-over cost more than the
// whole reduction: 24 -> 14 us per step).  Then the pose narrowed to float like `rotationMatrix().cast<float>()`: R column-major.
// `pose`: 16 doubles of LDS, declared by the kernel (declared here, the compiler lays the LDS out differently and the shuffle tree of
// gn_block_sums comes out with some forty more s_waitcnt: LABNOTES.md).
template <bool COLOUR = false>
__device__ __forceinline__ void gn_step_begin(const double *__restrict__ state_in, double *__restrict__ state_out,
                                              const float *__restrict__ partial_prev, int pending, int prev_blocks, float colour_weight,
                                              double *pose, float *R, float *t) {
    if (pending) {
        icp_finish_step<COLOUR>(partial_prev, prev_blocks, state_in, 1, pose, blockIdx.x == 0 ? state_out : nullptr, colour_weight);
    } else {
        if (threadIdx.x < 16) {
            pose[threadIdx.x] = state_in[threadIdx.x];
            if (blockIdx.x == 0) state_out[threadIdx.x] = state_in[threadIdx.x];
        }
    }
    __syncthreads();
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) R[c * 3 + r] = (float)pose[c * 4 + r];
    for (int r = 0; r < 3; r++) t[r] = (float)pose[12 + r];
}

// An inlier's row into a thread's 29 fp32 sums: the 28 upper-triangular products in the reference's order, then the count.
__device__ __forceinline__ void gn_add_row(const float *row, float *sum) {
    int s = 0;
#pragma unroll
    for (int o = 0; o < 7; o++)
#pragma unroll
        for (int k = o; k < 7; k++) sum[s++] += row[o] * row[k];
    sum[28] += 1.0f;
}

// A workgroup's 29 sums to partial[32 blockIdx.x ..): the wave64 shuffle tree, lane 0 of each wave to LDS, then the four waves of the
// workgroup in a fixed order.  COLOUR: two blocks, 64 floats a workgroup, sum at [0, 29) and sum_c at [32, 61), their shuffles interleaved.
template <bool COLOUR = false>
__device__ __forceinline__ void gn_block_sums(float *sum, float *sum_c, float *__restrict__ partial) {
    constexpr int kStride = COLOUR ? 64 : 32;   // floats a workgroup
    __shared__ float shared[4][kStride];
#pragma unroll
    for (int i = 0; i < 29; i++) {
        float v = sum[i], c = COLOUR ? sum_c[i] : 0.0f;
        for (int o = 32; o > 0; o >>= 1) {
            v += __shfl_down(v, o);
            if (COLOUR) c += __shfl_down(c, o);
        }
        sum[i] = v;
        if (COLOUR) sum_c[i] = c;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 29; i++) {
            shared[wave][i] = sum[i];
            if (COLOUR) shared[wave][32 + i] = sum_c[i];
        }
    }
    __syncthreads();
    if (COLOUR ? threadIdx.x < 64 && (threadIdx.x & 31) < 29 : threadIdx.x < 29) {
        partial[blockIdx.x * kStride + threadIdx.x] =
            ((shared[0][threadIdx.x] + shared[1][threadIdx.x]) + shared[2][threadIdx.x]) + shared[3][threadIdx.x];
    }
}

// Finishes the last step of a sequence (nothing follows whose prologue would): one workgroup.
// `mirror` (pinned host memory, or null): pose, residual and inliers also go there, for the host to read after the stream's end;
// COLOUR: the colour term's residual and inliers behind them.
template <bool COLOUR>
__global__ __launch_bounds__(kIcpThreads) void gn_finish_kernel(const double *__restrict__ state_in, double *__restrict__ state_out,
                                                               const float *__restrict__ partial_prev, int n_blocks, int update,
                                                               float colour_weight, double *__restrict__ mirror) {
    __shared__ double pose[16];
    icp_finish_step<COLOUR>(partial_prev, n_blocks, state_in, update, pose, state_out, colour_weight);
    if (mirror && threadIdx.x == 0) {   // (thread 0 solved the step: what it has just written)
#pragma unroll
        for (int i = 0; i < 16; i++) mirror[i] = pose[i];
        mirror[16] = state_out[16];
        mirror[17] = state_out[17];
        if (COLOUR) {
            mirror[18] = state_out[60];
            mirror[19] = state_out[61];
        }
    }
}

// The host's side of a chain; tsdf_icp and tsdf_aligner embed one (plain, memset to zero with its handle).
struct GnChain {
    double *state;         // device, 2 x kIcpStateDoubles: [0..15] T (column-major), [16] residual, [17] inliers, [18..53] A (float
                           //         values), [54..59] b, [60], [61] the colour term's residual and inliers
    float *partial;        // 2 x kIcpBlocks x 32 floats: per-workgroup sums of the 29 entries (two steps)
    float *partial_c;      // colour alignment: 2 x kIcpBlocks x 64 floats (both blocks of sums), made by the first colour call
    int side;              // which copy of state / partial holds the latest step
    double *host_io;       // pinned host memory the device reads and writes in place: [0..15] the pose a chain starts from, behind it
    double *host_io_dev;   // the result (pose, residual, inliers: `mirror` doubles) -- no copy launches either side of the chain (4-5 us each)

    hipError_t alloc(int mirror) {
        hipError_t e = hipMalloc((void **)&partial, (size_t)2 * kIcpBlocks * 32 * sizeof(float));
        if (e == hipSuccess) e = hipMemset(partial, 0, (size_t)2 * kIcpBlocks * 32 * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void **)&state, 2 * kIcpStateDoubles * sizeof(double));
        if (e == hipSuccess) e = hipMemset(state, 0, 2 * kIcpStateDoubles * sizeof(double));
        // (fine-grained: the device reads and writes it past its caches)
        if (e == hipSuccess) e = hipHostMalloc((void **)&host_io, (16 + mirror) * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) std::memset(host_io, 0, (16 + mirror) * sizeof(double));
        if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&host_io_dev, host_io, 0);
        return e;
    }
    hipError_t alloc_colour() {
        if (partial_c) return hipSuccess;
        const size_t bytes = (size_t)2 * kIcpBlocks * 64 * sizeof(float);
        hipError_t e = hipMalloc((void **)&partial_c, bytes);
        if (e == hipSuccess) e = hipMemset(partial_c, 0, bytes);
        if (e != hipSuccess) device_free_all(partial_c);
        return e;
    }
    void free() {
        device_free_all(partial, state, partial_c);
        (void)hipHostFree(host_io);
        host_io = host_io_dev = nullptr;
    }
    // the slots of a launch: it reads the latest step's (`in`), writes the other side's, and flip() makes that the latest
    double *state_in() const { return state + side * kIcpStateDoubles; }
    double *state_out() const { return state + (1 - side) * kIcpStateDoubles; }
    float *sums(int s, bool colour) const { return colour ? partial_c + (size_t)s * kIcpBlocks * 64 : partial + (size_t)s * kIcpBlocks * 32; }
    const float *partial_in(bool colour = false) const { return sums(side, colour); }
    float *partial_out(bool colour = false) const { return sums(1 - side, colour); }
    void flip() { side = 1 - side; }

    // Finishes the step whose sums the last launch left (with or without the pose update).
    void finish(hipStream_t stream, int n_blocks, int update, double *mirror, const float *colour_weight = nullptr) {
        launch_gn_finish(stream, state_in(), state_out(), partial_in(colour_weight != nullptr), n_blocks, update, mirror, colour_weight);
        flip();
    }
    // The latest step's system to the host: A, b, then {residual, inliers} of n_terms terms.  Blocking.
    int download(hipStream_t stream, float A[36], float b[6], float *residual_inliers, int n_terms, const char *what_copy, const char *what_sync) {
        double out[kIcpStateDoubles];
        TSDF_HIP(hipMemcpyAsync(out, state_in(), sizeof(out), hipMemcpyDeviceToHost, stream), what_copy);
        TSDF_HIP(hipStreamSynchronize(stream), what_sync);
        for (int k = 0; k < n_terms; k++) {
            residual_inliers[2 * k] = (float)out[k ? 60 : 16];
            residual_inliers[2 * k + 1] = (float)out[k ? 61 : 17];
        }
        for (int i = 0; i < 36; i++) A[i] = (float)out[18 + i];
        for (int i = 0; i < 6; i++) b[i] = (float)out[54 + i];
        return TSDF_OK;
    }
};

}  // namespace tsdf
