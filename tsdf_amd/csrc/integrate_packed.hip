// integrate_kernel for volumes whose weights are stored as packed counts (weights.hip), standard cameras and implicit deformation
// nodes: the per-voxel arithmetic of the reference (src/TSDF/TSDFVolume.cu:337-390, src/Utilities/cuda_coordinate_transforms.cu:10-30,
// 108-146) in its operation order, bit for bit what integrate_kernel<false, *, true> of integrate.hip computes -- with roughly half
// the vector instructions and 10 (12) instead of 16 bytes moved per updated voxel.
//
// Why (round 4, knock-out builds of integrate_kernel, `profiles/r04n_*`): with every distance / weight access removed the kernel still
// took 0.097 of its 0.118 ms -- its vector instruction stream (80 issue slots per 64-voxel row x 6 waves per SIMD = the 31 us a brick
// takes) -- and the read-modify-write of 558 MB at the 5-6 TB/s an in-place walk reaches is 0.093-0.11 ms: two equal bounds, so that
// halving either alone changed nothing (what rounds 2 and 3 measured).  This kernel lowers both.
//   * weights: the reference only ever adds 1 to a weight (the clamp to max_weight is commented out, TSDFVolume.cu:377), so a
//     volume's weights are small integers unless a caller uploads something else.  They are kept as 8- (16-) bit counts, the four
//     (two) planes of a batch of one lane in ONE dword ("z-packed"): a wave still moves whole 256-byte rows, one per batch instead of
//     four.  Dense walks in this shape: 0.237 (0.274) ms against 0.360 for two fp32 arrays (tools/ubench_layout.hip).
//   * arithmetic: two planes at a time with packed fp32 (v_pk_add / v_pk_mul: separately rounded lanes, no contraction); one test
//     per pair of planes for "some quotient is near a rounding boundary" (v_maximum3, NaN-propagating) instead of a branch per
//     plane; (d w + tsdf) / (w + 1) as rcp + mul + two fmas (div_by_count, proven and checked exhaustively); the depth look-up addressed in fp32 into a tile with a ring of zeros (v_med3 clamps what misses the pixel box onto the
//     ring: no range tests, no select; bricks without a tile look up a copy of the whole image inside such a ring that
//     brick_cull_kernel leaves in memory); distance rows addressed as wave-uniform base + one 32-bit lane offset.
#include <type_traits>

#include "band_pass.hpp"

namespace tsdf {

#ifndef TSDF_PACKED_WAVES
#define TSDF_PACKED_WAVES 6   // waves per SIMD the kernel is compiled for (register budget)
#endif
#ifndef TSDF_PACKED_PIPELINE
#define TSDF_PACKED_PIPELINE 1   // two register sets, a batch of loads always in flight (0: one set, for the occupancy A/B of round 6: profiles/r06_integrate_occupancy_ab.txt)
#endif

// (knock-out builds for timing experiments only: -DTSDF_DIAG_NOLOAD / -DTSDF_DIAG_NOSTORE make the accesses depend on conditions that never hold)
#ifdef TSDF_DIAG_NOLOAD
#define DIAG_NOLOAD && r1 == 12345.678f
#else
#define DIAG_NOLOAD
#endif
#ifdef TSDF_DIAG_NOSTORE
#define DIAG_NOSTORE_D && new_distance == 12345.678f
#define DIAG_NOSTORE_W && r1 == 12345.678f
#else
#define DIAG_NOSTORE_D
#define DIAG_NOSTORE_W
#endif

typedef float f2 __attribute__((ext_vector_type(2)));   // two planes of one lane: arithmetic on it issues as v_pk_*_f32

// max(acc, |a|, |b|) that keeps a NaN (IEEE 754-2019 maximum; v_max3_f32 would drop it)
__device__ inline float max3_abs_keep_nan(float acc, float a, float b) {
    float r;
    asm("v_maximum3_f32 %0, |%1|, |%2|, %3" : "=v"(r) : "v"(a), "v"(b), "v"(acc));
    return r;
}
__device__ inline float med3(float x, float lo, float hi) { return __builtin_amdgcn_fmed3f(x, lo, hi); }

// a / b as the IEEE division rounds it, for b an integer-valued float in [1, 2^17] (a weight count + 1) and any float a.
//   y = rcp(b) (relative error e, |e| <= 2^-22 and far less in practice), q0 = fl(a y), r = a - q0 b, q1 = fl(q0 + r y).
//   * |q0 - a / b| < 2.5 ulp of the quotient, so r = b (a / b - q0) is a multiple of ulp(q) / 2 below 2^24 of them: the fma forms it
//     exactly;
//   * q0 + r y = a / b + (a / b - q0) e, off the true quotient by less than 2.5 * 2^-22 ulp;
//   * a quotient by an integer is never a rounding midpoint m (b m would need a 25th significant bit) and a - b m is a multiple of
//     ulp(q) / 2, so a / b stays ulp / (2 b) >= 2^-18 ulp away from every midpoint: rounding the perturbed value rounds like the true
//     one, q1 = RN(a / b).
// That needs every intermediate normal: |a| in [2^-90, 2^90].  Anything else (zeros, denormals, huge values, infinities, NaN -- what a
// caller may have uploaded) takes the division instruction sequence.  tsdf_selftest_count_division compares the two for every
// mantissa of a and every b (tests/test_weight_storage.py).
__device__ inline float div_by_count(float a, float b) {
    const float y = __builtin_amdgcn_rcpf(b);
    const float q0 = a * y;
    const float r = __builtin_fmaf(-q0, b, a);
    float q = __builtin_fmaf(r, y, q0);
    const float aa = __builtin_fabsf(a);
    if (__builtin_expect(!(aa >= 0x1p-90f && aa <= 0x1p90f), 0)) q = a / b;
    return q;
}

constexpr int kPairFloats = 8;   // LDS per pair of planes: {cz, cz', m13 cz, m13 cz', m23 cz, m23 cz', m33 cz, m33 cz'}
constexpr uint32_t kNoPixel = ~0u;   // (COLOUR) a voxel outside the colour update (frames have fewer than 2^31 / 3 pixels)

#ifndef TSDF_PACKED_COLOUR_WAVES
#define TSDF_PACKED_COLOUR_WAVES 5   // waves per SIMD integrate_packed_colour_kernel is compiled for
#endif
#define TSDF_PACKED_PARAMS                                                                                                           \
    float *__restrict__ dist, uint32_t *__restrict__ wpk, const Geom g, const BrickGrid bg, const Mat44 ip, const Mat33 k, const uint32_t width,  \
        const uint32_t height, const uint16_t *__restrict__ depth, const uint16_t *__restrict__ depth_pad, unsigned long long *__restrict__ counter, \
        const OccGrid occ, const uint32_t *__restrict__ list, const uint4 *__restrict__ boxes, const uint2 *__restrict__ coords,                   \
        const uint32_t *__restrict__ count, const float4 *__restrict__ plane_const, uint8_t *__restrict__ touched

// WBITS = 8 or 16: bits per weight; 32 / WBITS planes of one (x, y) share a dword, group g of planes at wpk + g * X * Y.
template <bool COUNT, int WBITS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TSDF_PACKED_WAVES, TSDF_PACKED_WAVES))) void integrate_packed_kernel(TSDF_PACKED_PARAMS) {
    __shared__ uint16_t tile[kTilePixels];                                   // the brick's pixel box inside a ring of zeros
    __shared__ __align__(16) float plane_lds[(kChunkZ + kBatchZ) / 2 * kPairFloats];
    constexpr bool COLOUR = false, CAPPED = false, REMOVE = false;
    uint32_t *const colour = nullptr;
    const uint8_t *const rgb = nullptr;
    const uint32_t cap = 0;
#include "integrate_packed_body.hpp"
}

// The same walk plus the colour update of the band pass (band_pass.hpp, ColourBlend), made on the voxels the walk updates from the pixel and
// the sdf it has formed: the same words as the separate pass, without a second projection of every listed voxel.  A kernel of its own
// name, so that the plain kernels and their rocprof rows stay as they are.  rgb: the frame's 3 * width * height bytes, registered to
// the depth image (any alignment).  (The COUNT instances spill two scalar registers -- the counter's address, kept in a vector lane
// across the walk, .sgpr_spill_count 2; no scratch.  The instances without COUNT spill nothing.)
template <bool COUNT, int WBITS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TSDF_PACKED_COLOUR_WAVES, TSDF_PACKED_COLOUR_WAVES))) void integrate_packed_colour_kernel(
    TSDF_PACKED_PARAMS, uint32_t *__restrict__ colour, const uint8_t *__restrict__ rgb) {
    __shared__ uint16_t tile[kTilePixels];
    __shared__ __align__(16) float plane_lds[(kChunkZ + kBatchZ) / 2 * kPairFloats];
    constexpr bool COLOUR = true, CAPPED = false, REMOVE = false;
    const uint32_t cap = 0;
#include "integrate_packed_body.hpp"
}

// The two kernels above with a weight cap (tsdf_volume_set_weight_cap; 1 <= cap <= the field's largest value -- launch_integrate's
// weights_make_room sees to it): the blend divides by count + 1 as ever, the count it STORES is min(count + 1, cap), each field of the
// packed word on its own -- a field at 255 (65535) takes no increment, so nothing carries into its neighbour -- and a word whose fields
// all sit at the cap comes out as it went in and is not stored.  Kernels of their own names, compiled for the occupancy of their plain
// counterparts: the plain kernels and their rocprof rows stay as they are.
template <bool COUNT, int WBITS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TSDF_PACKED_WAVES, TSDF_PACKED_WAVES))) void integrate_packed_capped_kernel(
    TSDF_PACKED_PARAMS, const uint32_t cap) {
    __shared__ uint16_t tile[kTilePixels];
    __shared__ __align__(16) float plane_lds[(kChunkZ + kBatchZ) / 2 * kPairFloats];
    constexpr bool COLOUR = false, CAPPED = true, REMOVE = false;
    uint32_t *const colour = nullptr;
    const uint8_t *const rgb = nullptr;
#include "integrate_packed_body.hpp"
}
template <bool COUNT, int WBITS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TSDF_PACKED_COLOUR_WAVES, TSDF_PACKED_COLOUR_WAVES))) void integrate_packed_colour_capped_kernel(
    TSDF_PACKED_PARAMS, uint32_t *__restrict__ colour, const uint8_t *__restrict__ rgb, const uint32_t cap) {
    __shared__ uint16_t tile[kTilePixels];
    __shared__ __align__(16) float plane_lds[(kChunkZ + kBatchZ) / 2 * kPairFloats];
    constexpr bool COLOUR = true, CAPPED = true, REMOVE = false;
#include "integrate_packed_body.hpp"
}

// De-integration (include/tsdf_amd.h, "de-integration"): the same walk over the same voxels -- the set a frame updates depends on the
// depth image and the camera only -- with the blend inverted: a count of at least 1 goes down by one in its own field (no borrow), the
// distance becomes ((D w) - tsdf) / (w - 1), or +trunc with the last frame.  div_by_count's divisor w - 1 is 1 .. 65534.  A kernel of its
// own name, compiled for the occupancy of the plain one: the plain kernels and their rocprof rows stay as they are.  No colour variant:
// the integer colour blend cannot be inverted.
template <bool COUNT, int WBITS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TSDF_PACKED_WAVES, TSDF_PACKED_WAVES))) void integrate_packed_remove_kernel(TSDF_PACKED_PARAMS) {
    __shared__ uint16_t tile[kTilePixels];
    __shared__ __align__(16) float plane_lds[(kChunkZ + kBatchZ) / 2 * kPairFloats];
    constexpr bool COLOUR = false, CAPPED = false, REMOVE = true;
    uint32_t *const colour = nullptr;
    const uint8_t *const rgb = nullptr;
    const uint32_t cap = 0;
#include "integrate_packed_body.hpp"
}
#undef TSDF_PACKED_PARAMS

// Launched by launch_integrate (integrate.hip) in place of integrate_kernel<false, *, true> when the volume's weights are packed.
// d_rgb != nullptr: integrate_packed_colour_kernel, which also makes the frame's colour update (v->colour).
// remove: integrate_packed_remove_kernel (tsdf_deintegrate*; no cap, no colour -- the callers see to it).
int launch_integrate_packed_kernel(tsdf_volume *v, dim3 grid, const BrickGrid &bg, const Mat44 &ip, const Mat33 &mk, uint32_t width,
                                   uint32_t height, const uint16_t *d_depth, unsigned long long *counter_arg, const uint4 *boxes,
                                   const uint2 *coords, const uint32_t *count, const float4 *plane_const, const uint8_t *d_rgb, bool remove) {
    const dim3 block(kTileX, kTileY, 1);
#define LAUNCH(CNT, BITS)                                                                                                       \
    do {                                                                                                                        \
        if (remove)                                                                                                             \
            TSDF_LAUNCH_TIMED(v, 0, (integrate_packed_remove_kernel<CNT, BITS>), grid, block, v->dist, v->wpacked, v->g, bg, ip, mk, width, height, d_depth, \
                              v->depth_pad, counter_arg, v->occ, v->brick_list, boxes, coords, count, plane_const, v->touched);                    \
        else if (v->weight_cap && d_rgb)                                                                                        \
            TSDF_LAUNCH_TIMED(v, 0, (integrate_packed_colour_capped_kernel<CNT, BITS>), grid, block, v->dist, v->wpacked, v->g, bg, ip, mk, width, height, \
                              d_depth, v->depth_pad, counter_arg, v->occ, v->brick_list, boxes, coords, count, plane_const, v->touched, v->colour, d_rgb, \
                              v->weight_cap);                                                                                   \
        else if (v->weight_cap)                                                                                                 \
            TSDF_LAUNCH_TIMED(v, 0, (integrate_packed_capped_kernel<CNT, BITS>), grid, block, v->dist, v->wpacked, v->g, bg, ip, mk, width, height, d_depth, \
                              v->depth_pad, counter_arg, v->occ, v->brick_list, boxes, coords, count, plane_const, v->touched, v->weight_cap);     \
        else if (d_rgb)                                                                                                         \
            TSDF_LAUNCH_TIMED(v, 0, (integrate_packed_colour_kernel<CNT, BITS>), grid, block, v->dist, v->wpacked, v->g, bg, ip, mk, width, height, \
                              d_depth, v->depth_pad, counter_arg, v->occ, v->brick_list, boxes, coords, count, plane_const, v->touched, v->colour, d_rgb); \
        else                                                                                                                    \
            TSDF_LAUNCH_TIMED(v, 0, (integrate_packed_kernel<CNT, BITS>), grid, block, v->dist, v->wpacked, v->g, bg, ip, mk, width, height, d_depth, \
                              v->depth_pad, counter_arg, v->occ, v->brick_list, boxes, coords, count, plane_const, v->touched);                    \
    } while (0)
    if (v->wmode == 8) {
        if (v->counting) LAUNCH(true, 8); else LAUNCH(false, 8);
    } else if (v->wmode == 16) {
        if (v->counting) LAUNCH(true, 16); else LAUNCH(false, 16);
    } else {
        set_error("integrate: packed kernel asked for with fp32 weights");
        return TSDF_ERR_INVALID;
    }
#undef LAUNCH
    return TSDF_OK;
}

// div_by_count against the division it replaces: one workgroup per divisor, every mantissa of the dividend, both signs
__global__ __launch_bounds__(256) void count_division_check_kernel(uint32_t b0, float scale, unsigned long long *__restrict__ bad) {
    const float b = (float)(b0 + blockIdx.x);
    uint32_t n = 0;
    for (uint32_t m = threadIdx.x; m < (1u << 23); m += 256) {
        const float a = __uint_as_float(0x3f800000u | m) * scale;   // (a power of two: exact)
        n += __float_as_uint(div_by_count(a, b)) != __float_as_uint(a / b);
        n += __float_as_uint(div_by_count(-a, b)) != __float_as_uint(-a / b);
    }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(bad, (unsigned long long)n);
}
__global__ void count_division_special_kernel(const float *__restrict__ a, uint32_t n_a, uint32_t b_end, unsigned long long *__restrict__ bad) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_a * b_end) return;
    const float x = a[t % n_a], b = (float)(t / n_a + 1u);
    const float q = div_by_count(x, b), r = x / b;
    if (__float_as_uint(q) != __float_as_uint(r) && !(q != q && r != r)) atomicAdd(bad, 1ull);
}

}  // namespace tsdf

extern "C" int tsdf_selftest_count_division(uint32_t b_begin, uint32_t b_end, unsigned long long *mismatches) {
    using namespace tsdf;
    TSDF_REQUIRE(mismatches && b_begin >= 1 && b_begin < b_end && b_end <= (1u << 17) + 1u, "tsdf_selftest_count_division: divisors are 1 .. 2^17");
    unsigned long long *bad = nullptr;
    TSDF_HIP(hipMalloc((void **)&bad, sizeof(*bad)), "selftest alloc");
    hipError_t e = hipMemset(bad, 0, sizeof(*bad));
    // every mantissa at three scales: 1, the bottom and the top of the range the short sequence is taken in
    for (float scale : {1.0f, 0x1p-90f, 0x1p89f})
        if (e == hipSuccess) {
            hipLaunchKernelGGL(count_division_check_kernel, dim3(b_end - b_begin), dim3(256), 0, nullptr, b_begin, scale, bad);
            e = hipGetLastError();
        }
    // and the values outside it (the division's own instruction sequence is taken: equal by construction, checked all the same)
    const float special[] = {0.0f, -0.0f, 1.0e-45f, -1.0e-40f, 0x1p-126f, 0x1p-91f, 0x1.fffffep-91f, 0x1.000002p90f, 0x1p100f, -0x1p127f,
                             3.4028235e38f, INFINITY, -INFINITY, NAN};
    const uint32_t n_a = sizeof(special) / sizeof(special[0]);
    float *a_dev = nullptr;
    if (e == hipSuccess) e = hipMalloc((void **)&a_dev, sizeof(special));
    if (e == hipSuccess) e = hipMemcpy(a_dev, special, sizeof(special), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const uint32_t n = n_a * (b_end - 1u);
        hipLaunchKernelGGL(count_division_special_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, a_dev, n_a, b_end - 1u, bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(mismatches, bad, sizeof(*bad), hipMemcpyDeviceToHost);
    (void)hipFree(bad);
    if (a_dev) (void)hipFree(a_dev);
    if (e != hipSuccess) return hip_fail(e, "tsdf_selftest_count_division");
    return TSDF_OK;
}
