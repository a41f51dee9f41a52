// The integer arithmetic of the frame differences (include/tsdf_amd.h, "frame differences"): the tolerance of a model
// depth and its saturation, the state of a pixel, the clipped dilation window, the any-bit test of a range of pixel ids and the image
// sizes that are refused -- these are what frame_diff.hip's kernels and argument checks call.  diff_neighbours is not called by any
// kernel: it is the SPECIFICATION of which pixels voxel_hook_kernel (voxel_set.hpp) joins on a W x H x 1 grid, written out so that a
// host program can check it at row ends and corners; the device's own rule is that kernel's grid.split and bounds test, which
// tests/test_frame_diff.py exercises.  Compiles for the host alone: tests/cpp/frame_diff_host.cpp runs it under the address and
// undefined-behaviour sanitizers (`make sanitize-frame-diff`).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace tsdf {

// the states, as the state image holds them and as counts[] is indexed (TSDF_DIFF_* of the public header)
enum : uint32_t { kDiffNoFrame = 0, kDiffNoModel = 1, kDiffSame = 2, kDiffFarther = 3, kDiffNearer = 4, kDiffStates = 5 };

constexpr uint32_t kDiffMaxSide = 65535u;     // x and y fit 16 bits: a wave's coordinate sum fits 32
constexpr uint32_t kDiffMaxDilate = 32u;      // a window of at most 65 ids spans at most two mask words

// W x H pixels that a compare takes: both sides in 1 .. 65535 and, formed in 64 bits, at most 2^32 - 1 pixel ids
__host__ __device__ inline uint64_t diff_pixels(uint32_t width, uint32_t height) { return (uint64_t)width * height; }
__host__ __device__ inline bool diff_shape_ok(uint32_t width, uint32_t height) {
    const uint64_t n = diff_pixels(width, height);
    return n >= 1 && n <= 0xffffffffull && width <= kDiffMaxSide && height <= kDiffMaxSide;
}

// tol = tolerance + ((quadratic * m * m) >> 32), the product in 64 bits (65535^2 * (2^32 - 1) < 2^64) and the sum too, saturated to
// 65535
__host__ __device__ inline uint32_t diff_tolerance(uint32_t tolerance, uint32_t quadratic, uint32_t m) {
    const uint64_t q = ((uint64_t)quadratic * m * m) >> 32;
    const uint64_t tol = (uint64_t)tolerance + q;
    return tol > 65535u ? 65535u : (uint32_t)tol;
}

// f, m <= 65535 and tol <= 65535: f + tol and m + tol are at most 131070
__host__ __device__ inline uint32_t diff_state(uint32_t f, uint32_t m, uint32_t tol) {
    if (f == 0) return kDiffNoFrame;
    if (m == 0) return kDiffNoModel;
    if (f + tol < m) return kDiffNearer;
    if (f > m + tol) return kDiffFarther;
    return kDiffSame;
}

// (specification only, see above) pixel ids a != b of an image `width` wide are neighbours: their x and y differ by at most 1 and, at connectivity 4, on one axis only.
// The last pixel of a row and the first of the next are consecutive ids and not neighbours.
__host__ __device__ inline bool diff_neighbours(uint32_t a, uint32_t b, uint32_t width, uint32_t connectivity) {
    const uint32_t ax = a % width, ay = a / width, bx = b % width, by = b / width;
    const uint32_t dx = ax > bx ? ax - bx : bx - ax, dy = ay > by ? ay - by : by - ay;
    if (dx > 1 || dy > 1 || dx + dy == 0) return false;
    return connectivity == 8u || dx + dy == 1;
}

// the window [lo, hi] of coordinate p on an axis of n pixels, clipped at the border: p < n, dilate <= kDiffMaxDilate
__host__ __device__ inline void diff_window(uint32_t p, uint32_t dilate, uint32_t n, uint32_t &lo, uint32_t &hi) {
    lo = p >= dilate ? p - dilate : 0u;
    hi = p + dilate < n ? p + dilate : n - 1;   // (p + dilate <= 65534 + 32)
}

// bits a .. b of one word, 0 <= a <= b <= 63
__host__ __device__ inline uint64_t diff_bits(uint32_t a, uint32_t b) { return ((~0ull) >> (63u - (b - a))) << a; }

// is any of the ids a .. b (a <= b, b - a <= 64, b below 64 * the number of words) set in a mask of one bit per id?  At most two words.
__host__ __device__ inline bool diff_any_bit(const uint64_t *mask, uint32_t a, uint32_t b) {
    const uint32_t wa = a >> 6, wb = b >> 6;
    if (wa == wb) return (mask[wa] & diff_bits(a & 63u, b & 63u)) != 0;
    return (mask[wa] & diff_bits(a & 63u, 63u)) != 0 || (mask[wb] & diff_bits(0u, b & 63u)) != 0;
}

}  // namespace tsdf
