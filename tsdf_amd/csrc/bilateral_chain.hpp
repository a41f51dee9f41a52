// The bilateral filter's accumulation chain: one tap in the reference's mixed precision, the same tap as one fp32 fma, and the test
// that tells when a run of taps gives the same bits either way.  Plain C++ for both sides: the staged kernel of bilateral.hip runs it
// on the GPU, tsdf_selftest_bilateral_chain_* run it on the host (tests/test_bilateral_fp32_chain.py needs no GPU for them).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TSDF_CHAIN_HD __host__ __device__
#else
#define TSDF_CHAIN_HD
#endif

namespace tsdf {

TSDF_CHAIN_HD inline uint32_t chain_bits(float x) {
    return __builtin_bit_cast(uint32_t, x);
}

// One tap of the reference's sum (src/BilateralFilter.cpp:99-102) on the staged kernel's operands: w = the float product
// kernel * similarity (>= 0), v4 = 4 * intensity (< 2^18), s = the running sum (>= 0).  The double product is exact (24 + 16
// significant bits), so mul-then-add in double is one fma in double:  s' = RN32(RN64(w v4 + s)).
TSDF_CHAIN_HD inline float chain_tap_f64(float w, uint32_t v4, float s) {
    return (float)__builtin_fma((double)w, (double)v4, (double)s);
}

// The same tap with one rounding:  s' = RN32(w v4 + s)  ((float)v4 is exact: 18 bits).
TSDF_CHAIN_HD inline float chain_tap_f32(float w, uint32_t v4, float s) {
    return __builtin_fmaf(w, (float)v4, s);
}

// true: a run of taps (a half column of the kernel) gave the same bits through chain_tap_f32 as it would through chain_tap_f64.
//   w_min     a lower bound of the run's nonzero weights (0 is allowed and only makes the test stricter),
//   s_before  the sum in front of the run,  s_after  the sum chain_tap_f32 left behind it.
// The two taps differ only by the inner rounding RN64, which does nothing when E = w v4 + s is a double.  Write e(x) for the
// exponent of a normal float x (x in [2^e, 2^(e+1)), x a multiple of 2^(e-23)); every nonzero weight of the staged kernel is
// >= 2^-120 (tsdf_bilateral::scale_exact), so weights and nonzero sums (>= 4 times a weight) are normal.
//   * Every term is >= 0 and fma rounding is monotone, so the sums of the run lie in [s_before, s_after]; and every E of the run is
//     below 2^(e(s_after) + 1), for an E at or above that power of two would have rounded to a sum at or above it.
//   * w v4 is a multiple of 2^(e(w) - 23) * 4 (v4 is a multiple of 4), hence of 2^(e(w_min) - 21).
//   * A nonzero sum in front of a tap is a multiple of its own ulp, which is at least 2^(e(s_before) - 23) when s_before != 0; when
//     s_before == 0 the sum stays 0 (E = w v4: 42 bits, exact) until the first nonzero product, and from then on it is >= 4 w_min,
//     so its ulp is >= 2^(e(w_min) + 2 - 23), the granularity of the products again.  A tap with w == 0 or v4 == 0 changes nothing
//     in either form.
//   So every E is a multiple of 2^b, b = min(e(w_min) - 21, e(s_before) - 23 [s_before != 0]), below 2^(e(s_after) + 1): an integer of
//   e(s_after) + 1 - b bits times 2^b.  It is a double when that is <= 53:
//       e(s_after) - min(e(w_min) + 2, e(s_before) [s_before != 0]) <= 29.
// In bits: biased exponents sit at bit 23.  bits(s_before) - 1 is 0xffffffff for 0 (the min then takes the weight's term) and
// otherwise lowers the exponent by one only for an exact power of two (stricter, never wrong).  With lo the smaller exponent field,
// bits(s_after) - lo = (e(s_after) - e_lo) 2^23 + mantissa, which is below 30 * 2^23 exactly when the exponents differ by <= 29; a
// negative difference (s_after == 0 among them: nothing was added) passes.
TSDF_CHAIN_HD inline bool chain_certified(float w_min, float s_before, float s_after) {
    const uint32_t from_w = chain_bits(w_min) + (2u << 23), from_s = chain_bits(s_before) - 1u;
    const uint32_t lo = (from_w < from_s ? from_w : from_s) & 0xff800000u;
    return (int32_t)(chain_bits(s_after) - lo) < (int32_t)(30u << 23);
}

}  // namespace tsdf
