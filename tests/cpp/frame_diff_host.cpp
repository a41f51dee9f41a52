// Host-side run of the frame differences' integer arithmetic (tsdf_amd/csrc/frame_diff_index.hpp) under the address and
// undefined-behaviour sanitizers (`make sanitize-frame-diff`): the tolerance at m = 65535 with quadratic = 2^32 - 1 and its saturation,
// f + tol at 65535 + 65535, the neighbour test at row ends and at the image's corners against brute force, the dilation window clipped
// at every border, the any-bit test of an id range against brute force, and W * H = 2^32 - 1.  Needs no GPU and links nothing of the
// library.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "frame_diff_index.hpp"

using namespace tsdf;

static int failures = 0;
#define EXPECT(c)                                                   \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("line %d: %s\n", __LINE__, #c);             \
            failures++;                                             \
        }                                                           \
    } while (0)

int main() {
    // the tolerance: the product in 64 bits, the sum in 64 bits, saturated
    const uint32_t all = 0xffffffffu;
    EXPECT(diff_tolerance(0, all, 65535) == 65535);                 // (65535^2 * (2^32 - 1)) >> 32 = 4294836224
    EXPECT(diff_tolerance(0, all, 255) == 65024);                   // (255^2 * (2^32 - 1)) >> 32, below the cap
    EXPECT(diff_tolerance(0, all, 256) == 65535);                   // 65535.99..: 65535 either way
    EXPECT(diff_tolerance(all, all, 65535) == 65535);               // the sum does not wrap
    EXPECT(diff_tolerance(all, 0, 0) == 65535);
    EXPECT(diff_tolerance(7, 0, 65535) == 7);
    EXPECT(diff_tolerance(10, 1u << 12, 4000) == 10 + ((4000u * 4000u) >> 20));
    EXPECT(diff_tolerance(65535, 0, 1) == 65535 && diff_tolerance(65536, 0, 1) == 65535);
    // the states, at 65535 + 65535 and at the tolerance and one either side
    EXPECT(diff_state(65535, 65535, 65535) == kDiffSame);
    EXPECT(diff_state(1, 65535, 65533) == kDiffNearer && diff_state(1, 65535, 65534) == kDiffSame);
    EXPECT(diff_state(65535, 1, 65533) == kDiffFarther && diff_state(65535, 1, 65534) == kDiffSame);
    EXPECT(diff_state(0, 0, 0) == kDiffNoFrame && diff_state(0, 65535, 65535) == kDiffNoFrame);
    EXPECT(diff_state(1, 0, 65535) == kDiffNoModel && diff_state(65535, 0, 0) == kDiffNoModel);
    for (uint32_t tol = 0; tol < 3; tol++)
        for (uint32_t m = 1; m < 8; m++)
            for (uint32_t f = 1; f < 8; f++) {
                const uint32_t d = f > m ? f - m : m - f;
                EXPECT(diff_state(f, m, tol) == (d <= tol ? kDiffSame : f < m ? kDiffNearer : kDiffFarther));
            }
    // neighbours against brute force on small images, the row ends and corners among them.  diff_neighbours is the specification of the
    // rule voxel_hook_kernel applies on a W x H x 1 grid, not code the kernels share: the device's rule is checked on the GPU
    // (tests/test_frame_diff.py, the row-end and diagonal cases).
    const uint32_t shapes[][2] = {{1, 1}, {1, 5}, {5, 1}, {2, 2}, {4, 3}, {7, 5}};
    for (const auto &s : shapes) {
        const uint32_t W = s[0], H = s[1];
        for (uint32_t a = 0; a < W * H; a++)
            for (uint32_t b = 0; b < W * H; b++) {
                const int dx = std::abs((int)(a % W) - (int)(b % W)), dy = std::abs((int)(a / W) - (int)(b / W));
                const bool n8 = a != b && dx <= 1 && dy <= 1, n4 = n8 && dx + dy == 1;
                EXPECT(diff_neighbours(a, b, W, 8) == n8 && diff_neighbours(a, b, W, 4) == n4);
            }
    }
    EXPECT(!diff_neighbours(3, 4, 4, 8) && !diff_neighbours(4, 3, 4, 4));   // the end of row 0 and the start of row 1
    EXPECT(diff_neighbours(0xfffffffeu, 0xfffffffdu, 65535, 4));          // the last ids of the largest image
    // the window, clipped at every border
    for (uint32_t n = 1; n <= 70; n++)
        for (uint32_t d = 0; d <= kDiffMaxDilate; d++)
            for (uint32_t p = 0; p < n; p++) {
                uint32_t lo, hi;
                diff_window(p, d, n, lo, hi);
                const int want_lo = (int)p - (int)d < 0 ? 0 : (int)p - (int)d, want_hi = p + d > n - 1 ? (int)n - 1 : (int)(p + d);
                EXPECT((int)lo == want_lo && (int)hi == want_hi && hi - lo <= 2 * kDiffMaxDilate);
            }
    {
        uint32_t lo, hi;
        diff_window(65534, 32, 65535, lo, hi);
        EXPECT(lo == 65502 && hi == 65534);
    }
    // the any-bit test against brute force: every range of at most 65 ids over three words, one bit set at a time
    {
        std::vector<uint64_t> mask(3);
        for (uint32_t bit = 0; bit < 192; bit += 7) {
            mask.assign(3, 0);
            mask[bit >> 6] = 1ull << (bit & 63);
            for (uint32_t a = 0; a < 192; a++)
                for (uint32_t b = a; b < 192 && b - a <= 64; b++) EXPECT(diff_any_bit(mask.data(), a, b) == (a <= bit && bit <= b));
        }
        EXPECT(diff_bits(0, 63) == ~0ull && diff_bits(63, 63) == 1ull << 63 && diff_bits(0, 0) == 1ull);
    }
    // the sizes: W * H in 64 bits
    EXPECT(diff_pixels(65535, 65537) == 0xffffffffull && !diff_shape_ok(65535, 65537));   // 2^32 - 1 pixels, but a side too long
    EXPECT(diff_pixels(all, all) == 0xfffffffe00000001ull && !diff_shape_ok(all, all));
    EXPECT(diff_shape_ok(65535, 65535) && diff_pixels(65535, 65535) == 4294836225ull);
    EXPECT(!diff_shape_ok(65536, 65536) && !diff_shape_ok(0, 1) && !diff_shape_ok(1, 0) && diff_shape_ok(1, 1) && !diff_shape_ok(65536, 1));
    if (failures) {
        std::printf("frame_diff_host: %d failures\n", failures);
        return 1;
    }
    std::printf("frame_diff_host: ok\n");
    return 0;
}
