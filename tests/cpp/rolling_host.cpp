// Host-side run of the rolling volume's brick arithmetic (tsdf_amd/csrc/brick_shift.hpp) under the address and undefined-behaviour
// sanitizers (`make sanitize-rolling`): every shift is an int32 and everything is formed in 64 bits, so nothing may wrap -- a signed
// overflow here is a sanitizer report.  Against brute force on small grids, and at the ends of the int32 range.  Needs no GPU and links
// nothing of the library.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brick_shift.hpp"

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
    const int32_t ends[] = {INT32_MIN, INT32_MIN + 1, -8193, -9, -8, -3, -1, 0, 1, 2, 7, 8, 8191, 8192, INT32_MAX - 1, INT32_MAX};
    const uint32_t grids[][3] = {{1, 1, 1}, {2, 1, 3}, {5, 5, 3}, {33, 8, 5}, {8192, 1, 1}};
    uint32_t out[3];
    for (const auto &nb : grids)
        for (int32_t sx : ends)
            for (int32_t sy : ends)
                for (int32_t sz : {INT32_MIN, -1, 0, 1, INT32_MAX}) {
                    // as tsdf_volume_restore_shifted forms it, and negated as tsdf_volume_shift does
                    for (int sign : {1, -1}) {
                        const BrickShift s = {sign * (long long)sx, sign * (long long)sy, sign * (long long)sz, nb[0], nb[1], nb[2]};
                        for (uint32_t b : {0u, nb[0] - 1u}) {
                            const bool in = brick_moved(s, b, nb[1] - 1u, 0u, out);
                            const long long x = (long long)b + s.x, y = (long long)(nb[1] - 1u) + s.y, z = s.z;
                            const bool want = x >= 0 && x < (long long)nb[0] && y >= 0 && y < (long long)nb[1] && z >= 0 && z < (long long)nb[2];
                            EXPECT(in == want);
                            if (in) EXPECT(out[0] == (uint32_t)x && out[1] == (uint32_t)y && out[2] == (uint32_t)z);
                        }
                    }
                    // the bricks that stay when the box moves by (sx, sy, sz): b - shift in [0, nb)
                    const int32_t shift[3] = {sx, sy, sz};
                    const BrickBox box = staying_box(shift, nb);
                    const BrickShift back = {-(long long)sx, -(long long)sy, -(long long)sz, nb[0], nb[1], nb[2]};
                    for (uint32_t bx : {0u, nb[0] / 2u, nb[0] - 1u})
                        for (uint32_t bz : {0u, nb[2] - 1u})
                            EXPECT(brick_in_box(box, bx, nb[1] - 1u, bz) == brick_moved(back, bx, nb[1] - 1u, bz, out));
                }
    // every brick of a small grid, every small shift: a shift there and its negation back is the identity where it lands inside
    const uint32_t nb[3] = {4, 3, 2};
    for (long long sx = -5; sx <= 5; sx++)
        for (long long sy = -4; sy <= 4; sy++)
            for (long long sz = -3; sz <= 3; sz++) {
                const BrickShift there = {sx, sy, sz, nb[0], nb[1], nb[2]}, back = {-sx, -sy, -sz, nb[0], nb[1], nb[2]};
                int landed = 0;
                for (uint32_t z = 0; z < nb[2]; z++)
                    for (uint32_t y = 0; y < nb[1]; y++)
                        for (uint32_t x = 0; x < nb[0]; x++) {
                            uint32_t d[3], s[3];
                            if (!brick_moved(there, x, y, z, d)) continue;
                            landed++;
                            EXPECT(brick_moved(back, d[0], d[1], d[2], s) && s[0] == x && s[1] == y && s[2] == z);
                        }
                const long long ox = 4 - std::llabs(sx), oy = 3 - std::llabs(sy), oz = 2 - std::llabs(sz);
                EXPECT(landed == (ox > 0 && oy > 0 && oz > 0 ? (int)(ox * oy * oz) : 0));
            }
    // boxes at the ends of the range
    const BrickBox all = {{INT32_MIN, INT32_MIN, INT32_MIN}, {INT32_MAX, INT32_MAX, INT32_MAX}}, none = {{3, 0, 0}, {2, 9, 9}};
    EXPECT(brick_in_box(all, 0, 0, 0) && brick_in_box(all, 8191, 8191, 8191) && !brick_in_box(none, 2, 0, 0) && !brick_in_box(none, 3, 0, 0));
    // the offset rule: exact products, one rounding per operation
    EXPECT(shifted_offset(100.0f, 1, 10.0f) == 180.0f && shifted_offset(-50.0f, -3, 12.5f) == -350.0f && shifted_offset(25.0f, 0, 9.0f) == 25.0f);
    EXPECT(shifted_offset(0.0f, INT32_MAX, 1.0f) == 17179869184.0f && shifted_offset(0.0f, INT32_MIN, 1.0f) == -17179869184.0f);
    std::printf(failures ? "brick arithmetic: %d failures\n" : "brick arithmetic ok\n", failures);
    return failures ? 1 : 0;
}
