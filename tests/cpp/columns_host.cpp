// Host-side run of the column maps' cell and band arithmetic (tsdf_amd/csrc/columns_index.hpp) under the address and
// undefined-behaviour sanitizers (`make sanitize-columns`): map axes, the voxel of every step of every cell against brute force on small
// grids, the strided walk against the same, the reversed index, the refusals, and the ends of the range -- the longest axis a map
// takes and a grid of 2^32 - 1 voxels, where U * V * L and the walk's products must be formed in 64 bits: a signed overflow here is a
// sanitizer report.  Needs no GPU and links nothing of the library.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "columns_index.hpp"

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
    // rule 2: the two other axes, ascending
    const uint32_t want_axes[3][2] = {{1, 2}, {0, 2}, {0, 1}};
    for (uint32_t axis = 0; axis < 3; axis++) {
        uint32_t au, av;
        columns_map_axes(axis, au, av);
        EXPECT(au == want_axes[axis][0] && av == want_axes[axis][1]);
    }
    // every cell and step of small grids: each voxel of the band is visited exactly once, forward and reversed visit the same voxels in
    // opposite order, and the strided walk names the same voxel as the coordinates do
    const uint32_t grids[][3] = {{1, 1, 1}, {5, 3, 2}, {2, 7, 3}, {4, 4, 9}, {65, 2, 3}};
    for (const auto &N : grids)
        for (uint32_t axis = 0; axis < 3; axis++)
            for (uint32_t lo = 0; lo < N[axis]; lo++)
                for (uint32_t hi = lo + 1; hi <= N[axis]; hi++) {
                    ColumnsShape fwd, rev;
                    EXPECT(columns_shape(N, axis, lo, hi, false, fwd) && columns_shape(N, axis, lo, hi, true, rev));
                    EXPECT(fwd.L == hi - lo && fwd.U == N[fwd.au] && fwd.V == N[fwd.av] && fwd.reversed == 0 && rev.reversed == 1);
                    EXPECT(columns_cells(fwd) == (uint64_t)fwd.U * fwd.V && columns_voxels(fwd) == (uint64_t)fwd.U * fwd.V * (hi - lo));
                    std::vector<int> seen((size_t)N[0] * N[1] * N[2], 0);
                    for (uint32_t v = 0; v < fwd.V; v++)
                        for (uint32_t u = 0; u < fwd.U; u++) {
                            const ColumnsWalk wf = columns_walk(fwd, u, v), wr = columns_walk(rev, u, v);
                            for (uint32_t p = 0; p < fwd.L; p++) {
                                uint32_t x, y, z, c[3];
                                columns_voxel(fwd, u, v, p, x, y, z);
                                c[0] = x; c[1] = y; c[2] = z;
                                EXPECT(c[fwd.au] == u && c[fwd.av] == v && c[axis] == lo + p && x < N[0] && y < N[1] && z < N[2]);
                                const uint64_t id = columns_voxel_id(fwd, x, y, z);
                                EXPECT(id == ((uint64_t)z * N[1] + y) * N[0] + x && id < seen.size());
                                if (id < seen.size()) seen[(size_t)id]++;
                                const int64_t xy = (int64_t)N[0] * N[1];
                                EXPECT((uint64_t)(xy * (wf.z0 + p * wf.z_step) + wf.ip0 + p * wf.ip_step) == id);
                                uint32_t rx, ry, rz;
                                columns_voxel(rev, u, v, fwd.L - 1 - p, rx, ry, rz);
                                EXPECT(rx == x && ry == y && rz == z);
                                const int64_t q = fwd.L - 1 - p;
                                EXPECT((uint64_t)(xy * (wr.z0 + q * wr.z_step) + wr.ip0 + q * wr.ip_step) == id);
                            }
                        }
                    // the groups of four steps: every step once; aligned with the packed dwords along z, so that a group's steps share
                    // z >> 2 and each of its pairs z >> 1
                    for (const ColumnsShape *sh : {&fwd, &rev})
                        for (bool align : {false, true}) {
                            const uint32_t pad = columns_group_pad(*sh, align), n_groups = columns_groups(*sh, pad);
                            EXPECT(pad <= 3 && (pad == 0 || (align && axis == 2)));
                            uint64_t steps = 0;
                            for (uint32_t k = 0; k < n_groups; k++) {
                                int64_t z4 = -1, z2[2] = {-1, -1};
                                uint32_t in_group = 0;
                                for (uint32_t t = 0; t < kColumnsGroup; t++) {
                                    const int64_t p = (int64_t)k * kColumnsGroup - pad + t;
                                    if (p < 0 || p >= (int64_t)sh->L) continue;
                                    EXPECT((uint64_t)p == steps);
                                    steps++;
                                    in_group++;
                                    if (!(align && axis == 2)) continue;
                                    const int64_t z = columns_axis_index(*sh, (uint32_t)p);
                                    EXPECT(z4 < 0 || z4 == (z >> 2));
                                    EXPECT(z2[t / 2] < 0 || z2[t / 2] == (z >> 1));
                                    z4 = z >> 2;
                                    z2[t / 2] = z >> 1;
                                }
                                EXPECT(in_group > 0);
                            }
                            EXPECT(steps == sh->L);
                        }
                    uint64_t visited = 0, twice = 0;
                    for (int n : seen) {
                        visited += n > 0;
                        twice += n > 1;
                    }
                    EXPECT(visited == columns_voxels(fwd) && twice == 0);
                }
    // hi == 0 is the axis' end
    const uint32_t N[3] = {7, 5, 3};
    ColumnsShape s;
    EXPECT(columns_shape(N, 1, 2, 0, false, s) && s.lo == 2 && s.hi == 5 && s.L == 3);
    EXPECT(columns_shape(N, 2, 0, 0, true, s) && s.hi == 3 && columns_axis_index(s, 0) == 2 && columns_axis_index(s, 2) == 0);
    // what rule 8 refuses
    EXPECT(!columns_shape(N, 3, 0, 0, false, s) && !columns_shape(N, 0xffffffffu, 0, 0, false, s));
    EXPECT(!columns_shape(N, 0, 7, 0, false, s) && !columns_shape(N, 0, 3, 3, false, s) && !columns_shape(N, 0, 4, 3, false, s));
    EXPECT(!columns_shape(N, 0, 0, 8, false, s) && !columns_shape(N, 1, 0, 0xffffffffu, false, s) && !columns_shape(N, 2, 0xffffffffu, 0, false, s));
    const uint32_t empty[3] = {4, 0, 4};
    EXPECT(!columns_shape(empty, 0, 0, 0, false, s));
    // the ends of the range: the longest axis, and the most voxels a grid may have (2^32 - 1 = 65535 * 65537)
    const uint32_t too_long[3] = {0x80000000u, 1, 1}, longest[3] = {kColumnsMaxAxis, 1, 2};
    EXPECT(!columns_shape(too_long, 0, 0, 0, false, s) && columns_shape(too_long, 1, 0, 0, false, s) && s.U == 0x80000000u && s.L == 1);
    for (bool reversed : {false, true}) {
        EXPECT(columns_shape(longest, 0, 0, 0, reversed, s) && s.L == kColumnsMaxAxis && columns_voxels(s) == 2ull * kColumnsMaxAxis);
        const uint32_t last = s.L - 1;
        EXPECT(columns_axis_index(s, last) == (reversed ? 0u : last) && columns_axis_index(s, 0) == (reversed ? last : 0u));
        const ColumnsWalk w = columns_walk(s, 0, 1);
        uint32_t x, y, z;
        columns_voxel(s, 0, 1, last, x, y, z);
        EXPECT((uint64_t)((int64_t)kColumnsMaxAxis * (w.z0 + (int64_t)last * w.z_step) + w.ip0 + (int64_t)last * w.ip_step) == columns_voxel_id(s, x, y, z));
    }
    // the most groups a walk has: along z over the longest axis, padded
    const uint32_t tall[3] = {1, 2, kColumnsMaxAxis};
    EXPECT(columns_shape(tall, 2, 3, 0, false, s) && columns_group_pad(s, true) == 3 && columns_groups(s, 3) == 0x20000000u);
    EXPECT(columns_shape(tall, 2, 0, kColumnsMaxAxis - 3, true, s) && columns_group_pad(s, true) == 0 && columns_groups(s, 0) == 0x1fffffffu);
    const uint32_t wide[3] = {65535, 65537, 1};
    for (uint32_t axis = 0; axis < 3; axis++)
        for (bool reversed : {false, true}) {
            EXPECT(columns_shape(wide, axis, 0, 0, reversed, s) && columns_voxels(s) == 0xffffffffull);
            const uint32_t u = s.U - 1, v = s.V - 1, last = s.L - 1;
            const ColumnsWalk w = columns_walk(s, u, v);
            for (uint32_t p : {0u, last}) {
                uint32_t x, y, z;
                columns_voxel(s, u, v, p, x, y, z);
                const uint64_t id = columns_voxel_id(s, x, y, z);
                EXPECT(id <= 0xfffffffeull);
                EXPECT((uint64_t)((int64_t)wide[0] * wide[1] * (w.z0 + (int64_t)p * w.z_step) + w.ip0 + (int64_t)p * w.ip_step) == id);
            }
        }
    std::printf(failures ? "column arithmetic: %d failures\n" : "column arithmetic ok\n", failures);
    return failures ? 1 : 0;
}
