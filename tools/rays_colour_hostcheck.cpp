// Rules 1 - 6 and 9 - 10 of ray integration on the host: rays_walk_sdf (tsdf_amd/csrc/rays_walk.hpp), the function rays_scatter_colour_kernel
// runs a lane per ray, compiled for the CPU with the colour-aware `observe` of that kernel, over the calls tools/rays_colour_hostcheck.py
// writes out, compared per voxel with the (c_v, R_v, G_v, B_v) of the CPU reference (tests/rays_colour_ref.py).  A stand-alone program
// with its own main, meant to be built with -ffp-contract=off and the address and undefined-behaviour sanitizers; it runs no device code.
//
//   rays_colour_hostcheck <call file> ...     -> per file "differing entries", exit status 1 if any differ
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rays_walk.hpp"

struct CallHeader {
    uint32_t dims[3];
    float vs[3], offset[3], trunc, min_range, max_range;
    int32_t flags;
    uint32_t pad;
    uint64_t n, n_origins;
};

template <typename T>
static bool read_n(std::FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    uint64_t total = 0;
    for (int a = 1; a < argc; a++) {
        std::FILE *f = std::fopen(argv[a], "rb");
        CallHeader h;
        if (!f || std::fread(&h, sizeof(h), 1, f) != 1) return 2;
        std::vector<float> origins, points;
        std::vector<uint8_t> rgb;
        std::vector<uint64_t> expected;
        const size_t voxels = (size_t)h.dims[0] * h.dims[1] * h.dims[2];
        if (!read_n(f, origins, 3 * h.n_origins) || !read_n(f, points, 3 * h.n) || !read_n(f, rgb, 3 * h.n) || !read_n(f, expected, 4 * voxels)) return 3;
        std::fclose(f);
        tsdf::Geom g = {};
        g.X = h.dims[0], g.Y = h.dims[1], g.Z = h.dims[2];
        g.z_store_end = g.Z;
        g.vs = {h.vs[0], h.vs[1], h.vs[2]};
        g.offset = {h.offset[0], h.offset[1], h.offset[2]};
        g.trunc = h.trunc;
        std::vector<uint64_t> got(4 * voxels, 0);
        const size_t row = g.X, plane = (size_t)g.X * g.Y;
        for (uint64_t i = 0; i < h.n; i++) {
            const float *const o = origins.data() + (h.n_origins == h.n && h.n > 1 ? 3 * i : 0), *const p = points.data() + 3 * i;
            const uint8_t *const c = rgb.data() + 3 * i;
            tsdf::rays_walk_sdf(g, o[0], o[1], o[2], p[0], p[1], p[2], h.min_range, h.max_range, h.flags & 1, [&](int ix, int iy, int iz, int, float sdf) {
                if (!(sdf <= g.trunc)) return;
                uint64_t *const e = &got.at(4 * (plane * (size_t)iz + row * (size_t)iy + (size_t)ix));
                e[0] += 1, e[1] += c[0], e[2] += c[1], e[3] += c[2];
            });
        }
        uint64_t differing = 0, coloured = 0;
        for (size_t v = 0; v < voxels; v++) {
            coloured += expected[4 * v] != 0;
            for (int k = 0; k < 4; k++) differing += got[4 * v + k] != expected[4 * v + k];
        }
        std::printf("%s: %llu rays, %llu coloured voxels, %llu differing entries\n", argv[a], (unsigned long long)h.n, (unsigned long long)coloured,
                    (unsigned long long)differing);
        total += differing;
    }
    std::printf("%d calls compared, %llu differing entries\n", argc - 1, (unsigned long long)total);
    return total ? 1 : 0;
}
