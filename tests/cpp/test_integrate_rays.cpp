// Ray integration through the C++ class surface: a 37 x 34 x 45 volume over 3000^3 mm at offset (60, -90, 120) takes the rays it is given
// -- all of them from the first origin, then, band only and with a range gate, each from its own origin -- with the scratch released in
// between, and the exceptions.  Dumps the volume's distances and weights for tests/test_cpp_integrate_rays.py.
//
//   test_integrate_rays <origins.f32 (n x 3)> <points.f32 (n x 3)> <n> <min_range> <max_range> <out_dir>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "TSDFVolume.hpp"
#include "tsdf_amd.h"

static void dump(const std::string &path, const void *p, size_t bytes) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char *)p, (std::streamsize)bytes);
}

template <typename T>
static bool load(const char *path, std::vector<T> &v) {
    std::ifstream f(path, std::ios::binary);
    f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(T)));
    return (bool)f;
}

template <typename Call>
static bool throws_invalid_argument(Call call) {
    try {
        call();
    } catch (const std::invalid_argument &) {
        return true;
    }
    return false;
}

int main(int argc, char **argv) {
    if (argc < 7) {
        std::cerr << "usage: test_integrate_rays origins.f32 points.f32 n min_range max_range out_dir" << std::endl;
        return 2;
    }
    const size_t n = (size_t)atoi(argv[3]);
    const float min_range = (float)atof(argv[4]), max_range = (float)atof(argv[5]);
    const std::string out = argv[6];
    std::vector<float3> origins(n), points(n);
    if (!load(argv[1], origins) || !load(argv[2], points)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{37, 34, 45}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    volume.offset(60.0f, -90.0f, 120.0f);
    // the refusals throw and change nothing: the parity below is made after them
    const std::vector<float3> two(origins.begin(), origins.begin() + 2), none;
    if (!throws_invalid_argument([&] { volume.integrate_rays(two, points); })) return 4;
    if (!throws_invalid_argument([&] { volume.integrate_rays(none, points); })) return 5;
    TSDFVolume with_nodes(TSDFVolume::UInt3{16, 16, 16}, TSDFVolume::Float3{1000.0f, 1000.0f, 1000.0f});
    (void)with_nodes.deformation();   // materialises the node array
    if (!throws_invalid_argument([&] { with_nodes.integrate_rays(origins, points); })) return 6;
    if (volume.integrate_rays(none, none) != 0) return 7;

    const std::vector<float3> first(origins.begin(), origins.begin() + 1);
    const uint64_t updated_a = volume.integrate_rays(first, points);
    volume.release_ray_scratch();
    const uint64_t updated_b = volume.integrate_rays(origins, points, true, min_range, max_range);
    const size_t voxels = (size_t)37 * 34 * 45;
    std::vector<float> distances(voxels), weights(voxels);
    if (tsdf_volume_get_distance_data(volume.handle(), distances.data()) != TSDF_OK) return 8;
    if (tsdf_volume_get_weight_data(volume.handle(), weights.data()) != TSDF_OK) return 9;
    dump(out + "/distances.f32", distances.data(), voxels * sizeof(float));
    dump(out + "/weights.f32", weights.data(), voxels * sizeof(float));
    std::printf("integrate_rays surface ok: %llu then %llu voxels updated\n", (unsigned long long)updated_a, (unsigned long long)updated_b);
    return 0;
}
