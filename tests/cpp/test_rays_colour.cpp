// Coloured ray integration and the colour at ray-query hits through the C++ class surface: a colour-enabled 37 x 34 x 45 volume over
// 3000^3 mm at offset (60, -90, 120), its colour words set from a file, takes the coloured rays it is given -- all of them from the first
// origin, then, band only and with a range gate, each from its own origin -- with the scratch released in between, casts the same rays
// back with colours, and checks the exceptions.  Dumps distances, weights, colour words, hit points and hit colours for
// tests/test_cpp_rays_colour.py.
//
//   test_rays_colour <origins.f32 (n x 3)> <points.f32 (n x 3)> <rgb.u8 (n x 3)> <words.u32 (voxels)> <directions.f32 (n x 3)> <n> <min_range>
//                    <max_range> <out_dir>
#include <cmath>
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
    if (argc < 10) {
        std::cerr << "usage: test_rays_colour origins.f32 points.f32 rgb.u8 words.u32 directions.f32 n min_range max_range out_dir" << std::endl;
        return 2;
    }
    const size_t n = (size_t)atoi(argv[6]), voxels = (size_t)37 * 34 * 45;
    const float min_range = (float)atof(argv[7]), max_range = (float)atof(argv[8]);
    const std::string out = argv[9];
    std::vector<float3> origins(n), points(n), directions(n);
    std::vector<uchar3> rgb(n);
    std::vector<uint32_t> words(voxels);
    if (!load(argv[1], origins) || !load(argv[2], points) || !load(argv[3], rgb) || !load(argv[4], words) || !load(argv[5], directions)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{37, 34, 45}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    volume.offset(60.0f, -90.0f, 120.0f);
    const std::vector<float3> first(origins.begin(), origins.begin() + 1);
    std::vector<float3> hits;
    std::vector<uchar3> hit_colours;
    // without colour enabled both throw, and no scratch is taken
    if (!throws_invalid_argument([&] { volume.integrate_rays(first, points, rgb); })) return 4;
    if (!throws_invalid_argument([&] { volume.cast_rays(origins, points, hits, hit_colours); })) return 5;
    if (volume.ray_scratch_bytes() != 0) return 6;
    volume.enable_colour(true);
    if (tsdf_volume_set_colour_data(volume.handle(), words.data()) != TSDF_OK) return 7;
    // the refusals throw and change nothing: the parity below is made after them
    const std::vector<uchar3> short_rgb(rgb.begin(), rgb.end() - 1);
    const std::vector<float3> two(origins.begin(), origins.begin() + 2);
    if (!throws_invalid_argument([&] { volume.integrate_rays(first, points, short_rgb); })) return 8;
    if (!throws_invalid_argument([&] { volume.integrate_rays(two, points, rgb); })) return 9;
    if (volume.integrate_rays(std::vector<float3>(), std::vector<float3>(), std::vector<uchar3>()) != 0) return 10;

    const uint64_t updated_a = volume.integrate_rays(first, points, rgb);
    if (volume.ray_scratch_bytes() < 24 * voxels) return 11;
    volume.release_ray_scratch();
    if (volume.ray_scratch_bytes() != 0) return 12;
    const uint64_t updated_b = volume.integrate_rays(origins, points, rgb, true, min_range, max_range);

    std::vector<float> distances(voxels), weights(voxels);
    if (tsdf_volume_get_distance_data(volume.handle(), distances.data()) != TSDF_OK) return 13;
    if (tsdf_volume_get_weight_data(volume.handle(), weights.data()) != TSDF_OK) return 14;
    if (tsdf_volume_get_colour_data(volume.handle(), words.data()) != TSDF_OK) return 15;
    // every ray cast back from its own origin along the direction given
    std::vector<float> t;
    volume.cast_rays(origins, directions, hits, hit_colours, &t);
    if (hits.size() != n || hit_colours.size() != n || t.size() != n) return 16;
    dump(out + "/distances.f32", distances.data(), voxels * sizeof(float));
    dump(out + "/weights.f32", weights.data(), voxels * sizeof(float));
    dump(out + "/colours.u32", words.data(), voxels * sizeof(uint32_t));
    dump(out + "/hits.f32", hits.data(), n * sizeof(float3));
    dump(out + "/hit_colours.u8", hit_colours.data(), n * sizeof(uchar3));
    std::printf("rays colour surface ok: %llu then %llu voxels updated\n", (unsigned long long)updated_a, (unsigned long long)updated_b);
    return 0;
}
