// Colour alignment through the C++ class surface: the 48 x 48 x 24 wall volume of tests/align_colour_ref.py set by upload,
// TSDFVolume::sample_intensity and the TSDFVolume::align_points overload with intensities from the pose given, and the exceptions.
// Dumps the pose, the sampled intensities and gradients for tests/test_cpp_align_colour.py.
//
//   test_align_colour <dist.f32> <weight.f32> <colour.u32> <points.f32 (n x 3)> <intensity.f32 (n)> <n> <T0.f64 (16, column-major)>
//                     <iterations> <gate> <colour_gate> <colour_weight> <out_dir>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "TSDFVolume.hpp"
#include "tsdf_amd.h"

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
    if (argc < 13) {
        std::cerr << "usage: test_align_colour dist.f32 weight.f32 colour.u32 points.f32 intensity.f32 n T0.f64 iterations gate colour_gate colour_weight out_dir"
                  << std::endl;
        return 2;
    }
    const size_t voxels = 48 * 48 * 24, n = (size_t)atoi(argv[6]);
    const uint32_t iterations = (uint32_t)atoi(argv[8]);
    const float gate = (float)atof(argv[9]), colour_gate = (float)atof(argv[10]), colour_weight = (float)atof(argv[11]);
    const std::string out = argv[12];
    std::vector<float> dist(voxels), weight(voxels), intensity(n);
    std::vector<uint32_t> colour(voxels);
    std::vector<float3> points(n);
    std::vector<double> t0(16);
    if (!load(argv[1], dist) || !load(argv[2], weight) || !load(argv[3], colour) || !load(argv[4], points) || !load(argv[5], intensity) ||
        !load(argv[7], t0))
        return 3;
    Eigen::Matrix4d T0;
    for (int i = 0; i < 16; i++) T0.data()[i] = t0[i];

    TSDFVolume volume(TSDFVolume::UInt3{48, 48, 24}, TSDFVolume::Float3{480.0f, 480.0f, 240.0f});
    volume.offset(-240.0f, -240.0f, 380.0f);
    volume.set_distance_data(dist.data());
    volume.set_weight_data(weight.data());
    // while colour is off both calls throw
    if (!throws_invalid_argument([&] { volume.sample_intensity(points); })) return 4;
    if (!throws_invalid_argument([&] { volume.align_points(points, intensity, T0, colour_gate, colour_weight); })) return 5;
    volume.enable_colour(true);
    if (tsdf_volume_set_colour_data(volume.handle(), colour.data()) != TSDF_OK) return 6;

    // the refusals throw
    Eigen::Matrix4d bad = T0;
    bad.data()[13] = NAN;
    if (!throws_invalid_argument([&] { volume.align_points(points, intensity, bad, colour_gate, colour_weight); })) return 7;
    if (!throws_invalid_argument([&] { volume.align_points(points, intensity, T0, 0.0f, colour_weight); })) return 8;
    if (!throws_invalid_argument([&] { volume.align_points(points, intensity, T0, NAN, colour_weight); })) return 9;
    if (!throws_invalid_argument([&] { volume.align_points(points, intensity, T0, colour_gate, -1.0f); })) return 10;
    if (!throws_invalid_argument([&] { volume.align_points(points, intensity, T0, colour_gate, INFINITY); })) return 11;
    if (!throws_invalid_argument([&] { volume.align_points(points, std::vector<float>(n + 1, 0.0f), T0, colour_gate, colour_weight); })) return 12;

    // no points: the pose as given, no inliers of either term
    float residual[2] = {-1.0f, -1.0f}, inliers[2] = {-1.0f, -1.0f};
    const Eigen::Matrix4d same =
        volume.align_points(std::vector<float3>(), std::vector<float>(), T0, colour_gate, colour_weight, 10, gate, residual, inliers);
    for (int i = 0; i < 16; i++)
        if (same.data()[i] != T0.data()[i]) return 13;
    if (inliers[0] != 0.0f || inliers[1] != 0.0f) return 14;
    if (!volume.sample_intensity(std::vector<float3>()).empty()) return 15;

    std::vector<float3> gradient;
    const std::vector<float> sampled = volume.sample_intensity(points, &gradient);
    if (sampled.size() != n || gradient.size() != n) return 16;
    const std::vector<float> alone = volume.sample_intensity(points);
    for (size_t i = 0; i < n; i++)
        if (!(alone[i] == sampled[i] || (std::isnan(alone[i]) && std::isnan(sampled[i])))) return 17;
    std::ofstream fi(out + "/intensity.f32", std::ios::binary), fg(out + "/gradient.f32", std::ios::binary);
    fi.write((const char *)sampled.data(), (std::streamsize)(n * sizeof(float)));
    fg.write((const char *)gradient.data(), (std::streamsize)(n * sizeof(float3)));

    const Eigen::Matrix4d T = volume.align_points(points, intensity, T0, colour_gate, colour_weight, iterations, gate, residual, inliers);
    std::ofstream f(out + "/pose.f64", std::ios::binary);
    f.write((const char *)T.data(), 16 * sizeof(double));
    std::printf("colour align surface ok: residual %.9g %.9g inliers %.9g %.9g\n", (double)residual[0], (double)residual[1], (double)inliers[0],
                (double)inliers[1]);
    return 0;
}
