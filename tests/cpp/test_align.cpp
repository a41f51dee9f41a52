// Field alignment through the C++ class surface: a 37 x 34 x 45 volume of 2900 x 3100 x 3300 mm at offset (-150, 40, 275) fused from F
// frames, TSDFVolume::align_points of the points given from the pose given, and the exceptions.  Dumps the pose, the residual and the
// inlier count for tests/test_cpp_align.py.
//
//   test_align <frames.u16 (F x 640 x 480)> <poses.f32 (F x 16, column-major)> <F> <points.f32 (n x 3)> <n> <T0.f64 (16, column-major)> <iterations> <out_dir>
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
    if (argc < 9) {
        std::cerr << "usage: test_align frames.u16 poses.f32 F points.f32 n T0.f64 iterations out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t F = (size_t)atoi(argv[3]), n = (size_t)atoi(argv[5]);
    const uint32_t iterations = (uint32_t)atoi(argv[7]);
    const std::string out = argv[8];
    std::vector<uint16_t> depth(F * W * H);
    std::vector<float> poses(F * 16);
    std::vector<float3> points(n);
    std::vector<double> t0(16);
    if (!load(argv[1], depth) || !load(argv[2], poses) || !load(argv[4], points) || !load(argv[6], t0)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{37, 34, 45}, TSDFVolume::Float3{2900.0f, 3100.0f, 3300.0f});
    volume.offset(-150.0f, 40.0f, 275.0f);
    Camera *camera = Camera::default_depth_camera();
    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        volume.integrate(depth.data() + f * W * H, W, H, *camera);
    }
    delete camera;

    Eigen::Matrix4d T0;
    for (int i = 0; i < 16; i++) T0.data()[i] = t0[i];
    // the refusals throw
    Eigen::Matrix4d bad = T0;
    bad.data()[13] = NAN;
    if (!throws_invalid_argument([&] { volume.align_points(points, bad); })) return 4;
    bad = T0;
    bad.data()[5] = INFINITY;
    if (!throws_invalid_argument([&] { volume.align_points(points, bad); })) return 5;
    if (!throws_invalid_argument([&] { volume.align_points(points, T0, 10, NAN); })) return 6;

    // no points: the pose as given, no inliers
    float residual = -1.0f, inliers = -1.0f;
    const Eigen::Matrix4d same = volume.align_points(std::vector<float3>(), T0, 10, 0.0f, &residual, &inliers);
    for (int i = 0; i < 16; i++)
        if (same.data()[i] != T0.data()[i]) return 7;
    if (inliers != 0.0f) return 8;

    const Eigen::Matrix4d T = volume.align_points(points, T0, iterations, 0.0f, &residual, &inliers);
    std::ofstream f(out + "/pose.f64", std::ios::binary);
    f.write((const char *)T.data(), 16 * sizeof(double));
    std::printf("align surface ok: residual %.9g inliers %.9g\n", (double)residual, (double)inliers);
    return 0;
}
