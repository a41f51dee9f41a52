// The weight cap through the C++ class surface: TSDFVolume::weight_cap(cap) / weight_cap(), F frames of integrate(), the largest
// weight, and std::invalid_argument for a cap above 65535.  Dumps the weights and distances for tests/test_cpp_weight_cap.py.
//
//   test_weight_cap <frames.u16 (F x 640 x 480)> <poses.f32 (F x 16, column-major)> <F> <grid> <cap> <out_dir>
#include <algorithm>
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

int main(int argc, char **argv) {
    if (argc < 7) {
        std::cerr << "usage: test_weight_cap frames.u16 poses.f32 F grid cap out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t F = (size_t)atoi(argv[3]);
    const unsigned n = (unsigned)atoi(argv[4]);
    const uint32_t cap = (uint32_t)atoi(argv[5]);
    const std::string out = argv[6];
    std::vector<uint16_t> depth(F * W * H);
    std::vector<float> poses(F * 16);
    if (!load(argv[1], depth) || !load(argv[2], poses)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    if (volume.weight_cap() != 0) return 4;   // off by default
    bool threw = false;
    try {
        volume.weight_cap(65536u);
    } catch (const std::invalid_argument &e) {
        threw = std::string(e.what()).find("65535") != std::string::npos;
    }
    if (!threw || volume.weight_cap() != 0) return 5;
    volume.weight_cap(cap);
    if (volume.weight_cap() != cap) return 6;

    Camera *camera = Camera::default_depth_camera();
    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        volume.integrate(depth.data() + f * W * H, W, H, *camera);
    }
    delete camera;
    std::vector<float> w((size_t)n * n * n), d(w.size());
    if (tsdf_volume_get_weight_data(volume.handle(), w.data()) != TSDF_OK) return 7;
    if (tsdf_volume_get_distance_data(volume.handle(), d.data()) != TSDF_OK) return 8;
    const float top = *std::max_element(w.begin(), w.end());
    if (top != (float)cap) {
        std::fprintf(stderr, "largest weight %g, cap %u\n", top, cap);
        return 9;
    }
    volume.clear();
    if (volume.weight_cap() != cap) return 10;   // clear() keeps the cap
    dump(out + "/weights.f32", w.data(), w.size() * sizeof(float));
    dump(out + "/distances.f32", d.data(), d.size() * sizeof(float));
    std::printf("weight cap surface ok: largest weight %g after %zu frames\n", top, F);
    return 0;
}
