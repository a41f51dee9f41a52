// Weighted integration through the C++ class surface: TSDFVolume::depth_weights (static) and TSDFVolume::integrate_weighted over F
// frames, the refusals as std::invalid_argument, the storage afterwards.  Dumps the weights of every frame and the volume for
// tests/test_cpp_weighted.py.
//
//   test_weighted <frames.u16 (F x 640 x 480)> <poses.f32 (F x 16, column-major)> <F> <grid> <flags> <z_ref> <out_dir>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
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

template <typename Fn>
static bool refused(Fn fn, const char *word) {
    try {
        fn();
    } catch (const std::invalid_argument &e) {
        return std::string(e.what()).find(word) != std::string::npos;
    }
    return false;
}

int main(int argc, char **argv) {
    if (argc < 8) {
        std::cerr << "usage: test_weighted frames.u16 poses.f32 F grid flags z_ref out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t F = (size_t)atoi(argv[3]);
    const unsigned n = (unsigned)atoi(argv[4]);
    const uint32_t flags = (uint32_t)atoi(argv[5]);
    const float z_ref = (float)atof(argv[6]);
    const std::string out = argv[7];
    std::vector<uint16_t> depth(F * W * H);
    std::vector<float> poses(F * 16);
    if (!load(argv[1], depth) || !load(argv[2], poses)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    Camera *camera = Camera::default_depth_camera();
    if (!refused([&] { TSDFVolume::depth_weights(depth.data(), W, H, *camera, 4u, 1.0f); }, "unknown flag bits")) return 4;
    if (!refused([&] { TSDFVolume::depth_weights(depth.data(), W, H, *camera, TSDF_WEIGHTS_INVERSE_SQUARE, 0.0f); }, "z_ref")) return 5;
    if (!refused([&] { volume.integrate_weighted(depth.data(), nullptr, W, H, *camera); }, "null argument")) return 6;
    std::vector<float> ones((size_t)W * H, 1.0f);
    std::vector<uint8_t> rgb((size_t)W * H * 3, 0);
    if (!refused([&] { volume.integrate_weighted(depth.data(), ones.data(), W, H, *camera, rgb.data()); }, "colour is not enabled")) return 7;

    std::vector<float> all_weights;
    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        const uint16_t *d = depth.data() + f * W * H;
        const std::vector<float> w = TSDFVolume::depth_weights(d, W, H, *camera, flags, z_ref);
        if (w.size() != (size_t)W * H) return 8;
        all_weights.insert(all_weights.end(), w.begin(), w.end());
        volume.integrate_weighted(d, w.data(), W, H, *camera);
    }
    delete camera;
    int bits = 0, pinned = 0;
    if (tsdf_volume_weight_storage(volume.handle(), &bits, &pinned) != TSDF_OK || bits != 32) return 9;
    std::vector<float> w((size_t)n * n * n), d(w.size());
    if (tsdf_volume_get_weight_data(volume.handle(), w.data()) != TSDF_OK) return 10;
    if (tsdf_volume_get_distance_data(volume.handle(), d.data()) != TSDF_OK) return 11;
    dump(out + "/pixel_weights.f32", all_weights.data(), all_weights.size() * sizeof(float));
    dump(out + "/weights.f32", w.data(), w.size() * sizeof(float));
    dump(out + "/distances.f32", d.data(), d.size() * sizeof(float));
    std::printf("weighted surface ok: %zu frames, flags %u\n", F, flags);
    return 0;
}
