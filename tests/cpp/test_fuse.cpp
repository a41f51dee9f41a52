// Volume fusion through the C++ class surface: a destination of 48 x 40 x 36 voxels fused from the first Fd frames, a source of 40^3
// voxels at offset (100, -50, 80) fused from the next Fs frames, TSDFVolume::fuse through the matrix given, and the exceptions.  Dumps
// the destination's distances and weights for tests/test_cpp_fuse.py.
//
//   test_fuse <frames.u16 ((Fd + Fs) x 640 x 480)> <poses.f32 ((Fd + Fs) x 16, column-major)> <Fd> <Fs> <matrix.f32 (16)> <out_dir>
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
    if (argc < 7) {
        std::cerr << "usage: test_fuse frames.u16 poses.f32 Fd Fs matrix.f32 out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t Fd = (size_t)atoi(argv[3]), Fs = (size_t)atoi(argv[4]);
    const std::string out = argv[6];
    std::vector<uint16_t> depth((Fd + Fs) * W * H);
    std::vector<float> poses((Fd + Fs) * 16), matrix(16);
    if (!load(argv[1], depth) || !load(argv[2], poses) || !load(argv[5], matrix)) return 3;

    TSDFVolume dst(TSDFVolume::UInt3{48, 40, 36}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    TSDFVolume src(TSDFVolume::UInt3{40, 40, 40}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    src.offset(100.0f, -50.0f, 80.0f);
    Camera *camera = Camera::default_depth_camera();
    for (size_t f = 0; f < Fd + Fs; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        (f < Fd ? dst : src).integrate(depth.data() + f * W * H, W, H, *camera);
    }
    delete camera;

    Eigen::Matrix4f m;
    for (int i = 0; i < 16; i++) m.data()[i] = matrix[i];
    // the refusals throw and change nothing: the parity below is made after them
    Eigen::Matrix4f bad = m;
    bad.data()[13] = NAN;
    if (!throws_invalid_argument([&] { dst.fuse(dst, m); })) return 4;
    if (!throws_invalid_argument([&] { dst.fuse(src, bad); })) return 5;
    TSDFVolume with_nodes(TSDFVolume::UInt3{16, 16, 16}, TSDFVolume::Float3{1000.0f, 1000.0f, 1000.0f});
    (void)with_nodes.deformation();   // materialises the node array
    if (!throws_invalid_argument([&] { dst.fuse(with_nodes, m); })) return 6;
    if (!throws_invalid_argument([&] { with_nodes.fuse(src, m); })) return 7;

    const uint64_t fused = dst.fuse(src, m);
    const size_t n = (size_t)48 * 40 * 36;
    std::vector<float> distances(n), weights(n);
    if (tsdf_volume_get_distance_data(dst.handle(), distances.data()) != TSDF_OK) return 8;
    if (tsdf_volume_get_weight_data(dst.handle(), weights.data()) != TSDF_OK) return 9;
    dump(out + "/distances.f32", distances.data(), n * sizeof(float));
    dump(out + "/weights.f32", weights.data(), n * sizeof(float));
    std::printf("fuse surface ok: %llu voxels fused\n", (unsigned long long)fused);
    return 0;
}
