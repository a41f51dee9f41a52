// The distance field through the C++ class surface: F frames of integrate() on a grid^3 volume, compute_esdf() as a host array and
// into a caller's handle, against the C ABI, and the refusals as exceptions.  Dumps the arrays for tests/test_cpp_esdf.py.
//
//   test_esdf <frames.u16 (F x 640 x 480)> <poses.f32 (F x 16, column-major)> <F> <grid> <max_distance> <out_dir>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
        std::cerr << "usage: test_esdf frames.u16 poses.f32 F grid max_distance out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t F = (size_t)atoi(argv[3]);
    const unsigned n = (unsigned)atoi(argv[4]);
    const float cap = (float)atof(argv[5]);
    const std::string out = argv[6];
    std::vector<uint16_t> depth(F * W * H);
    std::vector<float> poses(F * 16);
    if (!load(argv[1], depth) || !load(argv[2], poses)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    Camera *camera = Camera::default_depth_camera();
    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        volume.integrate(depth.data() + f * W * H, W, H, *camera);
    }
    delete camera;

    const size_t voxels = (size_t)n * n * n;
    const std::vector<float> capped = volume.compute_esdf(cap);
    const std::vector<float> filled = volume.compute_esdf(INFINITY, true);
    if (capped.size() != voxels || filled.size() != voxels) return 4;

    // the overload into a caller's handle is the C ABI's computation: same bytes, the info of this call
    tsdf_esdf *esdf = nullptr;
    if (tsdf_esdf_create(&esdf) != TSDF_OK) return 5;
    volume.compute_esdf(cap, false, esdf);
    tsdf_esdf_info info;
    if (tsdf_esdf_get_info(esdf, &info) != TSDF_OK) return 6;
    if (info.size[0] != n || info.size[1] != n || info.size[2] != n || info.flags != 0u || info.max_distance != cap || info.n_sites == 0) return 7;
    std::vector<float> through_handle(voxels), through_abi(voxels);
    if (tsdf_esdf_download(esdf, through_handle.data()) != TSDF_OK) return 8;
    if (memcmp(through_handle.data(), capped.data(), voxels * sizeof(float)) != 0) return 9;
    if (tsdf_volume_compute_esdf(volume.handle(), cap, 0u, esdf) != TSDF_OK || tsdf_esdf_download(esdf, through_abi.data()) != TSDF_OK) return 10;
    if (memcmp(through_abi.data(), capped.data(), voxels * sizeof(float)) != 0) return 11;
    const float *device = nullptr;
    if (tsdf_esdf_buffer(esdf, &device) != TSDF_OK || !device) return 12;

    // the refusals arrive as std::invalid_argument
    int threw = 0;
    const float bad[3] = {0.0f, -1.0f, NAN};
    for (int i = 0; i < 3; i++) {
        try {
            (void)volume.compute_esdf(bad[i]);
        } catch (const std::invalid_argument &) {
            threw++;
        }
    }
    try {
        volume.compute_esdf(cap, false, nullptr);
    } catch (const std::invalid_argument &) {
        threw++;
    }
    tsdf_esdf_destroy(esdf);
    if (threw != 4) return 13;

    dump(out + "/capped.f32", capped.data(), voxels * sizeof(float));
    dump(out + "/filled.f32", filled.data(), voxels * sizeof(float));
    std::printf("distance field ok: %zu voxels, %llu sites\n", voxels, (unsigned long long)info.n_sites);
    return 0;
}
