// The exploration queries through the C++ class surface: F frames of integrate() on a grid^3 volume, find_frontiers() into an
// Explorer, its clusters, a view gain along a fan of rays, against the C ABI, and the refusals as exceptions.  Dumps the arrays for
// tests/test_cpp_explore.py.
//
//   test_explore <frames.u16 (F x 640 x 480)> <poses.f32 (F x 16, column-major)> <F> <grid> <rays.f32 (R x 6: origin, direction)> <R> <out_dir>
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
    if (argc < 8) {
        std::cerr << "usage: test_explore frames.u16 poses.f32 F grid rays.f32 R out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t F = (size_t)atoi(argv[3]);
    const unsigned n = (unsigned)atoi(argv[4]);
    const size_t R = (size_t)atoi(argv[6]);
    const std::string out = argv[7];
    std::vector<uint16_t> depth(F * W * H);
    std::vector<float> poses(F * 16), rays(R * 6);
    if (!load(argv[1], depth) || !load(argv[2], poses) || !load(argv[5], rays)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    Camera *camera = Camera::default_depth_camera();
    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        volume.integrate(depth.data() + f * W * H, W, H, *camera);
    }
    delete camera;

    TSDFVolume::Explorer explorer;
    volume.find_frontiers(explorer);
    const std::vector<uint32_t> voxels = explorer.voxels();
    const size_t total = (size_t)n * n * n;
    if (voxels.size() != explorer.n_frontiers() || voxels.empty()) return 4;
    if (explorer.n_unknown() + explorer.n_free() + explorer.n_occupied() != total) return 5;
    const uint64_t n_clusters = explorer.cluster(26, 2);
    const std::vector<uint32_t> labels = explorer.labels();
    const std::vector<tsdf_frontier_cluster> rows = explorer.clusters();
    if (labels.size() != voxels.size() || rows.size() > n_clusters) return 6;

    // the class is the C ABI's computation: the same bytes through the handle
    tsdf_explorer_info info;
    if (tsdf_explorer_get_info(explorer.handle(), &info) != TSDF_OK) return 7;
    if (info.size[0] != n || info.connectivity != 26u || info.n_clusters != n_clusters || info.n_listed_clusters != rows.size()) return 8;
    std::vector<uint32_t> through_abi(voxels.size());
    if (tsdf_volume_find_frontiers(volume.handle(), 0u, explorer.handle()) != TSDF_OK ||
        tsdf_explorer_frontier_download(explorer.handle(), through_abi.data()) != TSDF_OK)
        return 9;
    if (memcmp(through_abi.data(), voxels.data(), voxels.size() * sizeof(uint32_t)) != 0) return 10;

    // view gain: the rays once, then their first half again with `keep` (the union is the first call's), then alone (the mask restarts)
    std::vector<float3> origins(R), directions(R);
    for (size_t r = 0; r < R; r++) {
        origins[r] = float3{rays[6 * r], rays[6 * r + 1], rays[6 * r + 2]};
        directions[r] = float3{rays[6 * r + 3], rays[6 * r + 4], rays[6 * r + 5]};
    }
    std::vector<uint32_t> unknown, free_voxels;
    std::vector<uint8_t> stop;
    const uint64_t gain = volume.view_gain(explorer, origins, directions, nullptr, false, &unknown, &free_voxels, &stop);
    const std::vector<float3> half_o(origins.begin(), origins.begin() + R / 2), half_d(directions.begin(), directions.begin() + R / 2);
    const uint64_t kept = volume.view_gain(explorer, half_o, half_d, nullptr, true);
    const uint64_t half = volume.view_gain(explorer, half_o, half_d);
    if (kept != gain || half > gain || unknown.size() != R || stop.size() != R) return 11;

    // the refusals arrive as std::invalid_argument
    int threw = 0;
    try {
        explorer.cluster(18, 1);
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        TSDFVolume::Explorer fresh;
        fresh.cluster(6, 1);   // no find_frontiers yet
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        (void)volume.view_gain(explorer, origins, half_d);
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        TSDFVolume other(TSDFVolume::UInt3{n / 2, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
        (void)other.view_gain(explorer, origins, directions);   // the explorer holds this volume's geometry
    } catch (const std::invalid_argument &) {
        threw++;
    }
    if (threw != 4) return 12;

    dump(out + "/voxels.u32", voxels.data(), voxels.size() * sizeof(uint32_t));
    dump(out + "/labels.u32", labels.data(), labels.size() * sizeof(uint32_t));
    dump(out + "/clusters.bin", rows.data(), rows.size() * sizeof(tsdf_frontier_cluster));
    dump(out + "/unknown.u32", unknown.data(), R * sizeof(uint32_t));
    dump(out + "/free.u32", free_voxels.data(), R * sizeof(uint32_t));
    dump(out + "/stop.u8", stop.data(), R);
    std::printf("exploration ok: %llu unknown, %llu free, %llu occupied, %zu frontiers (first %u, last %u), %llu clusters, %zu listed, gain %llu, half %llu\n",
                (unsigned long long)explorer.n_unknown(), (unsigned long long)explorer.n_free(), (unsigned long long)explorer.n_occupied(),
                voxels.size(), voxels.front(), voxels.back(), (unsigned long long)n_clusters, rows.size(), (unsigned long long)gain,
                (unsigned long long)half);
    return 0;
}
