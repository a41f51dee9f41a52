// Scene flow through the C++ class surface: process_frames (the reference's signature, SceneFusion_krnl.hpp) on one volume, the C ABI's
// tsdf_volume_extract_mesh + tsdf_volume_apply_scene_flow with the reference's threshold on a second one holding the same distances;
// the two node arrays, read back through tsdf_volume_get_deformation_planes, must be the same bytes.  Dumps the nodes and the camera's
// matrices for tests/test_cpp_scene_flow.py.
//
//   test_scene_flow <dist.f32 (X x Y x Z)> X Y Z <voxel mm> ox oy oz <depth.u16 (W x H)> <flow.f32 (W x H x 3)> W H cx cy cz <out_dir>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "SceneFusion_krnl.hpp"
#include "TSDFVolume.hpp"
#include "tsdf_amd.h"

extern "C" void tsdf_host_mc_table(signed char out[256 * 32]);   // the triangle table the host library generates (host_capi.cpp)

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
    if (argc < 17) {
        std::cerr << "usage: test_scene_flow dist.f32 X Y Z voxel ox oy oz depth.u16 flow.f32 W H cx cy cz out_dir" << std::endl;
        return 2;
    }
    const unsigned X = (unsigned)atoi(argv[2]), Y = (unsigned)atoi(argv[3]), Z = (unsigned)atoi(argv[4]);
    const float voxel = (float)atof(argv[5]);
    const float ox = (float)atof(argv[6]), oy = (float)atof(argv[7]), oz = (float)atof(argv[8]);
    const unsigned W = (unsigned)atoi(argv[11]), H = (unsigned)atoi(argv[12]);
    const std::string out = argv[16];
    const size_t n = (size_t)X * Y * Z;
    std::vector<float> dist(n), flow((size_t)W * H * 3);
    std::vector<uint16_t> depth((size_t)W * H);
    if (!load(argv[1], dist) || !load(argv[9], depth) || !load(argv[10], flow)) return 3;

    Camera camera(35.0f, 35.0f, 20.0f, 15.0f);
    camera.move_to((float)atof(argv[13]), (float)atof(argv[14]), (float)atof(argv[15]));
    const TSDFVolume::UInt3 size{X, Y, Z};
    const TSDFVolume::Float3 physical{X * voxel, Y * voxel, Z * voxel};

    // the reference's entry point
    TSDFVolume by_frames(size, physical);
    by_frames.offset(ox, oy, oz);
    by_frames.set_distance_data(dist.data());
    process_frames(&by_frames, &camera, (uint16_t)W, (uint16_t)H, depth.data(), reinterpret_cast<const float3 *>(flow.data()));
    std::vector<tsdf_deformation_node> a(n), b(n);
    if (tsdf_volume_get_deformation_planes(by_frames.handle(), 0, Z, a.data()) != TSDF_OK) return 4;

    // the C ABI
    TSDFVolume by_abi(size, physical);
    by_abi.offset(ox, oy, oz);
    by_abi.set_distance_data(dist.data());
    std::vector<tsdf_deformation_node> before(n);
    if (tsdf_volume_get_deformation_planes(by_abi.handle(), 0, Z, before.data()) != TSDF_OK) return 4;
    tsdf_mesh *mesh = nullptr;
    if (tsdf_mesh_create(&mesh) != TSDF_OK) return 5;
    const Eigen::Matrix3f k = camera.k(), kinv = camera.kinv();
    tsdf_scene_flow_info info;
    std::vector<int8_t> table(256 * 32);
    tsdf_host_mc_table(reinterpret_cast<signed char *>(table.data()));
    if (tsdf_volume_extract_mesh(by_abi.handle(), table.data(), nullptr, 0u, mesh) != TSDF_OK) return 6;
    if (tsdf_volume_apply_scene_flow(by_abi.handle(), mesh, depth.data(), flow.data(), W, H, camera.pose().data(), camera.inverse_pose().data(), k.data(),
                                     kinv.data(), 10.0f, 0u, &info) != TSDF_OK) {
        std::cerr << tsdf_last_error() << std::endl;
        return 7;
    }
    if (tsdf_volume_get_deformation_planes(by_abi.handle(), 0, Z, b.data()) != TSDF_OK) return 4;
    if (info.n_vertices == 0 || info.n_correspondences == 0 || info.n_nodes_moved == 0) return 8;
    if (memcmp(a.data(), b.data(), n * sizeof(tsdf_deformation_node)) != 0) return 9;
    if (memcmp(b.data(), before.data(), n * sizeof(tsdf_deformation_node)) == 0) return 10;

    // the class method on the same handle: a second frame accumulates, and reports the same counts; a threshold of 0 throws
    uint64_t correspondences = 0;
    const uint64_t moved = by_abi.apply_scene_flow(mesh, depth.data(), reinterpret_cast<const float3 *>(flow.data()), W, H, camera, 10.0f, false,
                                                   &correspondences);
    if (moved != info.n_nodes_moved || correspondences != info.n_correspondences) return 11;
    std::vector<tsdf_deformation_node> twice(n);
    if (tsdf_volume_get_deformation_planes(by_abi.handle(), 0, Z, twice.data()) != TSDF_OK) return 4;
    if (memcmp(twice.data(), b.data(), n * sizeof(tsdf_deformation_node)) == 0) return 12;
    bool threw = false;
    try {
        by_abi.apply_scene_flow(mesh, depth.data(), reinterpret_cast<const float3 *>(flow.data()), W, H, camera, 0.0f);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    if (!threw) return 13;
    tsdf_mesh_destroy(mesh);

    float matrices[50];
    memcpy(matrices, camera.pose().data(), 16 * sizeof(float));
    memcpy(matrices + 16, camera.inverse_pose().data(), 16 * sizeof(float));
    memcpy(matrices + 32, k.data(), 9 * sizeof(float));
    memcpy(matrices + 41, kinv.data(), 9 * sizeof(float));
    dump(out + "/camera.f32", matrices, sizeof(matrices));
    dump(out + "/nodes.f32", a.data(), n * sizeof(tsdf_deformation_node));
    dump(out + "/nodes_twice.f32", twice.data(), n * sizeof(tsdf_deformation_node));
    std::printf("scene flow ok: %llu vertices, %llu correspondences, %llu nodes\n", (unsigned long long)info.n_vertices,
                (unsigned long long)info.n_correspondences, (unsigned long long)info.n_nodes_moved);
    return 0;
}
