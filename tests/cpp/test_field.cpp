// Field queries through the C++ class surface: F frames of integrate() on a grid^3 volume, TSDFVolume::sample_field on the points
// given (raw and unit gradients), extract_surface with normals, write_to_ply with normals, and GPURaycaster::raycast_gradient_normals
// against raycast() and sample_field.  Dumps the arrays for tests/test_cpp_field.py.
//
//   test_field <frames.u16 (F x 640 x 480)> <poses.f32 (F x 16, column-major)> <F> <grid> <points.f32 (N x 3)> <N> <out_dir>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "GPURaycaster.hpp"
#include "MarkAndSweepMC.hpp"
#include "TSDFVolume.hpp"
#include "ply.hpp"
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
        std::cerr << "usage: test_field frames.u16 poses.f32 F grid points.f32 N out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t F = (size_t)atoi(argv[3]);
    const unsigned n = (unsigned)atoi(argv[4]);
    const size_t N = (size_t)atoi(argv[6]);
    const std::string out = argv[7];
    std::vector<uint16_t> depth(F * W * H);
    std::vector<float> poses(F * 16);
    std::vector<float3> points(N);
    if (!load(argv[1], depth) || !load(argv[2], poses) || !load(argv[5], points)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    Camera *camera = Camera::default_depth_camera();
    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        volume.integrate(depth.data() + f * W * H, W, H, *camera);
    }

    // all outputs; then the unit gradient alone, which must leave the others' vectors alone
    std::vector<float> distances, weights, untouched(3, 7.0f);
    std::vector<float3> gradients, unit;
    volume.sample_field(points, &distances, &gradients, &weights);
    volume.sample_field(points, nullptr, &unit, nullptr, true);
    if (distances.size() != N || gradients.size() != N || weights.size() != N || unit.size() != N) return 4;
    bool threw = false;
    try {
        volume.sample_field(points, nullptr, nullptr, nullptr);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    if (!threw) return 5;
    std::vector<float3> none;
    volume.sample_field(none, &untouched, nullptr, nullptr);   // no points: an empty result
    if (!untouched.empty()) return 6;

    // the surface with a normal per vertex, and its PLY
    std::vector<float3> vertices, normals, vertices_plain;
    std::vector<int3> triangles, triangles_plain;
    extract_surface(&volume, vertices, triangles, normals);
    extract_surface(&volume, vertices_plain, triangles_plain);
    if (normals.size() != vertices.size() || vertices.size() != vertices_plain.size() || triangles.size() != triangles_plain.size()) return 7;
    if (!vertices.empty() && memcmp(vertices.data(), vertices_plain.data(), vertices.size() * sizeof(float3)) != 0) return 8;
    write_to_ply(out + "/mesh.ply", vertices, triangles, normals);

    // the ray cast with gradient normals: raycast()'s vertices, sample_field's unit gradients
    GPURaycaster caster(W, H);
    Eigen::Matrix<float, 3, Eigen::Dynamic> cast_v, cast_n, grad_v, grad_n;
    caster.raycast(volume, *camera, cast_v, cast_n);
    caster.raycast_gradient_normals(volume, *camera, grad_v, grad_n);
    const size_t pixels = (size_t)W * H;
    if ((size_t)grad_v.cols() != pixels || (size_t)grad_n.cols() != pixels) return 9;
    if (memcmp(cast_v.data(), grad_v.data(), pixels * 3 * sizeof(float)) != 0) return 10;
    std::vector<float3> cast_points(pixels), cast_unit;
    memcpy(cast_points.data(), grad_v.data(), pixels * sizeof(float3));
    volume.sample_field(cast_points, nullptr, &cast_unit, nullptr, true);
    if (memcmp(cast_unit.data(), grad_n.data(), pixels * sizeof(float3)) != 0) return 11;
    size_t with_normal = 0;
    for (size_t i = 0; i < pixels; i++) with_normal += grad_n(0, i) == grad_n(0, i) ? 1 : 0;
    delete camera;

    dump(out + "/distances.f32", distances.data(), N * sizeof(float));
    dump(out + "/gradients.f32", gradients.data(), N * sizeof(float3));
    dump(out + "/unit_gradients.f32", unit.data(), N * sizeof(float3));
    dump(out + "/weights.f32", weights.data(), N * sizeof(float));
    dump(out + "/vertices.f32", vertices.data(), vertices.size() * sizeof(float3));
    dump(out + "/normals.f32", normals.data(), normals.size() * sizeof(float3));
    std::printf("field surface ok: %zu points, %zu mesh vertices, %zu of %zu pixels with a gradient normal\n", N, vertices.size(),
                with_normal, pixels);
    return 0;
}
