// The mesh smoothing through the C++ class surface: a grid^3 volume whose distances come from a file, extract_surface_smoothed with
// Taubin's factors (with the normals of the smoothed faces), inside a box with the border pinned, the same through the C ABI, and a PLY
// of the smoothed mesh.  Dumps the arrays for tests/test_cpp_smooth.py.
//
//   test_smooth <distances.f32 (grid^3)> <grid> <iterations> <out_dir>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "MarkAndSweepMC.hpp"
#include "TSDFVolume.hpp"
#include "ply.hpp"
#include "tsdf_amd.h"

const int8_t *tsdf_host_mc_triangle_table();   // libtsdf_host.so (MarkAndSweepMC.cpp): the table extract_surface_indexed marches with

static void dump(const std::string &path, const void *p, size_t bytes) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char *)p, (std::streamsize)bytes);
}

int main(int argc, char **argv) {
    if (argc < 5) {
        std::cerr << "usage: test_smooth distances.f32 grid iterations out_dir" << std::endl;
        return 2;
    }
    const unsigned n = (unsigned)atoi(argv[2]), iterations = (unsigned)atoi(argv[3]);
    const float lambda = 0.5f, mu = -0.53f;
    const std::string out = argv[4];
    std::vector<float> dist((size_t)n * n * n);
    {
        std::ifstream f(argv[1], std::ios::binary);
        f.read((char *)dist.data(), (std::streamsize)(dist.size() * sizeof(float)));
        if (!f) return 3;
    }
    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{n * 10.0f, n * 10.0f, n * 10.0f});
    volume.set_distance_data(dist.data());

    std::vector<float3> all_vertices, vertices, normals, box_vertices;
    std::vector<int3> all_triangles, triangles, box_triangles;
    extract_surface_indexed(&volume, all_vertices, all_triangles);
    extract_surface_smoothed(&volume, nullptr, iterations, lambda, mu, false, vertices, triangles, &normals);
    if (vertices.empty() || vertices.size() != all_vertices.size() || triangles.size() != all_triangles.size()) return 4;
    if (normals.size() != vertices.size()) return 5;
    if (std::memcmp(triangles.data(), all_triangles.data(), triangles.size() * sizeof(int3)) != 0) return 6;
    if (std::memcmp(vertices.data(), all_vertices.data(), vertices.size() * sizeof(float3)) == 0) return 7;   // something moved
    const unsigned box[6] = {0, 0, 0, 24, n, n};
    extract_surface_smoothed(&volume, box, iterations, lambda, mu, true, box_vertices, box_triangles);

    // the same through the C ABI: byte for byte what the class surface gave
    {
        tsdf_mesh *mesh = nullptr, *smoothed = nullptr;
        void *stream = nullptr;
        if (tsdf_mesh_create(&mesh) != TSDF_OK || tsdf_mesh_create(&smoothed) != TSDF_OK) return 8;
        if (tsdf_volume_extract_mesh(volume.handle(), tsdf_host_mc_triangle_table(), nullptr, 0u, mesh) != TSDF_OK) return 8;
        if (tsdf_volume_stream(volume.handle(), &stream) != TSDF_OK) return 8;
        if (tsdf_mesh_smooth(mesh, iterations, lambda, mu, TSDF_SMOOTH_NORMALS, smoothed, stream) != TSDF_OK) return 8;
        tsdf_mesh_info info;
        if (tsdf_mesh_get_info(smoothed, &info) != TSDF_OK || info.n_vertices != vertices.size() || !(info.flags & TSDF_MESH_NORMALS)) return 9;
        std::vector<float3> v((size_t)info.n_vertices), nrm((size_t)info.n_vertices);
        if (tsdf_mesh_download(smoothed, (float *)v.data(), nullptr, (float *)nrm.data(), nullptr) != TSDF_OK) return 9;
        if (std::memcmp(v.data(), vertices.data(), v.size() * sizeof(float3)) != 0) return 10;
        if (std::memcmp(nrm.data(), normals.data(), nrm.size() * sizeof(float3)) != 0) return 11;
        tsdf_mesh_destroy(smoothed);
        tsdf_mesh_destroy(mesh);
    }
    // arguments that are refused
    const float nan = std::strtof("nan", nullptr), inf = std::strtof("inf", nullptr);
    const struct { unsigned iterations; float lambda, mu; } bad[4] = {{1, nan, mu}, {1, lambda, inf}, {1, -inf, mu}, {1025, lambda, mu}};
    for (int k = 0; k < 4; k++) {
        bool threw = false;
        try {
            std::vector<float3> none;
            std::vector<int3> none_triangles;
            extract_surface_smoothed(&volume, nullptr, bad[k].iterations, bad[k].lambda, bad[k].mu, false, none, none_triangles);
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        if (!threw) return 12;
    }

    write_to_ply(out + "/smoothed.ply", vertices, triangles, normals);
    dump(out + "/all_vertices.f32", all_vertices.data(), all_vertices.size() * sizeof(float3));
    dump(out + "/all_triangles.i32", all_triangles.data(), all_triangles.size() * sizeof(int3));
    dump(out + "/vertices.f32", vertices.data(), vertices.size() * sizeof(float3));
    dump(out + "/triangles.i32", triangles.data(), triangles.size() * sizeof(int3));
    dump(out + "/normals.f32", normals.data(), normals.size() * sizeof(float3));
    dump(out + "/box_vertices.f32", box_vertices.data(), box_vertices.size() * sizeof(float3));
    dump(out + "/box_triangles.i32", box_triangles.data(), box_triangles.size() * sizeof(int3));
    std::printf("smooth ok: %zu vertices, %zu triangles, %u iterations; %zu vertices in the box\n", vertices.size(), triangles.size(), iterations,
                box_vertices.size());
    return 0;
}
