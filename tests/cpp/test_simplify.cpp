// The mesh simplification through the C++ class surface: a grid^3 volume whose distances come from a file, extract_surface_simplified
// at a cell size (with normals), at a tiny cell (the position weld), inside a box, and a PLY of the simplified mesh.  Dumps the arrays
// for tests/test_cpp_simplify.py.
//
//   test_simplify <distances.f32 (grid^3)> <grid> <cell_size> <out_dir>
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

static void dump(const std::string &path, const void *p, size_t bytes) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char *)p, (std::streamsize)bytes);
}

int main(int argc, char **argv) {
    if (argc < 5) {
        std::cerr << "usage: test_simplify distances.f32 grid cell_size out_dir" << std::endl;
        return 2;
    }
    const unsigned n = (unsigned)atoi(argv[2]);
    const float cell_size = (float)atof(argv[3]);
    const std::string out = argv[4];
    std::vector<float> dist((size_t)n * n * n);
    {
        std::ifstream f(argv[1], std::ios::binary);
        f.read((char *)dist.data(), (std::streamsize)(dist.size() * sizeof(float)));
        if (!f) return 3;
    }
    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{n * 10.0f, n * 10.0f, n * 10.0f});
    volume.set_distance_data(dist.data());

    std::vector<float3> all_vertices, all_normals, vertices, normals, weld_vertices, box_vertices;
    std::vector<int3> all_triangles, triangles, weld_triangles, box_triangles;
    extract_surface_indexed(&volume, all_vertices, all_triangles, all_normals);
    extract_surface_simplified(&volume, nullptr, cell_size, vertices, triangles, &normals);
    extract_surface_simplified(&volume, nullptr, 1.0f / 256.0f, weld_vertices, weld_triangles);
    if (vertices.empty() || vertices.size() * 4 >= all_vertices.size() || triangles.size() * 4 >= all_triangles.size()) return 4;
    if (normals.size() != vertices.size()) return 5;
    // the weld takes away coincident vertices only
    if (weld_vertices.empty() || weld_vertices.size() > all_vertices.size() || weld_vertices.size() * 10 < all_vertices.size() * 9) return 6;
    for (size_t t = 0; t < triangles.size(); t++) {
        const int corner[3] = {triangles[t].x, triangles[t].y, triangles[t].z};
        for (int c = 0; c < 3; c++)
            if (corner[c] < 0 || (size_t)corner[c] >= vertices.size()) return 7;
        if (corner[0] == corner[1] || corner[0] == corner[2] || corner[1] == corner[2]) return 8;
    }
    // a box, and cell sizes that are no lengths
    const unsigned box[6] = {2, 2, 2, n / 2 + 8, n - 2, n - 2};
    extract_surface_simplified(&volume, box, cell_size, box_vertices, box_triangles);
    const float bad[3] = {0.0f, -1.0f, std::strtof("inf", nullptr)};
    for (int k = 0; k < 3; k++) {
        bool threw = false;
        try {
            std::vector<float3> none;
            std::vector<int3> none_triangles;
            extract_surface_simplified(&volume, nullptr, bad[k], none, none_triangles);
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        if (!threw) return 9;
    }

    write_to_ply(out + "/simplified.ply", vertices, triangles, normals);
    dump(out + "/all_vertices.f32", all_vertices.data(), all_vertices.size() * sizeof(float3));
    dump(out + "/all_triangles.i32", all_triangles.data(), all_triangles.size() * sizeof(int3));
    dump(out + "/all_normals.f32", all_normals.data(), all_normals.size() * sizeof(float3));
    dump(out + "/vertices.f32", vertices.data(), vertices.size() * sizeof(float3));
    dump(out + "/triangles.i32", triangles.data(), triangles.size() * sizeof(int3));
    dump(out + "/normals.f32", normals.data(), normals.size() * sizeof(float3));
    dump(out + "/weld_vertices.f32", weld_vertices.data(), weld_vertices.size() * sizeof(float3));
    dump(out + "/weld_triangles.i32", weld_triangles.data(), weld_triangles.size() * sizeof(int3));
    dump(out + "/box_vertices.f32", box_vertices.data(), box_vertices.size() * sizeof(float3));
    dump(out + "/box_triangles.i32", box_triangles.data(), box_triangles.size() * sizeof(int3));
    std::printf("simplify ok: %zu of %zu vertices, %zu of %zu triangles at %g; %zu vertices after the weld\n", vertices.size(), all_vertices.size(),
                triangles.size(), all_triangles.size(), (double)cell_size, weld_vertices.size());
    return 0;
}
