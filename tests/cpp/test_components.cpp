// The mesh components through the C++ class surface: a grid^3 volume whose distances come from a file, extract_surface_components at
// a threshold (with normals), with keep_largest, at 0 (which must be extract_surface_indexed), inside a box, and a PLY of the filtered
// mesh.  Dumps the arrays for tests/test_cpp_components.py.
//
//   test_components <distances.f32 (grid^3)> <grid> <min_triangles> <out_dir>
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
        std::cerr << "usage: test_components distances.f32 grid min_triangles out_dir" << std::endl;
        return 2;
    }
    const unsigned n = (unsigned)atoi(argv[2]);
    const size_t min_triangles = (size_t)atoll(argv[3]);
    const std::string out = argv[4];
    std::vector<float> dist((size_t)n * n * n);
    {
        std::ifstream f(argv[1], std::ios::binary);
        f.read((char *)dist.data(), (std::streamsize)(dist.size() * sizeof(float)));
        if (!f) return 3;
    }
    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{n * 10.0f, n * 10.0f, n * 10.0f});
    volume.set_distance_data(dist.data());

    std::vector<float3> all_vertices, vertices, normals, one_vertices, same_vertices, box_vertices;
    std::vector<int3> all_triangles, triangles, one_triangles, same_triangles, box_triangles;
    extract_surface_indexed(&volume, all_vertices, all_triangles);
    extract_surface_components(&volume, nullptr, min_triangles, false, vertices, triangles, &normals);
    extract_surface_components(&volume, nullptr, min_triangles, true, one_vertices, one_triangles);
    extract_surface_components(&volume, nullptr, 0, false, same_vertices, same_triangles);
    if (vertices.empty() || vertices.size() >= all_vertices.size() || normals.size() != vertices.size()) return 4;
    if (one_vertices.empty() || one_vertices.size() >= vertices.size() || one_triangles.size() >= triangles.size()) return 5;
    // a threshold of 0 without keep_largest is the indexed mesh, array for array
    if (same_vertices.size() != all_vertices.size() || same_triangles.size() != all_triangles.size()) return 6;
    if (memcmp(same_vertices.data(), all_vertices.data(), all_vertices.size() * sizeof(float3)) != 0) return 7;
    if (memcmp(same_triangles.data(), all_triangles.data(), all_triangles.size() * sizeof(int3)) != 0) return 8;
    for (size_t t = 0; t < triangles.size(); t++) {
        const int corner[3] = {triangles[t].x, triangles[t].y, triangles[t].z};
        for (int c = 0; c < 3; c++)
            if (corner[c] < 0 || (size_t)corner[c] >= vertices.size()) return 9;
    }
    // a box, and a box whose begin is not below its end
    const unsigned box[6] = {2, 2, 2, n / 2 + 8, n - 2, n - 2}, bad[6] = {5, 0, 0, 5, 9, 9};
    extract_surface_components(&volume, box, min_triangles, false, box_vertices, box_triangles);
    bool threw = false;
    try {
        std::vector<float3> none;
        std::vector<int3> none_triangles;
        extract_surface_components(&volume, bad, 0, false, none, none_triangles);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    if (!threw) return 10;

    write_to_ply(out + "/kept.ply", vertices, triangles, normals);
    dump(out + "/vertices.f32", vertices.data(), vertices.size() * sizeof(float3));
    dump(out + "/triangles.i32", triangles.data(), triangles.size() * sizeof(int3));
    dump(out + "/normals.f32", normals.data(), normals.size() * sizeof(float3));
    dump(out + "/one_vertices.f32", one_vertices.data(), one_vertices.size() * sizeof(float3));
    dump(out + "/one_triangles.i32", one_triangles.data(), one_triangles.size() * sizeof(int3));
    dump(out + "/box_vertices.f32", box_vertices.data(), box_vertices.size() * sizeof(float3));
    dump(out + "/box_triangles.i32", box_triangles.data(), box_triangles.size() * sizeof(int3));
    std::printf("components ok: %zu of %zu vertices, %zu of %zu triangles kept, %zu in the largest\n", vertices.size(), all_vertices.size(),
                triangles.size(), all_triangles.size(), one_triangles.size());
    return 0;
}
