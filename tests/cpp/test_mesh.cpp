// The indexed mesh through the C++ class surface: F frames of integrate() with colour on a grid^3 volume, extract_surface_indexed
// with normals and colours (whole grid and a box), against extract_surface's soup, and a PLY with shared vertices.  Dumps the arrays
// for tests/test_cpp_mesh.py.
//
//   test_mesh <frames.u16 (F x 640 x 480)> <colours.u8 (F x 640 x 480 x 3)> <poses.f32 (F x 16, column-major)> <F> <grid> <out_dir>
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

template <typename T>
static bool load(const char *path, std::vector<T> &v) {
    std::ifstream f(path, std::ios::binary);
    f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(T)));
    return (bool)f;
}

int main(int argc, char **argv) {
    if (argc < 7) {
        std::cerr << "usage: test_mesh frames.u16 colours.u8 poses.f32 F grid out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t F = (size_t)atoi(argv[4]);
    const unsigned n = (unsigned)atoi(argv[5]);
    const std::string out = argv[6];
    std::vector<uint16_t> depth(F * W * H);
    std::vector<uint8_t> rgb(F * W * H * 3);
    std::vector<float> poses(F * 16);
    if (!load(argv[1], depth) || !load(argv[2], rgb) || !load(argv[3], poses)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    volume.enable_colour(true);
    Camera *camera = Camera::default_depth_camera();
    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        volume.integrate(depth.data() + f * W * H, rgb.data() + f * W * H * 3, W, H, *camera);
    }
    delete camera;

    std::vector<float3> vertices, normals, plain_vertices, soup;
    std::vector<int3> triangles, plain_triangles, soup_triangles;
    std::vector<uchar3> colours;
    extract_surface_indexed(&volume, vertices, triangles, normals, colours);
    extract_surface_indexed(&volume, plain_vertices, plain_triangles);
    extract_surface(&volume, soup, soup_triangles);
    if (normals.size() != vertices.size() || colours.size() != vertices.size()) return 4;
    if (plain_vertices.size() != vertices.size() || plain_triangles.size() != triangles.size() || triangles.size() != soup_triangles.size()) return 5;
    if (!vertices.empty() && memcmp(vertices.data(), plain_vertices.data(), vertices.size() * sizeof(float3)) != 0) return 6;
    if (!triangles.empty() && memcmp(triangles.data(), plain_triangles.data(), triangles.size() * sizeof(int3)) != 0) return 7;
    // the corners of the indexed triangles are the soup's vertices, bit for bit (the soup's triangle t is (3t, 3t+2, 3t+1))
    for (size_t t = 0; t < triangles.size(); t++) {
        const int corner[3] = {triangles[t].x, triangles[t].y, triangles[t].z};
        const size_t at[3] = {3 * t, 3 * t + 2, 3 * t + 1};
        for (int c = 0; c < 3; c++) {
            if (corner[c] < 0 || (size_t)corner[c] >= vertices.size()) return 8;
            if (memcmp(&vertices[(size_t)corner[c]], &soup[at[c]], sizeof(float3)) != 0) return 9;
        }
    }
    // a box: fewer vertices, a begin that is not below its end throws
    const unsigned box[6] = {3, 5, 7, 40, 41, 42}, bad[6] = {5, 0, 0, 5, 9, 9};
    std::vector<float3> box_vertices, box_normals;
    std::vector<int3> box_triangles;
    extract_surface_indexed(&volume, box, box_vertices, box_triangles, &box_normals);
    if (box_vertices.empty() || box_vertices.size() >= vertices.size() || box_normals.size() != box_vertices.size()) return 10;
    bool threw = false;
    try {
        std::vector<float3> none;
        std::vector<int3> none_triangles;
        extract_surface_indexed(&volume, bad, none, none_triangles);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    if (!threw) return 11;

    write_to_ply(out + "/mesh.ply", vertices, triangles, normals, colours);
    dump(out + "/vertices.f32", vertices.data(), vertices.size() * sizeof(float3));
    dump(out + "/triangles.i32", triangles.data(), triangles.size() * sizeof(int3));
    dump(out + "/normals.f32", normals.data(), normals.size() * sizeof(float3));
    dump(out + "/colours.u8", colours.data(), colours.size() * sizeof(uchar3));
    dump(out + "/box_vertices.f32", box_vertices.data(), box_vertices.size() * sizeof(float3));
    dump(out + "/box_triangles.i32", box_triangles.data(), box_triangles.size() * sizeof(int3));
    std::printf("indexed mesh ok: %zu vertices, %zu triangles, %zu soup vertices\n", vertices.size(), triangles.size(), soup.size());
    return 0;
}
