// The mesh renderer through the C++ class surface (MeshRenderer): a grid^3 volume whose distances come from a file is meshed with
// normals into a handle, the handle is rendered into every map but rgb, the same mesh is rendered again from its downloaded arrays
// (byte for byte the same maps), with back faces culled, and into a second image size with the warm renderer; bad arguments throw.
// Dumps the mesh and the maps for tests/test_cpp_render.py.
//
//   test_render <distances.f32 (grid^3)> <grid> <width> <height> <out_dir>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "MeshRenderer.hpp"
#include "TSDFVolume.hpp"
#include "tsdf_amd.h"

const int8_t *tsdf_host_mc_triangle_table();   // libtsdf_host.so (MarkAndSweepMC.cpp): the table extract_surface_indexed marches with

static void dump(const std::string &path, const void *p, size_t bytes) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char *)p, (std::streamsize)bytes);
}

template <typename T>
static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static bool same_maps(const MeshRenderer::Maps &a, const MeshRenderer::Maps &b) {
    return same(a.triangle, b.triangle) && same(a.z, b.z) && same(a.depth, b.depth) && same(a.vertices, b.vertices) && same(a.normals, b.normals) &&
           a.n_live == b.n_live && a.n_dropped == b.n_dropped && a.n_large == b.n_large && a.n_pixels_hit == b.n_pixels_hit;
}

int main(int argc, char **argv) {
    if (argc < 6) {
        std::cerr << "usage: test_render distances.f32 grid width height out_dir" << std::endl;
        return 2;
    }
    const unsigned n = (unsigned)atoi(argv[2]), width = (unsigned)atoi(argv[3]), height = (unsigned)atoi(argv[4]);
    const std::string out = argv[5];
    std::vector<float> dist((size_t)n * n * n);
    {
        std::ifstream f(argv[1], std::ios::binary);
        f.read((char *)dist.data(), (std::streamsize)(dist.size() * sizeof(float)));
        if (!f) return 3;
    }
    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{n * 10.0f, n * 10.0f, n * 10.0f});
    volume.set_distance_data(dist.data());

    // the camera: in front of the grid's z = 0 face, looking along +z (column-major)
    const float half = n * 5.0f;
    const float inv_pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -half, -half, 600.0f, 1};
    const float k[9] = {(float)width, 0, 0, 0, (float)width, 0, width * 0.5f, height * 0.5f, 1};
    const float z_near = 100.0f, z_far = 4000.0f;

    tsdf_mesh *mesh = nullptr;
    if (tsdf_mesh_create(&mesh) != TSDF_OK) return 4;
    if (tsdf_volume_extract_mesh(volume.handle(), tsdf_host_mc_triangle_table(), nullptr, TSDF_MESH_NORMALS, mesh) != TSDF_OK) return 4;
    tsdf_mesh_info info;
    if (tsdf_mesh_get_info(mesh, &info) != TSDF_OK || info.n_vertices == 0) return 5;
    std::vector<float3> vertices((size_t)info.n_vertices), normals((size_t)info.n_vertices);
    std::vector<uint32_t> indices((size_t)info.n_indices);
    if (tsdf_mesh_download(mesh, (float *)vertices.data(), indices.data(), (float *)normals.data(), nullptr) != TSDF_OK) return 5;
    std::vector<int3> triangles;
    for (size_t i = 0; i + 2 < indices.size(); i += 3) triangles.push_back(int3{(int)indices[i], (int)indices[i + 2], (int)indices[i + 1]});

    MeshRenderer renderer;
    const MeshRenderer::Maps maps = renderer.render(mesh, width, height, inv_pose, k, z_near, z_far, 0, MeshRenderer::ALL_BUT_RGB);
    if (maps.z.size() != (size_t)width * height || !maps.rgb.empty() || maps.n_pixels_hit == 0 || maps.n_triangles != triangles.size()) return 6;
    const uint64_t warm = renderer.scratch_bytes();
    // the arrays give the handle's maps; a repeat allocates nothing
    const MeshRenderer::Maps again = renderer.render(vertices, triangles, &normals, nullptr, width, height, inv_pose, k, z_near, z_far, 0, MeshRenderer::ALL_BUT_RGB);
    if (!same_maps(maps, again)) return 7;
    if (renderer.scratch_bytes() != warm) return 8;
    // culling the back faces of a closed surface seen from outside changes no pixel
    const MeshRenderer::Maps culled = renderer.render(mesh, width, height, inv_pose, k, z_near, z_far, TSDF_RENDER_CULL_BACK, MeshRenderer::ALL_BUT_RGB);
    if (!(same(maps.triangle, culled.triangle) && same(maps.z, culled.z) && culled.n_live < maps.n_live)) return 9;
    // without vertex normals: the face normals
    const MeshRenderer::Maps faces = renderer.render(vertices, triangles, nullptr, nullptr, width, height, inv_pose, k, z_near, z_far, 0,
                                                     MeshRenderer::NORMALS | MeshRenderer::DEPTH);
    if (!same(maps.depth, faces.depth) || !faces.z.empty()) return 10;
    // another image size with the warm handle
    const MeshRenderer::Maps small = renderer.render(mesh, 37, 29, inv_pose, k, z_near, z_far, 0, MeshRenderer::DEPTH | MeshRenderer::TRIANGLE);

    // arguments that are refused
    const float nan = std::strtof("nan", nullptr);
    float bad_k[9];
    std::memcpy(bad_k, k, sizeof(k));
    bad_k[3] = 0.5f;
    const struct { unsigned w, h; const float *k; float z_near, z_far; uint32_t flags, targets; } bad[7] = {
        {0, height, k, z_near, z_far, 0, MeshRenderer::DEPTH},      {width, height, bad_k, z_near, z_far, 0, MeshRenderer::DEPTH},
        {width, height, k, 0.0f, z_far, 0, MeshRenderer::DEPTH},    {width, height, k, z_far, z_near, 0, MeshRenderer::DEPTH},
        {width, height, k, nan, z_far, 0, MeshRenderer::DEPTH},     {width, height, k, z_near, z_far, 2, MeshRenderer::DEPTH},
        {width, height, k, z_near, z_far, 0, MeshRenderer::RGB}};   // (the mesh has no colours)
    for (int i = 0; i < 7; i++) {
        bool threw = false;
        try {
            renderer.render(mesh, bad[i].w, bad[i].h, inv_pose, bad[i].k, bad[i].z_near, bad[i].z_far, bad[i].flags, bad[i].targets);
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        if (!threw) return 20 + i;
    }
    {   // an index that is not below the vertex count
        std::vector<int3> broken = triangles;
        broken[broken.size() / 2].y = (int)vertices.size();
        bool threw = false;
        try {
            renderer.render(vertices, broken, nullptr, nullptr, width, height, inv_pose, k, z_near, z_far);
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        if (!threw) return 30;
    }
    // ... and a good render follows
    if (!same_maps(maps, renderer.render(mesh, width, height, inv_pose, k, z_near, z_far, 0, MeshRenderer::ALL_BUT_RGB))) return 31;
    tsdf_mesh_destroy(mesh);

    dump(out + "/vertices.f32", vertices.data(), vertices.size() * sizeof(float3));
    dump(out + "/indices.u32", indices.data(), indices.size() * sizeof(uint32_t));
    dump(out + "/normals.f32", normals.data(), normals.size() * sizeof(float3));
    dump(out + "/inv_pose.f32", inv_pose, sizeof(inv_pose));
    dump(out + "/k.f32", k, sizeof(k));
    dump(out + "/triangle.u32", maps.triangle.data(), maps.triangle.size() * 4);
    dump(out + "/z.f32", maps.z.data(), maps.z.size() * 4);
    dump(out + "/depth.u16", maps.depth.data(), maps.depth.size() * 2);
    dump(out + "/map_vertices.f32", maps.vertices.data(), maps.vertices.size() * sizeof(float3));
    dump(out + "/map_normals.f32", maps.normals.data(), maps.normals.size() * sizeof(float3));
    dump(out + "/face_normals.f32", faces.normals.data(), faces.normals.size() * sizeof(float3));
    dump(out + "/small_depth.u16", small.depth.data(), small.depth.size() * 2);
    dump(out + "/small_triangle.u32", small.triangle.data(), small.triangle.size() * 4);
    const uint64_t counts[5] = {maps.n_triangles, maps.n_live, maps.n_dropped, maps.n_large, maps.n_pixels_hit};
    dump(out + "/counts.u64", counts, sizeof(counts));
    std::printf("render ok: %zu vertices, %zu triangles, %llu of %u pixels hit\n", vertices.size(), triangles.size(), (unsigned long long)maps.n_pixels_hit,
                width * height);
    return 0;
}
