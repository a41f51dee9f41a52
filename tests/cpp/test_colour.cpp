// Colour fusion through the C++ class surface: TSDFVolume::enable_colour + integrate(depth, rgb, ...), extract_surface with
// colours, write_to_ply with colours, GPURaycaster::raycast with colours, and the .tsdf round trip of the colour block.  Dumps raw
// results for tests/test_colour_fusion.py to compare with the Python path.
//
//   test_colour <frames.u16 (F x 640 x 480)> <frames.rgb (F x 640 x 480 x 3)> <poses.f32 (F x 16, column-major)> <F> <grid> <out_dir>
#include <cstdio>
#include <cstdlib>
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

static std::vector<uint32_t> colours_of(const TSDFVolume &v) {
    const TSDFVolume::UInt3 s = v.size();
    std::vector<uint32_t> c((size_t)s.x * s.y * s.z);
    if (tsdf_volume_get_colour_data(v.handle(), c.data()) != TSDF_OK) throw std::runtime_error(tsdf_last_error());
    return c;
}

int main(int argc, char **argv) {
    if (argc < 7) {
        std::cerr << "usage: test_colour frames.u16 frames.rgb poses.f32 F grid out_dir" << std::endl;
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
    Camera *camera = Camera::default_depth_camera();
    // colour calls on a volume without colour are refused with std::invalid_argument
    bool threw = false;
    try {
        volume.integrate(depth.data(), rgb.data(), W, H, *camera);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    if (!threw || volume.colour_enabled()) return 4;
    volume.enable_colour(true);
    if (!volume.colour_enabled() || !volume.colour_data()) return 5;

    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        volume.integrate(depth.data() + f * W * H, rgb.data() + f * W * H * 3, W, H, *camera);
    }
    const std::vector<uint32_t> colour = colours_of(volume);
    dump(out + "/colour.u32", colour.data(), colour.size() * 4);

    std::vector<float3> vertices;
    std::vector<int3> triangles;
    std::vector<uchar3> colours;
    extract_surface(&volume, vertices, triangles, colours);
    if (colours.size() != vertices.size() || vertices.empty()) return 6;
    write_to_ply(out + "/mesh.ply", vertices, triangles, colours);

    Eigen::Matrix<float, 3, Eigen::Dynamic> v, nrm;
    std::vector<uchar3> ray_colours;
    GPURaycaster raycaster(W, H);
    raycaster.raycast(volume, *camera, v, nrm, ray_colours);
    if (ray_colours.size() != (size_t)W * H) return 7;
    dump(out + "/ray_vertices.f32", v.data(), (size_t)W * H * 3 * sizeof(float));
    dump(out + "/ray_rgb.u8", ray_colours.data(), ray_colours.size() * 3);

    // .tsdf: the colour block round trip, and the n rule of the file constructor
    if (!volume.save_to_file(out + "/colour.tsdf")) return 8;
    {
        TSDFVolume loaded(out + "/colour.tsdf");
        if (!loaded.colour_enabled()) return 9;
        const std::vector<uint32_t> c = colours_of(loaded);
        dump(out + "/loaded.u32", c.data(), c.size() * 4);
    }
    // a volume without colour saves zeros and loads without colour
    {
        TSDFVolume plain(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
        plain.integrate(depth.data(), W, H, *camera);
        if (!plain.save_to_file(out + "/plain.tsdf")) return 10;
        TSDFVolume loaded(out + "/plain.tsdf");
        if (loaded.colour_enabled()) return 11;
    }
    delete camera;
    std::printf("colour surface ok: %zu vertices, %zu triangles\n", vertices.size(), triangles.size());
    return 0;
}
