// Class fusion through the C++ class surface: TSDFVolume::enable_classes, integrate_classes, sample_classes, class_counts and
// GPURaycaster::raycast_classes.  Checks the refusals and dumps raw results for tests/test_cpp_classes.py to compare with the numpy
// reference and the Python path.
//
//   test_classes <frames.u16 (F x 640 x 480)> <classes.u16 (F x 640 x 480)> <confidence.u8 (F x 640 x 480)> <poses.f32 (F x 16,
//                column-major)> <F> <grid> <out_dir>
// The even frames are fused with their confidence, the odd ones without (strength 1).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "GPURaycaster.hpp"
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

template <typename F>
static bool refused(F call) {
    try {
        call();
    } catch (const std::invalid_argument &) {
        return true;
    }
    return false;
}

int main(int argc, char **argv) {
    if (argc < 8) {
        std::cerr << "usage: test_classes frames.u16 classes.u16 confidence.u8 poses.f32 F grid out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t F = (size_t)atoi(argv[5]);
    const unsigned n = (unsigned)atoi(argv[6]);
    const std::string out = argv[7];
    std::vector<uint16_t> depth(F * W * H), classes(F * W * H);
    std::vector<uint8_t> conf(F * W * H);
    std::vector<float> poses(F * 16);
    if (!load(argv[1], depth) || !load(argv[2], classes) || !load(argv[3], conf) || !load(argv[4], poses)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    Camera *camera = Camera::default_depth_camera();
    GPURaycaster raycaster(W, H);
    Eigen::Matrix<float, 3, Eigen::Dynamic> v, nrm;
    std::vector<uint16_t> ray_classes, ray_votes, got_classes, got_votes;
    const std::vector<float3> probe(4, float3{100.0f, 100.0f, 100.0f});
    // class calls on a volume without classes are refused with std::invalid_argument
    if (volume.classes_enabled()) return 4;
    if (!refused([&] { volume.integrate_classes(depth.data(), classes.data(), W, H, *camera); })) return 4;
    if (!refused([&] { volume.sample_classes(probe, got_classes); })) return 4;
    if (!refused([&] { volume.class_counts(4); })) return 4;
    if (!refused([&] { raycaster.raycast_classes(volume, *camera, v, nrm, ray_classes); })) return 4;
    volume.enable_classes(true);
    if (!volume.classes_enabled()) return 5;
    // null classes, rgb without colour, n_classes out of range
    if (!refused([&] { volume.integrate_classes(depth.data(), nullptr, W, H, *camera); })) return 5;
    if (!refused([&] { volume.integrate_classes(depth.data(), classes.data(), W, H, *camera, nullptr, conf.data()); })) return 5;
    if (!refused([&] { volume.class_counts(0); }) || !refused([&] { volume.class_counts(65536); })) return 5;

    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        volume.integrate_classes(depth.data() + f * W * H, classes.data() + f * W * H, W, H, *camera,
                                 f % 2 == 0 ? conf.data() + f * W * H : nullptr);
    }
    const TSDFVolume::UInt3 s = volume.size();
    std::vector<uint32_t> words((size_t)s.x * s.y * s.z);
    if (tsdf_volume_get_class_data(volume.handle(), words.data()) != TSDF_OK) return 6;
    dump(out + "/classes.u32", words.data(), words.size() * 4);

    const std::vector<uint64_t> counts = volume.class_counts(8, 2);
    if (counts.size() != 8) return 7;
    dump(out + "/counts.u64", counts.data(), counts.size() * 8);

    raycaster.raycast_classes(volume, *camera, v, nrm, ray_classes, &ray_votes);
    if (ray_classes.size() != (size_t)W * H || ray_votes.size() != (size_t)W * H) return 8;
    dump(out + "/ray_vertices.f32", v.data(), (size_t)W * H * 3 * sizeof(float));
    dump(out + "/ray_classes.u16", ray_classes.data(), ray_classes.size() * 2);
    dump(out + "/ray_votes.u16", ray_votes.data(), ray_votes.size() * 2);

    // sample_classes at the cast's vertices is the cast's class map
    std::vector<float3> points((size_t)W * H);
    for (size_t i = 0; i < points.size(); i++) points[i] = float3{v(0, i), v(1, i), v(2, i)};
    volume.sample_classes(points, got_classes, &got_votes);
    if (got_classes != ray_classes || got_votes != ray_votes) return 9;
    volume.sample_classes(std::vector<float3>(), got_classes);
    if (!got_classes.empty()) return 10;

    volume.enable_classes(false);
    if (volume.classes_enabled()) return 11;
    delete camera;
    std::printf("class surface ok: %zu voxels classified\n", (size_t)(counts[1] + counts[2] + counts[3]));
    return 0;
}
