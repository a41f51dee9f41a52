// The class objects through the C++ class surface: a hand-made class field on a 6 x 2 x 2 grid whose objects, rows and lookups are worked
// out below, then F frames of integrate_classes() on a grid^3 volume, find_objects() into an Objects, its table and a lookup, against the
// C ABI, and the refusals as exceptions.  Dumps the arrays for tests/test_cpp_objects.py.
//
//   test_objects <frames.u16 (F x 640 x 480)> <classes.u16 (F x 640 x 480)> <poses.f32 (F x 16, column-major)> <F> <grid>
//                <points.f32 (P x 3)> <P> <out_dir>
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

template <typename F>
static bool refused(F call) {
    try {
        call();
    } catch (const std::invalid_argument &) {
        return true;
    }
    return false;
}

static bool row_is(const tsdf_class_object &r, uint32_t label, uint32_t size, uint32_t x0, uint32_t y0, uint32_t z0, uint32_t x1, uint32_t y1, uint32_t z1,
                   uint64_t sx, uint64_t sy, uint64_t sz, uint64_t votes, uint32_t class_id) {
    return r.label == label && r.size == size && r.lo[0] == x0 && r.lo[1] == y0 && r.lo[2] == z0 && r.hi[0] == x1 && r.hi[1] == y1 && r.hi[2] == z1 &&
           r.sum[0] == sx && r.sum[1] == sy && r.sum[2] == sz && r.votes == votes && r.class_id == class_id && r.reserved == 0;
}

// Voxels of 10 x 20 x 30 mm, id = (z * 2 + y) * 6 + x.  Class 1: (0,0,0) and (1,0,0), ids 0 and 1, votes 1 and 2; class 2: (3,0,0), id 3,
// votes 7; class 1 again: (4,0,1), (4,1,1), (5,1,1), ids 16, 22, 23, votes 3, 4, 5; and a word with class bits but no votes at (2,0,0).
// The list is 0 1 3 16 22 23, so L = 0 0 2 3 3 3: three objects, labels 0, 2, 3.
static int hand_made() {
    TSDFVolume volume(TSDFVolume::UInt3{6, 2, 2}, TSDFVolume::Float3{60.0f, 40.0f, 60.0f});
    volume.enable_classes(true);
    std::vector<uint32_t> words(24, 0u);
    words[0] = 1u | (1u << 16);
    words[1] = 1u | (2u << 16);
    words[2] = 1u;
    words[3] = 2u | (7u << 16);
    words[16] = 1u | (3u << 16);
    words[22] = 1u | (4u << 16);
    words[23] = 1u | (5u << 16);
    if (tsdf_volume_set_class_data(volume.handle(), words.data()) != TSDF_OK) return 20;
    TSDFVolume::Objects objects;
    volume.find_objects(objects, 1, nullptr, 26, 1);
    if (objects.n_labelled() != 6 || objects.n_objects() != 3) return 21;
    if (objects.voxels() != std::vector<uint32_t>{0, 1, 3, 16, 22, 23} || objects.labels() != std::vector<uint32_t>{0, 0, 2, 3, 3, 3}) return 22;
    std::vector<tsdf_class_object> rows = objects.objects();
    if (rows.size() != 3 || !row_is(rows[0], 0, 2, 0, 0, 0, 1, 0, 0, 1, 0, 0, 3, 1) || !row_is(rows[1], 2, 1, 3, 0, 0, 3, 0, 0, 3, 0, 0, 7, 2) ||
        !row_is(rows[2], 3, 3, 4, 0, 1, 5, 1, 1, 13, 2, 3, 12, 1))
        return 23;
    // voxel centres of (1,0,0), (3,0,0), (5,1,1), the voteless (2,0,0), a point off the grid
    const std::vector<float3> points = {float3{15.0f, 10.0f, 15.0f}, float3{35.0f, 10.0f, 15.0f}, float3{55.0f, 30.0f, 45.0f}, float3{25.0f, 10.0f, 15.0f},
                                        float3{65.0f, 10.0f, 15.0f}};
    if (objects.lookup(points) != std::vector<uint32_t>{0, 1, 2, TSDF_OBJECT_NONE, TSDF_OBJECT_NONE}) return 24;
    // min_size 2 drops the object of class 2: its voxel resolves to no row, the last object moves up
    volume.find_objects(objects, 1, nullptr, 26, 2);
    rows = objects.objects();
    if (objects.n_objects() != 3 || rows.size() != 2 || rows[1].label != 3) return 25;
    if (objects.lookup(points) != std::vector<uint32_t>{0, TSDF_OBJECT_NONE, 1, TSDF_OBJECT_NONE, TSDF_OBJECT_NONE}) return 26;
    // at connectivity 6 (5,1,1) - (4,1,1) - (4,0,1) still hang together by faces; three votes and more leave 3 16 22 23
    volume.find_objects(objects, 3, nullptr, 6, 1);
    if (objects.voxels() != std::vector<uint32_t>{3, 16, 22, 23} || objects.labels() != std::vector<uint32_t>{0, 1, 1, 1}) return 27;
    // a selection of class 2 alone; one that ends before class 2
    const std::vector<uint8_t> only_two = {0, 0, 1}, short_one = {1, 1};
    volume.find_objects(objects, 1, &only_two, 26, 1);
    if (objects.voxels() != std::vector<uint32_t>{3}) return 28;
    volume.find_objects(objects, 1, &short_one, 26, 1);
    rows = objects.objects();
    if (objects.n_labelled() != 5 || rows.size() != 2 || rows[0].class_id != 1 || rows[1].class_id != 1) return 29;
    if (!objects.lookup(std::vector<float3>()).empty()) return 30;
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 9) {
        std::cerr << "usage: test_objects frames.u16 classes.u16 poses.f32 F grid points.f32 P out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t F = (size_t)atoi(argv[4]);
    const unsigned n = (unsigned)atoi(argv[5]);
    const size_t P = (size_t)atoi(argv[7]);
    const std::string out = argv[8];
    std::vector<uint16_t> depth(F * W * H), classes(F * W * H);
    std::vector<float> poses(F * 16), coords(P * 3);
    if (!load(argv[1], depth) || !load(argv[2], classes) || !load(argv[3], poses) || !load(argv[6], coords)) return 3;

    const int rc = hand_made();
    if (rc) return rc;

    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    TSDFVolume::Objects objects;
    // before classes are enabled, and before any find
    if (!refused([&] { volume.find_objects(objects); })) return 4;
    if (!refused([&] { objects.voxels(); }) || !refused([&] { objects.lookup(std::vector<float3>(1, float3{0.0f, 0.0f, 0.0f})); })) return 4;
    volume.enable_classes(true);
    if (!refused([&] { volume.find_objects(objects, 1, nullptr, 18, 1); })) return 5;
    const std::vector<uint8_t> too_long(65536, 1);
    if (!refused([&] { volume.find_objects(objects, 1, &too_long, 26, 1); })) return 5;

    Camera *camera = Camera::default_depth_camera();
    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        volume.integrate_classes(depth.data() + f * W * H, classes.data() + f * W * H, W, H, *camera);
    }
    delete camera;
    std::vector<uint32_t> words((size_t)n * n * n);
    if (tsdf_volume_get_class_data(volume.handle(), words.data()) != TSDF_OK) return 6;

    const std::vector<uint8_t> select = {0, 1, 0, 1};   // classes 1 and 3
    volume.find_objects(objects, 2, &select, 26, 4);
    const std::vector<uint32_t> voxels = objects.voxels(), labels = objects.labels();
    const std::vector<tsdf_class_object> rows = objects.objects();
    if (voxels.size() != objects.n_labelled() || labels.size() != voxels.size() || rows.size() > objects.n_objects() || rows.empty()) return 7;

    // the class is the C ABI's computation: the same bytes through the handle
    tsdf_objects_info info;
    if (tsdf_objects_get_info(objects.handle(), &info) != TSDF_OK) return 8;
    if (info.size[0] != n || info.connectivity != 26u || info.min_votes != 2u || info.min_size != 4u || info.n_listed_objects != rows.size()) return 8;
    std::vector<tsdf_class_object> through_abi(rows.size());
    if (tsdf_volume_find_objects(volume.handle(), 2u, select.data(), 4u, 26u, 4u, 0u, objects.handle()) != TSDF_OK ||
        tsdf_objects_download(objects.handle(), nullptr, nullptr, through_abi.data()) != TSDF_OK)
        return 9;
    if (memcmp(through_abi.data(), rows.data(), rows.size() * sizeof(tsdf_class_object)) != 0) return 10;

    std::vector<float3> points(P);
    for (size_t p = 0; p < P; p++) points[p] = float3{coords[3 * p], coords[3 * p + 1], coords[3 * p + 2]};
    const std::vector<uint32_t> found = objects.lookup(points);
    if (found.size() != P) return 11;

    dump(out + "/classes.u32", words.data(), words.size() * sizeof(uint32_t));
    dump(out + "/voxels.u32", voxels.data(), voxels.size() * sizeof(uint32_t));
    dump(out + "/labels.u32", labels.data(), labels.size() * sizeof(uint32_t));
    dump(out + "/objects.bin", rows.data(), rows.size() * sizeof(tsdf_class_object));
    dump(out + "/lookup.u32", found.data(), P * sizeof(uint32_t));
    std::printf("class objects ok: %zu labelled, %llu objects, %zu listed\n", voxels.size(), (unsigned long long)objects.n_objects(), rows.size());
    return 0;
}
