// The column maps through the C++ class surface: TSDFVolume::column_map() into a TSDFVolume::ColumnMap on a 13 x 7 x 5 state field that
// tests/test_cpp_columns.py writes -- every axis whole and forward, an inner band reversed, one map with an ESDF -- columns(),
// classify(), height_world(), info() against the C ABI, and the refusals as exceptions.  Dumps the arrays for the Python side to compare
// with the CPU reference.
//
//   test_columns <dir>     reads <dir>/dist.f32 and <dir>/weight.f32
#include <cmath>
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

static std::vector<float> load(const std::string &path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) {
        std::cerr << "cannot read " << path << std::endl;
        exit(3);
    }
    std::vector<float> v((size_t)f.tellg() / sizeof(float));
    f.seekg(0);
    f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(float)));
    return v;
}

template <class F>
static int throws(F f) {
    try {
        f();
    } catch (const std::invalid_argument &) {
        return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::cerr << "usage: test_columns dir" << std::endl;
        return 2;
    }
    static_assert(sizeof(tsdf_column) == 32, "a row is 32 bytes");
    const std::string dir = argv[1];
    // the volume of tests/test_columns.py::volume_of: 10 x 12.5 x 9 mm voxels and an offset
    TSDFVolume volume(TSDFVolume::UInt3{13, 7, 5}, TSDFVolume::Float3{130.0f, 87.5f, 45.0f});
    volume.offset(100.0f, -50.0f, 25.0f);
    const std::vector<float> d = load(dir + "/dist.f32"), w = load(dir + "/weight.f32");
    if (d.size() != 13 * 7 * 5 || w.size() != d.size()) return 4;
    volume.set_distance_data(d.data());
    volume.set_weight_data(w.data());

    TSDFVolume::ColumnMap map;
    const uint32_t N[3] = {13, 7, 5};
    unsigned long long printed[3 * 4];
    for (uint32_t axis = 0; axis < 3; axis++) {
        volume.column_map(map, axis);
        const std::vector<tsdf_column> rows = map.columns();
        const tsdf_columns_info info = map.info();
        if (rows.size() != (size_t)info.map_size[0] * info.map_size[1] || info.axis != axis || info.lo != 0 || info.hi != N[axis] || info.flags != 0 || info.has_esdf) return 5;
        if (info.n_unknown + info.n_free + info.n_occupied != 13 * 7 * 5) return 6;
        // the class is the C ABI's computation: the same bytes through the handle
        std::vector<tsdf_column> through_abi(rows.size());
        if (tsdf_columns_download(map.handle(), through_abi.data()) != TSDF_OK || memcmp(through_abi.data(), rows.data(), rows.size() * sizeof(tsdf_column)) != 0) return 7;
        dump(dir + "/rows" + std::to_string(axis) + ".bin", rows.data(), rows.size() * sizeof(tsdf_column));
        printed[4 * axis] = info.n_unknown;
        printed[4 * axis + 1] = info.n_free;
        printed[4 * axis + 2] = info.n_occupied;
        printed[4 * axis + 3] = info.n_ground;
    }

    // an inner band, reversed, classified; the world heights
    volume.column_map(map, 2, 1, 4, true);
    const std::vector<tsdf_column> band = map.columns();
    const std::vector<uint8_t> cells = map.classify(1, 1);
    const tsdf_columns_info info = map.info();
    if (cells.size() != band.size() || info.lo != 1 || info.hi != 4 || info.flags != TSDF_COLUMNS_REVERSED || info.max_step != 1 || info.min_headroom != 1) return 8;
    if (info.n_no_ground + info.n_traversable + info.n_blocked != band.size() || info.n_traversable + info.n_blocked != info.n_ground) return 9;
    std::vector<float> world(band.size());
    for (size_t i = 0; i < band.size(); i++) {
        world[i] = map.height_world(band[i]);
        if (std::isnan(world[i]) != (band[i].top < 0)) return 10;
    }
    dump(dir + "/band.bin", band.data(), band.size() * sizeof(tsdf_column));
    dump(dir + "/cells.u8", cells.data(), cells.size());
    dump(dir + "/world.f32", world.data(), world.size() * sizeof(float));

    // with an ESDF: the array it was computed into goes to the Python side too
    tsdf_esdf *esdf = nullptr;
    if (tsdf_esdf_create(&esdf) != TSDF_OK) return 11;
    volume.compute_esdf(40.0f, false, esdf);
    std::vector<float> e(d.size());
    if (tsdf_esdf_download(esdf, e.data()) != TSDF_OK) return 12;
    volume.column_map(map, 1, 0, 0, false, esdf);
    const std::vector<tsdf_column> with_esdf = map.columns();
    if (!map.info().has_esdf) return 13;
    dump(dir + "/esdf.f32", e.data(), e.size() * sizeof(float));
    dump(dir + "/with_esdf.bin", with_esdf.data(), with_esdf.size() * sizeof(tsdf_column));

    // the refusals arrive as std::invalid_argument
    int threw = 0;
    threw += throws([&] { volume.column_map(map, 3); });
    threw += throws([&] { volume.column_map(map, 2, 3, 3); });
    threw += throws([&] { volume.column_map(map, 2, 0, 6); });
    threw += throws([&] {
        TSDFVolume::ColumnMap fresh;
        (void)fresh.classify(1, 1);   // no projection yet
    });
    threw += throws([&] {
        TSDFVolume::ColumnMap fresh;
        (void)fresh.columns();
    });
    threw += throws([&] {
        TSDFVolume other(TSDFVolume::UInt3{12, 7, 5}, TSDFVolume::Float3{120.0f, 87.5f, 45.0f});
        other.column_map(map, 2, 0, 0, false, esdf);   // the ESDF is this volume's
    });
    tsdf_esdf_destroy(esdf);
    if (threw != 6) return 14;
    // ... and a refusal leaves the map as it was
    if (map.columns().size() != with_esdf.size()) return 15;

    std::printf("columns ok:");
    for (unsigned long long v : printed) std::printf(" %llu", v);
    std::printf(" | %llu %llu %llu\n", (unsigned long long)info.n_no_ground, (unsigned long long)info.n_traversable, (unsigned long long)info.n_blocked);
    return 0;
}
