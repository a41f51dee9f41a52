// The rolling volume through the C++ class surface: a volume filled from dense arrays, Snapshot::select of a box, shift() with the bricks
// that fall out, the way back with those bricks paged in (restore with TSDF_RESTORE_KEEP_OTHERS), a shifted restore over the cleared
// volume, and the refusals as std::invalid_argument.  Dumps the arrays for tests/test_cpp_rolling.py, which holds them against the CPU
// reference.
//
//   test_rolling <distances.f32> <weights.f32> <X> <Y> <Z> <out_dir>      (voxels of 10 x 12.5 x 9 mm, offset 100, -50, 25)
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

static bool load(const char *path, std::vector<float> &v) {
    std::ifstream f(path, std::ios::binary);
    f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(float)));
    return (bool)f;
}

static bool dense(const TSDFVolume &v, std::vector<float> &d, std::vector<float> &w) {
    const TSDFVolume::UInt3 s = v.size();
    d.resize((size_t)s.x * s.y * s.z);
    w.resize(d.size());
    return tsdf_volume_get_distance_data(v.handle(), d.data()) == TSDF_OK && tsdf_volume_get_weight_data(v.handle(), w.data()) == TSDF_OK;
}

static bool same(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

static void dump_list(const std::string &stem, const TSDFVolume::Snapshot &s) {
    std::vector<uint32_t> ids, colours;
    std::vector<float> dist;
    std::vector<unsigned char> weights;
    s.download(ids, dist, weights, colours);
    dump(stem + "_ids.u32", ids.data(), ids.size() * sizeof(uint32_t));
    dump(stem + "_distances.f32", dist.data(), dist.size() * sizeof(float));
    dump(stem + "_weights.u8", weights.data(), weights.size());
}

template <typename F>
static int throws(F call) {
    try {
        call();
    } catch (const std::invalid_argument &e) {
        std::printf("refused: %s\n", e.what());
        return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 7) {
        std::cerr << "usage: test_rolling distances.f32 weights.f32 X Y Z out_dir" << std::endl;
        return 2;
    }
    const unsigned X = (unsigned)atoi(argv[3]), Y = (unsigned)atoi(argv[4]), Z = (unsigned)atoi(argv[5]);
    const std::string out = argv[6];
    std::vector<float> d0((size_t)X * Y * Z), w0(d0.size()), d1, w1;
    if (!load(argv[1], d0) || !load(argv[2], w0)) return 3;
    TSDFVolume volume(TSDFVolume::UInt3{X, Y, Z}, TSDFVolume::Float3{10.0f * X, 12.5f * Y, 9.0f * Z});
    volume.offset(100.0f, -50.0f, 25.0f);
    if (tsdf_volume_set_distance_data(volume.handle(), d0.data()) != TSDF_OK || tsdf_volume_set_weight_data(volume.handle(), w0.data()) != TSDF_OK) return 4;

    // the bricks of a box, and those outside it
    TSDFVolume::Snapshot snap, inside, outside;
    volume.snapshot(snap);
    const int32_t lo[3] = {1, 0, 1}, hi[3] = {3, 2, 2};
    snap.select(lo, hi, 0u, inside);
    snap.select(lo, hi, TSDF_SELECT_OUTSIDE, outside);
    if (inside.n_bricks() == 0 || inside.n_bricks() + outside.n_bricks() != snap.n_bricks()) return 5;
    if (inside.weight_bits() != snap.weight_bits() || inside.has_colour()) return 6;
    dump_list(out + "/inside", inside);
    dump_list(out + "/outside", outside);

    // the box moves by (1, 0, -1) bricks
    const int32_t step[3] = {1, 0, -1}, back[3] = {-1, 0, 1}, zero[3] = {0, 0, 0};
    TSDFVolume::Snapshot work, leaving;
    volume.shift(step, work, &leaving);
    if (leaving.n_bricks() == 0 || !dense(volume, d1, w1)) return 7;
    dump(out + "/shifted_distances.f32", d1.data(), d1.size() * sizeof(float));
    dump(out + "/shifted_weights.f32", w1.data(), w1.size() * sizeof(float));
    dump_list(out + "/leaving", leaving);
    const TSDFVolume::Float3 o = volume.offset();
    const float offset[3] = {o.x, o.y, o.z};
    dump(out + "/shifted_offset.f32", offset, sizeof(offset));
    // ... and back, the bricks that left paged in: the state it began with
    volume.shift(back, work, nullptr);
    volume.restore(leaving, zero, TSDF_RESTORE_KEEP_OTHERS);
    if (!dense(volume, d1, w1) || !same(d0, d1) || !same(w0, w1)) return 8;
    const TSDFVolume::Float3 o1 = volume.offset();
    if (o1.x != 100.0f || o1.y != -50.0f || o1.z != 25.0f) return 9;

    // a shifted restore without flags clears what it does not write
    const int32_t by[3] = {-1, 1, 0};
    volume.restore(snap, by, 0u);
    if (!dense(volume, d1, w1)) return 10;
    dump(out + "/restored_distances.f32", d1.data(), d1.size() * sizeof(float));
    dump(out + "/restored_weights.f32", w1.data(), w1.size() * sizeof(float));

    // the refusals
    int threw = 0;
    TSDFVolume::Snapshot never;
    threw += throws([&] { snap.select(lo, hi, 0u, snap); });
    threw += throws([&] { never.select(lo, hi, 0u, inside); });
    threw += throws([&] { volume.restore(never, by, 0u); });
    threw += throws([&] { volume.restore(snap, by, 2u); });
    threw += throws([&] { volume.shift(step, work, &work); });
    TSDFVolume partial(TSDFVolume::UInt3{9, 8, 8}, TSDFVolume::Float3{90.0f, 100.0f, 72.0f});
    threw += throws([&] { partial.shift(step, work, nullptr); });
    if (threw != 6) return 11;
    if (!dense(volume, d0, w0) || !same(d0, d1) || !same(w0, w1)) return 12;   // a refused call leaves the volume alone

    std::printf("rolling ok: %llu bricks, %llu in the box, %llu left\n", (unsigned long long)snap.n_bricks(), (unsigned long long)inside.n_bricks(),
                (unsigned long long)leaving.n_bricks());
    return 0;
}
