// Sparse snapshots through the C++ class surface: F frames of integrate() on a grid^3 volume, snapshot() into a Snapshot, save_sparse(),
// clear(), load_sparse() and restore(), against the dense arrays taken before, and the refusals as the class surface's errors (exceptions
// from snapshot / restore, false with a message from the file calls).  Dumps the brick arrays and the file for tests/test_cpp_snapshot.py.
//
//   test_snapshot <frames.u16 (F x 640 x 480)> <poses.f32 (F x 16, column-major)> <F> <grid> <out_dir>
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

// the dense state as every accessor reports it
static bool dense(const TSDFVolume &v, std::vector<float> &d, std::vector<float> &w) {
    const TSDFVolume::UInt3 s = v.size();
    d.resize((size_t)s.x * s.y * s.z);
    w.resize(d.size());
    return tsdf_volume_get_distance_data(v.handle(), d.data()) == TSDF_OK && tsdf_volume_get_weight_data(v.handle(), w.data()) == TSDF_OK;
}

static bool same(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

int main(int argc, char **argv) {
    if (argc < 6) {
        std::cerr << "usage: test_snapshot frames.u16 poses.f32 F grid out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t F = (size_t)atoi(argv[3]);
    const unsigned n = (unsigned)atoi(argv[4]);
    const std::string out = argv[5];
    std::vector<uint16_t> depth(F * W * H);
    std::vector<float> poses(F * 16);
    if (!load(argv[1], depth) || !load(argv[2], poses)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    Camera *camera = Camera::default_depth_camera();
    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        volume.integrate(depth.data() + f * W * H, W, H, *camera);
    }
    delete camera;
    volume.offset(10.0f, -20.0f, 30.0f);   // (after the fusion: it goes into the file's header)
    std::vector<float> d0, w0, d1, w1;
    if (!dense(volume, d0, w0)) return 4;

    // snapshot into a handle, its arrays
    TSDFVolume::Snapshot snap;
    volume.snapshot(snap);
    if (snap.n_bricks() == 0 || snap.weight_bits() != 8 || snap.has_colour()) return 5;
    if (snap.bytes() != snap.n_bricks() * (4 + 512 * 5)) return 6;
    std::vector<uint32_t> ids, colours;
    std::vector<float> dist;
    std::vector<unsigned char> weights;
    snap.download(ids, dist, weights, colours);
    if (ids.size() != snap.n_bricks() || dist.size() != 512 * ids.size() || weights.size() != 512 * ids.size() || !colours.empty()) return 7;
    if (!dense(volume, d1, w1) || !same(d0, d1) || !same(w0, w1)) return 8;   // the volume is as it was

    // the file, then the state back from it and from the handle
    const std::string file = out + "/volume.tsdfs";
    if (!volume.save_sparse(file)) return 9;
    volume.clear();
    {
        TSDFVolume::Snapshot empty;
        volume.snapshot(empty);
        if (empty.n_bricks() != 0 || empty.bytes() != 0) return 10;
    }
    volume.offset(0.0f, 0.0f, 0.0f);
    if (!volume.load_sparse(file)) return 11;
    if (!dense(volume, d1, w1) || !same(d0, d1) || !same(w0, w1)) return 12;
    const TSDFVolume::Float3 o = volume.offset();
    if (o.x != 10.0f || o.y != -20.0f || o.z != 30.0f) return 13;   // the file's header came back with it
    volume.clear();
    volume.restore(snap);
    if (!dense(volume, d1, w1) || !same(d0, d1) || !same(w0, w1)) return 14;

    // refusals: false with a message from the file calls ...
    TSDFVolume other(TSDFVolume::UInt3{n, n, n / 2}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    if (other.load_sparse(file)) return 15;                          // a grid of another size
    if (volume.load_sparse(out + "/no-such-file.tsdfs")) return 16;
    {
        std::ifstream in(file, std::ios::binary);
        std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        dump(out + "/cut.tsdfs", raw.data(), raw.size() - 1);
        raw[0] = 'X';
        dump(out + "/magic.tsdfs", raw.data(), raw.size());
    }
    if (volume.load_sparse(out + "/cut.tsdfs") || volume.load_sparse(out + "/magic.tsdfs")) return 17;
    if (!dense(volume, d1, w1) || !same(d0, d1) || !same(w0, w1)) return 18;   // a refused file leaves the volume alone
    // ... and std::invalid_argument from snapshot / restore
    int threw = 0;
    try {
        other.restore(snap);
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        TSDFVolume::Snapshot never;
        volume.restore(never);
    } catch (const std::invalid_argument &) {
        threw++;
    }
    (void)other.deformation();   // materialises the node array
    try {
        TSDFVolume::Snapshot s;
        other.snapshot(s);
    } catch (const std::invalid_argument &) {
        threw++;
    }
    if (threw != 3) return 19;
    if (other.save_sparse(out + "/nodes.tsdfs")) return 20;

    dump(out + "/ids.u32", ids.data(), ids.size() * sizeof(uint32_t));
    dump(out + "/distances.f32", dist.data(), dist.size() * sizeof(float));
    dump(out + "/weights.u8", weights.data(), weights.size());
    std::printf("snapshot ok: %llu bricks\n", (unsigned long long)ids.size());
    return 0;
}
