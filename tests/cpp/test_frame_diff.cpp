// The frame differences through the C++ class surface: a frame and a model image compared, clustered and masked by a FrameDiff,
// against the C ABI, and the refusals as exceptions.  Dumps the arrays for tests/test_cpp_frame_diff.py.
//
//   test_frame_diff <frame.u16> <model.u16> <width> <height> <tolerance> <quadratic> <connectivity> <depth_step> <min_pixels> <dilate> <out_dir>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "FrameDiff.hpp"

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
    if (argc < 12) {
        std::cerr << "usage: test_frame_diff frame.u16 model.u16 width height tolerance quadratic connectivity depth_step min_pixels dilate out_dir" << std::endl;
        return 2;
    }
    const uint32_t W = (uint32_t)atoi(argv[3]), H = (uint32_t)atoi(argv[4]);
    const uint32_t tolerance = (uint32_t)strtoul(argv[5], nullptr, 10), quadratic = (uint32_t)strtoul(argv[6], nullptr, 10);
    const uint32_t connectivity = (uint32_t)atoi(argv[7]), depth_step = (uint32_t)atoi(argv[8]), min_pixels = (uint32_t)atoi(argv[9]);
    const uint32_t dilate = (uint32_t)atoi(argv[10]);
    const std::string out = argv[11];
    const size_t n = (size_t)W * H;
    std::vector<uint16_t> frame(n), model(n);
    if (!load(argv[1], frame) || !load(argv[2], model)) return 3;

    FrameDiff diff;
    std::vector<uint8_t> states;
    const uint64_t listed = diff.compare(frame.data(), model.data(), W, H, tolerance, quadratic, &states);
    const std::vector<uint64_t> counts = diff.counts();
    if (states.size() != n || counts.size() != 5 || counts[TSDF_DIFF_NEARER] != listed) return 4;
    if (counts[0] + counts[1] + counts[2] + counts[3] + counts[4] != n) return 5;
    const uint64_t n_blobs = diff.cluster(connectivity, depth_step, min_pixels);
    const std::vector<uint32_t> pixels = diff.pixels(), labels = diff.labels();
    const std::vector<tsdf_diff_blob> blobs = diff.blobs();
    if (pixels.size() != listed || labels.size() != listed || blobs.size() > n_blobs) return 6;
    const FrameDiff::Masked m = diff.mask(dilate, frame.data(), true);
    if (m.mask.size() != n || m.blob_index.size() != n || m.frame.size() != n) return 7;
    const FrameDiff::Masked only = diff.mask(dilate);
    if (only.mask != m.mask || !only.blob_index.empty() || !only.frame.empty()) return 8;

    // the class is the C ABI's computation: the same bytes through the handle
    const tsdf_frame_diff_info info = diff.info();
    if (info.width != W || info.height != H || info.connectivity != connectivity || info.n_blobs != n_blobs || info.n_kept_blobs != blobs.size()) return 9;
    std::vector<uint32_t> through_abi(listed + 1);
    if (tsdf_frame_diff_download(diff.handle(), through_abi.data(), nullptr, nullptr) != TSDF_OK) return 10;
    if (memcmp(through_abi.data(), pixels.data(), pixels.size() * sizeof(uint32_t)) != 0) return 11;

    // the refusals arrive as std::invalid_argument
    int threw = 0;
    try {
        diff.cluster(6, depth_step, min_pixels);
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        (void)diff.mask(33);
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        FrameDiff fresh;
        fresh.cluster(8, 50, 1);   // no compare yet
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        FrameDiff fresh;
        (void)fresh.compare(frame.data(), model.data(), W, H);
        (void)fresh.mask(0);   // no cluster yet
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        FrameDiff fresh;
        (void)fresh.compare(frame.data(), model.data(), 0, H);
    } catch (const std::invalid_argument &) {
        threw++;
    }
    if (threw != 5) return 12;

    dump(out + "/states.u8", states.data(), n);
    dump(out + "/pixels.u32", pixels.data(), pixels.size() * sizeof(uint32_t));
    dump(out + "/labels.u32", labels.data(), labels.size() * sizeof(uint32_t));
    dump(out + "/blobs.bin", blobs.data(), blobs.size() * sizeof(tsdf_diff_blob));
    dump(out + "/mask.u8", m.mask.data(), n);
    dump(out + "/blob_index.u32", m.blob_index.data(), n * sizeof(uint32_t));
    dump(out + "/frame_out.u16", m.frame.data(), n * sizeof(uint16_t));
    std::printf("frame differences ok: %llu %llu %llu %llu %llu by state, %llu blobs, %zu kept\n", (unsigned long long)counts[0],
                (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3], (unsigned long long)counts[4],
                (unsigned long long)n_blobs, blobs.size());
    return 0;
}
