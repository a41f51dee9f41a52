// Reader and header of the .tsdfs file (SparseFile.hpp).  Host only: nothing here touches a device.
#include "SparseFile.hpp"

#include <cstring>
#include <fstream>

#include "tsdf_amd.h"

namespace tsdf_host {

namespace {
const char kMagic[9] = "TSDFSPR1";

std::string number(uint64_t v) { return std::to_string((unsigned long long)v); }
}  // namespace

void pack_sparse_header(const SparseFileInfo &i, unsigned char out[kSparseHeaderBytes]) {
    unsigned char *p = out;
    auto put = [&p](const void *src, size_t bytes) {
        std::memcpy(p, src, bytes);
        p += bytes;
    };
    put(kMagic, 8);
    put(i.size, 12);
    put(i.physical_size, 12);
    put(i.offset, 12);
    put(&i.truncation_distance, 4);
    put(&i.max_weight, 4);
    put(i.global_translation, 12);
    put(i.global_rotation, 12);
    put(&i.brick, 4);
    put(&i.flags, 4);
    put(&i.weight_bits, 4);
    put(&i.weight_bound, 4);
    put(&i.fill_distance, 4);
    const uint32_t zero = 0;
    put(&zero, 4);
    put(&i.n_bricks, 8);
}

std::string read_sparse_file(const std::string &file_name, SparseFileInfo &i, std::vector<uint32_t> *ids, std::vector<float> *distances,
                             std::vector<unsigned char> *weights, std::vector<uint32_t> *colours) {
    std::memset(&i, 0, sizeof(i));
    std::ifstream ifs{file_name, std::ios::in | std::ios::binary};
    if (!ifs.good()) return "couldn't open the file";
    ifs.seekg(0, std::ios::end);
    const uint64_t length = (uint64_t)ifs.tellg();
    ifs.seekg(0, std::ios::beg);
    unsigned char head[kSparseHeaderBytes];
    if (length < kSparseHeaderBytes || !ifs.read((char *)head, kSparseHeaderBytes)) return "the file is shorter than the header (" + number(length) + " bytes)";
    if (std::memcmp(head, kMagic, 8) != 0) return "not a .tsdfs file: wrong magic";
    const unsigned char *p = head + 8;
    auto get = [&p](void *dst, size_t bytes) {
        std::memcpy(dst, p, bytes);
        p += bytes;
    };
    get(i.size, 12);
    get(i.physical_size, 12);
    get(i.offset, 12);
    get(&i.truncation_distance, 4);
    get(&i.max_weight, 4);
    get(i.global_translation, 12);
    get(i.global_rotation, 12);
    get(&i.brick, 4);
    get(&i.flags, 4);
    get(&i.weight_bits, 4);
    get(&i.weight_bound, 4);
    get(&i.fill_distance, 4);
    get(&i.reserved, 4);
    get(&i.n_bricks, 8);
    if (i.brick != TSDF_SNAPSHOT_BRICK) return "brick size " + number(i.brick) + ", expected " + number(TSDF_SNAPSHOT_BRICK);
    if (i.flags & ~(uint32_t)TSDF_SNAPSHOT_COLOUR) return "unknown flags " + number(i.flags);
    uint64_t total = 1;
    for (int a = 0; a < 3; a++) {
        if (i.size[a] < 1 || i.size[a] > 65535) return "size " + number(i.size[a]) + " is not in 1 .. 65535";
        total *= (i.size[a] + TSDF_SNAPSHOT_BRICK - 1) / TSDF_SNAPSHOT_BRICK;
    }
    if (i.weight_bits != 8 && i.weight_bits != 16 && i.weight_bits != 32) return "weight_bits = " + number(i.weight_bits) + " is not 8, 16 or 32";
    if (i.n_bricks > total) return "n_bricks = " + number(i.n_bricks) + ", the grid has " + number(total) + " bricks";
    const bool colour = (i.flags & TSDF_SNAPSHOT_COLOUR) != 0;
    const uint64_t per_brick = 4 + 512 * (uint64_t)(4 + i.weight_bits / 8 + (colour ? 4 : 0));
    const uint64_t expect = kSparseHeaderBytes + i.n_bricks * per_brick;   // (n_bricks <= 2^39: no overflow)
    if (length != expect) return "the file has " + number(length) + " bytes, its header implies " + number(expect);
    // the file is as long as its header says: the arrays are bounded by what is on disk
    const size_t n = (size_t)i.n_bricks;
    std::vector<uint32_t> own_ids;
    std::vector<uint32_t> &id = ids ? *ids : own_ids;
    id.resize(n);
    if (n && !ifs.read((char *)id.data(), n * sizeof(uint32_t))) return "couldn't read the brick ids";
    for (size_t k = 0; k < n; k++) {
        if (id[k] >= total) return "brick id " + number(id[k]) + " is not below the brick count " + number(total);
        if (k && id[k] <= id[k - 1]) return "brick ids are not strictly ascending at " + number(k);
    }
    if (!distances && !weights && !colours) return std::string();
    std::vector<float> own_d;
    std::vector<unsigned char> own_w;
    std::vector<float> &d = distances ? *distances : own_d;
    std::vector<unsigned char> &w = weights ? *weights : own_w;
    d.resize(n * 512);
    w.resize(n * 512 * (i.weight_bits / 8));
    if (n && !ifs.read((char *)d.data(), d.size() * sizeof(float))) return "couldn't read the distances";
    if (n && !ifs.read((char *)w.data(), w.size())) return "couldn't read the weights";
    if (colours) {
        colours->resize(colour ? n * 512 : 0);
        if (colour && n && !ifs.read((char *)colours->data(), colours->size() * sizeof(uint32_t))) return "couldn't read the colours";
    }
    return std::string();
}

}  // namespace tsdf_host
