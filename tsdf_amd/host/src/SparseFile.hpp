// The .tsdfs file of a sparse snapshot: little-endian, no padding.
//   8 bytes "TSDFSPR1"
//   the 68-byte header of .tsdf: dim3 size, float3 physical size, float3 offset, float truncation distance, float max weight,
//     float3 global translation, float3 global rotation
//   uint32 brick = 8, uint32 flags, uint32 weight_bits, uint32 weight_bound, float fill_distance, uint32 0, uint64 n_bricks
//   n_bricks ids (uint32), 512 n_bricks distances (float), weights (weight_bits / 8 bytes each) and, with TSDF_SNAPSHOT_COLOUR, colour words
// The reader parses and validates without touching a device.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace tsdf_host {

struct SparseFileInfo {
    uint32_t size[3];
    float physical_size[3];
    float offset[3];
    float truncation_distance;
    float max_weight;
    float global_translation[3];
    float global_rotation[3];
    uint32_t brick, flags, weight_bits, weight_bound;
    float fill_distance;
    uint32_t reserved;
    uint64_t n_bricks;
};

constexpr size_t kSparseHeaderBytes = 8 + 68 + 32;

// The header as it lies in the file
void pack_sparse_header(const SparseFileInfo &info, unsigned char out[kSparseHeaderBytes]);

// Reads and validates `file_name`: the magic, brick == 8, known flags, sizes in 1 .. 65535, weight_bits 8, 16 or 32, n_bricks at most the
// grid's brick count and the file's length equal to what the header implies -- all before anything is allocated -- then the ids
// (strictly ascending, below the brick count).  Returns the empty string, or why the file is refused.  The arrays that are not null
// receive the file's.
std::string read_sparse_file(const std::string &file_name, SparseFileInfo &info, std::vector<uint32_t> *ids = nullptr,
                             std::vector<float> *distances = nullptr, std::vector<unsigned char> *weights = nullptr,
                             std::vector<uint32_t> *colours = nullptr);

}  // namespace tsdf_host
