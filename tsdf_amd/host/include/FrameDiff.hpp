// Frame differences (include/tsdf_amd.h, "frame differences"; not in the reference, whose volume takes every pixel as static): a depth
// frame compared with the model's depth image, the pixels in front of the model clustered into blobs, and the dilated mask of the
// blobs that are kept, on the device, through a handle that keeps its scratch between frames.
#ifndef TSDF_AMD_FRAME_DIFF_HPP
#define TSDF_AMD_FRAME_DIFF_HPP

#include <cstdint>
#include <vector>

#include "tsdf_amd.h"

class FrameDiff {
public:
    // what mask() returns; the vectors that were not asked for stay empty
    struct Masked {
        std::vector<uint8_t> mask;          // 1 under a kept blob dilated by `dilate`
        std::vector<uint32_t> blob_index;   // the blob's row per listed pixel, TSDF_DIFF_NO_BLOB elsewhere
        std::vector<uint16_t> frame;        // the frame with the masked pixels set to 0
    };

    FrameDiff();    // throws std::invalid_argument / exits like every device failure when the handle cannot be made
    ~FrameDiff();
    FrameDiff(const FrameDiff &) = delete;
    FrameDiff &operator=(const FrameDiff &) = delete;

    // frame and model: width * height uint16 millimetres on the host.  Returns the number of listed (NEARER) pixels; states, when
    // given, takes the state of every pixel.  Blocking.  Throws std::invalid_argument on the refusals.
    uint64_t compare(const uint16_t *frame, const uint16_t *model, uint32_t width, uint32_t height, uint32_t tolerance = 50, uint32_t quadratic = 0,
                     std::vector<uint8_t> *states = nullptr);
    // the pixels in each state of the last compare, indexed by TSDF_DIFF_*
    std::vector<uint64_t> counts() const;
    // connectivity 4 or 8; returns the number of blobs, of any size
    uint64_t cluster(uint32_t connectivity = 8, uint32_t depth_step = 50, uint32_t min_pixels = 64);
    std::vector<uint32_t> pixels() const;
    std::vector<uint32_t> labels() const;
    std::vector<tsdf_diff_blob> blobs() const;   // the kept blobs, in ascending label
    // dilate in 0 .. 32; frame: the compared frame (or any of its size) to be masked, or null
    Masked mask(uint32_t dilate = 4, const uint16_t *frame = nullptr, bool blob_index = false);

    uint64_t scratch_bytes() const;
    tsdf_frame_diff_info info() const;
    tsdf_frame_diff *handle() const { return m_handle; }

private:
    tsdf_frame_diff *m_handle;
};

#endif
