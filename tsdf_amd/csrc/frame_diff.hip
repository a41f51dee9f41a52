// Frame differences for gfx950 (include/tsdf_amd.h, "frame differences"): which pixels of a depth frame lie in front of
// the model's depth image, how they hang together, and the dilated mask of the blobs that are kept.  No reference counterpart.  Nothing
// of a volume is read or written: the inputs are two uint16 images.
//
// Compare: DiffFlag, the state of a pixel (frame_diff_index.hpp) on two coalesced uint16 loads, five counters, the frame copied and the
// state stored on the way.  The flag walk, the chunk scan and the list are voxel_set.hpp's over a W x H x 1 grid.
// Cluster: voxel_set.hpp's clustering (voxel_set_cluster) with the policy NearInDepth: the blob row has a 2-D box and depth extremes, so
// the policy's three values are x, y and the depth.
// Mask:
//   diff_paint_kernel     a wave per 64 pixel ids: pixel -> list index -> label -> kept row; the row to blob_index, the kept bit by ballot
//   diff_dilate_kernel    a 64 x 16 tile: the row window of every tile row and the `dilate` rows above and below as an any-bit test on a
//                         range of ids, one ballot word per row in LDS; then the column window ORs those words.  One writer per output.
// Every result is a set, an integer sum, a minimum or a maximum: two runs give the same bytes whatever order the waves run in.  No float
// atomics, no lane waits for another, and every loop has a stated bound.
#include <algorithm>

#include "common.hpp"
#include "frame_diff_index.hpp"
#include "voxel_set.hpp"

namespace tsdf {

static_assert(sizeof(tsdf_diff_blob) == 56 && sizeof(tsdf_frame_diff_info) == 88, "the layouts include/tsdf_amd.h gives");
static_assert(TSDF_DIFF_NO_FRAME == kDiffNoFrame && TSDF_DIFF_NO_MODEL == kDiffNoModel && TSDF_DIFF_SAME == kDiffSame &&
                  TSDF_DIFF_FARTHER == kDiffFarther && TSDF_DIFF_NEARER == kDiffNearer,
              "the public states are the index header's");

// the handle's counter words: the flag kernel's five, the listed state last, then the set's two (roots, scan total: voxel_set.hpp)
using DiffSet = VoxelSet<tsdf_diff_blob, kDiffStates, 8>;
static_assert(DiffSet::kWordCounted == kDiffNearer, "the listed pixels are the NEARER ones");

// Two coalesced uint16 loads per pixel; the frame's value goes to the handle's copy and the state to the caller's image, one writer each.
struct DiffFlag {
    static constexpr uint32_t kCounts = kDiffStates, kListed = kDiffNearer;
    const uint16_t *frame, *model;
    uint16_t *copy;
    uint8_t *states;   // or null
    uint32_t tolerance, quadratic;
    __device__ uint32_t operator()(uint32_t id, const VoxelGrid &) const {
        const uint32_t f = frame[id], m = model[id];
        const uint32_t s = diff_state(f, m, diff_tolerance(tolerance, quadratic, m));
        copy[id] = (uint16_t)f;
        if (states) states[id] = (uint8_t)s;
        return 1u << s;
    }
};

// listed neighbours are adjacent when their frame depths differ by at most `step`; the row's values are x, y and the depth (each at
// most 65535)
struct NearInDepth {
    using Row = tsdf_diff_blob;
    static constexpr int kSummed = 0;
    const uint16_t *depth;   // the handle's copy of the frame
    uint32_t step;
    __device__ static void clear(Row &r) {
        r.lo[0] = r.lo[1] = 0xffffffffu;
        r.hi[0] = r.hi[1] = 0;
        r.min_depth = 0xffffffffu;
        r.max_depth = 0;
        r.sum_x = r.sum_y = r.sum_depth = 0;
    }
    __device__ uint32_t word(uint32_t id) const { return depth[id]; }
    __device__ bool adjacent(uint32_t own, uint32_t id2) const {
        const uint32_t d = depth[id2];
        return (d > own ? d - own : own - d) <= step;
    }
    __device__ void values(uint32_t id, const VoxelGrid &grid, bool, Row &, uint32_t (&v)[3], uint32_t *) const {
        v[1] = id / grid.X;
        v[0] = id - v[1] * grid.X;
        v[2] = depth[id];
    }
    __device__ static void add(Row *row, uint32_t n, const uint32_t *lo, const uint32_t *hi, const uint32_t *sum, const uint32_t *) {
        atomicAdd(&row->size, n);
        for (int k = 0; k < 2; k++) {
            atomicMin(&row->lo[k], lo[k]);
            atomicMax(&row->hi[k], hi[k]);
        }
        atomicMin(&row->min_depth, lo[2]);
        atomicMax(&row->max_depth, hi[2]);
        atomicAdd((unsigned long long *)&row->sum_x, (unsigned long long)sum[0]);
        atomicAdd((unsigned long long *)&row->sum_y, (unsigned long long)sum[1]);
        atomicAdd((unsigned long long *)&row->sum_depth, (unsigned long long)sum[2]);
    }
};

// what a paint reads of the handle; labels, row_mask and row_base are touched only behind a set mask bit (have_rows: there is a table)
struct DiffView {
    const uint64_t *mask;
    const uint32_t *base, *labels;
    const uint64_t *row_mask;
    const uint32_t *row_base;
    int have_rows;
};

// A wave per chunk of 64 pixel ids.  kept[chunk]: the pixels of kept blobs, no bit beyond the image.
__global__ __launch_bounds__(256) void diff_paint_kernel(const DiffView d, const uint32_t n, const uint32_t n_chunks, uint64_t *__restrict__ kept,
                                                         uint32_t *__restrict__ blob_index) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;   // (the whole wave)
    const uint64_t id = (uint64_t)chunk * 64 + lane;
    uint32_t row = TSDF_DIFF_NO_BLOB;
    if (id < n && d.have_rows && mask_bit(d.mask, (uint32_t)id)) {
        const uint32_t label = d.labels[compact_index(d.mask, d.base, (uint32_t)id)];
        if (mask_bit(d.row_mask, label)) row = compact_index(d.row_mask, d.row_base, label);
    }
    const uint64_t bits = __ballot(row != TSDF_DIFF_NO_BLOB);
    if (lane == 0) kept[chunk] = bits;
    if (blob_index && id < n) blob_index[id] = row;
}

constexpr uint32_t kDilateTileX = 64, kDilateTileY = 16, kDilateRows = kDilateTileY + 2 * kDiffMaxDilate;

// A workgroup per 64 x 16 tile of outputs, a lane per column.  Row pass: wave w takes the tile's rows r = w, w + 4, ... of the
// 16 + 2 * dilate rows that begin `dilate` above the tile; image row y = y0 - dilate + r, nothing outside the image; the lane's
// window on that row is the id range [y * W + xlo, y * W + xhi], at most 65 ids, two mask words.  Column pass: output row y ORs the
// words of rows ylo .. yhi (the same words for every lane: LDS broadcasts) and takes its column's bit.  frame_out may be frame_in:
// a pixel is read and written by its own lane only.  Bounded: 20 and 65 trips.
__global__ __launch_bounds__(256) void diff_dilate_kernel(const uint64_t *__restrict__ kept, const uint32_t width, const uint32_t height, const uint32_t dilate,
                                                          uint8_t *__restrict__ mask, const uint16_t *frame_in, uint16_t *frame_out) {
    __shared__ uint64_t rows[kDilateRows];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * kDilateTileX + lane, y0 = blockIdx.y * kDilateTileY;
    const uint32_t n_rows = kDilateTileY + 2 * dilate;
    uint32_t xlo = 0, xhi = 0;
    if (x < width) diff_window(x, dilate, width, xlo, xhi);
    for (uint32_t r = wave; r < n_rows; r += 4) {
        const int64_t y = (int64_t)y0 - dilate + r;
        bool any = false;
        if (x < width && y >= 0 && y < (int64_t)height) {
            const uint32_t at = (uint32_t)y * width;   // (below 2^32: the image has at most 2^32 - 1 pixels)
            any = diff_any_bit(kept, at + xlo, at + xhi);
        }
        const uint64_t bits = __ballot(any);
        if (lane == 0) rows[r] = bits;
    }
    __syncthreads();   // (every lane gets here: no lane has returned)
    for (uint32_t ty = wave; ty < kDilateTileY; ty += 4) {
        const uint32_t y = y0 + ty;
        if (y >= height) break;   // (the whole wave)
        uint32_t ylo, yhi;
        diff_window(y, dilate, height, ylo, yhi);
        uint64_t bits = 0;
        for (uint32_t yy = ylo; yy <= yhi; yy++) bits |= rows[yy + dilate - y0];   // (yy + dilate >= y0: yy >= y - dilate)
        if (x < width) {
            const uint32_t m = (uint32_t)((bits >> lane) & 1u);
            const size_t at = (size_t)y * width + x;
            if (mask) mask[at] = (uint8_t)m;
            if (frame_out) frame_out[at] = m ? (uint16_t)0 : frame_in[at];
        }
    }
}

}  // namespace tsdf

using namespace tsdf;

struct tsdf_frame_diff : DiffSet {
    int compared;           // the list, masks, bases and the frame copy are a compare's of info.width x info.height
    int clustered;          // labels and rows are of that list
    uint16_t *depth;        // the frame as it was compared
    uint64_t *kept;         // one bit per pixel: the pixels of kept blobs, of the last mask call
    size_t depth_cap, kept_cap;
    tsdf_frame_diff_info info;
};

namespace {

constexpr VoxelSetText kDiffText = {
    "frame diff stream order", "frame diff event", "frame diff wait",
    "frame diff scratch alloc failed", "frame diff counts reset", "frame diff count kernels failed", "frame diff counts download", "frame diff count", "frame diff list alloc failed",
    "frame diff cluster alloc failed", "frame diff cluster kernels failed", "frame diff cluster counts download", "frame diff cluster count", "frame diff table alloc failed", "frame diff rows kernel failed"};

void diff_free(tsdf_frame_diff *s) {
    s->release();
    device_free_all(s->depth, s->kept);
    delete s;
}

VoxelGrid diff_grid(const tsdf_frame_diff *s) { return {s->info.width, s->info.height, 1u, (uint32_t)diff_pixels(s->info.width, s->info.height)}; }

// the labels and the table are the list's, and nothing is in flight on them
int blobs_ready(const char *who, const tsdf_frame_diff *s) {
    TSDF_REQUIRE(s, "%s: null handle", who);
    TSDF_REQUIRE(s->compared && s->clustered, "%s: the handle has not been clustered since its last compare (tsdf_frame_diff_cluster)", who);
    return s->wait();
}

}  // namespace

extern "C" {

int tsdf_frame_diff_create(tsdf_frame_diff **out) {
    return handle_create(out, "tsdf_frame_diff_create", "frame diff alloc failed", [](tsdf_frame_diff *s) { return s->create(&kDiffText); }, diff_free);
}

void tsdf_frame_diff_destroy(tsdf_frame_diff *s) {
    if (s) diff_free(s);
}

int tsdf_frame_diff_get_info(const tsdf_frame_diff *s, tsdf_frame_diff_info *info) {
    TSDF_REQUIRE(s && info, "tsdf_frame_diff_get_info: null argument");
    *info = s->info;
    return TSDF_OK;
}

int tsdf_frame_diff_scratch_bytes(const tsdf_frame_diff *s, uint64_t *bytes) {
    TSDF_REQUIRE(s && bytes, "tsdf_frame_diff_scratch_bytes: null argument");
    *bytes = s->scratch_bytes() + (uint64_t)s->depth_cap * sizeof(uint16_t) + (uint64_t)s->kept_cap * sizeof(uint64_t);
    return TSDF_OK;
}

int tsdf_frame_diff_compare_device(tsdf_frame_diff *s, const uint16_t *device_frame, const uint16_t *device_model, uint32_t width, uint32_t height,
                                   const tsdf_diff_params *params, uint8_t *device_states, void *hip_stream) {
    const char *who = "tsdf_frame_diff_compare_device";
    // (what the arguments alone decide comes first: it is refused whatever the handle is)
    TSDF_REQUIRE(device_frame && device_model, "%s: null frame or model", who);
    TSDF_REQUIRE(params, "%s: null params", who);
    TSDF_REQUIRE(width <= kDiffMaxSide && height <= kDiffMaxSide, "%s: %u x %u pixels: a side is above 65535", who, width, height);
    TSDF_REQUIRE(diff_shape_ok(width, height), "%s: %u x %u pixels: width * height must be in 1 .. 2^32 - 1", who, width, height);
    TSDF_REQUIRE(s, "%s: null handle", who);
    hipStream_t stream = (hipStream_t)hip_stream;
    int rc = s->join(stream);
    if (rc != TSDF_OK) return rc;
    s->compared = s->clustered = 0;
    const VoxelGrid grid = {width, height, 1u, (uint32_t)diff_pixels(width, height)};
    hipError_t e = device_reserve(s->depth, s->depth_cap, (size_t)grid.n);
    if (e == hipSuccess) e = device_reserve(s->kept, s->kept_cap, ((size_t)grid.n + 63) / 64);
    if (e != hipSuccess) return hip_fail(e, "frame diff scratch alloc failed");
    tsdf_frame_diff_info &info = s->info;
    uint64_t n_list = 0;
    rc = voxel_set_list(s, who, "nearer pixels", grid, stream, [&](uint32_t n_chunks) -> int {
        info = tsdf_frame_diff_info{};
        info.width = width;
        info.height = height;
        info.tolerance = params->tolerance;
        info.quadratic = params->quadratic;
        s->g = Geom{};
        s->g.X = width;
        s->g.Y = height;
        s->g.Z = 1;
        voxel_flag(DiffFlag{device_frame, device_model, s->depth, device_states, params->tolerance, params->quadratic}, grid, n_chunks, s->masks,
                   s->bases, s->words.dev, stream);
        return TSDF_OK;
    }, &n_list);
    if (rc != TSDF_OK) return rc;
    for (uint32_t k = 0; k < kDiffStates; k++) info.counts[k] = s->words.host[k];
    if (n_list) {
        TSDF_HIP(hipGetLastError(), "frame diff list kernel failed");
        rc = s->leave(stream);
        if (rc != TSDF_OK) return rc;
    }
    s->compared = 1;
    return TSDF_OK;
}

int tsdf_frame_diff_cluster(tsdf_frame_diff *s, uint32_t connectivity, uint32_t depth_step, uint32_t min_pixels, void *hip_stream) {
    const char *who = "tsdf_frame_diff_cluster";
    TSDF_REQUIRE(connectivity == 4u || connectivity == 8u, "%s: connectivity must be 4 or 8, got %u", who, connectivity);
    TSDF_REQUIRE(s, "%s: null handle", who);
    TSDF_REQUIRE(s->compared, "%s: the handle holds no comparison (tsdf_frame_diff_compare_device)", who);
    hipStream_t stream = (hipStream_t)hip_stream;
    int rc = s->join(stream);
    if (rc != TSDF_OK) return rc;
    s->clustered = 0;
    tsdf_frame_diff_info &info = s->info;
    info.connectivity = connectivity;
    info.depth_step = depth_step;
    info.min_pixels = min_pixels;
    info.n_blobs = info.n_kept_blobs = 0;
    const uint64_t n64 = info.counts[kDiffNearer];
    if (n64 == 0) {
        s->clustered = 1;
        return TSDF_OK;
    }
    // (a compare zeroes every word; a second clustering of its list counts the roots again)
    TSDF_HIP(s->words.reset(s->words.dev + DiffSet::kWordRoots, 1, stream), "frame diff cluster count reset");
    uint64_t n_roots = 0, n_rows = 0;
    // (on a grid one plane deep the hook's forward neighbours at 6 / 26 are the image's at 4 / 8)
    rc = voxel_set_cluster(s, NearInDepth{s->depth, depth_step}, (uint32_t)n64, connectivity == 4u ? 6u : 26u, std::max(min_pixels, 1u), stream, &n_roots,
                           &n_rows);
    if (rc != TSDF_OK) return rc;
    info.n_blobs = n_roots;
    info.n_kept_blobs = n_rows;
    s->clustered = 1;
    return TSDF_OK;
}

int tsdf_frame_diff_buffers(const tsdf_frame_diff *s, const uint32_t **device_pixels, const uint64_t **device_masks, const uint32_t **device_bases,
                            const uint32_t **device_labels, const tsdf_diff_blob **device_blobs) {
    const int rc = blobs_ready("tsdf_frame_diff_buffers", s);
    if (rc != TSDF_OK) return rc;
    const bool any = s->info.counts[kDiffNearer] != 0;
    if (device_pixels) *device_pixels = any ? s->list : nullptr;
    if (device_masks) *device_masks = s->masks;
    if (device_bases) *device_bases = s->bases;
    if (device_labels) *device_labels = any ? s->labels : nullptr;
    if (device_blobs) *device_blobs = s->info.n_kept_blobs ? s->rows : nullptr;
    return TSDF_OK;
}

int tsdf_frame_diff_download(const tsdf_frame_diff *s, uint32_t *host_pixels, uint32_t *host_labels, tsdf_diff_blob *host_blobs) {
    const int rc = blobs_ready("tsdf_frame_diff_download", s);
    if (rc != TSDF_OK) return rc;
    const size_t list_bytes = (size_t)s->info.counts[kDiffNearer] * sizeof(uint32_t);
    if (host_pixels && list_bytes) TSDF_HIP(hipMemcpy(host_pixels, s->list, list_bytes, hipMemcpyDeviceToHost), "frame diff download");
    if (host_labels && list_bytes) TSDF_HIP(hipMemcpy(host_labels, s->labels, list_bytes, hipMemcpyDeviceToHost), "frame diff download");
    if (host_blobs && s->info.n_kept_blobs)
        TSDF_HIP(hipMemcpy(host_blobs, s->rows, (size_t)s->info.n_kept_blobs * sizeof(tsdf_diff_blob), hipMemcpyDeviceToHost), "frame diff download");
    return TSDF_OK;
}

int tsdf_frame_diff_mask_device(tsdf_frame_diff *s, uint32_t dilate, uint8_t *device_mask, uint32_t *device_blob_index, const uint16_t *device_frame_in,
                                uint16_t *device_frame_out, void *hip_stream) {
    const char *who = "tsdf_frame_diff_mask_device";
    TSDF_REQUIRE(dilate <= kDiffMaxDilate, "%s: dilate %u is above 32", who, dilate);
    TSDF_REQUIRE(!device_frame_in == !device_frame_out, "%s: frame_in and frame_out are given together or not at all", who);
    TSDF_REQUIRE(s, "%s: null handle", who);
    TSDF_REQUIRE(s->compared && s->clustered, "%s: the handle has not been clustered since its last compare (tsdf_frame_diff_cluster)", who);
    if (!device_mask && !device_blob_index && !device_frame_out) return TSDF_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    int rc = s->join(stream);
    if (rc != TSDF_OK) return rc;
    const VoxelGrid grid = diff_grid(s);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)grid.n + 63) / 64);
    const DiffView d = {s->masks, s->bases, s->labels, s->row_masks, s->row_bases, s->info.n_kept_blobs != 0};
    hipLaunchKernelGGL(diff_paint_kernel, dim3((n_chunks + 3) / 4), dim3(256), 0, stream, d, grid.n, n_chunks, s->kept, device_blob_index);
    if (device_mask || device_frame_out)
        hipLaunchKernelGGL(diff_dilate_kernel, dim3((grid.X + kDilateTileX - 1) / kDilateTileX, (grid.Y + kDilateTileY - 1) / kDilateTileY), dim3(256), 0, stream,
                           s->kept, grid.X, grid.Y, dilate, device_mask, device_frame_in, device_frame_out);
    TSDF_HIP(hipGetLastError(), "frame diff mask kernels failed");
    return s->leave(stream);
}

}  // extern "C"
