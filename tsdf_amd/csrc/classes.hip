// Class fusion for gfx950: a per-voxel class id with a vote count beside the distances (include/tsdf_amd.h, "class fusion").
//
// Opt-in per volume, one dword per voxel, {class: bits 0-15, votes: bits 16-31}, x fastest like the distances; a word without votes
// is 0x00000000.  Colour (colour.hip) is the template: the same opt-in dword (voxel_words.hpp), the same band pass behind the integrate
// kernel over the frame's brick list (band_pass.hpp), the same nearest-voxel sample.  Where colour blends, this votes: the weighted
// Boyer-Moore majority vote keeps one candidate and its lead, which fits the dword and needs one writer per word and no atomics.
//
// The kernels:
//   band_pass_kernel<STD, ClassVote>  (band_pass.hpp) runs behind the integrate kernel (and the colour update) of a
//                           tsdf_integrate_classes call: a voxel in the band whose pixel has a class and a strength takes the vote.
//   class_sample_kernel     one thread per point: class and votes of the voxel the point lies in (tsdf_volume_sample_classes_device).
//   class_counts_kernel     voxels per class: a histogram of the class words, per workgroup in LDS where the classes fit, else
//                           straight to global integer atomics (tsdf_volume_class_counts_device).
#include <algorithm>
#include <cstring>

#include "band_pass.hpp"
#include "voxel_grid.hpp"
#include "voxel_words.hpp"

namespace tsdf {

// One thread per point: the voxel colour_sample_kernel reads (point_voxel_at, voxel_grid.hpp, shared with objects.hip's lookup);
// (VOID, 0) for NaN, off-grid or unclassified (votes = 0) voxels.  votes may be null.
__global__ __launch_bounds__(256) void class_sample_kernel(const uint32_t *__restrict__ cls, const Geom g, const uint64_t n_points,
                                                           const float *__restrict__ points, uint16_t *__restrict__ classes,
                                                           uint16_t *__restrict__ votes) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_points) return;
    size_t at;
    const uint32_t w = point_voxel_at(g, points + 3 * i, at) ? cls[at] : 0u;
    const uint32_t n = w >> 16;
    classes[i] = (uint16_t)(n ? (w & 0xFFFFu) : kClassVoid);
    if (votes) votes[i] = (uint16_t)n;
}

// Voxels per class.  A grid-stride walk of the class words, a wave on 64 consecutive words per step.  LDS = true: a histogram of
// n_classes 32-bit bins per workgroup in LDS (a workgroup sees far fewer than 2^32 voxels), its non-zero bins added to the 64-bit counts
// at the end; LDS = false: straight to the counts in global memory, one add per wave and distinct class among its 64 words -- a scene's
// band holds a handful of classes, and 64 lanes adding 1 to the same three addresses serialise in the L2 (2.5 ms at 256^3 before the
// lanes were grouped).  Integer atomics either way: the counts are unique.
//
// The threshold (kClassCountsLdsBins) is 4096 bins = 16 KiB a workgroup.  A compute unit has 160 KiB of LDS and room for 32 waves =
// 8 workgroups of 256 lanes: at 16 KiB each the 8 of them take 128 KiB, so the histogram never costs a resident wave, and one more
// doubling would (32 KiB x 8 > 160 KiB).  Label sets of segmentation networks (tens to a few thousand classes) all fit.
constexpr uint32_t kClassCountsLdsBins = 4096;
constexpr uint32_t kClassCountsGrid = 2048;   // workgroups at most: 8 per compute unit

template <bool LDS>
__global__ __launch_bounds__(256) void class_counts_kernel(const uint32_t *__restrict__ cls, const size_t n_voxels, const uint32_t n_classes,
                                                           const uint32_t min_votes, unsigned long long *__restrict__ counts) {
    extern __shared__ uint32_t bins[];
    if (LDS) {
        for (uint32_t j = threadIdx.x; j < n_classes; j += 256u) bins[j] = 0;
        __syncthreads();
    }
    const size_t stride = (size_t)gridDim.x * 256u;
    const uint32_t lane = threadIdx.x & 63u;
    // (the loop's bounds are the wave's, not the lane's: every lane of a wave makes the same trips, the ballots below need that)
    for (size_t base = (size_t)blockIdx.x * 256u + (threadIdx.x - lane); base < n_voxels; base += stride) {
        const size_t i = base + lane;
        const uint32_t w = i < n_voxels ? cls[i] : 0u;
        const uint32_t c = w & 0xFFFFu;
        bool counted = (w >> 16) >= min_votes && c < n_classes;   // (min_votes >= 1: an unclassified word, and the tail's 0, never counts)
        if (LDS) {
            if (counted) atomicAdd(&bins[c], 1u);
        } else {
            unsigned long long left = __ballot(counted);
            while (left) {
                const int leader = __ffsll((long long)left) - 1;
                const uint32_t lc = (uint32_t)__shfl((int)c, leader);
                const bool mine = counted && c == lc;
                const unsigned long long group = __ballot(mine);
                if ((int)lane == leader) atomicAdd(&counts[lc], (unsigned long long)__popcll(group));
                if (mine) counted = false;
                left &= ~group;
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < n_classes; j += 256u) {
            const uint32_t m = bins[j];
            if (m) atomicAdd(&counts[j], (unsigned long long)m);
        }
    }
}

// integrate.hip calls this behind the integrate kernel (and the colour update) of the same frame
int launch_class_integrate(tsdf_volume *v, const BrickGrid &bg, const Mat44 &ip, const Mat33 &mk, const Mat33 &mkinv, bool std_camera,
                           uint32_t width, uint32_t height, const uint16_t *d_depth, const uint16_t *d_classes, const uint8_t *d_confidence,
                           const uint32_t *count) {
    return launch_band_pass(v, v->classes, bg, ip, mk, mkinv, std_camera, width, height, d_depth, ClassVote{d_classes, d_confidence}, count,
                            "Class integrate kernel failed");
}

static int sample_classes(const tsdf_volume *v, uint64_t n, const float *d_points, uint16_t *d_classes, uint16_t *d_votes,
                          hipStream_t stream) {
    if (n == 0) return TSDF_OK;
    const uint64_t blocks = (n + 255) / 256;
    TSDF_REQUIRE(blocks <= 0x7FFFFFFFull, "tsdf_volume_sample_classes: too many points");
    hipLaunchKernelGGL(class_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, v->classes, v->g, n, d_points, d_classes, d_votes);
    TSDF_HIP(hipGetLastError(), "Class sample kernel failed");
    return TSDF_OK;
}

constexpr VoxelWords kClassWords = {&tsdf_volume::classes,
                                    "%s: classes are not enabled on this volume (tsdf_volume_enable_classes)",
                                    "%s: classes are not supported on a Z-slab volume (tsdf_volume_create_slab)",
                                    "class free", "Couldn't allocate space for class data", "Couldn't clear class data",
                                    "Failed to copy class data to device", "Failed to copy class data from device"};

// everything tsdf_integrate_classes* refuses, before anything is written
static int check_class_integrate(const tsdf_volume *v, const void *depth, const void *rgb, const void *classes, uint32_t width,
                                 uint32_t height, const float *inv_pose, const float *k, const float *kinv) {
    const int rc = voxel_words_require(v, kClassWords, "tsdf_integrate_classes");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(depth && classes && inv_pose && k && kinv, "tsdf_integrate_classes: null argument");
    TSDF_REQUIRE(width > 0 && height > 0, "tsdf_integrate_classes: empty depth map");
    TSDF_REQUIRE(!v->nodes, "tsdf_integrate_classes: not supported once the deformation nodes are explicit (deformation() / set_deformation())");
    TSDF_REQUIRE(!rgb || v->colour, "tsdf_integrate_classes: rgb given but colour is not enabled on this volume (tsdf_volume_enable_colour)");
    return TSDF_OK;
}

}  // namespace tsdf

using namespace tsdf;

extern "C" {

int tsdf_volume_enable_classes(tsdf_volume *v, int enabled) { return voxel_words_enable(v, kClassWords, "tsdf_volume_enable_classes", enabled); }

int tsdf_volume_classes_enabled(const tsdf_volume *v, int *enabled) {
    return voxel_words_enabled(v, kClassWords, "tsdf_volume_classes_enabled", enabled);
}

int tsdf_volume_classes(const tsdf_volume *v, uint32_t **device_ptr) {
    return voxel_words_pointer(v, kClassWords, "tsdf_volume_classes", device_ptr);
}

int tsdf_volume_get_class_data(const tsdf_volume *v, uint32_t *host) {
    return voxel_words_copy(v, kClassWords, "tsdf_volume_get_class_data", host, nullptr);
}

int tsdf_volume_set_class_data(tsdf_volume *v, const uint32_t *host) {
    return voxel_words_copy(v, kClassWords, "tsdf_volume_set_class_data", nullptr, host);
}

int tsdf_integrate_classes_device(tsdf_volume *v, const uint16_t *device_depth, const uint8_t *device_rgb, const uint16_t *device_classes,
                                  const uint8_t *device_confidence, uint32_t width, uint32_t height, const float pose[16],
                                  const float inv_pose[16], const float k[9], const float kinv[9]) {
    const int rc = check_class_integrate(v, device_depth, device_rgb, device_classes, width, height, inv_pose, k, kinv);
    if (rc != TSDF_OK) return rc;
    (void)pose;   // (as tsdf_integrate: the reference never reads it)
    IntegrateFrame f{device_depth, width, height, inv_pose, k, kinv};
    f.rgb = device_rgb;
    f.classes = device_classes;
    f.confidence = device_confidence;
    return launch_integrate(v, f);
}

int tsdf_integrate_classes(tsdf_volume *v, const uint16_t *host_depth, const uint8_t *host_rgb, const uint16_t *host_classes,
                           const uint8_t *host_confidence, uint32_t width, uint32_t height, const float pose[16], const float inv_pose[16],
                           const float k[9], const float kinv[9]) {
    const int rc0 = check_class_integrate(v, host_depth, host_rgb, host_classes, width, height, inv_pose, k, kinv);
    if (rc0 != TSDF_OK) return rc0;
    const size_t pixels = (size_t)width * height;
    TSDF_HIP(device_reserve_bytes(v->depth_buf, v->depth_cap, pixels * sizeof(uint16_t)), "Couldn't allocate storage for depth map");
    TSDF_HIP(device_reserve(v->class_buf, v->class_cap, pixels), "Couldn't allocate storage for class frame");
    if (host_rgb) TSDF_HIP(device_reserve(v->rgb_buf, v->rgb_cap, pixels * 3), "Couldn't allocate storage for colour frame");
    if (host_confidence) TSDF_HIP(device_reserve(v->conf_buf, v->conf_cap, pixels), "Couldn't allocate storage for confidence frame");
    TSDF_HIP(hipMemcpyAsync(v->depth_buf, host_depth, pixels * sizeof(uint16_t), hipMemcpyHostToDevice, v->stream),
             "Failed to copy depth map to GPU");
    TSDF_HIP(hipMemcpyAsync(v->class_buf, host_classes, pixels * sizeof(uint16_t), hipMemcpyHostToDevice, v->stream),
             "Failed to copy class frame to GPU");
    if (host_rgb)
        TSDF_HIP(hipMemcpyAsync(v->rgb_buf, host_rgb, pixels * 3, hipMemcpyHostToDevice, v->stream), "Failed to copy colour frame to GPU");
    if (host_confidence)
        TSDF_HIP(hipMemcpyAsync(v->conf_buf, host_confidence, pixels, hipMemcpyHostToDevice, v->stream),
                 "Failed to copy confidence frame to GPU");
    const int rc = tsdf_integrate_classes_device(v, v->depth_buf, host_rgb ? v->rgb_buf : nullptr, v->class_buf,
                                                 host_confidence ? v->conf_buf : nullptr, width, height, pose, inv_pose, k, kinv);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipStreamSynchronize(v->stream), "Class integrate failed");
    return TSDF_OK;
}

int tsdf_volume_sample_classes_device(const tsdf_volume *v, uint64_t n, const float *device_points, uint16_t *device_classes,
                                      uint16_t *device_votes, void *hip_stream) {
    const int rc = voxel_words_require(v, kClassWords, "tsdf_volume_sample_classes");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(n == 0 || (device_points && device_classes), "tsdf_volume_sample_classes: null argument");
    return sample_classes(v, n, device_points, device_classes, device_votes, (hipStream_t)hip_stream);
}

int tsdf_raycast_classes_device(const tsdf_volume *v, uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                                float *device_vertices, float *device_normals, uint16_t *device_classes, uint16_t *device_votes) {
    const int rc0 = voxel_words_require(v, kClassWords, "tsdf_raycast_classes");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(device_vertices && device_classes, "tsdf_raycast_classes: null buffer");
    const int rc = tsdf_raycast_device(v, width, height, pose, kinv, device_vertices, device_normals);
    if (rc != TSDF_OK) return rc;
    return sample_classes(v, (uint64_t)width * height, device_vertices, device_classes, device_votes, v->stream);
}

int tsdf_raycast_classes(const tsdf_volume *cv, uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                         float *host_vertices, float *host_normals, uint16_t *host_classes, uint16_t *host_votes) {
    const int rc0 = voxel_words_require(cv, kClassWords, "tsdf_raycast_classes");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(host_vertices && host_classes, "tsdf_raycast_classes: null buffer");
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);   // per-call temporaries are cached in the handle
    const size_t pixels = (size_t)width * height;
    // tsdf_raycast leaves the vertex map in the handle's vertex buffer: the classes are sampled from there, {classes, votes} into the
    // class upload buffer
    int rc = tsdf_raycast(v, width, height, pose, kinv, host_vertices, host_normals);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(device_reserve(v->class_buf, v->class_cap, 2 * pixels), "Couldn't allocate storage for class map");
    rc = sample_classes(v, pixels, v->vert_buf, v->class_buf, v->class_buf + pixels, v->stream);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipMemcpyAsync(host_classes, v->class_buf, pixels * sizeof(uint16_t), hipMemcpyDeviceToHost, v->stream), "Classes Memcpy failed");
    if (host_votes)
        TSDF_HIP(hipMemcpyAsync(host_votes, v->class_buf + pixels, pixels * sizeof(uint16_t), hipMemcpyDeviceToHost, v->stream),
                 "Classes Memcpy failed");
    TSDF_HIP(hipStreamSynchronize(v->stream), "Class sample failed");
    return TSDF_OK;
}

int tsdf_volume_class_counts_device(const tsdf_volume *v, uint32_t n_classes, uint32_t min_votes, uint64_t *device_counts, void *hip_stream) {
    const int rc = voxel_words_require(v, kClassWords, "tsdf_volume_class_counts");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(device_counts, "tsdf_volume_class_counts: null argument");
    TSDF_REQUIRE(n_classes >= 1 && n_classes <= 65535u, "tsdf_volume_class_counts: n_classes %u is not in 1..65535", n_classes);
    const hipStream_t stream = (hipStream_t)hip_stream;
    const size_t n = v->resident_voxels();
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(device_counts);
    TSDF_HIP(hipMemsetAsync(counts, 0, (size_t)n_classes * sizeof(uint64_t), stream), "Couldn't clear the class counts");
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, kClassCountsGrid);
    const uint32_t votes = std::max(min_votes, 1u);
    if (n_classes <= kClassCountsLdsBins)
        hipLaunchKernelGGL(class_counts_kernel<true>, dim3(grid), dim3(256), n_classes * sizeof(uint32_t), stream, v->classes, n, n_classes,
                           votes, counts);
    else
        hipLaunchKernelGGL(class_counts_kernel<false>, dim3(grid), dim3(256), 0, stream, v->classes, n, n_classes, votes, counts);
    TSDF_HIP(hipGetLastError(), "Class counts kernel failed");
    return TSDF_OK;
}

int tsdf_volume_class_counts(const tsdf_volume *v, uint32_t n_classes, uint32_t min_votes, uint64_t *host_counts) {
    const int rc0 = voxel_words_require(v, kClassWords, "tsdf_volume_class_counts");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(host_counts, "tsdf_volume_class_counts: null argument");
    TSDF_REQUIRE(n_classes >= 1 && n_classes <= 65535u, "tsdf_volume_class_counts: n_classes %u is not in 1..65535", n_classes);
    HostStage st;
    const size_t bytes = (size_t)n_classes * sizeof(uint64_t);
    int rc = st.begin(v->stream, bytes, "tsdf_volume_class_counts: couldn't allocate %zu bytes for the counts");
    if (rc != TSDF_OK) return rc;
    rc = tsdf_volume_class_counts_device(v, n_classes, min_votes, (uint64_t *)st.buf, v->stream);
    if (rc == TSDF_OK) st.down(host_counts, st.buf, bytes);
    return st.finish(rc, "Class counts failed");
}

}  // extern "C"
