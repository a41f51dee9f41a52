// Exploration queries for gfx950 (include/tsdf_amd.h, "exploration"): which free voxels border unseen space, how they
// hang together, and how much unseen space a set of rays would see.  No reference counterpart.  Nothing of the volume is written.
//
// Frontiers: FrontierFlag, the state of a voxel (unknown / free / occupied) and the frontier test, four counters.  The flag walk, the
// list and the clusters are voxel_set.hpp's, with the policy "any listed neighbour is adjacent".
// View gain: a lane per ray.
//   view_gain_kernel         gain_walk (explore_walk.hpp); an unknown voxel sets its bit in the handle's mask with atomicOr
//   mask_count_kernel        the set bits, by popcount and a wave sum, one integer atomic per wave that has any
// Every result is a set, an integer sum, a minimum or a maximum: two runs give the same bytes whatever order the waves run in.  No float
// atomics, no lane waits for another, and every loop has a stated bound.
#include "common.hpp"
#include "explore_walk.hpp"
#include "field_sample.hpp"
#include "voxel_set.hpp"

namespace tsdf {

// the handle's counter words: the flag kernel's four, then the set's two (roots, scan total: voxel_set.hpp), then the gain
enum { kWordUnknown = 0, kWordFree = 1, kWordOccupied = 2, kWordFrontiers = 3, kWordGain = 6 };
using FrontierSet = VoxelSet<tsdf_frontier_cluster, 4, 8>;

constexpr uint64_t kGainMaxRays = (uint64_t)0x7fffffff * 256;   // what a launch of 256-lane workgroups holds

// The state of every voxel (unknown / free / occupied: voxel_state, field_sample.hpp) and the frontier test: free, with a 6-neighbour
// inside the grid that is unknown.  The counters in the order of kWordUnknown .. kWordFrontiers; the frontiers are listed.
struct FrontierFlag {
    static constexpr uint32_t kCounts = 4, kListed = kWordFrontiers;
    const float *dist;
    WeightView wv;
    __device__ uint32_t operator()(uint32_t id, const VoxelGrid &grid) const {
        uint32_t x, y, z;
        grid.split(id, x, y, z);
        const size_t xy = (size_t)grid.X * grid.Y, ip = (size_t)grid.X * y + x;
        const int state = voxel_state(dist, wv, xy, ip, z);
        bool frontier = false;
        if (state == kVoxelFree) {
            auto unseen = [&](size_t ip2, uint32_t z2) { return !voxel_observed(wv, xy, ip2, z2); };
            frontier = (x > 0 && unseen(ip - 1, z)) || (x + 1 < grid.X && unseen(ip + 1, z)) || (y > 0 && unseen(ip - grid.X, z)) ||
                       (y + 1 < grid.Y && unseen(ip + grid.X, z)) || (z > 0 && unseen(ip, z - 1)) || (z + 1 < grid.Z && unseen(ip, z + 1));
        }
        // (a bit per test, each selected on its own: the walk's ballots then read the tests themselves)
        return (state == kVoxelUnknown ? 1u << kWordUnknown : 0u) | (state == kVoxelFree ? 1u << kWordFree : 0u) |
               (state == kVoxelOccupied ? 1u << kWordOccupied : 0u) | (frontier ? 1u << kWordFrontiers : 0u);
    }
};

struct GainView {
    const float *dist;
    WeightView wv;
    Geom g;
};

__global__ __launch_bounds__(256) void view_gain_kernel(const GainView f, const uint64_t n, const float *__restrict__ origins,
                                                        const float *__restrict__ directions, const float *__restrict__ t_max,
                                                        uint32_t *__restrict__ unknown, uint32_t *__restrict__ free_out, uint8_t *__restrict__ stop,
                                                        uint32_t *gain_mask) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t xy = (size_t)f.g.X * f.g.Y;
    uint32_t n_unknown, n_free;
    const uint8_t code = gain_walk(f.g, origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], directions[3 * i], directions[3 * i + 1],
                                   directions[3 * i + 2], t_max ? t_max[i] : INFINITY, n_unknown, n_free, [&](int ix, int iy, int iz) {
                                       const size_t ip = (size_t)f.g.X * (uint32_t)iy + (uint32_t)ix;
                                       if (!voxel_observed(f.wv, xy, ip, (uint32_t)iz)) {
                                           const uint32_t id = (uint32_t)(xy * (uint32_t)iz + ip);
                                           atomicOr(gain_mask + (id >> 5), 1u << (id & 31u));   // (a set: order-free)
                                           return (int)kVoxelUnknown;
                                       }
                                       return voxel_occupied(f.dist, xy * (uint32_t)iz + ip) ? (int)kVoxelOccupied : (int)kVoxelFree;
                                   });
    if (unknown) unknown[i] = n_unknown;
    if (free_out) free_out[i] = n_free;
    if (stop) stop[i] = code;
}

__global__ __launch_bounds__(256) void mask_count_kernel(const uint32_t n_words, const uint32_t *__restrict__ gain_mask,
                                                         unsigned long long *__restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t bits = i < n_words ? (uint32_t)__popc(gain_mask[i]) : 0u;
    for (int o = 32; o > 0; o >>= 1) bits += (uint32_t)__shfl_xor(bits, o);
    if (bits && (threadIdx.x & 63u) == 0) atomicAdd(words + kWordGain, (unsigned long long)bits);
}

}  // namespace tsdf

using namespace tsdf;

struct tsdf_explorer : FrontierSet {
    int has_geometry;       // a find_frontiers or a view gain has given the handle a geometry (g)
    int found;              // the list, masks and bases are a find_frontiers' of that geometry
    int clustered;          // labels and rows are of that list
    int mask_ready;         // the gain mask is allocated for that geometry and holds only bits that view-gain calls have set
    uint32_t *gain_mask;    // one bit per voxel
    size_t gain_mask_cap;
    tsdf_explorer_info info;
};

namespace {

constexpr VoxelSetText kExplorerText = {
    "explorer stream order", "explorer event", "explorer wait",
    "frontier scratch alloc failed", "frontier counts reset", "frontier count kernels failed", "frontier counts download", "frontier count", "frontier list alloc failed",
    "frontier cluster alloc failed", "frontier cluster kernels failed", "frontier cluster counts download", "frontier cluster count", "frontier cluster table alloc failed", "frontier rows kernel failed"};

void explorer_free(tsdf_explorer *s) {
    s->release();
    (void)hipFree(s->gain_mask);
    delete s;
}

void adopt_geometry(tsdf_explorer *s, const Geom &g) {
    if (!s->has_geometry || s->g.X != g.X || s->g.Y != g.Y || s->g.Z != g.Z) s->mask_ready = 0;   // the bits are voxel ids of another grid
    s->g = g;
    s->has_geometry = 1;
    geometry_into(s->info, g);
}

// what every entry point that reads a volume refuses, under its own name
int volume_checked(const char *who, const tsdf_volume *v, const tsdf_explorer *s) {
    TSDF_REQUIRE(v, "%s: null volume", who);
    TSDF_REQUIRE(s, "%s: null explorer handle", who);
    return whole_volume_checked(who, v, s->device, "a voxel's neighbours and a ray's voxels lie in other slabs");
}

// the labels and the table are the list's, and nothing is in flight on them
int clusters_ready(const char *who, const tsdf_explorer *s) {
    TSDF_REQUIRE(s, "%s: null handle", who);
    TSDF_REQUIRE(s->found && s->clustered, "%s: the handle has not been clustered since its last tsdf_volume_find_frontiers (tsdf_explorer_cluster_frontiers)", who);
    return s->wait();
}

int gain_checked(const char *who, const tsdf_volume *v, const tsdf_explorer *s, uint64_t n, const float *origins, const float *directions,
                 uint32_t flags, const void *unknown, const void *free_out, const void *stop, const void *gain) {
    const int rc = volume_checked(who, v, s);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE((flags & ~(uint32_t)TSDF_GAIN_KEEP_MASK) == 0, "%s: unknown flags %#x", who, flags);
    TSDF_REQUIRE(unknown || free_out || stop || gain, "%s: no output asked for (all four are NULL)", who);
    TSDF_REQUIRE(n == 0 || (origins && directions), "%s: null origins or directions with n = %llu", who, (unsigned long long)n);
    TSDF_REQUIRE(n <= kGainMaxRays, "%s: %llu rays are more than a launch holds (%llu)", who, (unsigned long long)n, (unsigned long long)kGainMaxRays);
    TSDF_REQUIRE(!s->has_geometry || same_geometry(s->g, v->g),
                 "%s: the handle holds the geometry of another volume (%u x %u x %u, or other voxel sizes or offset): use a fresh handle or "
                 "tsdf_volume_find_frontiers into this one", who, s->g.X, s->g.Y, s->g.Z);
    return TSDF_OK;
}

// the launches of a view gain on the volume's stream; the arrays are device arrays.  Synchronises once when host_gain is asked for.
int gain_on(tsdf_volume *v, tsdf_explorer *s, uint64_t n, const float *origins, const float *directions, const float *t_max, uint32_t flags,
            uint32_t *unknown, uint32_t *free_out, uint8_t *stop, uint64_t *host_gain) {
    hipStream_t stream = v->stream;
    int rc = s->join(stream);
    if (rc != TSDF_OK) return rc;
    adopt_geometry(s, v->g);
    const VoxelGrid grid = voxel_grid(v->g);
    const size_t n_words = ((size_t)grid.n + 31) / 32;
    if (n_words > s->gain_mask_cap) s->mask_ready = 0;
    const hipError_t e = device_reserve(s->gain_mask, s->gain_mask_cap, n_words);
    if (e != hipSuccess) {
        s->mask_ready = 0;
        return hip_fail(e, "view gain mask alloc failed");
    }
    if (!s->mask_ready || !(flags & TSDF_GAIN_KEEP_MASK)) TSDF_HIP(hipMemsetAsync(s->gain_mask, 0, n_words * sizeof(uint32_t), stream), "view gain mask reset");
    s->mask_ready = 1;
    if (n) {
        const GainView f = {v->dist, {v->weight, v->wpacked, v->wmode}, v->g};
        hipLaunchKernelGGL(view_gain_kernel, grid_for(n, 256), dim3(256), 0, stream, f, n, origins, directions, t_max, unknown, free_out, stop, s->gain_mask);
    }
    if (host_gain) {
        TSDF_HIP(s->words.reset(s->words.dev + kWordGain, 1, stream), "view gain count reset");
        hipLaunchKernelGGL(mask_count_kernel, grid_for(n_words, 256), dim3(256), 0, stream, (uint32_t)n_words, s->gain_mask, s->words.dev);
        TSDF_HIP(s->words.download(s->words.dev + kWordGain, 1, stream), "view gain count download");
    }
    TSDF_HIP(hipGetLastError(), "view gain kernels failed");
    rc = s->leave(stream);
    if (rc != TSDF_OK) return rc;
    if (host_gain) {
        TSDF_HIP(hipStreamSynchronize(stream), "view gain count");
        s->pending = 0;
        *host_gain = s->words.host[kWordGain];
    }
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_explorer_create(tsdf_explorer **out) {
    return handle_create(out, "tsdf_explorer_create", "explorer alloc failed", [](tsdf_explorer *s) { return s->create(&kExplorerText); }, explorer_free);
}

void tsdf_explorer_destroy(tsdf_explorer *s) {
    if (s) explorer_free(s);
}

int tsdf_volume_find_frontiers(const tsdf_volume *cv, uint32_t flags, tsdf_explorer *s) {
    const int rcc = volume_checked("tsdf_volume_find_frontiers", cv, s);
    if (rcc != TSDF_OK) return rcc;
    TSDF_REQUIRE(flags == 0, "tsdf_volume_find_frontiers: unknown flags %#x", flags);
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);
    hipStream_t stream = v->stream;
    int rc = s->join(stream);
    if (rc != TSDF_OK) return rc;
    s->found = s->clustered = 0;
    const VoxelGrid grid = voxel_grid(v->g);
    uint64_t n_list = 0;
    rc = voxel_set_list(s, "tsdf_volume_find_frontiers", "frontiers", grid, stream, [&](uint32_t n_chunks) -> int {
        adopt_geometry(s, v->g);
        s->info.connectivity = 0;
        s->info.n_unknown = s->info.n_free = s->info.n_occupied = s->info.n_frontiers = s->info.n_clusters = s->info.n_listed_clusters = 0;
        voxel_flag(FrontierFlag{v->dist, {v->weight, v->wpacked, v->wmode}}, grid, n_chunks, s->masks, s->bases, s->words.dev, stream);
        return TSDF_OK;
    }, &n_list);
    if (rc != TSDF_OK) return rc;
    s->info.n_unknown = s->words.host[kWordUnknown];
    s->info.n_free = s->words.host[kWordFree];
    s->info.n_occupied = s->words.host[kWordOccupied];
    s->info.n_frontiers = n_list;
    if (n_list) {
        TSDF_HIP(hipGetLastError(), "frontier list kernel failed");
        rc = s->leave(stream);
        if (rc != TSDF_OK) return rc;
    }
    s->found = 1;
    return TSDF_OK;
}

int tsdf_explorer_get_info(const tsdf_explorer *s, tsdf_explorer_info *info) {
    TSDF_REQUIRE(s && info, "tsdf_explorer_get_info: null argument");
    *info = s->info;
    return TSDF_OK;
}

int tsdf_explorer_frontier_buffers(const tsdf_explorer *s, const uint32_t **device_voxels, const uint64_t **device_masks, const uint32_t **device_bases) {
    TSDF_REQUIRE(s, "tsdf_explorer_frontier_buffers: null handle");
    TSDF_REQUIRE(s->found, "tsdf_explorer_frontier_buffers: the handle holds no frontiers (tsdf_volume_find_frontiers)");
    const int rc = s->wait();
    if (rc != TSDF_OK) return rc;
    if (device_voxels) *device_voxels = s->info.n_frontiers ? s->list : nullptr;
    if (device_masks) *device_masks = s->masks;
    if (device_bases) *device_bases = s->bases;
    return TSDF_OK;
}

int tsdf_explorer_frontier_download(const tsdf_explorer *s, uint32_t *host_voxels) {
    TSDF_REQUIRE(s && host_voxels, "tsdf_explorer_frontier_download: null argument");
    TSDF_REQUIRE(s->found, "tsdf_explorer_frontier_download: the handle holds no frontiers (tsdf_volume_find_frontiers)");
    const int rc = s->wait();
    if (rc != TSDF_OK) return rc;
    if (s->info.n_frontiers) TSDF_HIP(hipMemcpy(host_voxels, s->list, (size_t)s->info.n_frontiers * sizeof(uint32_t), hipMemcpyDeviceToHost), "frontier download");
    return TSDF_OK;
}

int tsdf_explorer_scratch_bytes(const tsdf_explorer *s, uint64_t *bytes) {
    TSDF_REQUIRE(s && bytes, "tsdf_explorer_scratch_bytes: null argument");
    *bytes = s->scratch_bytes() + (uint64_t)s->gain_mask_cap * sizeof(uint32_t);
    return TSDF_OK;
}

int tsdf_explorer_cluster_frontiers(tsdf_explorer *s, uint32_t connectivity, uint32_t min_size, void *hip_stream) {
    TSDF_REQUIRE(s, "tsdf_explorer_cluster_frontiers: null handle");
    TSDF_REQUIRE(connectivity == 6u || connectivity == 26u, "tsdf_explorer_cluster_frontiers: connectivity must be 6 or 26, got %u", connectivity);
    TSDF_REQUIRE(s->found, "tsdf_explorer_cluster_frontiers: the handle holds no frontiers (tsdf_volume_find_frontiers)");
    hipStream_t stream = (hipStream_t)hip_stream;
    int rc = s->join(stream);
    if (rc != TSDF_OK) return rc;
    s->clustered = 0;
    s->info.connectivity = connectivity;
    s->info.n_clusters = s->info.n_listed_clusters = 0;
    const uint64_t n64 = s->info.n_frontiers;
    if (n64 == 0) {
        s->clustered = 1;
        return TSDF_OK;
    }
    // (a find_frontiers zeroes every word; a second clustering of its list counts the roots again)
    TSDF_HIP(s->words.reset(s->words.dev + FrontierSet::kWordRoots, 1, stream), "frontier cluster count reset");
    uint64_t n_roots = 0, n_rows = 0;
    rc = voxel_set_cluster(s, AnyListedNeighbour{}, (uint32_t)n64, connectivity, min_size, stream, &n_roots, &n_rows);
    if (rc != TSDF_OK) return rc;
    s->info.n_clusters = n_roots;
    s->info.n_listed_clusters = n_rows;
    s->clustered = 1;
    return TSDF_OK;
}

int tsdf_explorer_cluster_buffers(const tsdf_explorer *s, const uint32_t **device_labels, const tsdf_frontier_cluster **device_clusters) {
    const int rc = clusters_ready("tsdf_explorer_cluster_buffers", s);
    if (rc != TSDF_OK) return rc;
    if (device_labels) *device_labels = s->info.n_frontiers ? s->labels : nullptr;
    if (device_clusters) *device_clusters = s->info.n_listed_clusters ? s->rows : nullptr;
    return TSDF_OK;
}

int tsdf_explorer_cluster_download(const tsdf_explorer *s, uint32_t *host_labels, tsdf_frontier_cluster *host_clusters) {
    const int rc = clusters_ready("tsdf_explorer_cluster_download", s);
    if (rc != TSDF_OK) return rc;
    if (host_labels && s->info.n_frontiers)
        TSDF_HIP(hipMemcpy(host_labels, s->labels, (size_t)s->info.n_frontiers * sizeof(uint32_t), hipMemcpyDeviceToHost), "frontier cluster download");
    if (host_clusters && s->info.n_listed_clusters)
        TSDF_HIP(hipMemcpy(host_clusters, s->rows, (size_t)s->info.n_listed_clusters * sizeof(tsdf_frontier_cluster), hipMemcpyDeviceToHost), "frontier cluster download");
    return TSDF_OK;
}

int tsdf_volume_view_gain_device(const tsdf_volume *cv, tsdf_explorer *s, uint64_t n, const float *device_origins, const float *device_directions,
                                 const float *device_t_max, uint32_t flags, uint32_t *device_unknown, uint32_t *device_free, uint8_t *device_stop,
                                 uint64_t *host_gain) {
    const int rc = gain_checked("tsdf_volume_view_gain_device", cv, s, n, device_origins, device_directions, flags, device_unknown, device_free,
                                device_stop, host_gain);
    if (rc != TSDF_OK) return rc;
    return gain_on(const_cast<tsdf_volume *>(cv), s, n, device_origins, device_directions, device_t_max, flags, device_unknown, device_free, device_stop,
                   host_gain);
}

int tsdf_volume_view_gain(const tsdf_volume *cv, tsdf_explorer *s, uint64_t n, const float *host_origins, const float *host_directions,
                          const float *host_t_max, uint32_t flags, uint32_t *host_unknown, uint32_t *host_free, uint8_t *host_stop, uint64_t *host_gain) {
    const int rc0 = gain_checked("tsdf_volume_view_gain", cv, s, n, host_origins, host_directions, flags, host_unknown, host_free, host_stop, host_gain);
    if (rc0 != TSDF_OK) return rc0;
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);
    if (n == 0) return gain_on(v, s, 0, nullptr, nullptr, nullptr, flags, nullptr, nullptr, nullptr, host_gain);
    // one allocation: origins and directions (3n floats each), t_max (n), then unknown and free (n words each) and stop (n bytes), as far as asked for
    const size_t fn = (size_t)n;
    const size_t o_dir = 3 * fn, o_t = 6 * fn, o_u = o_t + (host_t_max ? fn : 0), o_f = o_u + (host_unknown ? fn : 0), o_s = o_f + (host_free ? fn : 0);
    const size_t bytes = o_s * sizeof(float) + (host_stop ? fn : 0);
    HostStage st;
    int rc = st.begin(v->stream, bytes, "tsdf_volume_view_gain: couldn't allocate %zu bytes for the rays and results");
    if (rc != TSDF_OK) return rc;
    float *const buf = static_cast<float *>(st.buf);
    uint32_t *const words = static_cast<uint32_t *>(st.buf);
    float *t = host_t_max ? buf + o_t : nullptr;
    uint32_t *u = host_unknown ? words + o_u : nullptr, *f = host_free ? words + o_f : nullptr;
    uint8_t *sp = host_stop ? reinterpret_cast<uint8_t *>(words + o_s) : nullptr;
    st.up(buf, host_origins, 3 * fn * sizeof(float));
    st.up(buf + o_dir, host_directions, 3 * fn * sizeof(float));
    if (t) st.up(t, host_t_max, fn * sizeof(float));
    if (st.ok()) rc = gain_on(v, s, n, buf, buf + o_dir, t, flags, u, f, sp, host_gain);
    if (rc == TSDF_OK) {
        if (u) st.down(host_unknown, u, fn * sizeof(uint32_t));
        if (f) st.down(host_free, f, fn * sizeof(uint32_t));
        if (sp) st.down(host_stop, sp, fn);
    }
    return st.finish(rc, "View gain failed");
}

}  // extern "C"
