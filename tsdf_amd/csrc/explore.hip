// Exploration queries for gfx950 (include/tsdf_amd.h, "exploration"): which free voxels border unseen space, how they
// hang together, and how much unseen space a set of rays would see.  No reference counterpart.  Nothing of the volume is written.
//
// Frontiers: chunks of 64 consecutive voxel ids, a wave at a time.
//   frontier_flag_kernel     the state of every voxel (unknown / free / occupied) and the frontier test; per chunk the ballot mask and
//                            its popcount; the four counts by ballot and popcount over the 64 chunks a wave walks, one integer atomic
//                            per workgroup that has any
//   (the chunk scan of mesh_scan.hip turns the popcounts into bases)
//   frontier_list_kernel     list[compact_index(mask, base, id)] = id: ascending, no atomics, one writer per word
// Clusters: the union-find of union_find.hpp over the list indices, a lane per listed voxel.
//   frontier_init_kernel     parent[i] = i, the accumulator rows emptied
//   frontier_hook_kernel     the 3 or 13 forward neighbours, looked up through mask + base, united with the lane's own index
//   frontier_flatten_kernel  L[i] = root(i) (a launch of its own: the kernel boundary makes every hook visible); roots counted
//   frontier_stats_kernel    size, coordinate sums and the box, to the root's row with integer atomics; one set per wave and root
//   frontier_keep_kernel     per 64 list indices: the mask of roots with size >= min_size and its popcount (then the chunk scan)
//   frontier_rows_kernel     the kept rows, in ascending label, to where compact_index says
// View gain: a lane per ray.
//   view_gain_kernel         gain_walk (explore_walk.hpp); an unknown voxel sets its bit in the handle's mask with atomicOr
//   mask_count_kernel        the set bits, by popcount and a wave sum, one integer atomic per wave that has any
// Every result is a set, an integer sum, a minimum or a maximum: two runs give the same bytes whatever order the waves run in.  No float
// atomics, no lane waits for another, and every loop has a stated bound.
#include <new>

#include "common.hpp"
#include "explore_walk.hpp"
#include "field_sample.hpp"
#include "mesh_device.hpp"
#include "mesh_handle.hpp"
#include "union_find.hpp"
#include "voxel_grid.hpp"

namespace tsdf {

enum { kWordUnknown = 0, kWordFree = 1, kWordOccupied = 2, kWordFrontiers = 3, kWordClusters = 4, kWordGain = 5, kWordTotal = 6, kExploreWords = 8 };

constexpr uint64_t kGainMaxRays = (uint64_t)0x7fffffff * 256;   // what a launch of 256-lane workgroups holds

// A wave walks kFlagChunks consecutive chunks and adds its counts up in registers, the four waves of a workgroup add theirs up in LDS
// (integer atomics), and the four counters see one atomic per workgroup and 16 384 voxels.  With one per chunk, two million waves queue
// on the same four words at 512^3 and the kernel takes 31 ms; with one per wave and 32 chunks, 1.5 ms, still twice esdf_sites_kernel.
constexpr uint32_t kFlagChunks = 64;

__global__ __launch_bounds__(256) void frontier_flag_kernel(const float *__restrict__ dist, const WeightView wv, const VoxelGrid grid,
                                                            const uint32_t n_chunks, uint64_t *__restrict__ mask, uint32_t *__restrict__ base,
                                                            unsigned long long *__restrict__ words) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t first = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kFlagChunks;
    const size_t xy = (size_t)grid.X * grid.Y;
    __shared__ uint32_t totals[4];   // in the order of kWordUnknown .. kWordFrontiers
    if (threadIdx.x < 4) totals[threadIdx.x] = 0;
    __syncthreads();
    uint32_t n_unknown = 0, n_free = 0, n_occupied = 0, n_frontiers = 0;   // (at most 64 * kFlagChunks each)
    for (uint32_t k = 0; k < kFlagChunks; k++) {   // bounded: kFlagChunks trips
        if (first + k >= n_chunks) break;   // (the whole wave)
        const uint32_t chunk = (uint32_t)(first + k);
        const uint64_t id = (uint64_t)chunk * 64 + lane;
        bool unknown = false, occupied = false, is_free = false, frontier = false;
        if (id < grid.n) {
            uint32_t x, y, z;
            grid.split((uint32_t)id, x, y, z);
            const size_t ip = (size_t)grid.X * y + x;
            unknown = !(weight_at(wv, xy, ip, z) > 0.0f);   // (true for a NaN weight)
            // the distance is read only where the voxel is observed: the mesh's sign test, NaN and both zeros are not negative
            occupied = !unknown && dist[id] < 0.0f;
            is_free = !unknown && !occupied;
            if (is_free) {
                auto unseen = [&](size_t ip2, uint32_t z2) { return !(weight_at(wv, xy, ip2, z2) > 0.0f); };
                frontier = (x > 0 && unseen(ip - 1, z)) || (x + 1 < grid.X && unseen(ip + 1, z)) || (y > 0 && unseen(ip - grid.X, z)) ||
                           (y + 1 < grid.Y && unseen(ip + grid.X, z)) || (z > 0 && unseen(ip, z - 1)) || (z + 1 < grid.Z && unseen(ip, z + 1));
            }
        }
        store_keep_mask(frontier, lane, chunk, mask, base);
        n_unknown += (uint32_t)__popcll(__ballot(unknown));
        n_free += (uint32_t)__popcll(__ballot(is_free));
        n_occupied += (uint32_t)__popcll(__ballot(occupied));
        n_frontiers += (uint32_t)__popcll(__ballot(frontier));
    }
    if (lane == 0) {
        if (n_unknown) atomicAdd(&totals[kWordUnknown], n_unknown);
        if (n_free) atomicAdd(&totals[kWordFree], n_free);
        if (n_occupied) atomicAdd(&totals[kWordOccupied], n_occupied);
        if (n_frontiers) atomicAdd(&totals[kWordFrontiers], n_frontiers);
    }
    __syncthreads();   // (every lane gets here: the loop is left by break, never by return)
    if (threadIdx.x < 4 && totals[threadIdx.x]) atomicAdd(words + threadIdx.x, (unsigned long long)totals[threadIdx.x]);
}

__global__ __launch_bounds__(256) void frontier_list_kernel(const uint32_t n_chunks, const uint64_t *__restrict__ mask,
                                                            const uint32_t *__restrict__ base, uint32_t *__restrict__ list) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    if (!((mask[chunk] >> lane) & 1u)) return;   // (no bit beyond the grid is ever set)
    const uint32_t id = chunk * 64 + lane;
    list[compact_index(mask, base, id)] = id;
}

// what a root's row holds before the first voxel reaches it
__device__ inline void empty_row(tsdf_frontier_cluster &r, uint32_t label) {
    r.label = label;
    r.size = 0;
    for (int k = 0; k < 3; k++) {
        r.lo[k] = 0xffffffffu;
        r.hi[k] = 0;
        r.sum[k] = 0;
    }
}

__global__ __launch_bounds__(256) void frontier_init_kernel(const uint32_t n_list, uint32_t *__restrict__ parent, tsdf_frontier_cluster *__restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_list) return;
    parent[i] = (uint32_t)i;
    empty_row(acc[i], (uint32_t)i);
}

// A lane per listed voxel: its forward neighbours -- the offsets (dx, dy, dz) that come after (0, 0, 0) in the order z, then y, then x,
// 3 of them at connectivity 6 and 13 at 26 -- that lie inside the grid and are listed are united with it.  Every pair of neighbours is
// forward from one of its two ends, so all of them are seen.  Bounded: 13 trips, and the bounds of components_unite.
__global__ __launch_bounds__(256) void frontier_hook_kernel(const uint32_t n_list, const uint32_t *__restrict__ list, const uint64_t *__restrict__ mask,
                                                            const uint32_t *__restrict__ base, const VoxelGrid grid, const uint32_t connectivity,
                                                            uint32_t *parent) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_list) return;
    const uint32_t id = list[i];
    uint32_t x, y, z;
    grid.split(id, x, y, z);
    for (int k = 14; k < 27; k++) {   // k = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); 13 is the voxel itself
        const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
        if (connectivity == 6u && abs(dx) + abs(dy) + abs(dz) != 1) continue;
        const int64_t nx = (int64_t)x + dx, ny = (int64_t)y + dy, nz = (int64_t)z + dz;
        if (nx < 0 || nx >= (int64_t)grid.X || ny < 0 || ny >= (int64_t)grid.Y || nz >= (int64_t)grid.Z) continue;   // (nz >= 0: dz >= 0)
        const uint32_t id2 = (uint32_t)((nz * grid.Y + ny) * grid.X + nx);
        if (mask_bit(mask, id2)) components_unite(parent, (uint32_t)i, compact_index(mask, base, id2));
    }
}

__global__ __launch_bounds__(256) void frontier_flatten_kernel(const uint32_t n_list, uint32_t *labels, unsigned long long *__restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool is_root = false;
    if (i < n_list) {
        const uint32_t root = components_find<false>(labels, (uint32_t)i);
        is_root = root == (uint32_t)i;
        // (another lane may be walking through i: it reads the old ancestor or the root, both on its way)
        if (!is_root) __hip_atomic_store(labels + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t roots = __ballot(is_root);
    if (roots && (threadIdx.x & 63u) == 0) atomicAdd(words + kWordClusters, (unsigned long long)__popcll(roots));
}

__device__ inline void row_add(tsdf_frontier_cluster *row, uint32_t count, const uint32_t lo[3], const uint32_t hi[3], const uint32_t sum[3]) {
    atomicAdd(&row->size, count);
    for (int k = 0; k < 3; k++) {
        atomicMin(&row->lo[k], lo[k]);
        atomicMax(&row->hi[k], hi[k]);
        atomicAdd((unsigned long long *)&row->sum[k], (unsigned long long)sum[k]);
    }
}

// One set of atomics per wave and root: the wave takes its distinct roots in turn, the lanes of a root reduce among themselves (the
// others hold the neutral values) and the root's first lane adds the result.  Neighbours in the list are neighbours in the grid, so
// most waves have one root or two; adding lane by lane wherever a wave is mixed queued thousands of atomics on the rows of the large
// clusters (5 ms at half a million frontiers).  Bounded: at most 64 trips, every trip retires its leading lane.  (A wave's coordinate
// sum is at most 64 * 65535: it fits 32 bits.)
__global__ __launch_bounds__(256) void frontier_stats_kernel(const uint32_t n_list, const uint32_t *__restrict__ list, const uint32_t *__restrict__ labels,
                                                             const VoxelGrid grid, tsdf_frontier_cluster *__restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n_list;
    const uint32_t label = valid ? labels[i] : 0xffffffffu;
    uint32_t c[3] = {0, 0, 0};
    if (valid) grid.split(list[i], c[0], c[1], c[2]);
    uint64_t remaining = __ballot(valid);
    for (int trip = 0; trip < 64 && remaining; trip++) {
        const int first = __ffsll((unsigned long long)remaining) - 1;
        const uint32_t lead = __shfl(label, first);
        const bool mine = valid && label == lead;
        const uint64_t same = __ballot(mine);
        uint32_t lo[3], hi[3], sum[3];
        for (int k = 0; k < 3; k++) {
            lo[k] = mine ? c[k] : 0xffffffffu;
            hi[k] = mine ? c[k] : 0u;
            sum[k] = mine ? c[k] : 0u;
            for (int o = 32; o > 0; o >>= 1) {
                lo[k] = min(lo[k], (uint32_t)__shfl_xor(lo[k], o));
                hi[k] = max(hi[k], (uint32_t)__shfl_xor(hi[k], o));
                sum[k] += (uint32_t)__shfl_xor(sum[k], o);
            }
        }
        if ((int)(threadIdx.x & 63u) == first) row_add(acc + lead, (uint32_t)__popcll(same), lo, hi, sum);
        remaining &= ~same;
    }
}

__global__ __launch_bounds__(256) void frontier_keep_kernel(const uint32_t n_list, const uint32_t *__restrict__ labels,
                                                            const tsdf_frontier_cluster *__restrict__ acc, const uint32_t min_size, const uint32_t n_chunks,
                                                            uint64_t *__restrict__ row_mask, uint32_t *__restrict__ row_base) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    const uint64_t i = (uint64_t)chunk * 64 + lane;
    store_keep_mask(i < n_list && labels[i] == (uint32_t)i && acc[i].size >= min_size, lane, chunk, row_mask, row_base);
}

__global__ __launch_bounds__(256) void frontier_rows_kernel(const uint32_t n_chunks, const uint64_t *__restrict__ row_mask, const uint32_t *__restrict__ row_base,
                                                            const tsdf_frontier_cluster *__restrict__ acc, tsdf_frontier_cluster *__restrict__ rows) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    if (!((row_mask[chunk] >> lane) & 1u)) return;
    const uint32_t i = chunk * 64 + lane;
    rows[compact_index(row_mask, row_base, i)] = acc[i];
}

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
                                       if (!(weight_at(f.wv, xy, ip, (uint32_t)iz) > 0.0f)) {
                                           const uint32_t id = (uint32_t)(xy * (uint32_t)iz + ip);
                                           atomicOr(gain_mask + (id >> 5), 1u << (id & 31u));   // (a set: order-free)
                                           return (int)kVoxelUnknown;
                                       }
                                       return f.dist[xy * (uint32_t)iz + ip] < 0.0f ? (int)kVoxelOccupied : (int)kVoxelFree;
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

struct tsdf_explorer {
    int device;
    hipEvent_t done;        // recorded behind the last call's launches
    int pending;            // ... and not waited for yet
    int has_geometry;       // a find_frontiers or a view gain has given the handle a geometry
    int found;              // the list, masks and bases are a find_frontiers' of that geometry
    int clustered;          // labels and rows are of that list
    int mask_ready;         // the gain mask is allocated for that geometry and holds only bits that view-gain calls have set
    Geom g;
    uint64_t *masks;        // one frontier mask per 64 voxel ids
    uint32_t *bases;        // ... and the list index of the chunk's first frontier
    uint64_t *parts;        // the chunk scan's sums
    uint32_t *list;         // the frontier voxel ids, ascending
    uint32_t *labels;       // L, one per listed voxel
    tsdf_frontier_cluster *acc;    // one accumulator row per listed voxel; the roots' are filled
    uint64_t *row_masks;    // one keep mask per 64 list indices
    uint32_t *row_bases;
    tsdf_frontier_cluster *rows;   // the table
    uint32_t *gain_mask;    // one bit per voxel
    size_t masks_cap, bases_cap, parts_cap, list_cap, labels_cap, acc_cap, row_masks_cap, row_bases_cap, rows_cap, gain_mask_cap;
    unsigned long long *words;        // kExploreWords device words
    unsigned long long *host_words;   // pinned: where they land
    tsdf_explorer_info info;
};

namespace {

void explorer_free(tsdf_explorer *s) {
    if (s->done) (void)hipEventSynchronize(s->done);
    device_free_all(s->masks, s->bases, s->parts, s->list, s->labels, s->acc, s->row_masks, s->row_bases, s->rows, s->gain_mask, s->words);
    (void)hipHostFree(s->host_words);
    if (s->done) (void)hipEventDestroy(s->done);
    delete s;
}

// the stream waits for what is in flight on the handle / what has just been enqueued is in flight on it / the host waits for it
int explorer_join(tsdf_explorer *s, hipStream_t stream) {
    if (s->pending) TSDF_HIP(hipStreamWaitEvent(stream, s->done, 0), "explorer stream order");
    return TSDF_OK;
}

int explorer_leave(tsdf_explorer *s, hipStream_t stream) {
    TSDF_HIP(hipEventRecord(s->done, stream), "explorer event");
    s->pending = 1;
    return TSDF_OK;
}

int explorer_wait(const tsdf_explorer *cs) {
    tsdf_explorer *s = const_cast<tsdf_explorer *>(cs);
    if (s->pending) {
        TSDF_HIP(hipEventSynchronize(s->done), "explorer wait");
        s->pending = 0;
    }
    return TSDF_OK;
}

bool same_geometry(const Geom &a, const Geom &b) {
    return a.X == b.X && a.Y == b.Y && a.Z == b.Z && a.vs.x == b.vs.x && a.vs.y == b.vs.y && a.vs.z == b.vs.z && a.offset.x == b.offset.x &&
           a.offset.y == b.offset.y && a.offset.z == b.offset.z;
}

void adopt_geometry(tsdf_explorer *s, const Geom &g) {
    if (!s->has_geometry || s->g.X != g.X || s->g.Y != g.Y || s->g.Z != g.Z) s->mask_ready = 0;   // the bits are voxel ids of another grid
    s->g = g;
    s->has_geometry = 1;
    s->info.size[0] = g.X; s->info.size[1] = g.Y; s->info.size[2] = g.Z;
    s->info.voxel_size[0] = g.vs.x; s->info.voxel_size[1] = g.vs.y; s->info.voxel_size[2] = g.vs.z;
    s->info.offset[0] = g.offset.x; s->info.offset[1] = g.offset.y; s->info.offset[2] = g.offset.z;
}

// what every entry point that reads a volume refuses, under its own name
int volume_checked(const char *who, const tsdf_volume *v, const tsdf_explorer *s) {
    TSDF_REQUIRE(v, "%s: null volume", who);
    TSDF_REQUIRE(s, "%s: null explorer handle", who);
    const Geom &g = v->g;
    TSDF_REQUIRE(!v->slab && g.z_store_begin == 0 && g.z_store_end == g.Z,
                 "%s: a Z-slab volume (tsdf_volume_create_slab) is not supported: a voxel's neighbours and a ray's voxels lie in other slabs", who);
    TSDF_REQUIRE(!v->nodes, "%s: the volume has a materialised deformation-node array: voxel centres must be the implicit grid", who);
    TSDF_REQUIRE((uint64_t)g.X * g.Y * g.Z <= 0xffffffffull, "%s: %u x %u x %u voxels do not fit 32-bit voxel ids", who, g.X, g.Y, g.Z);
    TSDF_REQUIRE(v->device == s->device, "%s: the handle was created on device %d, the volume on device %d", who, s->device, v->device);
    return TSDF_OK;
}

// the labels and the table are the list's, and nothing is in flight on them
int clusters_ready(const char *who, const tsdf_explorer *s) {
    TSDF_REQUIRE(s, "%s: null handle", who);
    TSDF_REQUIRE(s->found && s->clustered, "%s: the handle has not been clustered since its last tsdf_volume_find_frontiers (tsdf_explorer_cluster_frontiers)", who);
    return explorer_wait(s);
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
    int rc = explorer_join(s, stream);
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
        TSDF_HIP(hipMemsetAsync(s->words + kWordGain, 0, sizeof(unsigned long long), stream), "view gain count reset");
        hipLaunchKernelGGL(mask_count_kernel, grid_for(n_words, 256), dim3(256), 0, stream, (uint32_t)n_words, s->gain_mask, s->words);
        TSDF_HIP(hipMemcpyAsync(s->host_words + kWordGain, s->words + kWordGain, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream), "view gain count download");
    }
    TSDF_HIP(hipGetLastError(), "view gain kernels failed");
    rc = explorer_leave(s, stream);
    if (rc != TSDF_OK) return rc;
    if (host_gain) {
        TSDF_HIP(hipStreamSynchronize(stream), "view gain count");
        s->pending = 0;
        *host_gain = s->host_words[kWordGain];
    }
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_explorer_create(tsdf_explorer **out) {
    TSDF_REQUIRE(out, "tsdf_explorer_create: null argument");
    *out = nullptr;
    tsdf_explorer *s = new (std::nothrow) tsdf_explorer();
    if (!s) {
        set_error("out of host memory");
        return TSDF_ERR_NOMEM;
    }
    std::memset(s, 0, sizeof(*s));
    hipError_t e = hipGetDevice(&s->device);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void **)&s->words, kExploreWords * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->host_words, kExploreWords * sizeof(unsigned long long), hipHostMallocDefault);
    if (e != hipSuccess) {
        explorer_free(s);
        return hip_fail(e, "explorer alloc failed");
    }
    std::memset(s->host_words, 0, kExploreWords * sizeof(unsigned long long));
    *out = s;
    return TSDF_OK;
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
    int rc = explorer_join(s, stream);
    if (rc != TSDF_OK) return rc;
    s->found = s->clustered = 0;
    const VoxelGrid grid = voxel_grid(v->g);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)grid.n + 63) / 64), n_parts = mesh_scan_parts(n_chunks);
    hipError_t e = device_reserve(s->masks, s->masks_cap, (size_t)n_chunks);
    if (e == hipSuccess) e = device_reserve(s->bases, s->bases_cap, (size_t)n_chunks);
    if (e == hipSuccess) e = device_reserve(s->parts, s->parts_cap, 2 * ((size_t)n_parts + 1));
    if (e != hipSuccess) return hip_fail(e, "frontier scratch alloc failed");
    adopt_geometry(s, v->g);
    s->info.connectivity = 0;
    s->info.n_unknown = s->info.n_free = s->info.n_occupied = s->info.n_frontiers = s->info.n_clusters = s->info.n_listed_clusters = 0;

    const WeightView wv = {v->weight, v->wpacked, v->wmode};
    const dim3 chunk_grid((n_chunks + 3) / 4), flag_grid((n_chunks + 4 * kFlagChunks - 1) / (4 * kFlagChunks));
    TSDF_HIP(hipMemsetAsync(s->words, 0, kExploreWords * sizeof(unsigned long long), stream), "frontier counts reset");
    hipLaunchKernelGGL(frontier_flag_kernel, flag_grid, dim3(256), 0, stream, v->dist, wv, grid, n_chunks, s->masks, s->bases, s->words);
    mesh_scan(ArrayCounts{s->bases, n_chunks, nullptr, 0}, n_parts, s->parts, stream);
    TSDF_HIP(hipGetLastError(), "frontier count kernels failed");
    TSDF_HIP(hipMemcpyAsync(s->host_words, s->words, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream), "frontier counts download");
    TSDF_HIP(hipMemcpyAsync(s->host_words + kWordTotal, s->parts + 2 * (size_t)n_parts, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "frontier counts download");
    TSDF_HIP(hipStreamSynchronize(stream), "frontier count");   // the list is sized from the count
    s->pending = 0;
    const uint64_t n_list = s->host_words[kWordTotal];
    s->info.n_unknown = s->host_words[kWordUnknown];
    s->info.n_free = s->host_words[kWordFree];
    s->info.n_occupied = s->host_words[kWordOccupied];
    s->info.n_frontiers = s->host_words[kWordFrontiers];
    if (n_list != s->info.n_frontiers) {
        set_error("tsdf_volume_find_frontiers: the scan's total (%llu) is not the counted frontiers (%llu)", (unsigned long long)n_list,
                  (unsigned long long)s->info.n_frontiers);
        return TSDF_ERR_DEVICE;
    }
    if (n_list) {
        e = device_reserve(s->list, s->list_cap, (size_t)n_list);
        if (e != hipSuccess) return hip_fail(e, "frontier list alloc failed");
        hipLaunchKernelGGL(frontier_list_kernel, chunk_grid, dim3(256), 0, stream, n_chunks, s->masks, s->bases, s->list);
        TSDF_HIP(hipGetLastError(), "frontier list kernel failed");
        rc = explorer_leave(s, stream);
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
    const int rc = explorer_wait(s);
    if (rc != TSDF_OK) return rc;
    if (device_voxels) *device_voxels = s->info.n_frontiers ? s->list : nullptr;
    if (device_masks) *device_masks = s->masks;
    if (device_bases) *device_bases = s->bases;
    return TSDF_OK;
}

int tsdf_explorer_frontier_download(const tsdf_explorer *s, uint32_t *host_voxels) {
    TSDF_REQUIRE(s && host_voxels, "tsdf_explorer_frontier_download: null argument");
    TSDF_REQUIRE(s->found, "tsdf_explorer_frontier_download: the handle holds no frontiers (tsdf_volume_find_frontiers)");
    const int rc = explorer_wait(s);
    if (rc != TSDF_OK) return rc;
    if (s->info.n_frontiers) TSDF_HIP(hipMemcpy(host_voxels, s->list, (size_t)s->info.n_frontiers * sizeof(uint32_t), hipMemcpyDeviceToHost), "frontier download");
    return TSDF_OK;
}

int tsdf_explorer_scratch_bytes(const tsdf_explorer *s, uint64_t *bytes) {
    TSDF_REQUIRE(s && bytes, "tsdf_explorer_scratch_bytes: null argument");
    *bytes = (uint64_t)s->masks_cap * sizeof(uint64_t) + (uint64_t)s->bases_cap * sizeof(uint32_t) + (uint64_t)s->parts_cap * sizeof(uint64_t) +
             (uint64_t)s->acc_cap * sizeof(tsdf_frontier_cluster) + (uint64_t)s->row_masks_cap * sizeof(uint64_t) +
             (uint64_t)s->row_bases_cap * sizeof(uint32_t) + (uint64_t)s->gain_mask_cap * sizeof(uint32_t) + kExploreWords * sizeof(unsigned long long);
    return TSDF_OK;
}

int tsdf_explorer_cluster_frontiers(tsdf_explorer *s, uint32_t connectivity, uint32_t min_size, void *hip_stream) {
    TSDF_REQUIRE(s, "tsdf_explorer_cluster_frontiers: null handle");
    TSDF_REQUIRE(connectivity == 6u || connectivity == 26u, "tsdf_explorer_cluster_frontiers: connectivity must be 6 or 26, got %u", connectivity);
    TSDF_REQUIRE(s->found, "tsdf_explorer_cluster_frontiers: the handle holds no frontiers (tsdf_volume_find_frontiers)");
    hipStream_t stream = (hipStream_t)hip_stream;
    int rc = explorer_join(s, stream);
    if (rc != TSDF_OK) return rc;
    s->clustered = 0;
    s->info.connectivity = connectivity;
    s->info.n_clusters = s->info.n_listed_clusters = 0;
    const uint64_t n64 = s->info.n_frontiers;
    if (n64 == 0) {
        s->clustered = 1;
        return TSDF_OK;
    }
    const uint32_t n_list = (uint32_t)n64, n_chunks = (uint32_t)((n64 + 63) / 64), n_parts = mesh_scan_parts(n_chunks);
    hipError_t e = device_reserve(s->labels, s->labels_cap, (size_t)n_list);
    if (e == hipSuccess) e = device_reserve(s->acc, s->acc_cap, (size_t)n_list);
    if (e == hipSuccess) e = device_reserve(s->row_masks, s->row_masks_cap, (size_t)n_chunks);
    if (e == hipSuccess) e = device_reserve(s->row_bases, s->row_bases_cap, (size_t)n_chunks);
    if (e == hipSuccess) e = device_reserve(s->parts, s->parts_cap, 2 * ((size_t)n_parts + 1));
    if (e != hipSuccess) return hip_fail(e, "frontier cluster alloc failed");
    const VoxelGrid grid = voxel_grid(s->g);
    const dim3 lanes = grid_for(n_list, 256), chunk_grid((n_chunks + 3) / 4);
    TSDF_HIP(hipMemsetAsync(s->words + kWordClusters, 0, sizeof(unsigned long long), stream), "frontier cluster count reset");
    hipLaunchKernelGGL(frontier_init_kernel, lanes, dim3(256), 0, stream, n_list, s->labels, s->acc);
    hipLaunchKernelGGL(frontier_hook_kernel, lanes, dim3(256), 0, stream, n_list, s->list, s->masks, s->bases, grid, connectivity, s->labels);
    hipLaunchKernelGGL(frontier_flatten_kernel, lanes, dim3(256), 0, stream, n_list, s->labels, s->words);
    hipLaunchKernelGGL(frontier_stats_kernel, lanes, dim3(256), 0, stream, n_list, s->list, s->labels, grid, s->acc);
    hipLaunchKernelGGL(frontier_keep_kernel, chunk_grid, dim3(256), 0, stream, n_list, s->labels, s->acc, min_size, n_chunks, s->row_masks, s->row_bases);
    mesh_scan(ArrayCounts{s->row_bases, n_chunks, nullptr, 0}, n_parts, s->parts, stream);
    TSDF_HIP(hipGetLastError(), "frontier cluster kernels failed");
    TSDF_HIP(hipMemcpyAsync(s->host_words + kWordClusters, s->words + kWordClusters, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream), "frontier cluster counts download");
    TSDF_HIP(hipMemcpyAsync(s->host_words + kWordTotal, s->parts + 2 * (size_t)n_parts, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "frontier cluster counts download");
    TSDF_HIP(hipStreamSynchronize(stream), "frontier cluster count");   // the table is sized from the count
    s->pending = 0;
    const uint64_t n_rows = s->host_words[kWordTotal];
    if (n_rows) {
        e = device_reserve(s->rows, s->rows_cap, (size_t)n_rows);
        if (e != hipSuccess) return hip_fail(e, "frontier cluster table alloc failed");
        hipLaunchKernelGGL(frontier_rows_kernel, chunk_grid, dim3(256), 0, stream, n_chunks, s->row_masks, s->row_bases, s->acc, s->rows);
        TSDF_HIP(hipGetLastError(), "frontier rows kernel failed");
        rc = explorer_leave(s, stream);
        if (rc != TSDF_OK) return rc;
    }
    s->info.n_clusters = s->host_words[kWordClusters];
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
