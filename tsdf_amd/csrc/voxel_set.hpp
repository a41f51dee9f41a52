// A set of voxels, flagged, listed and clustered: what explore.hip (frontier voxels, any two listed neighbours
// adjacent), objects.hip (voxels with class votes, adjacent when their classes are equal), frame_diff.hip (the NEARER pixels of a
// W x H x 1 grid, adjacent when their depths are close) and reach.hip (traversable voxels: the flag walk and its masks only) share.
// The user gives the test of one voxel and, for a clustered set, a policy; the chain is the same:
//   voxel_flag_kernel     the user's Flag per voxel id; per chunk of 64 ids the ballot mask and, for a set that is listed, its popcount;
//                         the counts over the 64 chunks a wave walks, one integer atomic per counter and workgroup that has any
//   (the chunk scan of mesh_scan.hip turns the popcounts into bases)
//   voxel_list_kernel     list[compact_index(mask, base, id)] = id: ascending, no atomics, one writer per word
// Clusters: the union-find of union_find.hpp over the list indices, a lane per listed voxel.
//   voxel_init_kernel     parent[i] = i, the accumulator rows emptied
//   voxel_hook_kernel     the 3 or 13 forward neighbours that are listed and adjacent by the policy, united with the lane's own index
//   voxel_flatten_kernel  L[i] = root(i) (a launch of its own: the kernel boundary makes every hook visible); roots counted
//   voxel_stats_kernel    size and the policy's three values as minimum, maximum and sum (with votes: their sum too), to the root's row
//                         with integer atomics, one set per wave and root; with votes, the class id stored once, by the root's own lane
//   voxel_keep_kernel     per 64 list indices: the mask of roots with size >= min_size and its popcount (then the chunk scan)
//   voxel_rows_kernel     the kept rows, in ascending label, to where compact_index says
// Every result is a set, an integer sum, a minimum or a maximum: two runs give the same bytes whatever order the waves run in.  No float
// atomics, no lane waits for another, and every loop has a stated bound.
#pragma once

#include <cstring>
#include <type_traits>

#include "common.hpp"
#include "handle_counters.hpp"
#include "mesh_device.hpp"
#include "mesh_handle.hpp"
#include "union_find.hpp"
#include "voxel_grid.hpp"

namespace tsdf {

// ---- the policies of the clustered sets: the row type; what an empty row holds besides its label and a size of 0; the word read once per
// listed voxel and when a listed neighbour is adjacent (asked only behind its set mask bit); the three values of a listed id that are
// reduced to a minimum, a maximum and a sum, and kSummed more that are summed only (the votes); how a wave's result for one root is added
// to the root's row.  values() is also told whether the lane is its root's own: the one writer of a row's class id.  The third policy,
// NearInDepth with the blob row, is frame_diff.hip's. ------------------------------------------------------------------------------------
template <class Row>
__device__ inline void voxel_row_clear(Row &r) {
    for (int k = 0; k < 3; k++) {
        r.lo[k] = 0xffffffffu;
        r.hi[k] = 0;
        r.sum[k] = 0;
    }
}

template <class Row>
__device__ inline void voxel_row_add(Row *row, uint32_t n, const uint32_t *lo, const uint32_t *hi, const uint32_t *sum) {
    atomicAdd(&row->size, n);
    for (int k = 0; k < 3; k++) {
        atomicMin(&row->lo[k], lo[k]);
        atomicMax(&row->hi[k], hi[k]);
        atomicAdd((unsigned long long *)&row->sum[k], (unsigned long long)sum[k]);
    }
}

struct AnyListedNeighbour {
    using Row = tsdf_frontier_cluster;
    static constexpr int kSummed = 0;
    __device__ static void clear(Row &r) { voxel_row_clear(r); }
    __device__ uint32_t word(uint32_t) const { return 0u; }
    __device__ bool adjacent(uint32_t, uint32_t) const { return true; }
    __device__ void values(uint32_t id, const VoxelGrid &grid, bool, Row &, uint32_t (&v)[3], uint32_t *) const { grid.split(id, v[0], v[1], v[2]); }
    __device__ static void add(Row *row, uint32_t n, const uint32_t *lo, const uint32_t *hi, const uint32_t *sum, const uint32_t *) {
        voxel_row_add(row, n, lo, hi, sum);
    }
};

struct SameClass {
    using Row = tsdf_class_object;
    static constexpr int kSummed = 1;
    const uint32_t *cls;   // the volume's class words, {votes, class}
    __device__ static void clear(Row &r) {
        voxel_row_clear(r);
        r.votes = 0;
        r.class_id = 0;
        r.reserved = 0;
    }
    __device__ uint32_t word(uint32_t id) const { return cls[id]; }
    __device__ bool adjacent(uint32_t own_word, uint32_t id2) const { return (cls[id2] & 0xFFFFu) == (own_word & 0xFFFFu); }
    __device__ void values(uint32_t id, const VoxelGrid &grid, bool own_root, Row &own, uint32_t (&v)[3], uint32_t *votes) const {
        grid.split(id, v[0], v[1], v[2]);
        const uint32_t w = cls[id];
        if (own_root) own.class_id = w & 0xFFFFu;
        votes[0] = w >> 16;
    }
    __device__ static void add(Row *row, uint32_t n, const uint32_t *lo, const uint32_t *hi, const uint32_t *sum, const uint32_t *votes) {
        voxel_row_add(row, n, lo, hi, sum);
        atomicAdd((unsigned long long *)&row->votes, (unsigned long long)votes[0]);
    }
};

// ---- the flag walk -----------------------------------------------------------------------------------------------------------------
// A wave walks kFlagChunks consecutive chunks and adds its counts up in registers, the four waves of a workgroup add theirs up in LDS
// (integer atomics), and every counter sees one atomic per workgroup and 16 384 voxels.  With one per chunk, two million waves queue
// on the same four words at 512^3 and the frontier walk takes 31 ms; with one per wave and 32 chunks, 1.5 ms, still twice
// esdf_sites_kernel.
constexpr uint32_t kFlagChunks = 64;

// Flag: a small struct passed by value.  flag(id, grid), for a voxel id below grid.n, returns one bit per counter: bit k counts into
// words[k], k < Flag::kCounts, and bit Flag::kListed is the voxel's bit in mask[chunk].  base: the popcount per chunk for the chunk
// scan, or null for a set that is never listed.  No bit beyond the grid is ever set.
template <class Flag>
__global__ __launch_bounds__(256) void voxel_flag_kernel(const Flag flag, const VoxelGrid grid, const uint32_t n_chunks, uint64_t *__restrict__ mask,
                                                         uint32_t *__restrict__ base, unsigned long long *__restrict__ words) {
    constexpr uint32_t kCounts = Flag::kCounts;
    static_assert(Flag::kListed < kCounts && kCounts <= 32, "a bit per counter, the listed one among them");
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t first = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kFlagChunks;
    __shared__ uint32_t totals[kCounts];
    block_counts_clear(totals);
    uint32_t counts[kCounts] = {};   // (at most 64 * kFlagChunks each)
    for (uint32_t k = 0; k < kFlagChunks; k++) {   // bounded: kFlagChunks trips
        if (first + k >= n_chunks) break;   // (the whole wave)
        const uint32_t chunk = (uint32_t)(first + k);
        const uint64_t id = (uint64_t)chunk * 64 + lane;
        const uint32_t bits = id < grid.n ? flag((uint32_t)id, grid) : 0u;
        const uint64_t listed = __ballot((bits >> Flag::kListed) & 1u);
        if (lane == 0) {
            mask[chunk] = listed;
            if (base) base[chunk] = (uint32_t)__popcll(listed);
        }
#pragma unroll
        for (uint32_t c = 0; c < kCounts; c++) counts[c] += (uint32_t)__popcll(c == Flag::kListed ? listed : __ballot((bits >> c) & 1u));
    }
    block_counts_wave(totals, counts);
    block_counts_flush(totals, words, 0);   // (every lane gets here: the loop is left by break, never by return)
}

// its launch: a workgroup per 4 * kFlagChunks chunks
template <class Flag>
void voxel_flag(const Flag &flag, const VoxelGrid &grid, uint32_t n_chunks, uint64_t *mask, uint32_t *base, unsigned long long *words,
                hipStream_t stream) {
    hipLaunchKernelGGL(voxel_flag_kernel<Flag>, dim3((n_chunks + 4 * kFlagChunks - 1) / (4 * kFlagChunks)), dim3(256), 0, stream, flag, grid, n_chunks,
                       mask, base, words);
}

static __global__ __launch_bounds__(256) void voxel_list_kernel(const uint32_t n_chunks, const uint64_t *__restrict__ mask,
                                                                const uint32_t *__restrict__ base, uint32_t *__restrict__ list) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    if (!((mask[chunk] >> lane) & 1u)) return;   // (no bit beyond the grid is ever set)
    const uint32_t id = chunk * 64 + lane;
    list[compact_index(mask, base, id)] = id;
}

template <class Policy>
__global__ __launch_bounds__(256) void voxel_init_kernel(const uint32_t n_list, uint32_t *__restrict__ parent, typename Policy::Row *__restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_list) return;
    parent[i] = (uint32_t)i;
    // what a root's row holds before the first voxel reaches it
    typename Policy::Row &r = acc[i];
    r.label = (uint32_t)i;
    r.size = 0;
    Policy::clear(r);
}

// A lane per listed voxel: its forward neighbours -- the offsets (dx, dy, dz) that come after (0, 0, 0) in the order z, then y, then x,
// 3 of them at connectivity 6 and 13 at 26 -- that lie inside the grid, are listed and are adjacent by the policy are united with it.
// The policy is asked only where the neighbour's mask bit is set.  Every pair of neighbours is forward from one of its two ends, so
// all of them are seen.  Bounded: 13 trips, and the bounds of components_unite.
template <class Policy>
__global__ __launch_bounds__(256) void voxel_hook_kernel(const uint32_t n_list, const uint32_t *__restrict__ list, const uint64_t *__restrict__ mask,
                                                         const uint32_t *__restrict__ base, const Policy policy, const VoxelGrid grid,
                                                         const uint32_t connectivity, uint32_t *parent) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_list) return;
    const uint32_t id = list[i];
    const uint32_t word = policy.word(id);
    uint32_t x, y, z;
    grid.split(id, x, y, z);
    for (int k = 14; k < 27; k++) {   // k = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); 13 is the voxel itself
        const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
        if (connectivity == 6u && abs(dx) + abs(dy) + abs(dz) != 1) continue;
        const int64_t nx = (int64_t)x + dx, ny = (int64_t)y + dy, nz = (int64_t)z + dz;
        if (nx < 0 || nx >= (int64_t)grid.X || ny < 0 || ny >= (int64_t)grid.Y || nz >= (int64_t)grid.Z) continue;   // (nz >= 0: dz >= 0)
        const uint32_t id2 = (uint32_t)((nz * grid.Y + ny) * grid.X + nx);
        if (mask_bit(mask, id2) && policy.adjacent(word, id2)) components_unite(parent, (uint32_t)i, compact_index(mask, base, id2));
    }
}

static __global__ __launch_bounds__(256) void voxel_flatten_kernel(const uint32_t n_list, uint32_t *labels, unsigned long long *__restrict__ n_roots) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool is_root = false;
    if (i < n_list) {
        const uint32_t root = components_find<false>(labels, (uint32_t)i);
        is_root = root == (uint32_t)i;
        // (another lane may be walking through i: it reads the old ancestor or the root, both on its way)
        if (!is_root) __hip_atomic_store(labels + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t roots = __ballot(is_root);
    if (roots && (threadIdx.x & 63u) == 0) atomicAdd(n_roots, (unsigned long long)__popcll(roots));
}

// One set of atomics per wave and root (wave_reduce_roots, handle_counters.hpp): the wave takes its distinct roots in turn, the lanes of
// a root reduce among themselves and the root's first lane adds the result.  Neighbours in the list are neighbours in the grid, so
// most waves have one root or two; adding lane by lane wherever a wave is mixed queued thousands of atomics on the rows of the large
// clusters (5 ms at half a million frontiers).  (A value is at most 65535 -- a coordinate, a vote count, a depth -- so a wave's sum
// fits 32 bits.)  The class id has one writer, the lane whose list index is the root.
template <class Policy>
__global__ __launch_bounds__(256) void voxel_stats_kernel(const uint32_t n_list, const uint32_t *__restrict__ list, const uint32_t *__restrict__ labels,
                                                          const Policy policy, const VoxelGrid grid, typename Policy::Row *__restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n_list;
    const uint32_t label = valid ? labels[i] : 0xffffffffu;
    uint32_t v[3] = {0, 0, 0}, more[Policy::kSummed ? Policy::kSummed : 1] = {};
    if (valid) policy.values(list[i], grid, label == (uint32_t)i, acc[i], v, more);
    wave_reduce_roots<3, Policy::kSummed>(valid, label, v, more,
                                          [&](uint32_t lead, uint32_t n, const uint32_t *lo, const uint32_t *hi, const uint32_t *sum, const uint32_t *summed) {
                                              Policy::add(acc + lead, n, lo, hi, sum, summed);
                                          });
}

template <class Row>
__global__ __launch_bounds__(256) void voxel_keep_kernel(const uint32_t n_list, const uint32_t *__restrict__ labels, const Row *__restrict__ acc,
                                                         const uint32_t min_size, const uint32_t n_chunks, uint64_t *__restrict__ row_mask,
                                                         uint32_t *__restrict__ row_base) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    const uint64_t i = (uint64_t)chunk * 64 + lane;
    store_keep_mask(i < n_list && labels[i] == (uint32_t)i && acc[i].size >= min_size, lane, chunk, row_mask, row_base);
}

template <class Row>
__global__ __launch_bounds__(256) void voxel_rows_kernel(const uint32_t n_chunks, const uint64_t *__restrict__ row_mask, const uint32_t *__restrict__ row_base,
                                                         const Row *__restrict__ acc, Row *__restrict__ rows) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    if (!((row_mask[chunk] >> lane) & 1u)) return;
    const uint32_t i = chunk * 64 + lane;
    rows[compact_index(row_mask, row_base, i)] = acc[i];
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
// what a user's runtime failures are called, step by step
struct VoxelSetText {
    const char *order, *event, *wait;                                                     // join, leave, wait
    const char *scratch_alloc, *counts_reset, *count_kernels, *counts_download, *count, *list_alloc;   // voxel_set_list
    const char *cluster_alloc, *cluster_kernels, *cluster_download, *cluster_count, *table_alloc, *rows_kernel;   // voxel_set_cluster
};

// What the listed sets' handles (tsdf_explorer, tsdf_objects, tsdf_frame_diff) have in common.  The flag kernel fills the first kFlagWords of the kWords counter words, the set's size last;
// then come the roots and the total of the last chunk scan.  Plain data: a handle is value-initialised to zero, then create()d.
template <class RowType, uint32_t kFlagWords, uint32_t kWords>
struct VoxelSet : HandleOrder {
    using Row = RowType;
    static constexpr uint32_t kCounterWords = kWords, kWordCounted = kFlagWords - 1, kWordRoots = kFlagWords, kWordTotal = kFlagWords + 1;
    static_assert(kWordTotal < kWords, "the counter words hold the flag kernel's, the roots and the scan's total");
    const VoxelSetText *text;
    Geom g;                 // the geometry the arrays belong to
    uint64_t *masks;        // one mask of listed voxels per 64 voxel ids
    uint32_t *bases;        // ... and the list index of the chunk's first listed voxel
    uint64_t *parts;        // the chunk scan's sums
    uint32_t *list;         // the listed voxel ids, ascending
    uint32_t *labels;       // L, one per listed voxel
    Row *acc;               // one accumulator row per listed voxel; the roots' are filled
    uint64_t *row_masks;    // one keep mask per 64 list indices
    uint32_t *row_bases;
    Row *rows;              // the table
    size_t masks_cap, bases_cap, parts_cap, list_cap, labels_cap, acc_cap, row_masks_cap, row_bases_cap, rows_cap;
    CounterBlock<unsigned long long, kWords> words;   // (handle_counters.hpp)

    hipError_t create(const VoxelSetText *names) {
        text = names;
        const hipError_t e = HandleOrder::create();
        return e == hipSuccess ? words.create() : e;
    }

    // waits for what is in flight, then frees everything above (a half-created handle too)
    void release() {
        destroy();
        device_free_all(masks, bases, parts, list, labels, acc, row_masks, row_bases, rows);
        words.release();
    }

    // the handle's stream order (handle_order.hpp), under the user's texts
    int join(hipStream_t stream) const { return HandleOrder::join(stream, text->order); }
    int leave(hipStream_t stream) const { return HandleOrder::leave(stream, text->event); }
    int wait() const { return HandleOrder::wait(text->wait); }

    // the device bytes besides the list, the labels and the table
    uint64_t scratch_bytes() const {
        return (uint64_t)masks_cap * sizeof(uint64_t) + (uint64_t)bases_cap * sizeof(uint32_t) + (uint64_t)parts_cap * sizeof(uint64_t) +
               (uint64_t)acc_cap * sizeof(Row) + (uint64_t)row_masks_cap * sizeof(uint64_t) + (uint64_t)row_bases_cap * sizeof(uint32_t) +
               words.device_bytes();
    }
};

// The list of a grid's voxels that flag(n_chunks) -- the user's voxel_flag launch, behind whatever it has to do once the scratch is
// there -- marks in s->masks and counts in s->bases and s->words: the chunk scan, the one synchronisation (the list is sized from the
// count), the list.  *n_list is also s->words.host[kWordTotal], and the flag kernel's words are in s->words.host.  Joining and leaving are
// the caller's.
template <class Set, class Flag>
int voxel_set_list(Set *s, const char *who, const char *noun, const VoxelGrid &grid, hipStream_t stream, Flag flag, uint64_t *n_list) {
    const VoxelSetText &t = *s->text;
    const uint32_t n_chunks = (uint32_t)(((uint64_t)grid.n + 63) / 64), n_parts = mesh_scan_parts(n_chunks);
    hipError_t e = device_reserve(s->masks, s->masks_cap, (size_t)n_chunks);
    if (e == hipSuccess) e = device_reserve(s->bases, s->bases_cap, (size_t)n_chunks);
    if (e == hipSuccess) e = device_reserve(s->parts, s->parts_cap, 2 * ((size_t)n_parts + 1));   // (a list has no more chunks than its grid)
    if (e != hipSuccess) return hip_fail(e, t.scratch_alloc);
    TSDF_HIP(s->words.reset(stream), t.counts_reset);
    const int rc = flag(n_chunks);
    if (rc != TSDF_OK) return rc;
    mesh_scan(ArrayCounts{s->bases, n_chunks, nullptr, 0}, n_parts, s->parts, stream);
    TSDF_HIP(hipGetLastError(), t.count_kernels);
    TSDF_HIP(s->words.download(s->words.dev, Set::kWordCounted + 1, stream), t.counts_download);
    TSDF_HIP(hipMemcpyAsync(s->words.host + Set::kWordTotal, s->parts + 2 * (size_t)n_parts, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), t.counts_download);
    TSDF_HIP(hipStreamSynchronize(stream), t.count);
    s->pending = 0;
    *n_list = s->words.host[Set::kWordTotal];
    const uint64_t counted = s->words.host[Set::kWordCounted];
    if (*n_list != counted) {
        set_error("%s: the scan's total (%llu) is not the counted %s (%llu)", who, (unsigned long long)*n_list, noun, (unsigned long long)counted);
        return TSDF_ERR_DEVICE;
    }
    if (*n_list) {
        e = device_reserve(s->list, s->list_cap, (size_t)*n_list);
        if (e != hipSuccess) return hip_fail(e, t.list_alloc);
        hipLaunchKernelGGL(voxel_list_kernel, dim3((n_chunks + 3) / 4), dim3(256), 0, stream, n_chunks, s->masks, s->bases, s->list);
    }
    return TSDF_OK;
}

// The list's n_list > 0 voxels, of the grid of s->g, into connected sets: labels, the roots counted behind whatever s->words holds at
// kWordRoots, one synchronisation (the table is sized from the count), and the rows of at least min_size voxels.  Leaves the handle
// with the rows in flight where there are any; joining is the caller's.
template <class Policy, class Set>
int voxel_set_cluster(Set *s, const Policy policy, uint32_t n_list, uint32_t connectivity, uint32_t min_size, hipStream_t stream, uint64_t *n_roots,
                      uint64_t *n_rows) {
    using Row = typename Set::Row;
    static_assert(std::is_same<Row, typename Policy::Row>::value, "the policy's rows are the handle's");
    const VoxelSetText &t = *s->text;
    const uint32_t n_chunks = (uint32_t)(((uint64_t)n_list + 63) / 64), n_parts = mesh_scan_parts(n_chunks);
    hipError_t e = device_reserve(s->labels, s->labels_cap, (size_t)n_list);
    if (e == hipSuccess) e = device_reserve(s->acc, s->acc_cap, (size_t)n_list);
    if (e == hipSuccess) e = device_reserve(s->row_masks, s->row_masks_cap, (size_t)n_chunks);
    if (e == hipSuccess) e = device_reserve(s->row_bases, s->row_bases_cap, (size_t)n_chunks);
    if (e != hipSuccess) return hip_fail(e, t.cluster_alloc);
    const VoxelGrid grid = voxel_grid(s->g);
    const dim3 lanes = grid_for(n_list, 256), chunk_grid((n_chunks + 3) / 4);
    unsigned long long *const roots = s->words.dev + Set::kWordRoots;
    hipLaunchKernelGGL(voxel_init_kernel<Policy>, lanes, dim3(256), 0, stream, n_list, s->labels, s->acc);
    hipLaunchKernelGGL(voxel_hook_kernel<Policy>, lanes, dim3(256), 0, stream, n_list, s->list, s->masks, s->bases, policy, grid, connectivity, s->labels);
    hipLaunchKernelGGL(voxel_flatten_kernel, lanes, dim3(256), 0, stream, n_list, s->labels, roots);
    hipLaunchKernelGGL(voxel_stats_kernel<Policy>, lanes, dim3(256), 0, stream, n_list, s->list, s->labels, policy, grid, s->acc);
    hipLaunchKernelGGL(voxel_keep_kernel<Row>, chunk_grid, dim3(256), 0, stream, n_list, s->labels, s->acc, min_size, n_chunks, s->row_masks, s->row_bases);
    mesh_scan(ArrayCounts{s->row_bases, n_chunks, nullptr, 0}, n_parts, s->parts, stream);
    TSDF_HIP(hipGetLastError(), t.cluster_kernels);
    TSDF_HIP(s->words.download(roots, 1, stream), t.cluster_download);
    TSDF_HIP(hipMemcpyAsync(s->words.host + Set::kWordTotal, s->parts + 2 * (size_t)n_parts, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), t.cluster_download);
    TSDF_HIP(hipStreamSynchronize(stream), t.cluster_count);
    s->pending = 0;
    *n_roots = s->words.host[Set::kWordRoots];
    *n_rows = s->words.host[Set::kWordTotal];
    if (*n_rows) {
        e = device_reserve(s->rows, s->rows_cap, (size_t)*n_rows);
        if (e != hipSuccess) return hip_fail(e, t.table_alloc);
        hipLaunchKernelGGL(voxel_rows_kernel<Row>, chunk_grid, dim3(256), 0, stream, n_chunks, s->row_masks, s->row_bases, s->acc, s->rows);
        TSDF_HIP(hipGetLastError(), t.rows_kernel);
        return s->leave(stream);
    }
    return TSDF_OK;
}

}  // namespace tsdf
