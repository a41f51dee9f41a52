// Class objects for gfx950 (include/tsdf_amd.h, "class objects"): the connected pieces of each fused class, their table,
// and the object a world point lies in.  No reference counterpart.  Only the class words are read; nothing of the volume is written.
// explore.hip is the template: the same chunks, masks, union-find and rows, with adjacency that also asks for equal classes.
//
// List: chunks of 64 consecutive voxel ids, a wave at a time.
//   objects_flag_kernel     one coalesced dword per lane, the vote and selection test; per chunk the ballot mask and its popcount; the
//                           count by popcount over the 64 chunks a wave walks, one integer atomic per workgroup that has any
//   (the chunk scan of mesh_scan.hip turns the popcounts into bases)
//   objects_list_kernel     list[compact_index(mask, base, id)] = id: ascending, no atomics, one writer per word
// Objects: the union-find of union_find.hpp over the list indices, a lane per listed voxel.
//   objects_init_kernel     parent[i] = i, the accumulator rows emptied
//   objects_hook_kernel     the 3 or 13 forward neighbours that are listed AND of the lane's class, united with the lane's own index
//   objects_flatten_kernel  L[i] = root(i) (a launch of its own: the kernel boundary makes every hook visible); roots counted
//   objects_stats_kernel    size, coordinate sums, the box and the votes, to the root's row with integer atomics, one set per wave and
//                           root; the class id stored once, by the root's own lane
//   objects_keep_kernel     per 64 list indices: the mask of roots with size >= min_size and its popcount (then the chunk scan)
//   objects_rows_kernel     the kept rows, in ascending label, to where compact_index says
// Lookup: a lane per point.
//   objects_lookup_kernel   the sampler's voxel (class_voxel.hpp) -> its list index -> its label -> the label's row, or NONE
// Every result is a set, an integer sum, a minimum or a maximum: two runs give the same bytes whatever order the waves run in.  No float
// atomics, no lane waits for another, and every loop has a stated bound.
#include <algorithm>
#include <new>

#include "class_voxel.hpp"
#include "common.hpp"
#include "mesh_device.hpp"
#include "mesh_handle.hpp"
#include "union_find.hpp"
#include "voxel_grid.hpp"

namespace tsdf {

static_assert(sizeof(tsdf_class_object) == 72 && sizeof(tsdf_objects_info) == 72, "the layouts include/tsdf_amd.h gives");

enum { kObjWordLabelled = 0, kObjWordObjects = 1, kObjWordTotal = 2, kObjectWords = 4 };

constexpr uint64_t kLookupMaxPoints = (uint64_t)0x7fffffff * 256;   // what a launch of 256-lane workgroups holds

// As frontier_flag_kernel (explore.hip): a wave walks kObjFlagChunks consecutive chunks and adds its count up in a register, the four
// waves of a workgroup add theirs up in LDS, and the counter sees one atomic per workgroup and 16 384 voxels.
constexpr uint32_t kObjFlagChunks = 64;

// select: the device copy of the caller's selection (n_select bytes), or null = every class.  min_votes >= 1.
__global__ __launch_bounds__(256) void objects_flag_kernel(const uint32_t *__restrict__ cls, const uint32_t n_voxels, const uint32_t n_chunks,
                                                           const uint32_t min_votes, const uint8_t *__restrict__ select, const uint32_t n_select,
                                                           uint64_t *__restrict__ mask, uint32_t *__restrict__ base,
                                                           unsigned long long *__restrict__ words) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t first = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kObjFlagChunks;
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    uint32_t n_labelled = 0;   // (at most 64 * kObjFlagChunks)
    for (uint32_t k = 0; k < kObjFlagChunks; k++) {   // bounded: kObjFlagChunks trips
        if (first + k >= n_chunks) break;   // (the whole wave)
        const uint32_t chunk = (uint32_t)(first + k);
        const uint64_t id = (uint64_t)chunk * 64 + lane;
        bool labelled = false;
        if (id < n_voxels) {
            const uint32_t w = cls[id];
            const uint32_t c = w & 0xFFFFu;
            labelled = (w >> 16) >= min_votes;
            // the selection byte is read only for a voxel with the votes (c < n_select before c is an address)
            if (labelled && select) labelled = c < n_select && select[c] != 0;
        }
        store_keep_mask(labelled, lane, chunk, mask, base);
        n_labelled += (uint32_t)__popcll(__ballot(labelled));
    }
    if (lane == 0 && n_labelled) atomicAdd(&total, n_labelled);
    __syncthreads();   // (every lane gets here: the loop is left by break, never by return)
    if (threadIdx.x == 0 && total) atomicAdd(words + kObjWordLabelled, (unsigned long long)total);
}

__global__ __launch_bounds__(256) void objects_list_kernel(const uint32_t n_chunks, const uint64_t *__restrict__ mask,
                                                           const uint32_t *__restrict__ base, uint32_t *__restrict__ list) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    if (!((mask[chunk] >> lane) & 1u)) return;   // (no bit beyond the grid is ever set)
    const uint32_t id = chunk * 64 + lane;
    list[compact_index(mask, base, id)] = id;
}

__global__ __launch_bounds__(256) void objects_init_kernel(const uint32_t n_list, uint32_t *__restrict__ parent, tsdf_class_object *__restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_list) return;
    parent[i] = (uint32_t)i;
    // what a root's row holds before the first voxel reaches it
    tsdf_class_object &r = acc[i];
    r.label = (uint32_t)i;
    r.size = 0;
    for (int k = 0; k < 3; k++) {
        r.lo[k] = 0xffffffffu;
        r.hi[k] = 0;
        r.sum[k] = 0;
    }
    r.votes = 0;
    r.class_id = 0;
    r.reserved = 0;
}

// A lane per listed voxel: its forward neighbours -- the offsets (dx, dy, dz) that come after (0, 0, 0) in the order z, then y, then x,
// 3 of them at connectivity 6 and 13 at 26 -- that lie inside the grid, are listed and carry the lane's class are united with it.  The
// neighbour's class word is read only where its mask bit is set.  Every pair of neighbours is forward from one of its two ends, so all
// of them are seen.  Bounded: 13 trips, and the bounds of components_unite.
__global__ __launch_bounds__(256) void objects_hook_kernel(const uint32_t n_list, const uint32_t *__restrict__ list, const uint64_t *__restrict__ mask,
                                                           const uint32_t *__restrict__ base, const uint32_t *__restrict__ cls, const VoxelGrid grid,
                                                           const uint32_t connectivity, uint32_t *parent) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_list) return;
    const uint32_t id = list[i];
    const uint32_t c = cls[id] & 0xFFFFu;
    uint32_t x, y, z;
    grid.split(id, x, y, z);
    for (int k = 14; k < 27; k++) {   // k = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); 13 is the voxel itself
        const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
        if (connectivity == 6u && abs(dx) + abs(dy) + abs(dz) != 1) continue;
        const int64_t nx = (int64_t)x + dx, ny = (int64_t)y + dy, nz = (int64_t)z + dz;
        if (nx < 0 || nx >= (int64_t)grid.X || ny < 0 || ny >= (int64_t)grid.Y || nz >= (int64_t)grid.Z) continue;   // (nz >= 0: dz >= 0)
        const uint32_t id2 = (uint32_t)((nz * grid.Y + ny) * grid.X + nx);
        if (mask_bit(mask, id2) && (cls[id2] & 0xFFFFu) == c) components_unite(parent, (uint32_t)i, compact_index(mask, base, id2));
    }
}

__global__ __launch_bounds__(256) void objects_flatten_kernel(const uint32_t n_list, uint32_t *labels, unsigned long long *__restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool is_root = false;
    if (i < n_list) {
        const uint32_t root = components_find<false>(labels, (uint32_t)i);
        is_root = root == (uint32_t)i;
        // (another lane may be walking through i: it reads the old ancestor or the root, both on its way)
        if (!is_root) __hip_atomic_store(labels + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t roots = __ballot(is_root);
    if (roots && (threadIdx.x & 63u) == 0) atomicAdd(words + kObjWordObjects, (unsigned long long)__popcll(roots));
}

// One set of atomics per wave and root, as frontier_stats_kernel (explore.hip): the wave takes its distinct roots in turn, the lanes of
// a root reduce among themselves (the others hold the neutral values) and the root's first lane adds the result.  Bounded: at most 64
// trips, every trip retires its leading lane.  (A wave's coordinate sum is at most 64 * 65535 and so is its vote sum: both fit 32 bits.)
// The class id has one writer, the lane whose list index is the root.
__global__ __launch_bounds__(256) void objects_stats_kernel(const uint32_t n_list, const uint32_t *__restrict__ list, const uint32_t *__restrict__ labels,
                                                            const uint32_t *__restrict__ cls, const VoxelGrid grid, tsdf_class_object *__restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n_list;
    const uint32_t label = valid ? labels[i] : 0xffffffffu;
    uint32_t c[3] = {0, 0, 0}, word = 0;
    if (valid) {
        const uint32_t id = list[i];
        grid.split(id, c[0], c[1], c[2]);
        word = cls[id];
        if (label == (uint32_t)i) acc[i].class_id = word & 0xFFFFu;
    }
    uint64_t remaining = __ballot(valid);
    for (int trip = 0; trip < 64 && remaining; trip++) {
        const int first = __ffsll((unsigned long long)remaining) - 1;
        const uint32_t lead = __shfl(label, first);
        const bool mine = valid && label == lead;
        const uint64_t same = __ballot(mine);
        uint32_t lo[3], hi[3], sum[3], votes = mine ? word >> 16 : 0u;
        for (int k = 0; k < 3; k++) {
            lo[k] = mine ? c[k] : 0xffffffffu;
            hi[k] = mine ? c[k] : 0u;
            sum[k] = mine ? c[k] : 0u;
        }
        for (int o = 32; o > 0; o >>= 1) {
            for (int k = 0; k < 3; k++) {
                lo[k] = min(lo[k], (uint32_t)__shfl_xor(lo[k], o));
                hi[k] = max(hi[k], (uint32_t)__shfl_xor(hi[k], o));
                sum[k] += (uint32_t)__shfl_xor(sum[k], o);
            }
            votes += (uint32_t)__shfl_xor(votes, o);
        }
        if ((int)(threadIdx.x & 63u) == first) {
            tsdf_class_object *row = acc + lead;
            atomicAdd(&row->size, (uint32_t)__popcll(same));
            for (int k = 0; k < 3; k++) {
                atomicMin(&row->lo[k], lo[k]);
                atomicMax(&row->hi[k], hi[k]);
                atomicAdd((unsigned long long *)&row->sum[k], (unsigned long long)sum[k]);
            }
            atomicAdd((unsigned long long *)&row->votes, (unsigned long long)votes);
        }
        remaining &= ~same;
    }
}

__global__ __launch_bounds__(256) void objects_keep_kernel(const uint32_t n_list, const uint32_t *__restrict__ labels,
                                                           const tsdf_class_object *__restrict__ acc, const uint32_t min_size, const uint32_t n_chunks,
                                                           uint64_t *__restrict__ row_mask, uint32_t *__restrict__ row_base) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    const uint64_t i = (uint64_t)chunk * 64 + lane;
    store_keep_mask(i < n_list && labels[i] == (uint32_t)i && acc[i].size >= min_size, lane, chunk, row_mask, row_base);
}

__global__ __launch_bounds__(256) void objects_rows_kernel(const uint32_t n_chunks, const uint64_t *__restrict__ row_mask, const uint32_t *__restrict__ row_base,
                                                           const tsdf_class_object *__restrict__ acc, tsdf_class_object *__restrict__ rows) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    if (!((row_mask[chunk] >> lane) & 1u)) return;
    const uint32_t i = chunk * 64 + lane;
    rows[compact_index(row_mask, row_base, i)] = acc[i];
}

// what a lookup reads of the handle; labels, row_mask and row_base are touched only behind a set mask bit, that is with a list
struct ObjectsView {
    Geom g;   // of the last tsdf_volume_find_objects: every plane resident, so class_voxel_at's place is the voxel id
    const uint64_t *mask;
    const uint32_t *base, *labels;
    const uint64_t *row_mask;
    const uint32_t *row_base;
};

__global__ __launch_bounds__(256) void objects_lookup_kernel(const ObjectsView o, const uint64_t n, const float *__restrict__ points,
                                                             uint32_t *__restrict__ rows) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t row = TSDF_OBJECT_NONE;
    size_t at;
    if (class_voxel_at(o.g, points + 3 * i, at) && mask_bit(o.mask, (uint32_t)at)) {
        const uint32_t label = o.labels[compact_index(o.mask, o.base, (uint32_t)at)];
        if (mask_bit(o.row_mask, label)) row = compact_index(o.row_mask, o.row_base, label);
    }
    rows[i] = row;
}

}  // namespace tsdf

using namespace tsdf;

struct tsdf_objects {
    int device;
    hipEvent_t done;        // recorded behind the last call's launches
    int pending;            // ... and not waited for yet
    int found;              // the arrays are a tsdf_volume_find_objects' of the geometry below
    Geom g;
    uint64_t *masks;        // one mask of labelled voxels per 64 voxel ids
    uint32_t *bases;        // ... and the list index of the chunk's first labelled voxel
    uint64_t *parts;        // the chunk scan's sums
    uint8_t *select;        // the device copy of the caller's selection
    uint32_t *list;         // the labelled voxel ids, ascending
    uint32_t *labels;       // L, one per listed voxel
    tsdf_class_object *acc;    // one accumulator row per listed voxel; the roots' are filled
    uint64_t *row_masks;    // one keep mask per 64 list indices
    uint32_t *row_bases;
    tsdf_class_object *rows;   // the table
    size_t masks_cap, bases_cap, parts_cap, select_cap, list_cap, labels_cap, acc_cap, row_masks_cap, row_bases_cap, rows_cap;
    unsigned long long *words;        // kObjectWords device words
    unsigned long long *host_words;   // pinned: where they land
    uint8_t *host_select;             // pinned, 65535 bytes: where the selection is staged for its upload
    tsdf_objects_info info;
};

namespace {

constexpr uint32_t kMaxSelect = 65535;

void objects_free(tsdf_objects *s) {
    if (s->done) (void)hipEventSynchronize(s->done);
    device_free_all(s->masks, s->bases, s->parts, s->select, s->list, s->labels, s->acc, s->row_masks, s->row_bases, s->rows, s->words);
    (void)hipHostFree(s->host_words);
    (void)hipHostFree(s->host_select);
    if (s->done) (void)hipEventDestroy(s->done);
    delete s;
}

// the stream waits for what is in flight on the handle / what has just been enqueued is in flight on it / the host waits for it
int objects_join(tsdf_objects *s, hipStream_t stream) {
    if (s->pending) TSDF_HIP(hipStreamWaitEvent(stream, s->done, 0), "objects stream order");
    return TSDF_OK;
}

int objects_leave(tsdf_objects *s, hipStream_t stream) {
    TSDF_HIP(hipEventRecord(s->done, stream), "objects event");
    s->pending = 1;
    return TSDF_OK;
}

int objects_wait(const tsdf_objects *cs) {
    tsdf_objects *s = const_cast<tsdf_objects *>(cs);
    if (s->pending) {
        TSDF_HIP(hipEventSynchronize(s->done), "objects wait");
        s->pending = 0;
    }
    return TSDF_OK;
}

// the arrays are a find's, and nothing is in flight on them
int objects_ready(const char *who, const tsdf_objects *s) {
    TSDF_REQUIRE(s, "%s: null handle", who);
    TSDF_REQUIRE(s->found, "%s: the handle holds no objects (tsdf_volume_find_objects)", who);
    return objects_wait(s);
}

int lookup_checked(const char *who, const tsdf_objects *s, uint64_t n, const float *points, const uint32_t *rows) {
    TSDF_REQUIRE(s, "%s: null handle", who);
    TSDF_REQUIRE(s->found, "%s: the handle holds no objects (tsdf_volume_find_objects)", who);
    TSDF_REQUIRE(n == 0 || (points && rows), "%s: null points or rows with n = %llu", who, (unsigned long long)n);
    TSDF_REQUIRE(n <= kLookupMaxPoints, "%s: %llu points are more than a launch holds (%llu)", who, (unsigned long long)n,
                 (unsigned long long)kLookupMaxPoints);
    return TSDF_OK;
}

// the lookup's launch on `stream`, behind the handle's pending work; device arrays, n > 0
int lookup_on(const tsdf_objects *cs, uint64_t n, const float *points, uint32_t *rows, hipStream_t stream) {
    tsdf_objects *s = const_cast<tsdf_objects *>(cs);   // (the event and its flag)
    int rc = objects_join(s, stream);
    if (rc != TSDF_OK) return rc;
    const ObjectsView o = {s->g, s->masks, s->bases, s->labels, s->row_masks, s->row_bases};
    hipLaunchKernelGGL(objects_lookup_kernel, grid_for(n, 256), dim3(256), 0, stream, o, n, points, rows);
    TSDF_HIP(hipGetLastError(), "objects lookup kernel failed");
    return objects_leave(s, stream);   // the handle's arrays are read by what has just been enqueued
}

}  // namespace

extern "C" {

int tsdf_objects_create(tsdf_objects **out) {
    TSDF_REQUIRE(out, "tsdf_objects_create: null argument");
    *out = nullptr;
    tsdf_objects *s = new (std::nothrow) tsdf_objects();
    if (!s) {
        set_error("out of host memory");
        return TSDF_ERR_NOMEM;
    }
    std::memset(s, 0, sizeof(*s));
    hipError_t e = hipGetDevice(&s->device);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void **)&s->words, kObjectWords * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->host_words, kObjectWords * sizeof(unsigned long long), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->host_select, kMaxSelect, hipHostMallocDefault);
    if (e != hipSuccess) {
        objects_free(s);
        return hip_fail(e, "objects alloc failed");
    }
    std::memset(s->host_words, 0, kObjectWords * sizeof(unsigned long long));
    *out = s;
    return TSDF_OK;
}

void tsdf_objects_destroy(tsdf_objects *s) {
    if (s) objects_free(s);
}

int tsdf_volume_find_objects(const tsdf_volume *cv, uint32_t min_votes, const uint8_t *host_select, uint32_t n_select, uint32_t connectivity,
                             uint32_t min_size, uint32_t flags, tsdf_objects *s) {
    const char *who = "tsdf_volume_find_objects";
    TSDF_REQUIRE(cv, "%s: null volume", who);
    TSDF_REQUIRE(s, "%s: null objects handle", who);
    TSDF_REQUIRE(cv->classes, "%s: classes are not enabled on this volume (tsdf_volume_enable_classes)", who);
    const Geom &g = cv->g;
    // (classes are refused on a Z-slab volume: every plane is resident)
    TSDF_REQUIRE(!cv->slab && g.z_store_begin == 0 && g.z_store_end == g.Z, "%s: a Z-slab volume (tsdf_volume_create_slab) is not supported", who);
    TSDF_REQUIRE((uint64_t)g.X * g.Y * g.Z <= 0xffffffffull, "%s: %u x %u x %u voxels do not fit 32-bit voxel ids", who, g.X, g.Y, g.Z);
    TSDF_REQUIRE(connectivity == 6u || connectivity == 26u, "%s: connectivity must be 6 or 26, got %u", who, connectivity);
    TSDF_REQUIRE(flags == 0, "%s: unknown flags %#x", who, flags);
    TSDF_REQUIRE(host_select || n_select == 0, "%s: null host_select with n_select = %u", who, n_select);
    TSDF_REQUIRE(n_select <= kMaxSelect, "%s: n_select %u is above 65535", who, n_select);
    TSDF_REQUIRE(cv->device == s->device, "%s: the handle was created on device %d, the volume on device %d", who, s->device, cv->device);
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);
    hipStream_t stream = v->stream;
    int rc = objects_join(s, stream);
    if (rc != TSDF_OK) return rc;
    s->found = 0;
    const VoxelGrid grid = voxel_grid(g);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)grid.n + 63) / 64), n_parts = mesh_scan_parts(n_chunks);
    hipError_t e = device_reserve(s->masks, s->masks_cap, (size_t)n_chunks);
    if (e == hipSuccess) e = device_reserve(s->bases, s->bases_cap, (size_t)n_chunks);
    if (e == hipSuccess) e = device_reserve(s->parts, s->parts_cap, 2 * ((size_t)n_parts + 1));   // (the list has no more chunks than the grid)
    if (e == hipSuccess && host_select) e = device_reserve(s->select, s->select_cap, std::max<size_t>(n_select, 1));
    if (e != hipSuccess) return hip_fail(e, "objects scratch alloc failed");
    s->g = g;
    tsdf_objects_info &info = s->info;
    info.size[0] = g.X; info.size[1] = g.Y; info.size[2] = g.Z;
    info.voxel_size[0] = g.vs.x; info.voxel_size[1] = g.vs.y; info.voxel_size[2] = g.vs.z;
    info.offset[0] = g.offset.x; info.offset[1] = g.offset.y; info.offset[2] = g.offset.z;
    info.connectivity = connectivity;
    info.min_votes = min_votes;
    info.min_size = min_size;
    info.n_labelled = info.n_objects = info.n_listed_objects = 0;

    // (nothing of an earlier call is in flight from the staging buffer: every call waits for its stream before it returns)
    if (host_select && n_select) {
        std::memcpy(s->host_select, host_select, n_select);
        TSDF_HIP(hipMemcpyAsync(s->select, s->host_select, n_select, hipMemcpyHostToDevice, stream), "objects selection upload");
    }
    const dim3 chunk_grid((n_chunks + 3) / 4), flag_grid((n_chunks + 4 * kObjFlagChunks - 1) / (4 * kObjFlagChunks));
    TSDF_HIP(hipMemsetAsync(s->words, 0, kObjectWords * sizeof(unsigned long long), stream), "objects counts reset");
    hipLaunchKernelGGL(objects_flag_kernel, flag_grid, dim3(256), 0, stream, v->classes, grid.n, n_chunks, std::max(min_votes, 1u),
                       host_select ? s->select : nullptr, n_select, s->masks, s->bases, s->words);
    mesh_scan(ArrayCounts{s->bases, n_chunks, nullptr, 0}, n_parts, s->parts, stream);
    TSDF_HIP(hipGetLastError(), "objects count kernels failed");
    TSDF_HIP(hipMemcpyAsync(s->host_words + kObjWordLabelled, s->words + kObjWordLabelled, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream), "objects counts download");
    TSDF_HIP(hipMemcpyAsync(s->host_words + kObjWordTotal, s->parts + 2 * (size_t)n_parts, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "objects counts download");
    TSDF_HIP(hipStreamSynchronize(stream), "objects count");   // the list is sized from the count
    s->pending = 0;
    const uint64_t n64 = s->host_words[kObjWordTotal];
    if (n64 != s->host_words[kObjWordLabelled]) {
        set_error("%s: the scan's total (%llu) is not the counted labelled voxels (%llu)", who, (unsigned long long)n64,
                  (unsigned long long)s->host_words[kObjWordLabelled]);
        return TSDF_ERR_DEVICE;
    }
    if (n64 == 0) {
        s->found = 1;
        return TSDF_OK;
    }
    const uint32_t n_list = (uint32_t)n64, n_list_chunks = (uint32_t)((n64 + 63) / 64), n_list_parts = mesh_scan_parts(n_list_chunks);
    e = device_reserve(s->list, s->list_cap, (size_t)n_list);
    if (e == hipSuccess) e = device_reserve(s->labels, s->labels_cap, (size_t)n_list);
    if (e == hipSuccess) e = device_reserve(s->acc, s->acc_cap, (size_t)n_list);
    if (e == hipSuccess) e = device_reserve(s->row_masks, s->row_masks_cap, (size_t)n_list_chunks);
    if (e == hipSuccess) e = device_reserve(s->row_bases, s->row_bases_cap, (size_t)n_list_chunks);
    if (e != hipSuccess) return hip_fail(e, "objects list alloc failed");
    const dim3 lanes = grid_for(n_list, 256), list_chunk_grid((n_list_chunks + 3) / 4);
    hipLaunchKernelGGL(objects_list_kernel, chunk_grid, dim3(256), 0, stream, n_chunks, s->masks, s->bases, s->list);
    hipLaunchKernelGGL(objects_init_kernel, lanes, dim3(256), 0, stream, n_list, s->labels, s->acc);
    hipLaunchKernelGGL(objects_hook_kernel, lanes, dim3(256), 0, stream, n_list, s->list, s->masks, s->bases, v->classes, grid, connectivity, s->labels);
    hipLaunchKernelGGL(objects_flatten_kernel, lanes, dim3(256), 0, stream, n_list, s->labels, s->words);
    hipLaunchKernelGGL(objects_stats_kernel, lanes, dim3(256), 0, stream, n_list, s->list, s->labels, v->classes, grid, s->acc);
    hipLaunchKernelGGL(objects_keep_kernel, list_chunk_grid, dim3(256), 0, stream, n_list, s->labels, s->acc, min_size, n_list_chunks, s->row_masks, s->row_bases);
    mesh_scan(ArrayCounts{s->row_bases, n_list_chunks, nullptr, 0}, n_list_parts, s->parts, stream);
    TSDF_HIP(hipGetLastError(), "objects label kernels failed");
    TSDF_HIP(hipMemcpyAsync(s->host_words + kObjWordObjects, s->words + kObjWordObjects, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream), "objects counts download");
    TSDF_HIP(hipMemcpyAsync(s->host_words + kObjWordTotal, s->parts + 2 * (size_t)n_list_parts, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "objects counts download");
    TSDF_HIP(hipStreamSynchronize(stream), "objects table count");   // the table is sized from the count
    const uint64_t n_rows = s->host_words[kObjWordTotal];
    if (n_rows) {
        e = device_reserve(s->rows, s->rows_cap, (size_t)n_rows);
        if (e != hipSuccess) return hip_fail(e, "objects table alloc failed");
        hipLaunchKernelGGL(objects_rows_kernel, list_chunk_grid, dim3(256), 0, stream, n_list_chunks, s->row_masks, s->row_bases, s->acc, s->rows);
        TSDF_HIP(hipGetLastError(), "objects rows kernel failed");
        rc = objects_leave(s, stream);
        if (rc != TSDF_OK) return rc;
    }
    info.n_labelled = n64;
    info.n_objects = s->host_words[kObjWordObjects];
    info.n_listed_objects = n_rows;
    s->found = 1;
    return TSDF_OK;
}

int tsdf_objects_get_info(const tsdf_objects *s, tsdf_objects_info *info) {
    TSDF_REQUIRE(s && info, "tsdf_objects_get_info: null argument");
    *info = s->info;
    return TSDF_OK;
}

int tsdf_objects_buffers(const tsdf_objects *s, const uint32_t **device_voxels, const uint64_t **device_masks, const uint32_t **device_bases,
                         const uint32_t **device_labels, const tsdf_class_object **device_rows) {
    const int rc = objects_ready("tsdf_objects_buffers", s);
    if (rc != TSDF_OK) return rc;
    if (device_voxels) *device_voxels = s->info.n_labelled ? s->list : nullptr;
    if (device_masks) *device_masks = s->masks;
    if (device_bases) *device_bases = s->bases;
    if (device_labels) *device_labels = s->info.n_labelled ? s->labels : nullptr;
    if (device_rows) *device_rows = s->info.n_listed_objects ? s->rows : nullptr;
    return TSDF_OK;
}

int tsdf_objects_download(const tsdf_objects *s, uint32_t *host_voxels, uint32_t *host_labels, tsdf_class_object *host_rows) {
    const int rc = objects_ready("tsdf_objects_download", s);
    if (rc != TSDF_OK) return rc;
    const size_t list_bytes = (size_t)s->info.n_labelled * sizeof(uint32_t);
    if (host_voxels && list_bytes) TSDF_HIP(hipMemcpy(host_voxels, s->list, list_bytes, hipMemcpyDeviceToHost), "objects download");
    if (host_labels && list_bytes) TSDF_HIP(hipMemcpy(host_labels, s->labels, list_bytes, hipMemcpyDeviceToHost), "objects download");
    if (host_rows && s->info.n_listed_objects)
        TSDF_HIP(hipMemcpy(host_rows, s->rows, (size_t)s->info.n_listed_objects * sizeof(tsdf_class_object), hipMemcpyDeviceToHost), "objects download");
    return TSDF_OK;
}

int tsdf_objects_lookup_device(const tsdf_objects *s, uint64_t n, const float *device_points, uint32_t *device_rows, void *hip_stream) {
    const int rc = lookup_checked("tsdf_objects_lookup_device", s, n, device_points, device_rows);
    if (rc != TSDF_OK) return rc;
    if (n == 0) return TSDF_OK;
    return lookup_on(s, n, device_points, device_rows, (hipStream_t)hip_stream);
}

int tsdf_objects_lookup(const tsdf_objects *s, uint64_t n, const float *host_points, uint32_t *host_rows) {
    const int rc0 = lookup_checked("tsdf_objects_lookup", s, n, host_points, host_rows);
    if (rc0 != TSDF_OK) return rc0;
    if (n == 0) return TSDF_OK;
    // one allocation: the points (3n floats), then the rows (n words)
    const size_t fn = (size_t)n;
    HostStage st;
    int rc = st.begin(nullptr, 4 * fn * sizeof(float), "tsdf_objects_lookup: couldn't allocate %zu bytes for the points and rows");
    if (rc != TSDF_OK) return rc;
    float *const points = static_cast<float *>(st.buf);
    uint32_t *const rows = static_cast<uint32_t *>(st.buf) + 3 * fn;
    st.up(points, host_points, 3 * fn * sizeof(float));
    if (st.ok()) rc = lookup_on(s, n, points, rows, nullptr);
    if (rc == TSDF_OK) st.down(host_rows, rows, fn * sizeof(uint32_t));
    return st.finish(rc, "Objects lookup failed");
}

int tsdf_objects_scratch_bytes(const tsdf_objects *s, uint64_t *bytes) {
    TSDF_REQUIRE(s && bytes, "tsdf_objects_scratch_bytes: null argument");
    *bytes = (uint64_t)s->masks_cap * sizeof(uint64_t) + (uint64_t)s->bases_cap * sizeof(uint32_t) + (uint64_t)s->parts_cap * sizeof(uint64_t) +
             (uint64_t)s->select_cap + (uint64_t)s->acc_cap * sizeof(tsdf_class_object) + (uint64_t)s->row_masks_cap * sizeof(uint64_t) +
             (uint64_t)s->row_bases_cap * sizeof(uint32_t) + kObjectWords * sizeof(unsigned long long);
    return TSDF_OK;
}

}  // extern "C"
