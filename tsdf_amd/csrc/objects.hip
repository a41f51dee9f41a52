// Class objects for gfx950 (include/tsdf_amd.h, "class objects"): the connected pieces of each fused class, their table,
// and the object a world point lies in.  No reference counterpart.  Only the class words are read; nothing of the volume is written.
//
// List: LabelledFlag, the vote and selection test on one coalesced dword per voxel, one counter.  The flag walk, the list and the
// objects are voxel_set.hpp's, with the policy "a listed neighbour of the same class is adjacent".
// Lookup: a lane per point.
//   objects_lookup_kernel   the sampler's voxel (point_voxel_at, voxel_grid.hpp) -> its list index -> its label -> the label's row, or NONE
// Every result is a set, an integer sum, a minimum or a maximum: two runs give the same bytes whatever order the waves run in.  No float
// atomics, no lane waits for another, and every loop has a stated bound.
#include <algorithm>

#include "common.hpp"
#include "voxel_set.hpp"

namespace tsdf {

static_assert(sizeof(tsdf_class_object) == 72 && sizeof(tsdf_objects_info) == 72, "the layouts include/tsdf_amd.h gives");

// the handle's counter words: the flag kernel's one, then the set's two (roots, scan total: voxel_set.hpp)
enum { kObjWordLabelled = 0 };
using LabelledSet = VoxelSet<tsdf_class_object, 1, 4>;

constexpr uint64_t kLookupMaxPoints = (uint64_t)0x7fffffff * 256;   // what a launch of 256-lane workgroups holds

// One coalesced dword per voxel: labelled = enough votes, and of a selected class.  select: the device copy of the caller's selection
// (n_select bytes), or null = every class.  min_votes >= 1.  One counter; the labelled voxels are listed.
struct LabelledFlag {
    static constexpr uint32_t kCounts = 1, kListed = kObjWordLabelled;
    const uint32_t *cls;
    uint32_t min_votes;
    const uint8_t *select;
    uint32_t n_select;
    __device__ uint32_t operator()(uint32_t id, const VoxelGrid &) const {
        const uint32_t w = cls[id];
        const uint32_t c = w & 0xFFFFu;
        bool labelled = (w >> 16) >= min_votes;
        // the selection byte is read only for a voxel with the votes (c < n_select before c is an address)
        if (labelled && select) labelled = c < n_select && select[c] != 0;
        return labelled ? 1u : 0u;
    }
};

// what a lookup reads of the handle; labels, row_mask and row_base are touched only behind a set mask bit, that is with a list
struct ObjectsView {
    Geom g;   // of the last tsdf_volume_find_objects: every plane resident, so point_voxel_at's place is the voxel id
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
    if (point_voxel_at(o.g, points + 3 * i, at) && mask_bit(o.mask, (uint32_t)at)) {
        const uint32_t label = o.labels[compact_index(o.mask, o.base, (uint32_t)at)];
        if (mask_bit(o.row_mask, label)) row = compact_index(o.row_mask, o.row_base, label);
    }
    rows[i] = row;
}

}  // namespace tsdf

using namespace tsdf;

struct tsdf_objects : LabelledSet {
    int found;              // the arrays are a tsdf_volume_find_objects' of the geometry g
    uint8_t *select;        // the device copy of the caller's selection
    size_t select_cap;
    uint8_t *host_select;   // pinned, 65535 bytes: where the selection is staged for its upload
    tsdf_objects_info info;
};

namespace {

constexpr uint32_t kMaxSelect = 65535;

constexpr VoxelSetText kObjectsText = {
    "objects stream order", "objects event", "objects wait",
    "objects scratch alloc failed", "objects counts reset", "objects count kernels failed", "objects counts download", "objects count", "objects list alloc failed",
    "objects list alloc failed", "objects label kernels failed", "objects counts download", "objects table count", "objects table alloc failed", "objects rows kernel failed"};

void objects_free(tsdf_objects *s) {
    s->release();
    (void)hipFree(s->select);
    (void)hipHostFree(s->host_select);
    delete s;
}

// the arrays are a find's, and nothing is in flight on them
int objects_ready(const char *who, const tsdf_objects *s) {
    TSDF_REQUIRE(s, "%s: null handle", who);
    TSDF_REQUIRE(s->found, "%s: the handle holds no objects (tsdf_volume_find_objects)", who);
    return s->wait();
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
    int rc = s->join(stream);
    if (rc != TSDF_OK) return rc;
    const ObjectsView o = {s->g, s->masks, s->bases, s->labels, s->row_masks, s->row_bases};
    hipLaunchKernelGGL(objects_lookup_kernel, grid_for(n, 256), dim3(256), 0, stream, o, n, points, rows);
    TSDF_HIP(hipGetLastError(), "objects lookup kernel failed");
    return s->leave(stream);   // the handle's arrays are read by what has just been enqueued
}

}  // namespace

extern "C" {

int tsdf_objects_create(tsdf_objects **out) {
    return handle_create(out, "tsdf_objects_create", "objects alloc failed", [](tsdf_objects *s) {
        const hipError_t e = s->create(&kObjectsText);
        return e == hipSuccess ? hipHostMalloc((void **)&s->host_select, kMaxSelect, hipHostMallocDefault) : e;
    }, objects_free);
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
    // (classes are refused on a Z-slab volume: every plane is resident; only the class words are read, so the nodes do not matter)
    const int rcv = whole_volume_checked(who, cv, s->device, nullptr, kAcceptsNodes);
    if (rcv != TSDF_OK) return rcv;
    TSDF_REQUIRE(connectivity == 6u || connectivity == 26u, "%s: connectivity must be 6 or 26, got %u", who, connectivity);
    TSDF_REQUIRE(flags == 0, "%s: unknown flags %#x", who, flags);
    TSDF_REQUIRE(host_select || n_select == 0, "%s: null host_select with n_select = %u", who, n_select);
    TSDF_REQUIRE(n_select <= kMaxSelect, "%s: n_select %u is above 65535", who, n_select);
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);
    hipStream_t stream = v->stream;
    int rc = s->join(stream);
    if (rc != TSDF_OK) return rc;
    s->found = 0;
    const VoxelGrid grid = voxel_grid(g);
    if (host_select) {
        const hipError_t e = device_reserve(s->select, s->select_cap, std::max<size_t>(n_select, 1));
        if (e != hipSuccess) return hip_fail(e, "objects scratch alloc failed");
    }
    tsdf_objects_info &info = s->info;
    uint64_t n64 = 0, n_roots = 0, n_rows = 0;
    rc = voxel_set_list(s, who, "labelled voxels", grid, stream, [&](uint32_t n_chunks) -> int {
        s->g = g;
        geometry_into(info, g);
        info.connectivity = connectivity;
        info.min_votes = min_votes;
        info.min_size = min_size;
        info.n_labelled = info.n_objects = info.n_listed_objects = 0;
        // (nothing of an earlier call is in flight from the staging buffer: every call waits for its stream before it returns)
        if (host_select && n_select) {
            std::memcpy(s->host_select, host_select, n_select);
            TSDF_HIP(hipMemcpyAsync(s->select, s->host_select, n_select, hipMemcpyHostToDevice, stream), "objects selection upload");
        }
        voxel_flag(LabelledFlag{v->classes, std::max(min_votes, 1u), host_select ? s->select : nullptr, n_select}, grid, n_chunks, s->masks, s->bases,
                   s->words.dev, stream);
        return TSDF_OK;
    }, &n64);
    if (rc != TSDF_OK) return rc;
    if (n64) {   // (an empty list: one synchronisation, no objects)
        rc = voxel_set_cluster(s, SameClass{v->classes}, (uint32_t)n64, connectivity, min_size, stream, &n_roots, &n_rows);
        if (rc != TSDF_OK) return rc;
    }
    info.n_labelled = n64;
    info.n_objects = n_roots;
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
    *bytes = s->scratch_bytes() + (uint64_t)s->select_cap;
    return TSDF_OK;
}

}  // extern "C"
