// Column maps for gfx950 (include/tsdf_amd.h, "column maps"): every column of voxels along one axis of the grid reduced to
// one 32-byte row of a 2-D map -- counts of the three states, the highest and lowest occupied voxel, the free run above the highest, the
// sub-voxel height of the crossing there and the smallest ESDF value -- and a 2.5-D traversability class per cell from the rows alone.  No
// reference counterpart.  Nothing of the volume or the ESDF is written.
//   columns_walk_kernel      a lane per cell, consecutive lanes along the map's u axis; written on strides (columns_index.hpp), so any axis.
//                            For axes 1 and 2 u is x: every step of the walk reads 64 consecutive words of a row.
//                            (A kernel of its own for axis 0, a wave per column with ballots and popcounts, was slower: DESIGN.md 33.)
//   columns_classify_kernel  a lane per cell: its own row and the tops of its four neighbours
// Every result is an integer, a minimum or one fixed fp32 expression evaluated by one lane: two runs give the same bytes whatever order the
// waves run in.  No float atomics, no lane waits for another, and every loop has a stated bound.
#include <cstring>

#include "common.hpp"
#include "columns_index.hpp"
#include "device_buffer.hpp"
#include "field_sample.hpp"
#include "handle_counters.hpp"
#include "handle_order.hpp"
#include "voxel_grid.hpp"

namespace tsdf {

// the handle's counter words: the projection's four, then the classification's three
enum { kWordUnknown = 0, kWordFree = 1, kWordOccupied = 2, kWordGround = 3, kWordNoGround = 4, kWordTraversable = 5, kWordBlocked = 6, kColumnWords = 8 };

struct ColumnsView {
    const float *dist;
    WeightView wv;
    const float *esdf;   // null: no minimum asked for
    ColumnsShape s;
};

__device__ inline float columns_nan() { return __uint_as_float(0x7fc00000u); }

// the minimum of the values that are not NaN (NaN while there is none)
__device__ inline float columns_min(float m, float e) {
    if (e != e) return m;
    return m != m ? e : fminf(m, e);
}

// rule 4's height from top, whether c_{top+1} exists and is FREE (headroom >= 1), and the two distances
__device__ inline float columns_height(int32_t top, bool free_above, float d0, float d1) {
    if (top < 0) return columns_nan();
    float height = (float)top + 1.0f;
    if (free_above) {
        const float f = d0 / (d0 - d1);
        if (f >= 0.0f && f <= 1.0f) height = ((float)top + 0.5f) + f;
    }
    return height;
}

// +0.0f for a minimum that compares equal to zero, the canonical NaN for none
__device__ inline float columns_min_out(float m) { return m != m ? columns_nan() : m == 0.0f ? 0.0f : m; }

// A lane per cell.  The walk goes in groups of four steps (columns_index.hpp): the weights of a group, then the distances of its observed
// voxels, and its ESDF values, are loaded before the first of them is used -- no load depends on the running state, so a group has up
// to twelve in flight -- and the state machine then runs over registers.  MODE is the weight storage (0: fp32, 8, 16).  A packed weight
// dword holds 4 (8-bit) or 2 (16-bit) consecutive z of an in-plane position: with ZWALK (axis 2) the groups are aligned with the dwords
// and a group loads one dword (8-bit) or two (16-bit), not one per voxel; on the other axes every step has a dword of its own.
template <int MODE, bool ZWALK>
__global__ __launch_bounds__(256) void columns_walk_kernel(const ColumnsView f, tsdf_column *__restrict__ rows, unsigned long long *__restrict__ words) {
    const ColumnsShape &s = f.s;
    const uint64_t cell = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = cell < columns_cells(s);
    uint32_t counts[4] = {0, 0, 0, 0};   // unknown, free, occupied (voxel_state's values), ground
    if (live) {
        const ColumnsWalk w = columns_walk(s, (uint32_t)(cell % s.U), (uint32_t)(cell / s.U));
        const int64_t xy = (int64_t)s.N[0] * s.N[1], last = (int64_t)s.L - 1;
        constexpr uint32_t shift = MODE == 8 ? 2u : 1u;   // z per packed dword, as a shift
        const uint32_t pad = columns_group_pad(s, MODE != 0 && ZWALK), n_groups = columns_groups(s, pad);
        int32_t top = -1, bottom = -1;
        uint32_t headroom = 0;
        bool open = false;      // the free run above top has not ended
        float d0 = 0.0f, d1 = 0.0f, m = columns_nan();
        for (uint32_t k = 0; k < n_groups; k++) {   // bounded: ceil((L + pad) / 4) trips, pad <= 3
            const int64_t first = (int64_t)k * kColumnsGroup - pad;   // (the group's steps: first .. first + 3, those in [0, L) are walked)
            float wt[kColumnsGroup], d[kColumnsGroup], e[kColumnsGroup];
            int64_t at[kColumnsGroup];
            uint32_t zz[kColumnsGroup], word[kColumnsGroup];
            bool valid[kColumnsGroup];
            // (a step outside the band loads the nearest step of the band again and is not used: every address is a voxel of the column)
            auto clamped = [&](int64_t p) { return p < 0 ? (int64_t)0 : p > last ? last : p; };
#pragma unroll
            for (uint32_t j = 0; j < kColumnsGroup; j++) {
                const int64_t p = first + j, pc = clamped(p);
                valid[j] = p == pc;
                const int64_t ip = w.ip0 + pc * w.ip_step, z = w.z0 + pc * w.z_step;
                at[j] = xy * z + ip;
                zz[j] = (uint32_t)z;
                if (MODE == 0) wt[j] = f.wv.f32[at[j]];
                else if (!ZWALK) word[j] = f.wv.packed[xy * (z >> shift) + ip];
            }
            if (MODE != 0 && ZWALK) {
                // the dword of the group's steps inside the band (8-bit), of each pair's (16-bit): by the alignment they share it
                const int64_t za = w.z0 + clamped(first + (MODE == 8 ? 0 : 1)) * w.z_step, zb = w.z0 + clamped(first + 3) * w.z_step;
                const uint32_t wa = f.wv.packed[xy * (za >> shift) + w.ip0];
                const uint32_t wb = MODE == 8 ? wa : f.wv.packed[xy * (zb >> shift) + w.ip0];
                word[0] = word[1] = wa;
                word[2] = word[3] = wb;
            }
#pragma unroll
            for (uint32_t j = 0; j < kColumnsGroup; j++) {
                if (MODE == 8) wt[j] = (float)((word[j] >> (8u * (zz[j] & 3u))) & 0xffu);
                if (MODE == 16) wt[j] = (float)((word[j] >> (16u * (zz[j] & 1u))) & 0xffffu);
                d[j] = valid[j] && wt[j] > 0.0f ? f.dist[at[j]] : 0.0f;   // (a distance is read only where the voxel is observed)
                e[j] = f.esdf ? f.esdf[at[j]] : columns_nan();
            }
#pragma unroll
            for (uint32_t j = 0; j < kColumnsGroup; j++) {
                if (!valid[j]) continue;
                const int32_t p = (int32_t)(first + j);
                const int state = !(wt[j] > 0.0f) ? kVoxelUnknown : d[j] < 0.0f ? kVoxelOccupied : kVoxelFree;
                counts[0] += state == kVoxelUnknown;
                counts[1] += state == kVoxelFree;
                counts[2] += state == kVoxelOccupied;
                if (state == kVoxelOccupied) {
                    top = p;
                    if (bottom < 0) bottom = p;
                    headroom = 0;
                    open = true;
                    d0 = d[j];
                } else if (open) {
                    if (state == kVoxelFree) {
                        if (headroom == 0) d1 = d[j];   // (c_{top+1})
                        headroom++;
                    } else {
                        open = false;
                    }
                }
                m = columns_min(m, e[j]);
            }
        }
        counts[3] = top >= 0;
        tsdf_column r;
        r.n_unknown = counts[0];
        r.n_free = counts[1];
        r.n_occupied = counts[2];
        r.top = top;
        r.bottom = bottom;
        r.headroom = headroom;
        r.height = columns_height(top, headroom >= 1, d0, d1);
        r.min_distance = columns_min_out(m);
        rows[cell] = r;
    }
    block_counts_add(counts, words, kWordUnknown);
}

// Rule 6, a lane per cell: the cell's own top and headroom, and the tops of the four neighbours inside the map.
__global__ __launch_bounds__(256) void columns_classify_kernel(const tsdf_column *__restrict__ rows, const uint32_t U, const uint32_t V, const uint32_t max_step,
                                                               const uint32_t min_headroom, uint8_t *__restrict__ out, unsigned long long *__restrict__ words) {
    const uint64_t cell = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t counts[3] = {0, 0, 0};   // no ground, traversable, blocked: the values of the classes
    if (cell < (uint64_t)U * V) {
        const uint32_t u = (uint32_t)(cell % U), v = (uint32_t)(cell / U);
        const int32_t top = rows[cell].top;
        uint32_t cls = TSDF_CELL_NO_GROUND;
        if (top >= 0) {
            // (both tops lie in [0, 2^31 - 1]: the difference fits an int32)
            auto steps = [&](uint64_t nb) {
                const int32_t t = rows[nb].top;
                return t >= 0 && (uint32_t)abs(top - t) > max_step;
            };
            const bool blocked = rows[cell].headroom < min_headroom || (u > 0 && steps(cell - 1)) || (u + 1 < U && steps(cell + 1)) ||
                                 (v > 0 && steps(cell - U)) || (v + 1 < V && steps(cell + U));
            cls = blocked ? TSDF_CELL_BLOCKED : TSDF_CELL_TRAVERSABLE;
        }
        out[cell] = (uint8_t)cls;
        counts[0] = cls == TSDF_CELL_NO_GROUND;
        counts[1] = cls == TSDF_CELL_TRAVERSABLE;
        counts[2] = cls == TSDF_CELL_BLOCKED;
    }
    block_counts_add(counts, words, kWordNoGround);
}

}  // namespace tsdf

using namespace tsdf;

struct tsdf_columns : HandleOrder {
    int projected;          // the rows are a projection's of the shape s
    ColumnsShape s;
    tsdf_column *rows;      // one per cell
    size_t rows_cap;
    CounterBlock<unsigned long long, kColumnWords> words;   // (handle_counters.hpp)
    tsdf_columns_info info;           // (the totals are filled from words.host by whoever has waited)
};

namespace {

constexpr const char *kColumnsOrder = "columns stream order", *kColumnsEvent = "columns event", *kColumnsWait = "columns wait";

void columns_free(tsdf_columns *s) {
    s->destroy();
    device_free_all(s->rows);
    s->words.release();
    delete s;
}

// the walk of the volume's weight storage; along z over packed counts the one whose groups are the packed dwords
void launch_walk(const ColumnsView &f, uint64_t n_cells, tsdf_column *rows, unsigned long long *words, hipStream_t stream) {
    const dim3 grid((unsigned)((n_cells + 255) / 256)), block(256);
    const bool zwalk = f.s.axis == 2;
    if (f.wv.mode == 0) hipLaunchKernelGGL((columns_walk_kernel<0, false>), grid, block, 0, stream, f, rows, words);
    else if (f.wv.mode == 8 && zwalk) hipLaunchKernelGGL((columns_walk_kernel<8, true>), grid, block, 0, stream, f, rows, words);
    else if (f.wv.mode == 8) hipLaunchKernelGGL((columns_walk_kernel<8, false>), grid, block, 0, stream, f, rows, words);
    else if (zwalk) hipLaunchKernelGGL((columns_walk_kernel<16, true>), grid, block, 0, stream, f, rows, words);
    else hipLaunchKernelGGL((columns_walk_kernel<16, false>), grid, block, 0, stream, f, rows, words);
}

int columns_projected(const char *who, const tsdf_columns *s) {
    TSDF_REQUIRE(s, "%s: null handle", who);
    TSDF_REQUIRE(s->projected, "%s: the handle has never been projected (tsdf_volume_project_columns)", who);
    return TSDF_OK;
}

int classify_checked(const char *who, const tsdf_columns *s, uint32_t flags, const uint8_t *out) {
    const int rc = columns_projected(who, s);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(flags == 0, "%s: unknown flags %#x", who, flags);
    TSDF_REQUIRE(out, "%s: null output", who);
    return TSDF_OK;
}

int classify_on(tsdf_columns *s, uint32_t max_step, uint32_t min_headroom, uint8_t *device_cells, hipStream_t stream) {
    int rc = s->join(stream, kColumnsOrder);
    if (rc != TSDF_OK) return rc;
    s->info.max_step = max_step;
    s->info.min_headroom = min_headroom;
    TSDF_HIP(s->words.reset(s->words.dev + kWordNoGround, 3, stream), "columns classify counts reset");
    hipLaunchKernelGGL(columns_classify_kernel, dim3((unsigned)((columns_cells(s->s) + 255) / 256)), dim3(256), 0, stream, s->rows, s->s.U, s->s.V, max_step,
                       min_headroom, device_cells, s->words.dev);
    TSDF_HIP(hipGetLastError(), "columns classify kernel failed");
    TSDF_HIP(s->words.download(s->words.dev + kWordNoGround, 3, stream), "columns classify counts download");
    return s->leave(stream, kColumnsEvent);
}

}  // namespace

extern "C" {

int tsdf_columns_create(tsdf_columns **out) {
    return handle_create(out, "tsdf_columns_create", "columns alloc failed", [](tsdf_columns *s) {
        const hipError_t e = s->create();
        return e == hipSuccess ? s->words.create() : e;
    }, columns_free);
}

void tsdf_columns_destroy(tsdf_columns *s) {
    if (s) columns_free(s);
}

int tsdf_volume_project_columns(const tsdf_volume *cv, uint32_t axis, uint32_t lo, uint32_t hi, const tsdf_esdf *esdf, uint32_t flags, tsdf_columns *s) {
    const char *who = "tsdf_volume_project_columns";
    TSDF_REQUIRE(cv, "%s: null volume", who);
    TSDF_REQUIRE(s, "%s: null columns handle", who);
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);
    int rc = whole_volume_checked(who, v, s->device, "a column's voxels lie in other slabs");
    if (rc != TSDF_OK) return rc;
    const Geom &g = v->g;
    TSDF_REQUIRE(axis <= 2, "%s: axis must be 0, 1 or 2, got %u", who, axis);
    TSDF_REQUIRE((flags & ~(uint32_t)TSDF_COLUMNS_REVERSED) == 0, "%s: unknown flags %#x", who, flags);
    const uint32_t N[3] = {g.X, g.Y, g.Z};
    ColumnsShape shape;
    TSDF_REQUIRE(columns_shape(N, axis, lo, hi, (flags & TSDF_COLUMNS_REVERSED) != 0, shape),
                 "%s: the band [%u, %u) is empty or leaves axis %u of %u x %u x %u (hi == 0: the axis' end), or the axis is longer than %u voxels", who, lo, hi,
                 axis, g.X, g.Y, g.Z, kColumnsMaxAxis);
    const float *esdf_array = nullptr;
    rc = esdf_array_checked(who, esdf, g, &esdf_array);
    if (rc != TSDF_OK) return rc;
    hipStream_t stream = v->stream;
    rc = s->join(stream, kColumnsOrder);
    if (rc != TSDF_OK) return rc;
    s->projected = 0;
    const uint64_t n_cells = columns_cells(shape);
    const hipError_t e = device_reserve(s->rows, s->rows_cap, (size_t)n_cells);
    if (e != hipSuccess) return hip_fail(e, "columns rows alloc failed");
    s->s = shape;
    std::memset(&s->info, 0, sizeof(s->info));
    geometry_into(s->info, g);
    s->info.axis = axis;
    s->info.lo = shape.lo;
    s->info.hi = shape.hi;
    s->info.flags = flags;
    s->info.has_esdf = esdf ? 1u : 0u;
    s->info.map_size[0] = shape.U;
    s->info.map_size[1] = shape.V;
    s->info.map_axes[0] = shape.au;
    s->info.map_axes[1] = shape.av;

    TSDF_HIP(s->words.reset(stream), "columns counts reset");
    const ColumnsView f = {v->dist, {v->weight, v->wpacked, v->wmode}, esdf_array, shape};
    launch_walk(f, n_cells, s->rows, s->words.dev, stream);
    TSDF_HIP(hipGetLastError(), "columns kernel failed");
    TSDF_HIP(s->words.download(stream), "columns counts download");
    rc = s->leave(stream, kColumnsEvent);
    if (rc != TSDF_OK) return rc;
    s->projected = 1;
    return TSDF_OK;
}

int tsdf_columns_get_info(const tsdf_columns *s, tsdf_columns_info *info) {
    TSDF_REQUIRE(s && info, "tsdf_columns_get_info: null argument");
    const int rc = s->wait(kColumnsWait);
    if (rc != TSDF_OK) return rc;
    *info = s->info;
    if (s->projected) {
        info->n_unknown = s->words.host[kWordUnknown];
        info->n_free = s->words.host[kWordFree];
        info->n_occupied = s->words.host[kWordOccupied];
        info->n_ground = s->words.host[kWordGround];
        info->n_no_ground = s->words.host[kWordNoGround];
        info->n_traversable = s->words.host[kWordTraversable];
        info->n_blocked = s->words.host[kWordBlocked];
    }
    return TSDF_OK;
}

int tsdf_columns_buffer(const tsdf_columns *s, const tsdf_column **device_rows) {
    TSDF_REQUIRE(s && device_rows, "tsdf_columns_buffer: null argument");
    int rc = columns_projected("tsdf_columns_buffer", s);
    if (rc == TSDF_OK) rc = s->wait(kColumnsWait);
    if (rc != TSDF_OK) return rc;
    *device_rows = s->rows;
    return TSDF_OK;
}

int tsdf_columns_download(const tsdf_columns *s, tsdf_column *host_rows) {
    TSDF_REQUIRE(s && host_rows, "tsdf_columns_download: null argument");
    int rc = columns_projected("tsdf_columns_download", s);
    if (rc == TSDF_OK) rc = s->wait(kColumnsWait);
    if (rc != TSDF_OK) return rc;
    TSDF_HIP(hipMemcpy(host_rows, s->rows, (size_t)columns_cells(s->s) * sizeof(tsdf_column), hipMemcpyDeviceToHost), "columns download");
    return TSDF_OK;
}

int tsdf_columns_scratch_bytes(const tsdf_columns *s, uint64_t *bytes) {
    TSDF_REQUIRE(s && bytes, "tsdf_columns_scratch_bytes: null argument");
    *bytes = (uint64_t)s->rows_cap * sizeof(tsdf_column) + s->words.device_bytes();
    return TSDF_OK;
}

int tsdf_columns_classify_device(tsdf_columns *s, uint32_t max_step, uint32_t min_headroom, uint32_t flags, uint8_t *device_cells, void *hip_stream) {
    const int rc = classify_checked("tsdf_columns_classify_device", s, flags, device_cells);
    if (rc != TSDF_OK) return rc;
    return classify_on(s, max_step, min_headroom, device_cells, (hipStream_t)hip_stream);
}

int tsdf_columns_classify(tsdf_columns *s, uint32_t max_step, uint32_t min_headroom, uint32_t flags, uint8_t *host_cells) {
    const int rc0 = classify_checked("tsdf_columns_classify", s, flags, host_cells);
    if (rc0 != TSDF_OK) return rc0;
    const size_t n = (size_t)columns_cells(s->s);
    HostStage st;
    int rc = st.begin(nullptr, n, "tsdf_columns_classify: couldn't allocate %zu bytes for the cells");
    if (rc != TSDF_OK) return rc;
    rc = classify_on(s, max_step, min_headroom, static_cast<uint8_t *>(st.buf), nullptr);
    if (rc == TSDF_OK) st.down(host_cells, st.buf, n);
    rc = st.finish(rc, "Column classification failed");
    if (rc == TSDF_OK) s->pending = 0;   // (the stream has been waited for)
    return rc;
}

}  // extern "C"
