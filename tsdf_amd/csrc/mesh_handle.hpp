// struct tsdf_mesh and the host side of what mesh.hip (extraction), mesh_components.hip (labelling, filtering), mesh_simplify.hip
// (clustering), mesh_smooth.hip (smoothing, face normals) and scene_flow.hip share: the stream order of a handle, the chunk scan's
// interface (mesh_scan.hip), the table's size, the argument checks and the frames of a call into a handle.  The device side is
// mesh_device.hpp.
#pragma once

#include <cstring>

#include "common.hpp"
#include "handle_order.hpp"

namespace tsdf {

struct MeshTable {
    int8_t tri[256][32];   // edge numbers, three per triangle, -1 terminated
    uint8_t count[256];    // vertices per configuration
};

// 32 bytes per 64 voxels of the marched range
struct MeshChunk {
    uint64_t mx, my, mz;   // bit l: the chunk's l-th voxel has a used edge towards +x / +y / +z
    uint32_t vbase;        // mesh_edges_kernel: the chunk's vertices; after the scan: the index of its first vertex
    uint32_t ibase;        // the same for the soup vertices (= indices) of the cubes rooted in the chunk
};

constexpr size_t kComponentWords = 4;   // tsdf_mesh::component_words, and what tsdf_label_components_device holds for a call

// ---- the chunk scan (mesh_scan.hip) ------------------------------------------------------------------------------------------------
// Where a chunk's two counts live, and where its two bases go: the two fields of an extraction's records ...
struct ChunkCounts {
    MeshChunk *chunks;
    uint32_t n_chunks;
    __device__ uint32_t first(uint32_t i) const { return i < n_chunks ? chunks[i].vbase : 0u; }
    __device__ uint32_t second(uint32_t i) const { return i < n_chunks ? chunks[i].ibase : 0u; }
    __device__ void store(uint32_t i, uint32_t a, uint32_t b) const {
        if (i < n_chunks) {
            chunks[i].vbase = a;
            chunks[i].ibase = b;
        }
    }
};

// ... or two arrays of their own lengths (a null second array has length 0)
struct ArrayCounts {
    uint32_t *a;
    uint32_t n_a;
    uint32_t *b;
    uint32_t n_b;
    __device__ uint32_t first(uint32_t i) const { return i < n_a ? a[i] : 0u; }
    __device__ uint32_t second(uint32_t i) const { return i < n_b ? b[i] : 0u; }
    __device__ void store(uint32_t i, uint32_t va, uint32_t vb) const {
        if (i < n_a) a[i] = va;
        if (i < n_b) b[i] = vb;
    }
};

inline uint32_t mesh_scan_parts(uint32_t chunks) { return (chunks + 1023) / 1024; }

// Counts -> bases in place, for the chunks of n_parts workgroups; parts[2 n_parts], [2 n_parts + 1] take the two totals (so parts holds
// at least 2 (n_parts + 1) words).  Three launches on `stream`.
template <typename Counts>
void mesh_scan(const Counts counts, uint32_t n_parts, uint64_t *parts, hipStream_t stream);

inline dim3 grid_for(uint64_t n, uint32_t per_block) { return dim3((uint32_t)((n + per_block - 1) / per_block)); }

// The open-addressed table (table_claim, mesh_device.hpp) for at most n keys: 2^bits slots, the smallest power of two >= 2 n.
inline uint32_t mesh_table_bits(uint64_t n) {
    uint32_t bits = 1;
    while ((1ull << bits) < 2 * n) bits++;
    return bits;
}

}  // namespace tsdf

struct tsdf_mesh : tsdf::HandleOrder {   // (the event: behind the last extraction's, labelling's or filter's launches)
    float *vertices;
    uint32_t *indices;
    float *normals;
    uint8_t *rgb;
    size_t vertices_cap, indices_cap, normals_cap, rgb_cap;   // in elements of the arrays (vertices, indices)
    tsdf::MeshChunk *chunks;
    size_t chunks_cap;
    uint64_t *parts;        // two sums per 1024 chunks + the two totals
    size_t parts_cap;       // in words
    tsdf::MeshTable *table;       // the device copy of host_table (uploaded again only when the caller's table changes)
    tsdf::MeshTable host_table;
    int table_valid;
    uint64_t *totals;       // pinned: where the two totals land
    tsdf_mesh_info info;
    // mesh components (mesh_components.hip): all null until the first components call on / filter into the handle
    uint32_t *labels, *sizes;          // L and T of the arrays above, one word per vertex each
    size_t labels_cap, sizes_cap;
    uint64_t *component_words;         // kComponentWords: error, roots, the largest component's packed word
    int labelled;                      // labels / sizes / components are those of the arrays above
    tsdf_components_info components;
    uint64_t *keep_masks;              // a filter into this handle: one keep mask per 64 vertices, then one per 64 triples, of its source
    uint32_t *keep_bases;              // ... and their counts / bases
    size_t keep_masks_cap, keep_bases_cap;
    // mesh simplification (mesh_simplify.hip): all null until the first simplification INTO the handle; of its source:
    uint64_t *cell_keys;               // the open-addressed table of cell keys, a power of two >= 2 n_vertices words
    uint32_t *cell_reps;               // ... and per slot the smallest vertex index that holds the key
    size_t cell_keys_cap, cell_reps_cap;
    uint32_t *cluster_of;              // per vertex: its slot, then its cluster's representative, then its output index
    size_t cluster_of_cap;
    int64_t *cluster_sums;             // per cluster: the count and the integer sums of positions (normals, colours)
    size_t cluster_sums_cap;           // in words
    // mesh smoothing (mesh_smooth.hip): all null until the first smoothing INTO the handle; of its source (the edge table of the pins is
    // cell_keys and cell_reps above):
    uint32_t *row_begin, *row_end;     // per vertex: where its row of neighbour pairs begins and ends
    size_t row_begin_cap, row_end_cap;
    uint2 *rows;                       // one pair per live triple and corner: the triple's other two corners
    size_t rows_cap;                   // in pairs
    float *smooth_positions;           // the second position buffer the passes alternate with `vertices`
    size_t smooth_positions_cap;       // in floats
    uint8_t *pinned;                   // TSDF_SMOOTH_PIN_BOUNDARY: per vertex, 1 at an end of an edge that one live triple names
    size_t pinned_cap;
    int64_t *normal_sums;              // face normals (also tsdf_mesh_compute_normals ON the handle): three integer sums per vertex
    size_t normal_sums_cap;            // in words
    // scene flow (scene_flow.hip): grid is kept by every extraction; the arrays are null until the first scene-flow call with the handle
    uint32_t grid[3];                  // the arrays and chunk records are an extraction of the WHOLE grid of a volume of these sizes
                                       // (all zero: a box, or the output of a filter or a simplification)
    uint2 *flow_vertex;                // per vertex: {its pixel index or 0xffffffff, the soup vertices on its edge}
    size_t flow_vertex_cap;
    float *flow_points;                // TSDF_SCENE_FLOW_DEFORMED: the vertices pushed through the deformation field
    size_t flow_points_cap;            // in floats
    uint64_t *flow_counts;             // correspondences, nodes moved
    uint64_t *flow_totals;             // pinned: where the two land
    uint16_t *flow_depth;              // the host variant's uploads of the depth and scene-flow images
    float *flow_image;
    size_t flow_depth_cap, flow_image_cap;   // in pixels, in floats
};

namespace tsdf {

// ---- the stream order of a handle (handle_order.hpp), under the mesh's texts ---------------------------------------------------------
inline int mesh_join(const tsdf_mesh *m, hipStream_t stream) { return m->join(stream, "mesh stream order"); }
inline int mesh_leave(const tsdf_mesh *m, hipStream_t stream) { return m->leave(stream, "mesh event"); }
inline int mesh_wait(const tsdf_mesh *m) { return m->wait("mesh wait"); }

// ---- argument checks ---------------------------------------------------------------------------------------------------------------
// (labelling, which takes no vertex array, starts here)
inline int indices_checked(const char *who, uint64_t n_vertices, uint64_t n_indices, const uint32_t *indices) {
    TSDF_REQUIRE(indices || n_indices == 0, "%s: null device_indices with n_indices = %llu", who, (unsigned long long)n_indices);
    TSDF_REQUIRE(n_indices % 3 == 0, "%s: n_indices (%llu) is not a multiple of 3", who, (unsigned long long)n_indices);
    TSDF_REQUIRE(n_vertices <= 0xffffffffull && n_indices <= 0xffffffffull, "%s: %llu vertices and %llu indices do not fit 32-bit indices", who,
                 (unsigned long long)n_vertices, (unsigned long long)n_indices);
    return TSDF_OK;
}

inline int arrays_checked(const char *who, uint64_t n_vertices, uint64_t n_indices, const float *vertices, const uint32_t *indices) {
    TSDF_REQUIRE(vertices || n_vertices == 0, "%s: null device_vertices with n_vertices = %llu", who, (unsigned long long)n_vertices);
    return indices_checked(who, n_vertices, n_indices, indices);
}

// The refusal of an index: with no vertex at all (any index is one too many) on the host, otherwise from the error word the
// kernels raised (kErrorIndex, mesh_device.hpp).
inline int index_refused(const char *who, uint64_t n_vertices) {
    set_error("%s: an index is not below n_vertices (%u)", who, (uint32_t)n_vertices);
    return TSDF_ERR_INVALID;
}

// Download `n_words` device words that hold a call's error word at [error_at], synchronise (the call's one synchronisation), and refuse
// a bad index.  What other values of the word mean is the caller's.
inline int error_word_checked(const char *who, uint64_t n_vertices, const uint64_t *device_words, uint64_t *host_words, size_t n_words, size_t error_at,
                              hipStream_t stream) {
    TSDF_HIP(hipMemcpyAsync(host_words, device_words, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "mesh error word download");
    TSDF_HIP(hipStreamSynchronize(stream), "mesh error word");
    return host_words[error_at] == 1 ? index_refused(who, n_vertices) : TSDF_OK;
}

// ---- the frames of a call into a handle --------------------------------------------------------------------------------------------
// dst is about to be overwritten: an empty mesh that is no extraction's and carries no labels
inline void mesh_reset(tsdf_mesh *dst) {
    dst->labelled = 0;
    dst->grid[0] = dst->grid[1] = dst->grid[2] = 0;   // (scene_flow.hip: not an extraction's arrays and records any more)
    std::memset(&dst->info, 0, sizeof(dst->info));
}

// run() -- everything between the argument checks and the counts in dst->info, for n_vertices > 0 -- with dst's stream order round it.
// A failure leaves dst empty.
template <typename Run>
int mesh_into(const char *who, uint64_t n_vertices, uint64_t n_indices, uint32_t info_flags, tsdf_mesh *dst, hipStream_t stream, Run run) {
    int rc = mesh_join(dst, stream);
    if (rc != TSDF_OK) return rc;
    mesh_reset(dst);
    dst->info.flags = info_flags;
    if (n_vertices == 0) return n_indices ? index_refused(who, 0) : TSDF_OK;
    rc = run();
    const int rc2 = mesh_leave(dst, stream);
    if (rc != TSDF_OK) {
        dst->info.n_vertices = dst->info.n_indices = 0;
        return rc;
    }
    return rc2;
}

// run(n_vertices, n_indices, vertices, indices, normals, rgb) on src's arrays (null where src has none), which is a call into dst in
// the sense of mesh_into, with src's stream order round it; dst then takes src's flags, `more_flags` and box.  `verb` names the
// operation in the refusals.
template <typename Run>
int mesh_from_handle(const char *who, const char *verb, tsdf_mesh *src, tsdf_mesh *dst, uint32_t more_flags, hipStream_t stream, Run run) {
    TSDF_REQUIRE(src, "%s: null src", who);
    TSDF_REQUIRE(dst, "%s: null dst", who);
    TSDF_REQUIRE(src != dst, "%s: dst is src (%s into another handle)", who, verb);
    TSDF_REQUIRE(src->device == dst->device, "%s: src was created on device %d, dst on device %d", who, src->device, dst->device);
    int rc = mesh_join(src, stream);
    if (rc != TSDF_OK) return rc;
    const bool any = src->info.n_vertices != 0;
    const bool has_normals = (src->info.flags & TSDF_MESH_NORMALS) != 0, has_rgb = (src->info.flags & TSDF_MESH_COLOURS) != 0;
    rc = run(src->info.n_vertices, src->info.n_indices, any ? src->vertices : nullptr, any ? src->indices : nullptr,
             any && has_normals ? src->normals : nullptr, any && has_rgb ? src->rgb : nullptr);
    const int rc2 = any ? mesh_leave(src, stream) : TSDF_OK;   // src's arrays are read by what has just been enqueued
    if (rc != TSDF_OK) return rc;
    dst->info.flags = src->info.flags | more_flags;
    std::memcpy(dst->info.box, src->info.box, sizeof(dst->info.box));
    return rc2;
}

}  // namespace tsdf
