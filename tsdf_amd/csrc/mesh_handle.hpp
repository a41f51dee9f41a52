// struct tsdf_mesh: what mesh.hip (extraction), mesh_components.hip (labelling, filtering), mesh_simplify.hip (clustering) and
// mesh_smooth.hip (smoothing, face normals) share.
#pragma once

#include "common.hpp"

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

// Arrays only grow; what they held is not kept.
template <typename T>
hipError_t mesh_reserve(T *&p, size_t &cap, size_t want) {
    if (want <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
}

constexpr size_t kComponentWords = 4;   // tsdf_mesh::component_words, and what tsdf_label_components_device holds for a call

}  // namespace tsdf

struct tsdf_mesh {
    int device;
    hipEvent_t done;        // recorded behind the last extraction's (labelling's, filter's) launches
    int pending;            // ... and not waited for yet
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
