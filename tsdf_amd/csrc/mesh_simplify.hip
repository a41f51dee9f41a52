// Mesh simplification by vertex clustering on a cell grid (Rossignac-Borrel), on the device (include/tsdf_amd.h, "mesh
// simplification").  Vertices whose cell floorf(V / h) is the same become one output vertex: the mean of their
// positions (normals, colours); triples that lose a corner to a neighbour are dropped.  No sort, no float atomics, nothing waits.
//   simplify_cluster_kernel        one lane per vertex: the 63-bit cell key goes into the open-addressed table (table_claim,
//                                  mesh_device.hpp), atomicMin of the vertex index into the slot's representative word, the slot
//                                  stored per vertex.  A loose vertex (no cell: non-finite, too far out) touches no table.
//   simplify_keep_vertices_kernel  per vertex its cluster's representative (a loose vertex: itself); keep bit "I am the representative"
//                                  by ballot over 64, popcounts
//   simplify_keep_triples_kernel   validates the triple (the first kernel that reads I), keep bit "three distinct representatives"
//   mesh_scan_*_kernel             the chunk scans (mesh_scan.hip); then the one synchronisation: the two counts and the error word
//   simplify_accumulate_kernel     per vertex its output index (its representative's base plus popcount) and integer atomic adds of the
//                                  quantised position (normal, colour) into that cluster's words, neighbouring lanes of one cluster
//                                  summed in registers first
//   simplify_emit_vertices_kernel  one lane per representative: a cluster of one keeps its member's bytes, the others divide their sums
//   simplify_emit_triples_kernel   the stable compaction of the kept triples, indices replaced by output indices
// The table never makes a lane wait (the argument is at table_claim): at most n_vertices keys exist and the table has at least twice as
// many slots.  The representative word is only ever made smaller (atomicMin) and is read by later kernels only.
// Every result is a unique value -- a minimum, integer sums, a division of exact integers -- so two runs give the same bytes.
#include <cmath>

#include "common.hpp"
#include "mesh_device.hpp"
#include "mesh_handle.hpp"

namespace tsdf {

constexpr uint32_t kLoose = 0xffffffffu;          // tsdf_mesh::cluster_of of a loose vertex, before the representatives are known
constexpr uint64_t kSimplifyMaxVertices = 1ull << 30;   // the table's slots are numbered in 32 bits, below kLoose

// which words of a cluster's row hold what: the count, then three sums each
struct ClusterRow {
    uint32_t words, normals, rgb;   // the row's length; where the normal and colour sums start (0: there are none)
};

// The cell of a vertex: false for a loose one.  All tests are in float, before anything becomes an integer.
__device__ inline bool cell_key(float x, float y, float z, float h, unsigned long long *key) {
    const float c[3] = {x, y, z};
    unsigned long long k = 0;
    for (int a = 2; a >= 0; a--) {
        const float f = floorf(c[a] / h);
        if (!coordinate_in_range(c[a]) || !(fabsf(f) < 1048576.0f)) return false;   // (NaN fails both)
        k = k << 21 | (unsigned long long)((int)f + 1048576);
    }
    *key = k;
    return true;
}

__global__ __launch_bounds__(256) void simplify_cluster_kernel(uint32_t n_vertices, const float *__restrict__ vertices, float h, uint32_t bits,
                                                               unsigned long long *keys, uint32_t *reps, uint32_t *__restrict__ cluster_of,
                                                               uint64_t *__restrict__ error) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    unsigned long long key;
    if (!cell_key(vertices[3 * v], vertices[3 * v + 1], vertices[3 * v + 2], h, &key)) {
        cluster_of[v] = kLoose;
        return;
    }
    uint64_t slot;
    if (!table_claim(keys, bits, key, &slot)) {
        raise_error(error, kErrorTableFull);
        cluster_of[v] = kLoose;
        return;
    }
    atomicMin(reps + slot, (uint32_t)v);
    cluster_of[v] = (uint32_t)slot;   // (at most 2^31 slots: kSimplifyMaxVertices)
}

// cluster_of: slot -> representative, in place (each lane rewrites its own word; reps is complete: the kernel boundary)
__global__ __launch_bounds__(256) void simplify_keep_vertices_kernel(uint32_t n_vertices, const uint32_t *__restrict__ reps, uint32_t *__restrict__ cluster_of,
                                                                     uint32_t v_chunks, uint64_t *__restrict__ v_mask, uint32_t *__restrict__ v_base) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= v_chunks) return;
    const uint64_t at = (uint64_t)chunk * 64 + lane;
    bool keep = false;
    if (at < n_vertices) {
        const uint32_t slot = cluster_of[at];
        const uint32_t rep = slot == kLoose ? (uint32_t)at : reps[slot];
        cluster_of[at] = rep;
        keep = rep == (uint32_t)at;
    }
    store_keep_mask(keep, lane, chunk, v_mask, v_base);
}

// (an index >= n_vertices raises the error word before it is an address; the host reads the word before anything is emitted)
__global__ __launch_bounds__(256) void simplify_keep_triples_kernel(uint32_t n_vertices, uint32_t n_triples, const uint32_t *__restrict__ indices,
                                                                    const uint32_t *__restrict__ cluster_of, uint32_t t_chunks,
                                                                    uint64_t *__restrict__ t_mask, uint32_t *__restrict__ t_base, uint64_t *__restrict__ error) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= t_chunks) return;
    const uint64_t at = (uint64_t)chunk * 64 + lane;
    bool keep = false;
    if (at < n_triples) {
        uint32_t c[3];
        if (!load_triple(n_vertices, indices, at, c)) {
            raise_error(error, kErrorIndex);
        } else {
            const uint32_t ra = cluster_of[c[0]], rb = cluster_of[c[1]], rc = cluster_of[c[2]];
            keep = ra != rb && ra != rc && rb != rc;
        }
    }
    store_keep_mask(keep, lane, chunk, t_mask, t_base);
}

__device__ inline void cluster_add(int64_t *word, long long q) { atomicAdd((unsigned long long *)word, (unsigned long long)q); }

// cluster_of: representative -> output index, in place.  A loose vertex adds nothing: its cluster's count stays 0 and its bytes are kept.
// Neighbouring lanes of one cluster (an extracted mesh is sorted by lattice key, x fastest) sum in registers first, a segmented sum
// towards the first lane of each run, and that lane does the adds: measured 2 to 3 times faster than one add per lane.
__global__ __launch_bounds__(256) void simplify_accumulate_kernel(uint32_t n_vertices, const float *__restrict__ vertices, const float *__restrict__ normals,
                                                                  const uint8_t *__restrict__ rgb, float h, const uint64_t *__restrict__ v_mask,
                                                                  const uint32_t *__restrict__ v_base, uint32_t *__restrict__ cluster_of,
                                                                  const ClusterRow row, int64_t *sums) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t j = 0xffffffffu;   // (no output index: at most 2^30 exist)
    long long q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool live = false;
    if (v < n_vertices) {
        j = compact_index(v_mask, v_base, cluster_of[v]);
        cluster_of[v] = j;
        const float x = vertices[3 * v], y = vertices[3 * v + 1], z = vertices[3 * v + 2];
        unsigned long long key;
        live = cell_key(x, y, z, h, &key);
        if (live) {
            q[0] = 1;
            q[1] = quantise_coordinate(x);
            q[2] = quantise_coordinate(y);
            q[3] = quantise_coordinate(z);
            if (row.normals) {
                const float nx = normals[3 * v], ny = normals[3 * v + 1], nz = normals[3 * v + 2];
                if (isfinite(nx) && isfinite(ny) && isfinite(nz)) {
                    q[4] = llrintf(nx * 1048576.0f);
                    q[5] = llrintf(ny * 1048576.0f);
                    q[6] = llrintf(nz * 1048576.0f);
                }
            }
            if (row.rgb)
                for (int k = 0; k < 3; k++) q[7 + k] = rgb[3 * v + k];
        }
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t key = live ? j : 0xffffffffu;
    const uint32_t before = __shfl_up(key, 1);
    const bool head = lane == 0 || before != key;
    const uint64_t heads = __ballot(head);
    const uint32_t run = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));   // the lane my run begins at
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t theirs = __shfl_down(run, o);
        const bool mine = lane + o < 64 && theirs == run;
        if (!__ballot(mine)) break;   // no run is longer than o
        for (int k = 0; k < 10; k++) {
            const long long t = __shfl_down(q[k], o);
            if (mine) q[k] += t;
        }
    }
    if (!live || !head) return;
    int64_t *s = sums + (size_t)j * row.words;
    for (int k = 0; k < 4; k++) cluster_add(s + k, q[k]);
    if (row.normals)
        for (int k = 0; k < 3; k++)
            if (q[4 + k]) cluster_add(s + row.normals + k, q[4 + k]);
    if (row.rgb)
        for (int k = 0; k < 3; k++)
            if (q[7 + k]) cluster_add(s + row.rgb + k, q[7 + k]);
}

// One lane per representative, in the shape of components_compact_vertices_kernel.
__global__ __launch_bounds__(256) void simplify_emit_vertices_kernel(uint32_t v_chunks, const uint64_t *__restrict__ v_mask, const uint32_t *__restrict__ v_base,
                                                                     const float *__restrict__ vertices, const float *__restrict__ normals,
                                                                     const uint8_t *__restrict__ rgb, const ClusterRow row, const int64_t *__restrict__ sums,
                                                                     float *__restrict__ out_vertices, float *__restrict__ out_normals,
                                                                     uint8_t *__restrict__ out_rgb) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= v_chunks) return;
    if (!((v_mask[chunk] >> lane) & 1u)) return;
    const uint32_t at = chunk * 64 + lane;
    const size_t from = (size_t)at * 3, j = compact_index(v_mask, v_base, at), to = j * 3;
    const int64_t *s = sums + j * row.words;
    const uint64_t n = (uint64_t)s[0];
    if (n <= 1) {   // a cluster of one (0: a loose vertex) keeps its member's bytes
        for (int k = 0; k < 3; k++) out_vertices[to + k] = vertices[from + k];
        if (row.normals)
            for (int k = 0; k < 3; k++) out_normals[to + k] = normals[from + k];
        if (row.rgb)
            for (int k = 0; k < 3; k++) out_rgb[to + k] = rgb[from + k];
        return;
    }
    for (int k = 0; k < 3; k++) out_vertices[to + k] = (float)(((double)s[1 + k] / (double)n) / 1024.0);
    if (row.normals) store_unit_or_nan(out_normals + to, (double)s[row.normals], (double)s[row.normals + 1], (double)s[row.normals + 2]);
    if (row.rgb)
        for (int k = 0; k < 3; k++) out_rgb[to + k] = (uint8_t)((2 * (uint64_t)s[row.rgb + k] + n) / (2 * n));
}

__global__ __launch_bounds__(256) void simplify_emit_triples_kernel(uint32_t t_chunks, const uint64_t *__restrict__ t_mask, const uint32_t *__restrict__ t_base,
                                                                    const uint32_t *__restrict__ cluster_of, const uint32_t *__restrict__ indices,
                                                                    uint32_t *__restrict__ out_indices) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= t_chunks) return;
    if (!((t_mask[chunk] >> lane) & 1u)) return;
    const uint32_t at = chunk * 64 + lane;
    const size_t from = (size_t)at * 3, to = (size_t)compact_index(t_mask, t_base, at) * 3;
    for (int k = 0; k < 3; k++) out_indices[to + k] = cluster_of[indices[from + k]];
}

}  // namespace tsdf

using namespace tsdf;

namespace {

// Everything between the argument checks and the counts in dst->info.  n_vertices > 0; dst->info is already that of an empty mesh.
int simplify_on(uint32_t nv, uint32_t n_triples, const float *vertices, const uint32_t *indices, const float *normals, const uint8_t *rgb, float h,
                tsdf_mesh *dst, hipStream_t stream, const char *who) {
    const uint32_t bits = mesh_table_bits(nv);
    const size_t slots = (size_t)1 << bits;
    const uint32_t v_chunks = (nv + 63) / 64, t_chunks = (n_triples + 63) / 64;
    const uint32_t chunks = v_chunks > t_chunks ? v_chunks : t_chunks, n_parts = mesh_scan_parts(chunks);
    hipError_t e = device_reserve(dst->cell_keys, dst->cell_keys_cap, slots);
    if (e == hipSuccess) e = device_reserve(dst->cell_reps, dst->cell_reps_cap, slots);
    if (e == hipSuccess) e = device_reserve(dst->cluster_of, dst->cluster_of_cap, (size_t)nv);
    if (e == hipSuccess) e = device_reserve(dst->keep_masks, dst->keep_masks_cap, (size_t)v_chunks + t_chunks);
    if (e == hipSuccess) e = device_reserve(dst->keep_bases, dst->keep_bases_cap, (size_t)v_chunks + t_chunks);
    if (e == hipSuccess) e = device_reserve(dst->parts, dst->parts_cap, 2 * ((size_t)n_parts + 1) + 1);   // the sums, the two totals, the error word
    if (e != hipSuccess) return hip_fail(e, "mesh simplify scratch alloc failed");
    uint64_t *v_mask = dst->keep_masks, *t_mask = dst->keep_masks + v_chunks;
    uint32_t *v_base = dst->keep_bases, *t_base = dst->keep_bases + v_chunks;
    uint64_t *totals = dst->parts + 2 * (size_t)n_parts, *error = totals + 2;
    TSDF_HIP(hipMemsetAsync(dst->cell_keys, 0xff, slots * sizeof(uint64_t), stream), "mesh simplify table");
    TSDF_HIP(hipMemsetAsync(dst->cell_reps, 0xff, slots * sizeof(uint32_t), stream), "mesh simplify table");
    TSDF_HIP(hipMemsetAsync(error, 0, sizeof(uint64_t), stream), "mesh simplify error word");
    hipLaunchKernelGGL(simplify_cluster_kernel, grid_for(nv, 256), dim3(256), 0, stream, nv, vertices, h, bits, (unsigned long long *)dst->cell_keys,
                       dst->cell_reps, dst->cluster_of, error);
    hipLaunchKernelGGL(simplify_keep_vertices_kernel, dim3((v_chunks + 3) / 4), dim3(256), 0, stream, nv, dst->cell_reps, dst->cluster_of, v_chunks, v_mask,
                       v_base);
    if (t_chunks)
        hipLaunchKernelGGL(simplify_keep_triples_kernel, dim3((t_chunks + 3) / 4), dim3(256), 0, stream, nv, n_triples, indices, dst->cluster_of, t_chunks,
                           t_mask, t_base, error);
    mesh_scan(ArrayCounts{v_base, v_chunks, t_base, t_chunks}, n_parts, dst->parts, stream);
    TSDF_HIP(hipGetLastError(), "mesh simplify count kernels failed");
    uint64_t host[3] = {0, 0, 0};
    const int rc = error_word_checked(who, nv, totals, host, 3, 2, stream);   // the one synchronisation: the arrays are sized from the counts
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(host[2] == 0, "%s: the cell table overflowed", who);
    const uint64_t n_clusters = host[0], kept_triples = host[1];

    ClusterRow row;
    row.words = 4;
    row.normals = row.rgb = 0;
    if (normals) {
        row.normals = row.words;
        row.words += 3;
    }
    if (rgb) {
        row.rgb = row.words;
        row.words += 3;
    }
    e = device_reserve(dst->cluster_sums, dst->cluster_sums_cap, (size_t)n_clusters * row.words);
    if (e == hipSuccess) e = device_reserve(dst->vertices, dst->vertices_cap, (size_t)n_clusters * 3);
    if (e == hipSuccess) e = device_reserve(dst->indices, dst->indices_cap, (size_t)(kept_triples ? kept_triples * 3 : 1));
    if (e == hipSuccess && normals) e = device_reserve(dst->normals, dst->normals_cap, (size_t)n_clusters * 3);
    if (e == hipSuccess && rgb) e = device_reserve(dst->rgb, dst->rgb_cap, (size_t)n_clusters * 3);
    if (e != hipSuccess) return hip_fail(e, "mesh array alloc failed");
    TSDF_HIP(hipMemsetAsync(dst->cluster_sums, 0, (size_t)n_clusters * row.words * sizeof(int64_t), stream), "mesh simplify sums");
    hipLaunchKernelGGL(simplify_accumulate_kernel, grid_for(nv, 256), dim3(256), 0, stream, nv, vertices, normals, rgb, h, v_mask, v_base, dst->cluster_of, row,
                       dst->cluster_sums);
    hipLaunchKernelGGL(simplify_emit_vertices_kernel, dim3((v_chunks + 3) / 4), dim3(256), 0, stream, v_chunks, v_mask, v_base, vertices, normals, rgb, row,
                       dst->cluster_sums, dst->vertices, dst->normals, dst->rgb);
    if (kept_triples)
        hipLaunchKernelGGL(simplify_emit_triples_kernel, dim3((t_chunks + 3) / 4), dim3(256), 0, stream, t_chunks, t_mask, t_base, dst->cluster_of, indices,
                           dst->indices);
    TSDF_HIP(hipGetLastError(), "mesh simplify emit kernels failed");
    dst->info.n_vertices = n_clusters;
    dst->info.n_indices = kept_triples * 3;
    return TSDF_OK;
}

// the checks both entry points share, and the run as a call into dst
int simplify_checked(uint64_t n_vertices, uint64_t n_indices, const float *vertices, const uint32_t *indices, const float *normals, const uint8_t *rgb,
                     float cell_size, uint32_t flags, tsdf_mesh *dst, hipStream_t stream, const char *who) {
    const int rc = arrays_checked(who, n_vertices, n_indices, vertices, indices);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(std::isfinite(cell_size) && cell_size > 0.0f, "%s: cell_size (%g) is not a finite length above 0", who, (double)cell_size);
    TSDF_REQUIRE(flags == 0, "%s: unknown flags %#x", who, flags);
    TSDF_REQUIRE(n_vertices <= kSimplifyMaxVertices, "%s: %llu vertices are more than the 2^30 one call takes: simplify the mesh in boxes", who,
                 (unsigned long long)n_vertices);
    return mesh_into(who, n_vertices, n_indices, (normals ? TSDF_MESH_NORMALS : 0u) | (rgb ? TSDF_MESH_COLOURS : 0u), dst, stream, [&] {
        return simplify_on((uint32_t)n_vertices, (uint32_t)(n_indices / 3), vertices, indices, normals, rgb, cell_size, dst, stream, who);
    });
}

}  // namespace

extern "C" {

int tsdf_simplify_mesh_device(uint64_t n_vertices, uint64_t n_indices, const float *device_vertices, const uint32_t *device_indices,
                              const float *device_normals, const uint8_t *device_rgb, float cell_size, uint32_t flags, tsdf_mesh *dst, void *hip_stream) {
    TSDF_REQUIRE(dst, "tsdf_simplify_mesh_device: null dst");
    return simplify_checked(n_vertices, n_indices, device_vertices, device_indices, device_normals, device_rgb, cell_size, flags, dst,
                            (hipStream_t)hip_stream, "tsdf_simplify_mesh_device");
}

int tsdf_mesh_simplify(tsdf_mesh *src, float cell_size, uint32_t flags, tsdf_mesh *dst, void *hip_stream) {
    const char *who = "tsdf_mesh_simplify";
    hipStream_t stream = (hipStream_t)hip_stream;
    return mesh_from_handle(who, "simplify", src, dst, 0u, stream,
                            [&](uint64_t nv, uint64_t ni, const float *vertices, const uint32_t *indices, const float *normals, const uint8_t *rgb) {
                                return simplify_checked(nv, ni, vertices, indices, normals, rgb, cell_size, flags, dst, stream, who);
                            });
}

}  // extern "C"
