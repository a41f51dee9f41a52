// Connected components of an indexed mesh on the device, and the filter that drops the small ones (include/tsdf_amd.h, "mesh
// components").  L[v] = the smallest vertex index of v's component, T[v] = the index triples of that component.
//
// Labelling is a lock-free union-find over L itself, hooks towards the smaller index:
//   components_init_kernel       parent[v] = v, T[v] = 0
//   components_hook_kernel       one lane per triple: validate it, unite(a, b), unite(a, c)
//   components_flatten_kernel    L[v] = root(v) (a launch of its own: the kernel boundary makes every hook visible); roots counted
//                                by ballot and popcount, one integer atomic per wave that has any
//   components_count_kernel      T[L[I[3t]]] += 1, integer atomics; one add per wave where its lanes share a label
//   components_broadcast_kernel  T[v] = T[L[v]] in place (only roots are read, a root rewrites its own value) and one 64-bit
//                                atomicMax per wave that holds a root, of (T << 32) | (0xFFFFFFFF - L): the largest component
// The three invariants every line of the first two kernels keeps:
//   1. parent[v] <= v always; a word changes only from v to something smaller in the same component (the CAS of unite) or from one
//      ancestor to a smaller one (the atomicMin of find).  So every chain strictly decreases: find terminates, there are no cycles,
//      and the final root is the component's minimum.
//   2. A stale read sees v itself or a former ancestor -- still in the component, still <= v.  Nothing rests on a read being fresh,
//      only on the CAS, which executes at device scope and returns the true word.
//   3. No lane ever waits for another lane, wave or workgroup: no spin loops, locks or flags.  A failed CAS means another lane made
//      the word smaller, and the loop goes on from the value it returned; every loop is bounded by a strictly decreasing index.
// The results are unique values (a minimum, integer sums, a maximum with a total order), so two runs give the same bytes.
//
// The filter has no atomics: keep flags per vertex and per triple by ballot over 64, popcount bases, the chunk scan (mesh_scan.hip),
// and a stable compaction in which a new index is a base plus the popcount below the lane (mesh_device.hpp).
#include <new>

#include "common.hpp"
#include "mesh_device.hpp"
#include "mesh_handle.hpp"
#include "union_find.hpp"

namespace tsdf {

enum { kWordError = 0, kWordRoots = 1, kWordLargest = 2 };   // tsdf_mesh::component_words

// (parent_load, components_find and components_unite: union_find.hpp, shared with voxel_set.hpp)

__global__ __launch_bounds__(256) void components_init_kernel(uint32_t n_vertices, uint32_t *__restrict__ parent, uint32_t *__restrict__ sizes) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    parent[v] = (uint32_t)v;
    if (sizes) sizes[v] = 0;
}

__global__ __launch_bounds__(256) void components_hook_kernel(uint32_t n_vertices, uint32_t n_triples, const uint32_t *__restrict__ indices,
                                                              uint32_t *parent, uint64_t *__restrict__ words) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_triples) return;
    uint32_t c[3];
    if (!load_triple(n_vertices, indices, t, c)) {
        raise_error(words + kWordError, kErrorIndex);
        return;
    }
    if (c[0] != c[1]) components_unite(parent, c[0], c[1]);
    if (c[0] != c[2]) components_unite(parent, c[0], c[2]);
}

__global__ __launch_bounds__(256) void components_flatten_kernel(uint32_t n_vertices, uint32_t *labels, uint64_t *__restrict__ words) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool is_root = false;
    if (v < n_vertices) {
        const uint32_t root = components_find<false>(labels, (uint32_t)v);
        is_root = root == (uint32_t)v;
        // (another lane may be walking through v: it reads the old ancestor or the root, both on its way)
        if (!is_root) __hip_atomic_store(labels + v, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t roots = __ballot(is_root);
    if (roots && (threadIdx.x & 63u) == 0) atomicAdd((unsigned long long *)(words + kWordRoots), (unsigned long long)__popcll(roots));
}

// (an index >= n_vertices has raised the error word in components_hook_kernel; its triple is passed over here, so that nothing
// outside the arrays is touched before the host reads the word)
__global__ __launch_bounds__(256) void components_count_kernel(uint32_t n_vertices, uint32_t n_triples, const uint32_t *__restrict__ indices,
                                                               const uint32_t *__restrict__ labels, uint32_t *__restrict__ sizes) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t a = 0;
    const bool valid = t < n_triples && (a = indices[3 * t]) < n_vertices;
    const uint32_t label = valid ? labels[a] : 0xffffffffu;
    const uint64_t active = __ballot(valid);
    if (!active) return;
    const uint32_t lead = __shfl(label, __ffsll((unsigned long long)active) - 1);
    if (__ballot(valid && label == lead) == active) {   // a mesh's triples are cubes apart: nearly every wave has one label
        if ((threadIdx.x & 63u) == (uint32_t)(__ffsll((unsigned long long)active) - 1)) atomicAdd(sizes + lead, (uint32_t)__popcll(active));
    } else if (valid) {
        atomicAdd(sizes + label, 1u);
    }
}

__global__ __launch_bounds__(256) void components_broadcast_kernel(uint32_t n_vertices, const uint32_t *__restrict__ labels, uint32_t *sizes,
                                                                   uint64_t *__restrict__ words) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long best = 0;
    if (v < n_vertices) {
        const uint32_t label = labels[v], count = sizes[label];
        if (label != (uint32_t)v) sizes[v] = count;
        else best = (unsigned long long)count << 32 | (0xffffffffu - label);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o);
        best = other > best ? other : best;
    }
    if (best && (threadIdx.x & 63u) == 0) atomicMax((unsigned long long *)(words + kWordLargest), best);
}

// ---- the filter --------------------------------------------------------------------------------------------------------------------
struct KeepRule {
    uint64_t min_triangles;
    uint32_t only_label;   // with `only`: the one component that may be kept
    uint32_t only;
    __device__ bool keeps(uint32_t label, uint32_t count) const { return count >= min_triangles && (!only || label == only_label); }
};

// One wave per chunk of 64 vertices and, with the same number, of 64 triples: the keep masks and their popcounts.
__global__ __launch_bounds__(256) void components_keep_kernel(uint32_t n_vertices, uint32_t n_triples, const uint32_t *__restrict__ indices,
                                                              const uint32_t *__restrict__ labels, const uint32_t *__restrict__ sizes, const KeepRule rule,
                                                              uint32_t v_chunks, uint32_t t_chunks, uint64_t *__restrict__ v_mask,
                                                              uint32_t *__restrict__ v_base, uint64_t *__restrict__ t_mask, uint32_t *__restrict__ t_base) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t at = (uint64_t)chunk * 64 + lane;
    if (chunk < v_chunks) store_keep_mask(at < n_vertices && rule.keeps(labels[at], sizes[at]), lane, chunk, v_mask, v_base);
    if (chunk < t_chunks) {
        bool keep = false;
        if (at < n_triples) {
            const uint32_t a = indices[3 * at];
            keep = rule.keeps(labels[a], sizes[a]);
        }
        store_keep_mask(keep, lane, chunk, t_mask, t_base);
    }
}

// Stable compaction: a kept vertex goes where compact_index says; normals and colours go with it.
__global__ __launch_bounds__(256) void components_compact_vertices_kernel(uint32_t v_chunks, const uint64_t *__restrict__ v_mask, const uint32_t *__restrict__ v_base,
                                                                          const float *__restrict__ vertices, const float *__restrict__ normals,
                                                                          const uint8_t *__restrict__ rgb, float *__restrict__ out_vertices,
                                                                          float *__restrict__ out_normals, uint8_t *__restrict__ out_rgb) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= v_chunks) return;
    if (!((v_mask[chunk] >> lane) & 1u)) return;
    const uint32_t at = chunk * 64 + lane;
    const size_t from = (size_t)at * 3, to = (size_t)compact_index(v_mask, v_base, at) * 3;
    for (int k = 0; k < 3; k++) out_vertices[to + k] = vertices[from + k];
    if (normals)
        for (int k = 0; k < 3; k++) out_normals[to + k] = normals[from + k];
    if (rgb)
        for (int k = 0; k < 3; k++) out_rgb[to + k] = rgb[from + k];
}

// ... and a kept triple, with each index replaced by where its vertex went (all three are kept: they share the component).
__global__ __launch_bounds__(256) void components_compact_indices_kernel(uint32_t t_chunks, const uint64_t *__restrict__ t_mask, const uint32_t *__restrict__ t_base,
                                                                         const uint64_t *__restrict__ v_mask, const uint32_t *__restrict__ v_base,
                                                                         const uint32_t *__restrict__ indices, uint32_t *__restrict__ out_indices) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= t_chunks) return;
    if (!((t_mask[chunk] >> lane) & 1u)) return;
    const uint32_t at = chunk * 64 + lane;
    const size_t from = (size_t)at * 3, to = (size_t)compact_index(t_mask, t_base, at) * 3;
    for (int k = 0; k < 3; k++) out_indices[to + k] = compact_index(v_mask, v_base, indices[from + k]);
}

}  // namespace tsdf

using namespace tsdf;

namespace {

// The five launches and the one synchronisation.  `words`: kComponentWords device words.  n_vertices > 0.
int label_on(uint32_t n_vertices, uint32_t n_indices, const uint32_t *indices, uint32_t *labels, uint32_t *sizes, uint64_t *words,
             tsdf_components_info *info, hipStream_t stream, const char *who) {
    const uint32_t n_triples = n_indices / 3;
    uint64_t host[kComponentWords] = {0, 0, 0, 0};
    TSDF_HIP(hipMemsetAsync(words, 0, kComponentWords * sizeof(uint64_t), stream), "components words");
    hipLaunchKernelGGL(components_init_kernel, grid_for(n_vertices, 256), dim3(256), 0, stream, n_vertices, labels, sizes);
    if (n_triples) hipLaunchKernelGGL(components_hook_kernel, grid_for(n_triples, 256), dim3(256), 0, stream, n_vertices, n_triples, indices, labels, words);
    hipLaunchKernelGGL(components_flatten_kernel, grid_for(n_vertices, 256), dim3(256), 0, stream, n_vertices, labels, words);
    if (sizes) {
        if (n_triples) hipLaunchKernelGGL(components_count_kernel, grid_for(n_triples, 256), dim3(256), 0, stream, n_vertices, n_triples, indices, labels, sizes);
        hipLaunchKernelGGL(components_broadcast_kernel, grid_for(n_vertices, 256), dim3(256), 0, stream, n_vertices, labels, sizes, words);
    }
    TSDF_HIP(hipGetLastError(), "components kernels failed");
    const int rc = error_word_checked(who, n_vertices, words, host, kComponentWords, kWordError, stream);   // the one synchronisation
    if (rc != TSDF_OK) return rc;
    if (info) {
        info->n_components = host[kWordRoots];
        info->n_triangles = n_triples;
        info->largest_triangles = host[kWordLargest] >> 32;
        info->largest_label = host[kWordLargest] ? 0xffffffffu - (uint32_t)host[kWordLargest] : 0xffffffffu;
    }
    return TSDF_OK;
}

const tsdf_components_info kNoComponents = {0, 0, 0, 0xffffffffu};

int mesh_label(tsdf_mesh *m, hipStream_t stream, const char *who) {
    m->labelled = 0;
    const uint64_t nv = m->info.n_vertices, ni = m->info.n_indices;
    m->components = kNoComponents;
    m->components.n_triangles = ni / 3;
    if (nv == 0) {
        m->labelled = 1;
        return TSDF_OK;
    }
    int rc = mesh_join(m, stream);
    if (rc != TSDF_OK) return rc;
    hipError_t e = device_reserve(m->labels, m->labels_cap, (size_t)nv);
    if (e == hipSuccess) e = device_reserve(m->sizes, m->sizes_cap, (size_t)nv);
    if (e == hipSuccess && !m->component_words) e = hipMalloc((void **)&m->component_words, kComponentWords * sizeof(uint64_t));
    if (e != hipSuccess) return hip_fail(e, "mesh components alloc failed");
    rc = label_on((uint32_t)nv, (uint32_t)ni, m->indices, m->labels, m->sizes, m->component_words, &m->components, stream, who);
    const int rc2 = mesh_leave(m, stream);
    if (rc != TSDF_OK) return rc;
    if (rc2 != TSDF_OK) return rc2;
    m->labelled = 1;
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_label_components_device(uint64_t n_vertices, uint64_t n_indices, const uint32_t *device_indices, uint32_t *device_labels,
                                 uint32_t *device_component_triangles, tsdf_components_info *info, void *hip_stream) {
    TSDF_REQUIRE(device_labels, "tsdf_label_components_device: null device_labels");
    const int rcc = indices_checked("tsdf_label_components_device", n_vertices, n_indices, device_indices);
    if (rcc != TSDF_OK) return rcc;
    if (n_vertices == 0) {
        if (n_indices) return index_refused("tsdf_label_components_device", 0);
        if (info) *info = kNoComponents;
        return TSDF_OK;
    }
    uint64_t *words = nullptr;
    TSDF_HIP(hipMalloc((void **)&words, kComponentWords * sizeof(uint64_t)), "components words alloc failed");
    const int rc = label_on((uint32_t)n_vertices, (uint32_t)n_indices, device_indices, device_labels, device_component_triangles, words, info,
                            (hipStream_t)hip_stream, "tsdf_label_components_device");
    (void)hipFree(words);
    return rc;
}

int tsdf_mesh_label_components(tsdf_mesh *m, tsdf_components_info *info, void *hip_stream) {
    TSDF_REQUIRE(m, "tsdf_mesh_label_components: null mesh");
    const int rc = mesh_label(m, (hipStream_t)hip_stream, "tsdf_mesh_label_components");
    if (rc == TSDF_OK && info) *info = m->components;
    return rc;
}

int tsdf_mesh_component_buffers(const tsdf_mesh *cm, const uint32_t **device_labels, const uint32_t **device_component_triangles) {
    TSDF_REQUIRE(cm, "tsdf_mesh_component_buffers: null mesh");
    TSDF_REQUIRE(cm->labelled, "tsdf_mesh_component_buffers: the mesh has not been labelled since its last extraction (tsdf_mesh_label_components)");
    const int rc = mesh_wait(cm);
    if (rc != TSDF_OK) return rc;
    const bool any = cm->info.n_vertices != 0;
    if (device_labels) *device_labels = any ? cm->labels : nullptr;
    if (device_component_triangles) *device_component_triangles = any ? cm->sizes : nullptr;
    return TSDF_OK;
}

int tsdf_mesh_component_download(const tsdf_mesh *cm, uint32_t *host_labels, uint32_t *host_component_triangles) {
    TSDF_REQUIRE(cm, "tsdf_mesh_component_download: null mesh");
    const uint32_t *labels = nullptr, *sizes = nullptr;
    const int rc = tsdf_mesh_component_buffers(cm, &labels, &sizes);
    if (rc != TSDF_OK) return rc;
    const size_t bytes = (size_t)cm->info.n_vertices * sizeof(uint32_t);
    if (bytes == 0) return TSDF_OK;
    if (host_labels) TSDF_HIP(hipMemcpy(host_labels, labels, bytes, hipMemcpyDeviceToHost), "mesh components download");
    if (host_component_triangles) TSDF_HIP(hipMemcpy(host_component_triangles, sizes, bytes, hipMemcpyDeviceToHost), "mesh components download");
    return TSDF_OK;
}

int tsdf_mesh_filter_components(tsdf_mesh *src, uint64_t min_triangles, uint32_t flags, tsdf_mesh *dst, void *hip_stream) {
    TSDF_REQUIRE(src && dst, "tsdf_mesh_filter_components: null mesh");
    TSDF_REQUIRE(src != dst, "tsdf_mesh_filter_components: dst is src (filter into another handle)");
    TSDF_REQUIRE((flags & ~(uint32_t)TSDF_MESH_KEEP_LARGEST) == 0, "tsdf_mesh_filter_components: unknown flags %#x", flags);
    TSDF_REQUIRE(src->device == dst->device, "tsdf_mesh_filter_components: src was created on device %d, dst on device %d", src->device, dst->device);
    hipStream_t stream = (hipStream_t)hip_stream;
    int rc = TSDF_OK;
    if (!src->labelled) rc = mesh_label(src, stream, "tsdf_mesh_filter_components");   // (the first synchronisation)
    if (rc == TSDF_OK) rc = mesh_join(src, stream);
    if (rc == TSDF_OK) rc = mesh_join(dst, stream);
    if (rc != TSDF_OK) return rc;
    mesh_reset(dst);
    dst->info.flags = src->info.flags;
    std::memcpy(dst->info.box, src->info.box, sizeof(dst->info.box));
    const uint64_t nv = src->info.n_vertices, n_triples = src->info.n_indices / 3;
    if (nv == 0) return TSDF_OK;

    const bool has_normals = (src->info.flags & TSDF_MESH_NORMALS) != 0, has_rgb = (src->info.flags & TSDF_MESH_COLOURS) != 0;
    const uint32_t v_chunks = (uint32_t)((nv + 63) / 64), t_chunks = (uint32_t)((n_triples + 63) / 64);
    const uint32_t chunks = v_chunks > t_chunks ? v_chunks : t_chunks, n_parts = mesh_scan_parts(chunks);
    hipError_t e = device_reserve(dst->keep_masks, dst->keep_masks_cap, (size_t)v_chunks + t_chunks);
    if (e == hipSuccess) e = device_reserve(dst->keep_bases, dst->keep_bases_cap, (size_t)v_chunks + t_chunks);
    if (e == hipSuccess) e = device_reserve(dst->parts, dst->parts_cap, 2 * ((size_t)n_parts + 1));
    if (e != hipSuccess) return hip_fail(e, "mesh filter scratch alloc failed");
    uint64_t *v_mask = dst->keep_masks, *t_mask = dst->keep_masks + v_chunks;
    uint32_t *v_base = dst->keep_bases, *t_base = dst->keep_bases + v_chunks;
    KeepRule rule;
    rule.min_triangles = min_triangles;
    rule.only = (flags & TSDF_MESH_KEEP_LARGEST) ? 1u : 0u;
    rule.only_label = src->components.largest_label;
    const dim3 grid((chunks + 3) / 4);
    hipLaunchKernelGGL(components_keep_kernel, grid, dim3(256), 0, stream, (uint32_t)nv, (uint32_t)n_triples, src->indices, src->labels, src->sizes, rule,
                       v_chunks, t_chunks, v_mask, v_base, t_mask, t_base);
    mesh_scan(ArrayCounts{v_base, v_chunks, t_base, t_chunks}, n_parts, dst->parts, stream);
    TSDF_HIP(hipGetLastError(), "mesh filter count kernels failed");
    TSDF_HIP(hipMemcpyAsync(dst->totals, dst->parts + 2 * (size_t)n_parts, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "mesh filter counts download");
    TSDF_HIP(hipStreamSynchronize(stream), "mesh filter count");   // the arrays are sized from the counts
    const uint64_t kept_vertices = dst->totals[0], kept_triples = dst->totals[1];
    if (kept_vertices == 0) return mesh_leave(src, stream);
    e = device_reserve(dst->vertices, dst->vertices_cap, (size_t)kept_vertices * 3);
    if (e == hipSuccess) e = device_reserve(dst->indices, dst->indices_cap, (size_t)(kept_triples ? kept_triples * 3 : 1));
    if (e == hipSuccess && has_normals) e = device_reserve(dst->normals, dst->normals_cap, (size_t)kept_vertices * 3);
    if (e == hipSuccess && has_rgb) e = device_reserve(dst->rgb, dst->rgb_cap, (size_t)kept_vertices * 3);
    if (e != hipSuccess) return hip_fail(e, "mesh array alloc failed");
    hipLaunchKernelGGL(components_compact_vertices_kernel, dim3((v_chunks + 3) / 4), dim3(256), 0, stream, v_chunks, v_mask, v_base, src->vertices,
                       has_normals ? src->normals : nullptr, has_rgb ? src->rgb : nullptr, dst->vertices, dst->normals, dst->rgb);
    if (t_chunks)
        hipLaunchKernelGGL(components_compact_indices_kernel, dim3((t_chunks + 3) / 4), dim3(256), 0, stream, t_chunks, t_mask, t_base, v_mask, v_base,
                           src->indices, dst->indices);
    TSDF_HIP(hipGetLastError(), "mesh filter emit kernels failed");
    rc = mesh_leave(src, stream);
    if (rc == TSDF_OK) rc = mesh_leave(dst, stream);
    if (rc != TSDF_OK) return rc;
    dst->info.n_vertices = kept_vertices;
    dst->info.n_indices = kept_triples * 3;
    return TSDF_OK;
}

}  // extern "C"
