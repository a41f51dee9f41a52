// Scene flow into the deformation field (include/tsdf_amd.h, "scene flow"): the device part of the reference's
// SceneFusion step (src/SceneFusion/SceneFusion_krnl.cu: find_mesh_vertex_correspondences :74-114, update_deformation_field :211-232)
// on an indexed mesh of the whole grid, without its two defects -- the unsynchronised `translation +=` of many threads into one
// node and the round trip of the correspondence flags to the host.
//
// The indexed mesh has one vertex per lattice edge, in the order of the key ((z Y + y) X + x) 3 + axis, and the handle keeps the
// extraction's per-64-voxel records (MeshChunk: which voxels have a used edge towards +x, +y, +z, and the index of the chunk's
// first vertex).  So the two voxels that bracket a vertex are its key, and the vertices round a voxel are six mask bits:
//   scene_flow_match_kernel         one lane per shared vertex: its pixel index, or kNoPixel for no correspondence
//   scene_flow_multiplicity_kernel  m(e) = the soup vertices on edge e: integer atomicAdd over the index buffer
//   scene_flow_apply_kernel         a GATHER, one wave per chunk, one lane per voxel: its up to six edges in the fixed order
//                                   -x, +x, -y, +y, -z, +z, one writer per node, no float atomics
// The only atomics are integer adds (multiplicities, the two info counts): nothing depends on the order in which waves finish.
#include <climits>
#include <cmath>

#include "common.hpp"
#include "mesh_handle.hpp"

namespace tsdf {

constexpr uint32_t kNoPixel = 0xffffffffu, kNoEdge = 0xffffffffu;

// world_to_pixel (src/Utilities/cuda_coordinate_transforms.cu:10-30), the in-image test, depth > 0, pixel_to_world (:40-67, its
// division by w included) and the depth-only distance of find_mesh_vertex_correspondences, operation for operation; a flow triple
// with a non-finite component is no correspondence (ours).  counts[0] takes the correspondences.
__global__ __launch_bounds__(256) void scene_flow_match_kernel(const float *__restrict__ points, uint32_t n_vertices, const uint16_t *__restrict__ depth,
                                                               const float *__restrict__ flow, uint32_t width, uint32_t height, const Mat44 pose,
                                                               const Mat44 ip, const Mat33 k, const Mat33 kinv, float threshold,
                                                               uint2 *__restrict__ vertex, unsigned long long *__restrict__ counts) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    uint32_t pixel = kNoPixel;
    if (e < n_vertices) {
        const float px = points[(size_t)e * 3], py = points[(size_t)e * 3 + 1], pz = points[(size_t)e * 3 + 2];
        const float camx = ip.m11 * px + ip.m12 * py + ip.m13 * pz + ip.m14;
        const float camy = ip.m21 * px + ip.m22 * py + ip.m23 * pz + ip.m24;
        const float camz = ip.m31 * px + ip.m32 * py + ip.m33 * pz + ip.m34;
        const float imx = k.m11 * camx + k.m12 * camy + k.m13 * camz;
        const float imy = k.m21 * camx + k.m22 * camy + k.m23 * camz;
        const float imz = k.m31 * camx + k.m32 * camy + k.m33 * camz;
        const int ix = f2i_sat(roundf(imx / imz)), iy = f2i_sat(roundf(imy / imz));
        if (ix >= 0 && (uint32_t)ix < width && iy >= 0 && (uint32_t)iy < height) {
            const uint32_t at = (uint32_t)iy * width + (uint32_t)ix;
            const uint16_t d = depth[at];
            if (d > 0) {
                const float fd = (float)d;
                const float cx = fd * (kinv.m11 * ix + kinv.m12 * iy + kinv.m13);
                const float cy = fd * (kinv.m21 * ix + kinv.m22 * iy + kinv.m23);
                const float cz = fd * (kinv.m31 * ix + kinv.m32 * iy + kinv.m33);
                const float wz = pose.m31 * cx + pose.m32 * cy + pose.m33 * cz + pose.m34;
                const float w = pose.m41 * cx + pose.m42 * cy + pose.m43 * cz + pose.m44;
                if (fabsf(wz / w - pz) < threshold) {   // (false for NaN)
                    const float *f = flow + (size_t)at * 3;
                    if (isfinite(f[0]) && isfinite(f[1]) && isfinite(f[2])) pixel = at;
                }
            }
        }
        vertex[e] = make_uint2(pixel, 0u);   // (the multiplicity kernel counts into .y)
    }
    const uint64_t found = __ballot(pixel != kNoPixel);
    if ((threadIdx.x & 63u) == 0 && found) atomicAdd(counts, (unsigned long long)__popcll(found));
}

__global__ __launch_bounds__(256) void scene_flow_multiplicity_kernel(const uint32_t *__restrict__ indices, uint64_t n_indices, uint32_t n_vertices,
                                                                      uint2 *__restrict__ vertex) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_indices; i += (uint64_t)gridDim.x * 256) {
        const uint32_t e = indices[i];
        if (e < n_vertices) atomicAdd(&vertex[e].y, 1u);
    }
}

// The vertex of the edge along `axis` whose lower end is the l-th voxel of the chunk with record c: mesh_triangles_kernel's base
// plus popcounts (mesh.hip); kNoEdge when the edge is not used.
__device__ inline uint32_t flow_edge(const MeshChunk &c, uint32_t l, int axis, uint32_t n_vertices) {
    const uint64_t m = axis == 0 ? c.mx : axis == 1 ? c.my : c.mz;
    if (!((m >> l) & 1u)) return kNoEdge;
    const uint64_t below = (1ull << l) - 1;
    uint32_t index = c.vbase + __popcll(c.mx & below) + __popcll(c.my & below) + __popcll(c.mz & below);
    if (axis > 0) index += (uint32_t)(c.mx >> l) & 1u;
    if (axis > 1) index += (uint32_t)(c.my >> l) & 1u;
    return index < n_vertices ? index : kNoEdge;   // (always, for the records of the arrays at hand)
}

// One wave per chunk of 64 voxels of the whole grid (voxel = 64 chunk + lane, the grid's own index x + y W + z W H).  A lane's +x,
// +y, +z edges are its own mask bits; its -x, -y, -z edges are the +x, +y, +z bits of the voxels 1, W and W H earlier, in this
// chunk's record or an earlier chunk's.  The three guards below (lane 0 of chunk 0, the first row of the first plane, the first
// plane) are the ones that keep the address inside the array.  Where "1 / W / W H earlier" wraps to the end of the previous row or
// plane (x = 0, y = 0) the voxel found is the last of its row or plane along that axis, whose bit towards +axis mesh_edges_kernel
// never sets (an edge needs its upper end in the grid): no further test is needed, and none of the coordinates is ever formed.
// counts[1] takes the nodes written.
__global__ __launch_bounds__(256) void scene_flow_apply_kernel(const MeshChunk *__restrict__ chunks, uint32_t n_chunks, uint64_t n_voxels, uint64_t W,
                                                               uint64_t plane, const uint2 *__restrict__ vertex, uint32_t n_vertices,
                                                               const float *__restrict__ flow, tsdf_deformation_node *__restrict__ nodes,
                                                               unsigned long long *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    const uint64_t v = (uint64_t)chunk * 64 + lane;
    const bool valid = v < n_voxels;
    const MeshChunk &c = chunks[chunk];
    uint32_t e[6];   // -x, +x, -y, +y, -z, +z
    e[0] = e[1] = e[2] = e[3] = e[4] = e[5] = kNoEdge;
    if (valid) {
        e[1] = flow_edge(c, lane, 0, n_vertices);
        e[3] = flow_edge(c, lane, 1, n_vertices);
        e[5] = flow_edge(c, lane, 2, n_vertices);
        if (lane > 0) e[0] = flow_edge(c, lane - 1, 0, n_vertices);
        else if (chunk > 0) e[0] = flow_edge(chunks[chunk - 1], 63, 0, n_vertices);
        if (v >= W) e[2] = flow_edge(chunks[(v - W) >> 6], (uint32_t)(v - W) & 63u, 1, n_vertices);
        if (v >= plane) e[4] = flow_edge(chunks[(v - plane) >> 6], (uint32_t)(v - plane) & 63u, 2, n_vertices);
    }
    const bool used = (e[0] & e[1] & e[2] & e[3] & e[4] & e[5]) != kNoEdge;
    if (!__any(used)) return;   // no surface near this chunk: the cost follows the surface, not the grid

    uint2 r[6];
#pragma unroll
    for (int j = 0; j < 6; j++) r[j] = e[j] != kNoEdge ? vertex[e[j]] : make_uint2(kNoPixel, 0u);
    uint32_t count = 0;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    bool any = false;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        count += r[j].y;
        if (r[j].x != kNoPixel) {
            const float m = (float)r[j].y;
            const float *f = flow + (size_t)r[j].x * 3;
            ax = ax + m * f[0];
            ay = ay + m * f[1];
            az = az + m * f[2];
            any = true;
        }
    }
    if (any) {   // (count >= the multiplicity of a used edge >= 1)
        const float s = 1.0f / (float)count;
        float *t = nodes[v].translation;
        t[0] = t[0] + s * ax;
        t[1] = t[1] + s * ay;
        t[2] = t[2] + s * az;
    }
    const uint64_t moved = __ballot(any);
    if (lane == 0 && moved) atomicAdd(counts + 1, (unsigned long long)__popcll(moved));
}

}  // namespace tsdf

using namespace tsdf;

namespace {

bool all_finite(const float *a, int n) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(a[i])) return false;
    return true;
}

// Everything the host can refuse, before any device work.
int scene_flow_check(const tsdf_volume *v, const tsdf_mesh *m, const void *depth, const void *flow, uint32_t width, uint32_t height, const float *pose,
                     const float *inv_pose, const float *k, const float *kinv, float threshold, uint32_t flags) {
    TSDF_REQUIRE(v && m && depth && flow && pose && inv_pose && k && kinv, "tsdf_volume_apply_scene_flow: null argument");
    TSDF_REQUIRE((flags & ~(uint32_t)TSDF_SCENE_FLOW_DEFORMED) == 0, "tsdf_volume_apply_scene_flow: unknown flags %#x", flags);
    TSDF_REQUIRE(!v->slab && v->z_begin == 0 && v->z_end == v->g.Z, "tsdf_volume_apply_scene_flow: a Z-slab volume (tsdf_volume_create_slab) is not supported");
    TSDF_REQUIRE(v->device == m->device, "tsdf_volume_apply_scene_flow: the mesh was created on device %d, the volume on device %d", m->device, v->device);
    TSDF_REQUIRE(width >= 1 && height >= 1 && (uint64_t)width * height < kNoPixel, "tsdf_volume_apply_scene_flow: a %u x %u image", width, height);
    TSDF_REQUIRE(all_finite(pose, 16) && all_finite(inv_pose, 16) && all_finite(k, 9) && all_finite(kinv, 9),
                 "tsdf_volume_apply_scene_flow: a matrix has a non-finite entry");
    TSDF_REQUIRE(threshold > 0.0f, "tsdf_volume_apply_scene_flow: the threshold is not > 0");   // (NaN is not)
    TSDF_REQUIRE(m->grid[0] == v->g.X && m->grid[1] == v->g.Y && m->grid[2] == v->g.Z,
                 "tsdf_volume_apply_scene_flow: the mesh is not an extraction of the whole grid of a %u x %u x %u volume (tsdf_volume_extract_mesh with a NULL box)",
                 v->g.X, v->g.Y, v->g.Z);
    return TSDF_OK;
}

int apply_scene_flow(tsdf_volume *v, tsdf_mesh *m, const uint16_t *depth, const float *flow, uint32_t width, uint32_t height, const float *pose,
                     const float *inv_pose, const float *k, const float *kinv, float threshold, uint32_t flags, tsdf_scene_flow_info *info,
                     hipStream_t stream) {
    if (info) memset(info, 0, sizeof(*info));
    const uint64_t n_vertices = m->info.n_vertices, n_indices = m->info.n_indices;
    if (n_vertices == 0) return TSDF_OK;   // an empty mesh: nothing corresponds, nothing is allocated or launched
    const uint64_t n_voxels = (uint64_t)v->g.X * v->g.Y * v->g.Z;
    const uint32_t n_chunks = (uint32_t)((n_voxels + 63) / 64);
    TSDF_REQUIRE(n_chunks <= m->chunks_cap, "tsdf_volume_apply_scene_flow: the mesh handle does not hold the records of this grid");
    TSDF_REQUIRE(!(flags & TSDF_SCENE_FLOW_DEFORMED) || n_vertices <= (uint64_t)INT_MAX,
                 "tsdf_volume_apply_scene_flow: TSDF_SCENE_FLOW_DEFORMED with more than 2^31 - 1 vertices");
    // side effects of set_deformation: the node array exists, a brick list prepared ahead is void
    tsdf_deformation_node *nodes = nullptr;
    const int rcn = tsdf_volume_deformation(v, &nodes);
    if (rcn != TSDF_OK) return rcn;
    v->prepared_valid = 0;

    hipError_t e = device_reserve(m->flow_vertex, m->flow_vertex_cap, (size_t)n_vertices);
    if (e == hipSuccess && (flags & TSDF_SCENE_FLOW_DEFORMED)) e = device_reserve(m->flow_points, m->flow_points_cap, (size_t)n_vertices * 3);
    if (e == hipSuccess && !m->flow_counts) e = hipMalloc((void **)&m->flow_counts, 2 * sizeof(uint64_t));
    if (e == hipSuccess && !m->flow_totals) e = hipHostMalloc((void **)&m->flow_totals, 2 * sizeof(uint64_t), hipHostMallocDefault);
    if (e != hipSuccess) return hip_fail(e, "scene flow scratch alloc failed");

    const int rcj = mesh_join(m, stream);   // the extraction's kernels
    if (rcj != TSDF_OK) return rcj;
    const float *points = m->vertices;
    if (flags & TSDF_SCENE_FLOW_DEFORMED) {
        TSDF_HIP(hipMemcpyAsync(m->flow_points, m->vertices, (size_t)n_vertices * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream), "scene flow vertices copy");
        const int rcd = deform_points_on(v, (int)n_vertices, m->flow_points, stream);
        if (rcd != TSDF_OK) return rcd;
        points = m->flow_points;
    }
    TSDF_HIP(hipMemsetAsync(m->flow_counts, 0, 2 * sizeof(uint64_t), stream), "scene flow counters");
    Mat44 mp, mip;
    Mat33 mk, mkinv;
    memcpy(&mp, pose, sizeof(mp));
    memcpy(&mip, inv_pose, sizeof(mip));
    memcpy(&mk, k, sizeof(mk));
    memcpy(&mkinv, kinv, sizeof(mkinv));
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(m->flow_counts);
    const uint32_t nv = (uint32_t)n_vertices;
    hipLaunchKernelGGL(scene_flow_match_kernel, dim3((nv + 255) / 256), dim3(256), 0, stream, points, nv, depth, flow, width, height, mp, mip, mk, mkinv,
                       threshold, m->flow_vertex, counts);
    const uint64_t index_blocks = (n_indices + 255) / 256;
    hipLaunchKernelGGL(scene_flow_multiplicity_kernel, dim3((unsigned)(index_blocks < 8192 ? index_blocks : 8192)), dim3(256), 0, stream, m->indices,
                       n_indices, nv, m->flow_vertex);
    hipLaunchKernelGGL(scene_flow_apply_kernel, dim3((n_chunks + 3) / 4), dim3(256), 0, stream, m->chunks, n_chunks, n_voxels, (uint64_t)v->g.X,
                       (uint64_t)v->g.X * v->g.Y, m->flow_vertex, nv, flow, nodes, counts);
    TSDF_HIP(hipGetLastError(), "scene flow kernels failed");
    // later extractions into the handle (they overwrite the records and the arrays) are ordered behind these launches
    const int rcl = mesh_leave(m, stream);
    if (rcl != TSDF_OK) return rcl;
    if (!info) return TSDF_OK;
    TSDF_HIP(hipMemcpyAsync(m->flow_totals, m->flow_counts, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "scene flow counts download");
    TSDF_HIP(hipStreamSynchronize(stream), "scene flow");   // the one synchronisation
    info->n_vertices = n_vertices;
    info->n_correspondences = m->flow_totals[0];
    info->n_nodes_moved = m->flow_totals[1];
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_volume_apply_scene_flow_device(tsdf_volume *v, tsdf_mesh *m, const uint16_t *device_depth, const float *device_flow, uint32_t width,
                                        uint32_t height, const float pose[16], const float inv_pose[16], const float k[9], const float kinv[9],
                                        float threshold, uint32_t flags, tsdf_scene_flow_info *info, void *hip_stream) {
    const int rc = scene_flow_check(v, m, device_depth, device_flow, width, height, pose, inv_pose, k, kinv, threshold, flags);
    if (rc != TSDF_OK) return rc;
    return apply_scene_flow(v, m, device_depth, device_flow, width, height, pose, inv_pose, k, kinv, threshold, flags, info, (hipStream_t)hip_stream);
}

int tsdf_volume_apply_scene_flow(tsdf_volume *v, tsdf_mesh *m, const uint16_t *host_depth, const float *host_flow, uint32_t width, uint32_t height,
                                 const float pose[16], const float inv_pose[16], const float k[9], const float kinv[9], float threshold,
                                 uint32_t flags, tsdf_scene_flow_info *info) {
    const int rc = scene_flow_check(v, m, host_depth, host_flow, width, height, pose, inv_pose, k, kinv, threshold, flags);
    if (rc != TSDF_OK) return rc;
    if (m->info.n_vertices == 0) {
        if (info) memset(info, 0, sizeof(*info));
        return TSDF_OK;
    }
    const size_t pixels = (size_t)width * height;
    hipError_t e = device_reserve(m->flow_depth, m->flow_depth_cap, pixels);
    if (e == hipSuccess) e = device_reserve(m->flow_image, m->flow_image_cap, pixels * 3);
    if (e != hipSuccess) return hip_fail(e, "scene flow image alloc failed");
    TSDF_HIP(hipMemcpyAsync(m->flow_depth, host_depth, pixels * sizeof(uint16_t), hipMemcpyHostToDevice, v->stream), "scene flow depth upload");
    TSDF_HIP(hipMemcpyAsync(m->flow_image, host_flow, pixels * 3 * sizeof(float), hipMemcpyHostToDevice, v->stream), "scene flow upload");
    const int rca = apply_scene_flow(v, m, m->flow_depth, m->flow_image, width, height, pose, inv_pose, k, kinv, threshold, flags, info, v->stream);
    // (the host arrays are the caller's again on return, with or without info)
    if (rca == TSDF_OK && !info) TSDF_HIP(hipStreamSynchronize(v->stream), "scene flow");
    return rca;
}

}  // extern "C"
