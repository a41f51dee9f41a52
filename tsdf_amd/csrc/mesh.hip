// Indexed mesh extraction on the device (include/tsdf_amd.h, "indexed mesh"): marching cubes whose output is one
// vertex per lattice edge the surface crosses plus one index per vertex of tsdf_volume_marching_cubes' triangle soup, such that
// vertices[indices[k]] is the soup's k-th vertex bit for bit.
//
// Why that is possible: all twelve cube edges run in the positive direction of an axis (kMeshEdge below, from the reference's corner
// and edge numbering, src/MarchingCubes/MarkAndSweepMC.cu:9-36 / :80-97), corner positions are a function of the absolute voxel
// coordinate only, and interpolate() (:47-63) orders its end points by sign -- so every cube that touches a lattice edge computes the
// same 12 bytes for the crossing on it, and a configuration uses exactly its sign-changing edges.  Welding is by lattice edge, never
// by position.
//
// The voxels of the marched box's CLOSED range (one more than its cubes per axis) are numbered x fastest, then y, then z, and cut
// into chunks of 64: one wave per chunk, lanes along the numbering (so along x, coalesced, wherever a row is long enough).  A chunk's
// record holds three 64-bit masks -- which of its voxels have a used edge towards +x, +y, +z -- and two bases:
//   mesh_edges_kernel      the masks (three __ballot), the chunk's vertex count (their popcount) and its soup-vertex count
//   mesh_scan_*_kernel     exclusive scans of both counts over the chunks (mesh_scan.hip)
//   mesh_vertices_kernel   every used edge writes its vertex at
//                              base + popcount of the three masks below its lane + (axis > 0: x-bit) + (axis > 1: y-bit)
//                          which is the order of the key ((z Y + y) X + x) 3 + axis: no per-edge index array is ever stored
//   mesh_triangles_kernel  the cube walk of mc_rows_kernel; for each table entry the index of its edge by the same formula, from
//                          the record of the chunk the edge's lower voxel lies in
// Nothing depends on the order in which waves finish: no atomics, every output word has one writer.
#include <cstring>
#include <new>

#include "common.hpp"
#include "mesh_device.hpp"
#include "mesh_handle.hpp"

namespace tsdf {

// the marched cubes [x0, x0 + bx) x [y0, y0 + by) x [z0, z0 + bz), all three counts >= 1, inside a grid of X x Y x Z voxels
struct MeshBox {
    uint32_t x0, y0, z0, bx, by, bz;
    uint32_t X, Y;
    uint64_t n_voxels;     // (bx + 1) (by + 1) (bz + 1): the closed range
};

// cube edge e: the offset of its lower end from the cube's root voxel and its axis (MarkAndSweepMC.cu:80-97 with :291-302)
__constant__ uint8_t kMeshEdge[12][4] = {{0, 0, 1, 0}, {1, 0, 0, 2}, {0, 0, 0, 0}, {0, 0, 0, 2}, {0, 1, 1, 0}, {1, 1, 0, 2},
                                         {0, 1, 0, 0}, {0, 1, 0, 2}, {0, 0, 1, 1}, {1, 0, 1, 1}, {1, 0, 0, 1}, {0, 0, 0, 1}};

// The voxel a lane of chunk `chunk` owns, relative to the box's first voxel; false past the range's end.
__device__ inline bool mesh_voxel(const MeshBox &b, uint32_t chunk, uint32_t lane, uint32_t &rx, uint32_t &ry, uint32_t &rz) {
    const uint32_t W = b.bx + 1, H = b.by + 1;
    const uint64_t first = (uint64_t)chunk * 64;
    uint32_t rx0, ry0, rz0;
    if (b.n_voxels <= 0xffffffffull) {
        const uint32_t plane = W * H, f = (uint32_t)first;
        rz0 = f / plane;
        const uint32_t rem = f - rz0 * plane;
        ry0 = rem / W;
        rx0 = rem - ry0 * W;
    } else {
        const uint64_t plane = (uint64_t)W * H;
        rz0 = (uint32_t)(first / plane);
        const uint64_t rem = first - rz0 * plane;
        ry0 = (uint32_t)(rem / W);
        rx0 = (uint32_t)(rem - (uint64_t)ry0 * W);
    }
    const uint32_t t = rx0 + lane, q = t / W;   // (W >= 2: at most 32 rows further)
    rx = t - q * W;
    const uint32_t u = ry0 + q, q2 = u / H;
    ry = u - q2 * H;
    rz = rz0 + q2;
    return first + lane < b.n_voxels;
}

// The configuration of the cube rooted at dist[base] (bit i: corner i negative, MarkAndSweepMC.cu:110-124).
__device__ inline int mesh_cube_type(const float *__restrict__ dist, size_t base, size_t dy, size_t dz) {
    return (dist[base + dz] < 0) | (dist[base + 1 + dz] < 0) << 1 | (dist[base + 1] < 0) << 2 | (dist[base] < 0) << 3 |
           (dist[base + dy + dz] < 0) << 4 | (dist[base + 1 + dy + dz] < 0) << 5 | (dist[base + 1 + dy] < 0) << 6 | (dist[base + dy] < 0) << 7;
}

// An edge is used when its ends differ in d < 0 and one of the cubes round it is marched: for the voxels of the closed range
// that is "the edge's upper end is in the range too".
__global__ __launch_bounds__(256) void mesh_edges_kernel(const float *__restrict__ dist, const MeshBox b, const MeshTable *__restrict__ table,
                                                         uint32_t n_chunks, MeshChunk *__restrict__ chunks) {
    __shared__ uint8_t count[256];
    count[threadIdx.x] = table->count[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    uint32_t rx, ry, rz;
    const bool valid = mesh_voxel(b, chunk, lane, rx, ry, rz);
    const size_t dy = b.X, dz = (size_t)b.X * b.Y;
    const size_t base = (size_t)(b.x0 + rx) + (b.y0 + ry) * dy + (b.z0 + rz) * dz;
    const bool hx = valid && rx < b.bx, hy = valid && ry < b.by, hz = valid && rz < b.bz;
    const bool s = valid && dist[base] < 0;
    const uint64_t mx = __ballot(hx && (dist[base + 1] < 0) != s);
    const uint64_t my = __ballot(hy && (dist[base + dy] < 0) != s);
    const uint64_t mz = __ballot(hz && (dist[base + dz] < 0) != s);
    uint32_t n = 0;
    if (hx && hy && hz) n = count[mesh_cube_type(dist, base, dy, dz)];
    n = wave_inclusive_sum(n, lane);
    if (lane == 63) {
        MeshChunk c;
        c.mx = mx;
        c.my = my;
        c.mz = mz;
        c.vbase = (uint32_t)(__popcll(mx) + __popcll(my) + __popcll(mz));
        c.ibase = n;
        chunks[chunk] = c;
    }
}

// interpolate (MarkAndSweepMC.cu:47-63) between the centres of voxel (x, y, z) and its neighbour along AXIS, the arithmetic of
// mc_rows_kernel operation for operation (centre_of_voxel_at, src/TSDF/TSDF_utilities.cu:10-17; the swap by sign; three components)
template <int AXIS>
__device__ inline void mesh_write_vertex(float *__restrict__ dst, uint32_t x, uint32_t y, uint32_t z, float w0, float w1, const F3 &vs, const F3 &offset) {
    float3 v0, v1;
    v0.x = ((int)x + 0.5f) * vs.x + offset.x;
    v0.y = ((int)y + 0.5f) * vs.y + offset.y;
    v0.z = ((int)z + 0.5f) * vs.z + offset.z;
    v1.x = ((int)(x + (AXIS == 0)) + 0.5f) * vs.x + offset.x;
    v1.y = ((int)(y + (AXIS == 1)) + 0.5f) * vs.y + offset.y;
    v1.z = ((int)(z + (AXIS == 2)) + 0.5f) * vs.z + offset.z;
    if ((w0 > 0) && (w1 < 0)) {
        const float tw = w0; w0 = w1; w1 = tw;
        const float3 tv = v0; v0 = v1; v1 = tv;
    }
    const float ratio = -(w0) / (w1 - w0);
    dst[0] = (ratio * (v1.x - v0.x)) + v0.x;
    dst[1] = (ratio * (v1.y - v0.y)) + v0.y;
    dst[2] = (ratio * (v1.z - v0.z)) + v0.z;
}

__global__ __launch_bounds__(256) void mesh_vertices_kernel(const float *__restrict__ dist, const MeshBox b, F3 vs, F3 offset, uint32_t n_chunks,
                                                            const MeshChunk *__restrict__ chunks, float *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    const MeshChunk c = chunks[chunk];
    const uint32_t ex = (uint32_t)(c.mx >> lane) & 1u, ey = (uint32_t)(c.my >> lane) & 1u, ez = (uint32_t)(c.mz >> lane) & 1u;
    if (!(ex | ey | ez)) return;
    uint32_t rx, ry, rz;
    (void)mesh_voxel(b, chunk, lane, rx, ry, rz);   // (a set bit is a voxel of the range)
    const size_t dy = b.X, dz = (size_t)b.X * b.Y;
    const uint32_t x = b.x0 + rx, y = b.y0 + ry, z = b.z0 + rz;
    const size_t base = (size_t)x + y * dy + z * dz;
    const uint64_t below = (1ull << lane) - 1;
    const float w = dist[base];
    float *dst = out + (size_t)(c.vbase + __popcll(c.mx & below) + __popcll(c.my & below) + __popcll(c.mz & below)) * 3;
    if (ex) mesh_write_vertex<0>(dst, x, y, z, w, dist[base + 1], vs, offset);
    if (ey) mesh_write_vertex<1>(dst + 3 * ex, x, y, z, w, dist[base + dy], vs, offset);
    if (ez) mesh_write_vertex<2>(dst + 3 * (ex + ey), x, y, z, w, dist[base + dz], vs, offset);
}

__global__ __launch_bounds__(256) void mesh_triangles_kernel(const float *__restrict__ dist, const MeshBox b, const MeshTable *__restrict__ table,
                                                             uint32_t n_chunks, const MeshChunk *__restrict__ chunks, uint32_t *__restrict__ out) {
    __shared__ uint8_t count[256];
    count[threadIdx.x] = table->count[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    uint32_t rx, ry, rz;
    const bool valid = mesh_voxel(b, chunk, lane, rx, ry, rz);
    const size_t dy = b.X, dz = (size_t)b.X * b.Y;
    const bool cube = valid && rx < b.bx && ry < b.by && rz < b.bz;
    int type = 0;
    if (cube) type = mesh_cube_type(dist, (size_t)(b.x0 + rx) + (b.y0 + ry) * dy + (b.z0 + rz) * dz, dy, dz);
    const uint32_t n = cube ? count[type] : 0u;
    const uint32_t incl = wave_inclusive_sum(n, lane);
    if (n == 0) return;
    const uint64_t W = b.bx + 1, plane = W * (b.by + 1), lin = (uint64_t)chunk * 64 + lane;
    uint32_t *dst = out + (size_t)chunks[chunk].ibase + (incl - n);
    for (uint32_t i = 0; i < n; i++) {
        const int e = table->tri[type][i];
        // the edge's lower voxel: in the closed range because the cube is marched
        const uint64_t at = lin + kMeshEdge[e][0] + kMeshEdge[e][1] * W + kMeshEdge[e][2] * plane;
        const uint32_t axis = kMeshEdge[e][3], l = (uint32_t)at & 63u;
        const MeshChunk c = chunks[at >> 6];
        const uint64_t below = (1ull << l) - 1;
        uint32_t index = c.vbase + __popcll(c.mx & below) + __popcll(c.my & below) + __popcll(c.mz & below);
        if (axis > 0) index += (uint32_t)(c.mx >> l) & 1u;
        if (axis > 1) index += (uint32_t)(c.my >> l) & 1u;
        dst[i] = index;
    }
}

}  // namespace tsdf

using namespace tsdf;

namespace {

void mesh_free(tsdf_mesh *m) {
    m->destroy();
    device_free_all(m->vertices, m->indices, m->normals, m->rgb, m->chunks, m->parts, m->table, m->labels, m->sizes, m->component_words,
                    m->keep_masks, m->keep_bases, m->cell_keys, m->cell_reps, m->cluster_of, m->cluster_sums, m->row_begin, m->row_end, m->rows,
                    m->smooth_positions, m->pinned, m->normal_sums, m->flow_vertex, m->flow_points, m->flow_counts, m->flow_depth, m->flow_image);
    (void)hipHostFree(m->flow_totals);
    (void)hipHostFree(m->totals);
    delete m;
}

}  // namespace

extern "C" {

int tsdf_mesh_create(tsdf_mesh **out) {
    TSDF_REQUIRE(out, "tsdf_mesh_create: null argument");
    *out = nullptr;
    tsdf_mesh *m = new (std::nothrow) tsdf_mesh();
    if (!m) {
        set_error("out of host memory");
        return TSDF_ERR_NOMEM;
    }
    std::memset(m, 0, sizeof(*m));
    hipError_t e = m->create();
    if (e == hipSuccess) e = hipMalloc((void **)&m->table, sizeof(MeshTable));
    if (e == hipSuccess) e = hipHostMalloc((void **)&m->totals, 2 * sizeof(uint64_t), hipHostMallocDefault);
    if (e != hipSuccess) {
        mesh_free(m);
        return hip_fail(e, "mesh alloc failed");
    }
    *out = m;
    return TSDF_OK;
}

void tsdf_mesh_destroy(tsdf_mesh *m) {
    if (m) mesh_free(m);
}

int tsdf_volume_extract_mesh(const tsdf_volume *cv, const int8_t *table, const uint32_t box[6], uint32_t flags, tsdf_mesh *m) {
    TSDF_REQUIRE(cv && table && m, "tsdf_volume_extract_mesh: null argument");
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);
    const Geom &g = v->g;
    TSDF_REQUIRE((flags & ~(uint32_t)(TSDF_MESH_NORMALS | TSDF_MESH_COLOURS)) == 0, "tsdf_volume_extract_mesh: unknown flags %#x", flags);
    TSDF_REQUIRE(!v->slab, "tsdf_volume_extract_mesh: a Z-slab volume (tsdf_volume_create_slab) is not supported; tsdf_volume_marching_cubes is");
    TSDF_REQUIRE(v->device == m->device, "tsdf_volume_extract_mesh: the mesh was created on device %d, the volume on device %d", m->device, v->device);
    TSDF_REQUIRE(!(flags & TSDF_MESH_COLOURS) || v->colour, "tsdf_volume_extract_mesh: TSDF_MESH_COLOURS on a volume without colour (tsdf_volume_enable_colour)");
    MeshTable t;
    memset(&t, 0, sizeof(t));
    for (int c = 0; c < 256; c++) {   // the rules of tsdf_volume_marching_cubes
        int n = 0;
        while (n < 32 && table[c * 32 + n] >= 0) {
            TSDF_REQUIRE(table[c * 32 + n] < 12, "tsdf_volume_extract_mesh: bad edge number in the table");
            t.tri[c][n] = table[c * 32 + n];
            n++;
        }
        TSDF_REQUIRE(n % 3 == 0, "tsdf_volume_extract_mesh: a configuration's vertices are not whole triangles");
        for (int i = n; i < 32; i++) t.tri[c][i] = -1;
        t.count[c] = (uint8_t)n;
    }
    const uint32_t last[3] = {g.X ? g.X - 1 : 0, g.Y ? g.Y - 1 : 0, g.Z ? g.Z - 1 : 0};   // cubes per axis
    uint32_t lo[3] = {0, 0, 0}, hi[3] = {last[0], last[1], last[2]};
    if (box) {
        for (int a = 0; a < 3; a++) {
            TSDF_REQUIRE(box[a] < box[a + 3], "tsdf_volume_extract_mesh: the box's begin (%u) is not below its end (%u) on axis %d", box[a], box[a + 3], a);
            lo[a] = box[a];
            hi[a] = box[a + 3] < last[a] ? box[a + 3] : last[a];
        }
    }
    const int rcj = mesh_join(m, v->stream);   // what a previous extraction into this handle left in flight
    if (rcj != TSDF_OK) return rcj;
    m->info.n_vertices = m->info.n_indices = 0;
    m->labelled = 0;   // (mesh_components.hip)
    m->info.flags = flags;
    for (int a = 0; a < 3; a++) {
        m->info.box[a] = lo[a];
        m->info.box[a + 3] = hi[a] > lo[a] ? hi[a] : lo[a];
    }
    // (scene_flow.hip) the whole grid: what follows leaves the records of every voxel, or an empty mesh
    const bool whole = lo[0] == 0 && lo[1] == 0 && lo[2] == 0 && hi[0] == last[0] && hi[1] == last[1] && hi[2] == last[2];
    m->grid[0] = whole ? g.X : 0;
    m->grid[1] = whole ? g.Y : 0;
    m->grid[2] = whole ? g.Z : 0;
    if (!(lo[0] < hi[0] && lo[1] < hi[1] && lo[2] < hi[2])) return TSDF_OK;   // clipped to nothing, or an axis shorter than 2

    MeshBox b;
    b.x0 = lo[0]; b.y0 = lo[1]; b.z0 = lo[2];
    b.bx = hi[0] - lo[0]; b.by = hi[1] - lo[1]; b.bz = hi[2] - lo[2];
    b.X = g.X; b.Y = g.Y;
    b.n_voxels = (uint64_t)(b.bx + 1) * (b.by + 1) * (b.bz + 1);
    const uint64_t n_chunks64 = (b.n_voxels + 63) / 64;
    TSDF_REQUIRE(n_chunks64 < (1ull << 32), "tsdf_volume_extract_mesh: the box holds too many voxels");
    const uint32_t n_chunks = (uint32_t)n_chunks64, n_parts = mesh_scan_parts(n_chunks);
    hipError_t e = device_reserve(m->chunks, m->chunks_cap, (size_t)n_chunks);
    if (e == hipSuccess) e = device_reserve(m->parts, m->parts_cap, 2 * ((size_t)n_parts + 1));
    if (e == hipSuccess && (!m->table_valid || memcmp(&t, &m->host_table, sizeof(t)) != 0)) {
        m->table_valid = 0;
        // (host_table outlives the copy; a handle is used by one thread at a time, and the stream waited for `done` above)
        TSDF_HIP(hipStreamSynchronize(v->stream), "mesh table upload");
        memcpy(&m->host_table, &t, sizeof(t));
        e = hipMemcpyAsync(m->table, &m->host_table, sizeof(t), hipMemcpyHostToDevice, v->stream);
        if (e == hipSuccess) m->table_valid = 1;
    }
    if (e != hipSuccess) return hip_fail(e, "mesh scratch alloc failed");
    const float *dist = v->dist - (size_t)g.z_store_begin * g.X * g.Y;   // (z_store_begin is 0: no slab here)
    const dim3 grid((n_chunks + 3) / 4);
    hipLaunchKernelGGL(mesh_edges_kernel, grid, dim3(256), 0, v->stream, dist, b, m->table, n_chunks, m->chunks);
    mesh_scan(ChunkCounts{m->chunks, n_chunks}, n_parts, m->parts, v->stream);
    TSDF_HIP(hipGetLastError(), "mesh count kernels failed");
    TSDF_HIP(hipMemcpyAsync(m->totals, m->parts + 2 * (size_t)n_parts, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, v->stream), "mesh counts download");
    TSDF_HIP(hipStreamSynchronize(v->stream), "mesh count");   // the one synchronisation: the arrays are sized from the counts
    const uint64_t n_vertices = m->totals[0], n_indices = m->totals[1];
    TSDF_REQUIRE(n_vertices <= 0xffffffffull && n_indices <= 0xffffffffull,
                 "tsdf_volume_extract_mesh: %llu vertices and %llu indices do not fit 32-bit indices: extract the volume in boxes",
                 (unsigned long long)n_vertices, (unsigned long long)n_indices);
    if (n_vertices == 0) return TSDF_OK;   // (no vertex, so no index either)
    e = device_reserve(m->vertices, m->vertices_cap, (size_t)n_vertices * 3);
    if (e == hipSuccess) e = device_reserve(m->indices, m->indices_cap, (size_t)n_indices);
    if (e == hipSuccess && (flags & TSDF_MESH_NORMALS)) e = device_reserve(m->normals, m->normals_cap, (size_t)n_vertices * 3);
    if (e == hipSuccess && (flags & TSDF_MESH_COLOURS)) e = device_reserve(m->rgb, m->rgb_cap, (size_t)n_vertices * 3);
    if (e != hipSuccess) return hip_fail(e, "mesh array alloc failed");
    hipLaunchKernelGGL(mesh_vertices_kernel, grid, dim3(256), 0, v->stream, dist, b, g.vs, g.offset, n_chunks, m->chunks, m->vertices);
    hipLaunchKernelGGL(mesh_triangles_kernel, grid, dim3(256), 0, v->stream, dist, b, m->table, n_chunks, m->chunks, m->indices);
    TSDF_HIP(hipGetLastError(), "mesh emit kernels failed");
    int rc = TSDF_OK;
    if (flags & TSDF_MESH_NORMALS)
        rc = tsdf_volume_sample_field_device(cv, n_vertices, m->vertices, nullptr, m->normals, nullptr, TSDF_FIELD_UNIT_GRADIENT, v->stream);
    if (rc == TSDF_OK && (flags & TSDF_MESH_COLOURS)) rc = tsdf_volume_sample_colours_device(cv, n_vertices, m->vertices, m->rgb, v->stream);
    const int rcl = mesh_leave(m, v->stream);
    if (rcl != TSDF_OK) return rcl;
    if (rc != TSDF_OK) return rc;
    m->info.n_vertices = n_vertices;
    m->info.n_indices = n_indices;
    return TSDF_OK;
}

int tsdf_mesh_get_info(const tsdf_mesh *m, tsdf_mesh_info *info) {
    TSDF_REQUIRE(m && info, "tsdf_mesh_get_info: null argument");
    *info = m->info;
    return TSDF_OK;
}

int tsdf_mesh_buffers(const tsdf_mesh *m, const float **device_vertices, const uint32_t **device_indices, const float **device_normals,
                      const uint8_t **device_rgb) {
    TSDF_REQUIRE(m, "tsdf_mesh_buffers: null mesh");
    const int rc = mesh_wait(m);
    if (rc != TSDF_OK) return rc;
    const bool any = m->info.n_vertices != 0;
    if (device_vertices) *device_vertices = any ? m->vertices : nullptr;
    if (device_indices) *device_indices = any ? m->indices : nullptr;
    if (device_normals) *device_normals = any && (m->info.flags & TSDF_MESH_NORMALS) ? m->normals : nullptr;
    if (device_rgb) *device_rgb = any && (m->info.flags & TSDF_MESH_COLOURS) ? m->rgb : nullptr;
    return TSDF_OK;
}

int tsdf_mesh_download(const tsdf_mesh *m, float *host_vertices, uint32_t *host_indices, float *host_normals, uint8_t *host_rgb) {
    TSDF_REQUIRE(m, "tsdf_mesh_download: null mesh");
    TSDF_REQUIRE(!host_normals || (m->info.flags & TSDF_MESH_NORMALS), "tsdf_mesh_download: the mesh was extracted without TSDF_MESH_NORMALS");
    TSDF_REQUIRE(!host_rgb || (m->info.flags & TSDF_MESH_COLOURS), "tsdf_mesh_download: the mesh was extracted without TSDF_MESH_COLOURS");
    const int rc = mesh_wait(m);
    if (rc != TSDF_OK) return rc;
    const size_t nv = (size_t)m->info.n_vertices, ni = (size_t)m->info.n_indices;
    if (nv == 0) return TSDF_OK;
    if (host_vertices) TSDF_HIP(hipMemcpy(host_vertices, m->vertices, nv * 3 * sizeof(float), hipMemcpyDeviceToHost), "mesh download");
    if (host_indices) TSDF_HIP(hipMemcpy(host_indices, m->indices, ni * sizeof(uint32_t), hipMemcpyDeviceToHost), "mesh download");
    if (host_normals) TSDF_HIP(hipMemcpy(host_normals, m->normals, nv * 3 * sizeof(float), hipMemcpyDeviceToHost), "mesh download");
    if (host_rgb) TSDF_HIP(hipMemcpy(host_rgb, m->rgb, nv * 3, hipMemcpyDeviceToHost), "mesh download");
    return TSDF_OK;
}

int tsdf_mesh_scratch_bytes(const tsdf_mesh *m, uint64_t *bytes) {
    TSDF_REQUIRE(m && bytes, "tsdf_mesh_scratch_bytes: null argument");
    *bytes = (uint64_t)m->chunks_cap * sizeof(MeshChunk) + (uint64_t)m->parts_cap * sizeof(uint64_t) + sizeof(MeshTable) + 2 * sizeof(uint64_t) +
             // mesh components: labels and sizes, the labelling's words, the keep masks and bases of a filter into the handle
             (uint64_t)(m->labels_cap + m->sizes_cap) * sizeof(uint32_t) + (m->component_words ? kComponentWords * sizeof(uint64_t) : 0) +
             (uint64_t)m->keep_masks_cap * sizeof(uint64_t) + (uint64_t)m->keep_bases_cap * sizeof(uint32_t) +
             // mesh simplification: the cell table, the per-vertex cluster word and the per-cluster sums of a simplification into the handle
             (uint64_t)m->cell_keys_cap * sizeof(uint64_t) + (uint64_t)(m->cell_reps_cap + m->cluster_of_cap) * sizeof(uint32_t) +
             (uint64_t)m->cluster_sums_cap * sizeof(int64_t) +
             // mesh smoothing: the neighbour rows, the second position buffer, the pin flags, the normal sums (the pins' edge table is the cell table)
             (uint64_t)(m->row_begin_cap + m->row_end_cap) * sizeof(uint32_t) + (uint64_t)m->rows_cap * sizeof(uint2) +
             (uint64_t)m->smooth_positions_cap * sizeof(float) + (uint64_t)m->pinned_cap + (uint64_t)m->normal_sums_cap * sizeof(int64_t) +
             // scene flow: 8 bytes per vertex, 12 more with TSDF_SCENE_FLOW_DEFORMED, the two counts, the host variant's two images
             (uint64_t)m->flow_vertex_cap * sizeof(uint2) + (uint64_t)m->flow_points_cap * sizeof(float) + (m->flow_counts ? 2 * sizeof(uint64_t) : 0) +
             (uint64_t)m->flow_depth_cap * sizeof(uint16_t) + (uint64_t)m->flow_image_cap * sizeof(float);
    return TSDF_OK;
}

}  // extern "C"
