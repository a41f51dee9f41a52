// Mesh rendering: an indexed mesh rasterised from a pinhole camera into depth, vertex, normal, colour and triangle-id maps, on the
// device (include/tsdf_amd.h, "mesh rendering").  Decisions are integers (raster_index.hpp), values are fp32 with every
// operation rounded on its own, visibility is the minimum of a 64-bit key: every target is a unique set of bytes.
//   render_project_kernel   one lane per SHARED vertex: world -> camera -> screen once, one 16-byte record {X, Y, r, usable}
//   (memset)                the key buffer to all ones
//   render_raster_kernel    one lane per triangle: three 16-byte gathers, the live test, the box clipped to the image, then the walk over
//                           the box; a box of more pixels than the handle's threshold (TSDF_RENDER_LARGE_BOX, tsdf_render_set_large_box)
//                           goes to the large list instead (one ballot and one atomic per wave)
//   render_large_kernel     one wave per listed triangle, the lanes over the box in 8 x 8 tiles
//   render_resolve_kernel   one lane per pixel: the winner decoded, its barycentrics recomputed with rule 5's expressions, the targets
// Visibility: one 64-bit atomicMin without return per fragment, behind a plain load of the word and a skip when the fragment's key is
// not smaller.  A word only ever falls, so a stale value read is never smaller than the live one and a skip is always right; a needless
// atomic only costs time.  No float atomics, no compare-and-swap loop, no lane waits for another.
#include <cmath>

#include "common.hpp"
#include "handle_counters.hpp"
#include "handle_order.hpp"
#include "mesh_device.hpp"
#include "mesh_handle.hpp"
#include "raster_index.hpp"

namespace tsdf {

constexpr uint32_t kLargeGrid = 1024;   // workgroups of render_large_kernel, four waves each, striding over the list

// the counters and the error word, on the device and in the pinned mirror
enum { kWordError = 0, kWordLive, kWordDropped, kWordLarge, kWordHit, kRenderWords };

struct RenderView {
    Mat44 ip;
    float fx, fy, cx, cy;
    float z_near, z_far;
    uint32_t width, height;
    uint32_t flags;
};

struct RenderTargets {
    uint32_t *triangle;
    float *z;
    uint16_t *depth;
    float *vertices;
    float *normals;
    uint8_t *rgb;
};

__device__ inline bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// rules 1 and 2
__global__ __launch_bounds__(256) void render_project_kernel(uint32_t n_vertices, const float *__restrict__ vertices, const RenderView view,
                                                             int4 *__restrict__ records) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    const float x = vertices[3 * v], y = vertices[3 * v + 1], z = vertices[3 * v + 2];
    const Mat44 &ip = view.ip;
    // world_to_camera (cuda_coordinate_transforms.cu:108-121), division by w included
    float camx = ((ip.m11 * x + ip.m12 * y) + ip.m13 * z) + ip.m14;
    float camy = ((ip.m21 * x + ip.m22 * y) + ip.m23 * z) + ip.m24;
    float camz = ((ip.m31 * x + ip.m32 * y) + ip.m33 * z) + ip.m34;
    const float w = ((ip.m41 * x + ip.m42 * y) + ip.m43 * z) + ip.m44;
    camx /= w;
    camy /= w;
    camz /= w;
    const float r = 1.0f / camz;
    const float sx = view.fx * (camx / camz) + view.cx, sy = view.fy * (camy / camz) + view.cy;
    const bool usable = finite3(camx, camy, camz) && camz >= view.z_near && camz <= view.z_far && raster_in_range(sx) && raster_in_range(sy);
    records[v] = usable ? make_int4(raster_snap(sx), raster_snap(sy), (int)__float_as_uint(r), 1) : make_int4(0, 0, 0, 0);
}

// What a live triangle is rasterised from
struct RenderTriangle {
    RasterEdges e;
    RasterBox box;
    float r0, r1, r2;
};

enum { kTriangleDead = 0, kTriangleDropped, kTriangleBadIndex, kTriangleLive };

// Rule 3 for triangle t: its corners' records, the twice-area, the culling, the edges, the box.  A live triangle whose box holds no pixel
// centre is live and has `any` false.
__device__ inline int render_setup(uint32_t n_vertices, const uint32_t *__restrict__ indices, const int4 *__restrict__ records, const RenderView &view,
                                   uint64_t t, RenderTriangle &tri, bool &any) {
    uint32_t c[3];
    any = false;
    if (!load_triple(n_vertices, indices, t, c)) return kTriangleBadIndex;
    const int4 v0 = records[c[0]], v1 = records[c[2]], v2 = records[c[1]];   // extract_surface's wiring
    if (!(v0.w && v1.w && v2.w)) return kTriangleDropped;
    const RasterPoint p0 = {v0.x, v0.y}, p1 = {v1.x, v1.y}, p2 = {v2.x, v2.y};
    const int64_t area2 = raster_area2(p0, p1, p2);
    if (area2 == 0 || ((view.flags & TSDF_RENDER_CULL_BACK) && area2 > 0)) return kTriangleDead;   // front-facing: A2 < 0
    tri.e = raster_edges(p0, p1, p2, area2);
    tri.r0 = __uint_as_float((uint32_t)v0.z);
    tri.r1 = __uint_as_float((uint32_t)v1.z);
    tri.r2 = __uint_as_float((uint32_t)v2.z);
    any = raster_box(p0, p1, p2, view.width, view.height, tri.box);
    return kTriangleLive;
}

// rule 5
__device__ inline float render_depth(int64_t e1, int64_t e2, int64_t area, float r0, float r1, float r2, float &b1, float &b2) {
    b1 = (float)e1 / (float)area;
    b2 = (float)e2 / (float)area;
    const float rr = r0 + (b1 * (r1 - r0) + b2 * (r2 - r0));
    return 1.0f / rr;
}

// rule 6 for one covered pixel
__device__ inline void render_fragment(const RenderTriangle &tri, const RenderView &view, uint32_t t, uint32_t i, uint32_t j, int64_t e1, int64_t e2,
                                       unsigned long long *keys) {
    float b1, b2;
    const float z = render_depth(e1, e2, tri.e.area, tri.r0, tri.r1, tri.r2, b1, b2);
    if (!(isfinite(z) && z >= view.z_near && z <= view.z_far)) return;
    const unsigned long long key = (unsigned long long)__float_as_uint(z) << 32 | t;
    unsigned long long *word = keys + ((size_t)j * view.width + i);
    if (key < *word) __hip_atomic_fetch_min(word, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the lanes' flags counted by wave into the workgroup's LDS totals (block_counts_*, handle_counters.hpp)
__device__ inline void render_count(uint32_t *lds, uint32_t slot, bool flag) { block_counts_wave(lds, slot, (uint32_t)__popcll(__ballot(flag))); }

__global__ __launch_bounds__(256) void render_raster_kernel(uint32_t n_vertices, uint32_t n_triangles, const uint32_t *__restrict__ indices,
                                                            const int4 *__restrict__ records, const RenderView view, uint32_t large_box,
                                                            unsigned long long *keys, uint32_t *__restrict__ large_list, unsigned long long *words) {
    __shared__ uint32_t counts[kRenderWords];
    block_counts_clear(counts);
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    RenderTriangle tri;
    bool any = false;
    const int state = t < n_triangles ? render_setup(n_vertices, indices, records, view, t, tri, any) : kTriangleDead;
    const bool large = any && raster_box_pixels(tri.box) > large_box;
    render_count(counts, kWordError, state == kTriangleBadIndex);
    render_count(counts, kWordLive, state == kTriangleLive);
    render_count(counts, kWordDropped, state == kTriangleDropped);
    render_count(counts, kWordLarge, large);
    // the large list: one ballot and one atomic per wave; its order does not matter, the result is a minimum
    const uint64_t m = __ballot(large);
    if (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(large_list, (uint32_t)__popcll(m));   // [0]: the list's length
        base = __shfl(base, leader);
        if (large) large_list[1 + base + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = (uint32_t)t;
    }
    if (any && !large) {
        for (uint32_t j = tri.box.y0; j <= tri.box.y1; j++) {
            int64_t e0 = raster_edge_at(tri.e, 0, tri.box.x0, j), e1 = raster_edge_at(tri.e, 1, tri.box.x0, j), e2 = raster_edge_at(tri.e, 2, tri.box.x0, j);
            for (uint32_t i = tri.box.x0; i <= tri.box.x1; i++) {
                if (raster_covered(tri.e, e0, e1, e2)) render_fragment(tri, view, (uint32_t)t, i, j, e1, e2, keys);
                e0 += tri.e.a[0] * kRasterSubpixel;   // (integers: the same value as raster_edge_at at i + 1)
                e1 += tri.e.a[1] * kRasterSubpixel;
                e2 += tri.e.a[2] * kRasterSubpixel;
            }
        }
    }
    block_counts_flush(counts, [&](uint32_t k, uint32_t total) {
        if (k == kWordError) raise_error((uint64_t *)words + kWordError, kErrorIndex);
        else atomicAdd(words + k, (unsigned long long)total);
    });
}

// One wave per listed triangle.  Every index was checked by render_raster_kernel, which listed live triangles only.
__global__ __launch_bounds__(256) void render_large_kernel(uint32_t n_vertices, const uint32_t *__restrict__ indices, const int4 *__restrict__ records,
                                                           const RenderView view, unsigned long long *keys, const uint32_t *__restrict__ large_list) {
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
    const uint32_t listed = large_list[0];
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    for (uint32_t at = wave; at < listed; at += waves) {
        const uint32_t t = large_list[1 + at];
        RenderTriangle tri;
        bool any;
        if (render_setup(n_vertices, indices, records, view, t, tri, any) != kTriangleLive || !any) continue;
        for (uint32_t j0 = tri.box.y0; j0 <= tri.box.y1; j0 += 8)
            for (uint32_t i0 = tri.box.x0; i0 <= tri.box.x1; i0 += 8) {
                const uint32_t i = i0 + lx, j = j0 + ly;
                if (i > tri.box.x1 || j > tri.box.y1) continue;
                const int64_t e0 = raster_edge_at(tri.e, 0, i, j), e1 = raster_edge_at(tri.e, 1, i, j), e2 = raster_edge_at(tri.e, 2, i, j);
                if (raster_covered(tri.e, e0, e1, e2)) render_fragment(tri, view, t, i, j, e1, e2, keys);
            }
    }
}

// a0 + (q1 * (a1 - a0) + q2 * (a2 - a0))
__device__ inline float render_mix(float a0, float a1, float a2, float q1, float q2) { return a0 + (q1 * (a1 - a0) + q2 * (a2 - a0)); }

// n / sqrtf((n.x n.x + n.y n.y) + n.z n.z); a NaN triple when a component is not finite or the length is 0
__device__ inline void render_unit(float nx, float ny, float nz, float out[3]) {
    const float length = sqrtf((nx * nx + ny * ny) + nz * nz);
    const bool good = finite3(nx, ny, nz) && length != 0.0f;
    out[0] = good ? nx / length : NAN;
    out[1] = good ? ny / length : NAN;
    out[2] = good ? nz / length : NAN;
}

// rule 7
__global__ __launch_bounds__(256) void render_resolve_kernel(uint32_t n_pixels, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ indices,
                                                             const int4 *__restrict__ records, const float *__restrict__ vertices,
                                                             const float *__restrict__ normals, const uint8_t *__restrict__ rgb, const RenderView view,
                                                             const RenderTargets out, unsigned long long *words) {
    __shared__ uint32_t counts[kRenderWords];
    block_counts_clear(counts);
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool mine = p < n_pixels;
    const unsigned long long key = mine ? keys[p] : ~0ull;
    const bool hit = key != ~0ull;
    render_count(counts, kWordHit, hit);
    if (mine) {
        const uint32_t t = (uint32_t)key;
        const float z = hit ? __uint_as_float((uint32_t)(key >> 32)) : NAN;
        if (out.triangle) out.triangle[p] = t;   // (all ones on a miss)
        if (out.z) out.z[p] = z;
        if (out.depth) {
            const float r = roundf(z);   // tsdf_vertices_to_depth's conversion
            out.depth[p] = (r == r && r > 0.0f && r < 65536.0f) ? (uint16_t)r : (uint16_t)0;
        }
        if (out.vertices || out.normals || out.rgb) {
            float vert[3] = {NAN, NAN, NAN}, norm[3] = {NAN, NAN, NAN};
            uint8_t colour[3] = {0, 0, 0};
            if (hit) {
                // the winner's indices were checked by render_raster_kernel
                const uint32_t c0 = indices[3 * (size_t)t], c1 = indices[3 * (size_t)t + 2], c2 = indices[3 * (size_t)t + 1];
                const int4 v0 = records[c0], v1 = records[c1], v2 = records[c2];
                const RasterPoint p0 = {v0.x, v0.y}, p1 = {v1.x, v1.y}, p2 = {v2.x, v2.y};
                const RasterEdges e = raster_edges(p0, p1, p2, raster_area2(p0, p1, p2));
                const uint32_t i = (uint32_t)(p % view.width), j = (uint32_t)(p / view.width);
                const float b1 = (float)raster_edge_at(e, 1, i, j) / (float)e.area, b2 = (float)raster_edge_at(e, 2, i, j) / (float)e.area;
                const float q1 = (b1 * __uint_as_float((uint32_t)v1.z)) * z, q2 = (b2 * __uint_as_float((uint32_t)v2.z)) * z;
                const float *A = vertices + 3 * (size_t)c0, *B = vertices + 3 * (size_t)c1, *C = vertices + 3 * (size_t)c2;
                for (int a = 0; a < 3; a++) vert[a] = render_mix(A[a], B[a], C[a], q1, q2);
                if (out.normals) {
                    if (normals) {
                        const float *na = normals + 3 * (size_t)c0, *nb = normals + 3 * (size_t)c1, *nc = normals + 3 * (size_t)c2;
                        render_unit(render_mix(na[0], nb[0], nc[0], q1, q2), render_mix(na[1], nb[1], nc[1], q1, q2), render_mix(na[2], nb[2], nc[2], q1, q2),
                                    norm);
                    } else {
                        // cross(V1 - V0, V2 - V0) of the wired triangle: out of a fused surface
                        const float ux = B[0] - A[0], uy = B[1] - A[1], uz = B[2] - A[2], wx = C[0] - A[0], wy = C[1] - A[1], wz = C[2] - A[2];
                        render_unit(uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx, norm);
                    }
                }
                if (out.rgb) {
                    const uint8_t *ca = rgb + 3 * (size_t)c0, *cb = rgb + 3 * (size_t)c1, *cc = rgb + 3 * (size_t)c2;
                    for (int a = 0; a < 3; a++) {
                        const float f = render_mix((float)ca[a], (float)cb[a], (float)cc[a], q1, q2) + 0.5f;
                        colour[a] = (uint8_t)(!(f > 0.0f) ? 0.0f : (f > 255.0f ? 255.0f : f));   // (NaN: 0)
                    }
                }
            }
            for (int a = 0; a < 3; a++) {
                if (out.vertices) out.vertices[3 * p + a] = vert[a];
                if (out.normals) out.normals[3 * p + a] = norm[a];
                if (out.rgb) out.rgb[3 * p + a] = colour[a];
            }
        }
    }
    // (its own closing: block_counts_flush over the one counter costs two more SGPRs here, profiles/handle_counters_refactor.txt)
    __syncthreads();
    if (threadIdx.x == kWordHit && counts[kWordHit]) atomicAdd(words + kWordHit, (unsigned long long)counts[kWordHit]);
}

}  // namespace tsdf

using namespace tsdf;

struct tsdf_render : tsdf::HandleOrder {
    unsigned long long *keys;    // 8 bytes per pixel
    int4 *records;               // 16 bytes per shared vertex
    uint32_t *large_list;        // the list's length, then 4 bytes per triangle
    size_t keys_cap, records_cap, large_list_cap;
    CounterBlock<unsigned long long, kRenderWords> words;   // the error word and the counters (handle_counters.hpp)
    uint64_t n_triangles, n_vertices;   // of the last render
    uint32_t large_box;                 // tsdf_render_set_large_box
    int rendered;
};

namespace {

constexpr const char *kRenderOrder = "render stream order", *kRenderEvent = "render event", *kRenderWait = "render wait";

void render_free(tsdf_render *r) {
    r->destroy();
    device_free_all(r->keys, r->records, r->large_list);
    r->words.release();
    delete r;
}

// Everything the host can refuse, before any device work
int render_checked(const char *who, const tsdf_render *r, uint64_t n_vertices, uint64_t n_indices, const float *vertices, const uint32_t *indices,
                   const uint8_t *rgb, uint32_t width, uint32_t height, const float *inv_pose, const float *k, float z_near, float z_far, uint32_t flags,
                   const tsdf_render_targets *targets) {
    TSDF_REQUIRE(r, "%s: null render handle", who);
    TSDF_REQUIRE(inv_pose && k, "%s: null inv_pose or k", who);
    TSDF_REQUIRE(targets, "%s: null targets", who);
    const int rc = arrays_checked(who, n_vertices, n_indices, vertices, indices);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(width != 0 && height != 0 && (uint64_t)width * height < 0xffffffffull, "%s: an image of %u x %u pixels (none, or 2^32 - 1 or more)", who, width,
                 height);
    for (int i = 0; i < 16; i++) TSDF_REQUIRE(std::isfinite(inv_pose[i]), "%s: inv_pose[%d] is not finite", who, i);
    for (int i = 0; i < 9; i++) TSDF_REQUIRE(std::isfinite(k[i]), "%s: k[%d] is not finite", who, i);
    TSDF_REQUIRE(k[1] == 0.0f && k[2] == 0.0f && k[3] == 0.0f && k[5] == 0.0f && k[8] == 1.0f,
                 "%s: a non-standard k (only fx, fy, cx, cy may differ from the standard camera's matrix)", who);
    TSDF_REQUIRE(std::isfinite(z_near) && std::isfinite(z_far) && z_near > 0.0f && z_near <= z_far, "%s: near (%g) and far (%g) must be finite with 0 < near <= far",
                 who, (double)z_near, (double)z_far);
    TSDF_REQUIRE((flags & ~(uint32_t)TSDF_RENDER_CULL_BACK) == 0, "%s: unknown flags %#x", who, flags);
    TSDF_REQUIRE(!targets->rgb || rgb, "%s: an rgb target, but the mesh has no colours", who);
    return TSDF_OK;
}

// the counters of the last render, once somebody has waited; the error word first
int render_verdict(const char *who, const tsdf_render *r, tsdf_render_info *info) {
    if (r->rendered && r->words.host[kWordError]) return index_refused(who, r->n_vertices);
    if (info) {
        info->n_triangles = r->n_triangles;
        info->n_live = r->rendered ? r->words.host[kWordLive] : 0;
        info->n_dropped = r->rendered ? r->words.host[kWordDropped] : 0;
        info->n_large = r->rendered ? r->words.host[kWordLarge] : 0;
        info->n_pixels_hit = r->rendered ? r->words.host[kWordHit] : 0;
    }
    return TSDF_OK;
}

// The launches of one render on `stream`, with the handle's stream order round them.  The arguments have passed render_checked.
int render_on(const char *who, tsdf_render *r, uint64_t n_vertices, uint64_t n_indices, const float *vertices, const uint32_t *indices, const float *normals,
              const uint8_t *rgb, uint32_t width, uint32_t height, const float *inv_pose, const float *k, float z_near, float z_far, uint32_t flags,
              const tsdf_render_targets *targets, tsdf_render_info *info, hipStream_t stream) {
    if (n_vertices == 0 && n_indices) return index_refused(who, 0);
    int rc = r->join(stream, kRenderOrder);
    if (rc != TSDF_OK) return rc;
    r->rendered = 0;
    const uint32_t n_pixels = width * height, nv = (uint32_t)n_vertices, n_triangles = (uint32_t)(n_indices / 3);
    hipError_t e = device_reserve(r->keys, r->keys_cap, (size_t)n_pixels);
    if (e == hipSuccess) e = device_reserve(r->records, r->records_cap, (size_t)(nv ? nv : 1));
    if (e == hipSuccess) e = device_reserve(r->large_list, r->large_list_cap, (size_t)n_triangles + 1);
    if (e != hipSuccess) return hip_fail(e, "render scratch alloc failed");
    RenderView view;
    std::memcpy(&view.ip, inv_pose, sizeof(view.ip));
    view.fx = k[0];
    view.fy = k[4];
    view.cx = k[6];
    view.cy = k[7];
    view.z_near = z_near;
    view.z_far = z_far;
    view.width = width;
    view.height = height;
    view.flags = flags;
    const RenderTargets out = {targets->triangle, targets->z, targets->depth, targets->vertices, targets->normals, targets->rgb};
    r->n_triangles = n_triangles;
    r->n_vertices = n_vertices;

    TSDF_HIP(r->words.reset(stream), "render counts reset");
    TSDF_HIP(hipMemsetAsync(r->large_list, 0, sizeof(uint32_t), stream), "render list reset");
    TSDF_HIP(hipMemsetAsync(r->keys, 0xff, (size_t)n_pixels * sizeof(unsigned long long), stream), "render keys fill");
    if (n_triangles) {
        hipLaunchKernelGGL(render_project_kernel, grid_for(nv, 256), dim3(256), 0, stream, nv, vertices, view, r->records);
        hipLaunchKernelGGL(render_raster_kernel, grid_for(n_triangles, 256), dim3(256), 0, stream, nv, n_triangles, indices, r->records, view, r->large_box,
                           r->keys, r->large_list, r->words.dev);
        const uint32_t large_grid = (n_triangles + 3) / 4 < kLargeGrid ? (n_triangles + 3) / 4 : kLargeGrid;
        hipLaunchKernelGGL(render_large_kernel, dim3(large_grid), dim3(256), 0, stream, nv, indices, r->records, view, r->keys, r->large_list);
    }
    hipLaunchKernelGGL(render_resolve_kernel, grid_for(n_pixels, 256), dim3(256), 0, stream, n_pixels, r->keys, indices, r->records, vertices, normals, rgb, view,
                       out, r->words.dev);
    TSDF_HIP(hipGetLastError(), "render kernels failed");
    TSDF_HIP(r->words.download(stream), "render counts download");
    rc = r->leave(stream, kRenderEvent);
    if (rc != TSDF_OK) return rc;
    r->rendered = 1;
    if (!info) return TSDF_OK;
    rc = r->wait(kRenderWait);   // the one synchronisation, only when the counts are asked for
    return rc != TSDF_OK ? rc : render_verdict(who, r, info);
}

// a render of a mesh handle's arrays, ordered behind its pending work
int render_handle_on(const char *who, tsdf_render *r, tsdf_mesh *mesh, uint32_t width, uint32_t height, const float *inv_pose, const float *k, float z_near,
                     float z_far, uint32_t flags, const tsdf_render_targets *targets, tsdf_render_info *info, hipStream_t stream) {
    int rc = mesh_join(mesh, stream);
    if (rc != TSDF_OK) return rc;
    const bool any = mesh->info.n_vertices != 0;
    rc = render_on(who, r, mesh->info.n_vertices, mesh->info.n_indices, any ? mesh->vertices : nullptr, any ? mesh->indices : nullptr,
                   any && (mesh->info.flags & TSDF_MESH_NORMALS) ? mesh->normals : nullptr, any && (mesh->info.flags & TSDF_MESH_COLOURS) ? mesh->rgb : nullptr,
                   width, height, inv_pose, k, z_near, z_far, flags, targets, info, stream);
    const int rc2 = any ? mesh_leave(mesh, stream) : TSDF_OK;   // the mesh's arrays are read by what has just been enqueued
    return rc != TSDF_OK ? rc : rc2;
}

int handle_checked(const char *who, const tsdf_render *r, const tsdf_mesh *mesh, uint32_t width, uint32_t height, const float *inv_pose, const float *k,
                   float z_near, float z_far, uint32_t flags, const tsdf_render_targets *targets) {
    TSDF_REQUIRE(r, "%s: null render handle", who);
    TSDF_REQUIRE(mesh, "%s: null mesh", who);
    TSDF_REQUIRE(inv_pose && k, "%s: null inv_pose or k", who);
    TSDF_REQUIRE(targets, "%s: null targets", who);
    TSDF_REQUIRE(r->device == mesh->device, "%s: the render handle was created on device %d, the mesh on device %d", who, r->device, mesh->device);
    // (a mesh handle's colour array stands for "has colours" here; nothing is read through the pointers)
    const bool any = mesh->info.n_vertices != 0;
    const float *some_vertices = any ? mesh->vertices : nullptr;
    const uint32_t *some_indices = mesh->info.n_indices ? mesh->indices : nullptr;
    const uint8_t *has_rgb = (mesh->info.flags & TSDF_MESH_COLOURS) ? reinterpret_cast<const uint8_t *>(mesh) : nullptr;
    return render_checked(who, r, mesh->info.n_vertices, mesh->info.n_indices, some_vertices, some_indices, has_rgb, width, height, inv_pose, k, z_near, z_far,
                          flags, targets);
}

}  // namespace

extern "C" {

int tsdf_render_create(tsdf_render **out) {
    return handle_create(out, "tsdf_render_create", "render alloc failed", [](tsdf_render *r) {
        r->large_box = TSDF_RENDER_LARGE_BOX;
        const hipError_t e = r->create();
        return e == hipSuccess ? r->words.create() : e;
    }, render_free);
}

void tsdf_render_destroy(tsdf_render *r) {
    if (r) render_free(r);
}

int tsdf_render_scratch_bytes(const tsdf_render *r, uint64_t *bytes) {
    TSDF_REQUIRE(r && bytes, "tsdf_render_scratch_bytes: null argument");
    *bytes = (uint64_t)r->keys_cap * sizeof(unsigned long long) + (uint64_t)r->records_cap * sizeof(int4) + (uint64_t)r->large_list_cap * sizeof(uint32_t) +
             r->words.device_bytes();
    return TSDF_OK;
}

int tsdf_render_set_large_box(tsdf_render *r, uint32_t pixels) {
    TSDF_REQUIRE(r, "tsdf_render_set_large_box: null argument");
    r->large_box = pixels;
    return TSDF_OK;
}

int tsdf_render_get_info(const tsdf_render *r, tsdf_render_info *info) {
    TSDF_REQUIRE(r && info, "tsdf_render_get_info: null argument");
    const int rc = r->wait(kRenderWait);
    return rc != TSDF_OK ? rc : render_verdict("tsdf_render_get_info", r, info);
}

int tsdf_render_mesh_device(tsdf_render *r, uint64_t n_vertices, uint64_t n_indices, const float *device_vertices, const uint32_t *device_indices,
                            const float *device_normals, const uint8_t *device_rgb, uint32_t width, uint32_t height, const float inv_pose[16], const float k[9],
                            float z_near, float z_far, uint32_t flags, const tsdf_render_targets *device_targets, tsdf_render_info *info, void *hip_stream) {
    const char *who = "tsdf_render_mesh_device";
    const int rc = render_checked(who, r, n_vertices, n_indices, device_vertices, device_indices, device_rgb, width, height, inv_pose, k, z_near, z_far, flags,
                                  device_targets);
    if (rc != TSDF_OK) return rc;
    return render_on(who, r, n_vertices, n_indices, device_vertices, device_indices, device_normals, device_rgb, width, height, inv_pose, k, z_near, z_far, flags,
                     device_targets, info, (hipStream_t)hip_stream);
}

int tsdf_mesh_render_device(tsdf_render *r, tsdf_mesh *mesh, uint32_t width, uint32_t height, const float inv_pose[16], const float k[9], float z_near,
                            float z_far, uint32_t flags, const tsdf_render_targets *device_targets, tsdf_render_info *info, void *hip_stream) {
    const char *who = "tsdf_mesh_render_device";
    const int rc = handle_checked(who, r, mesh, width, height, inv_pose, k, z_near, z_far, flags, device_targets);
    if (rc != TSDF_OK) return rc;
    return render_handle_on(who, r, mesh, width, height, inv_pose, k, z_near, z_far, flags, device_targets, info, (hipStream_t)hip_stream);
}

int tsdf_mesh_render(tsdf_render *r, tsdf_mesh *mesh, uint32_t width, uint32_t height, const float inv_pose[16], const float k[9], float z_near, float z_far,
                     uint32_t flags, const tsdf_render_targets *host_targets, tsdf_render_info *info) {
    const char *who = "tsdf_mesh_render";
    const int rc0 = handle_checked(who, r, mesh, width, height, inv_pose, k, z_near, z_far, flags, host_targets);
    if (rc0 != TSDF_OK) return rc0;
    // one device buffer for the requested targets, each at a 16-byte boundary
    const size_t n = (size_t)width * height;
    const size_t sizes[6] = {host_targets->triangle ? 4 * n : 0, host_targets->z ? 4 * n : 0, host_targets->depth ? 2 * n : 0,
                             host_targets->vertices ? 12 * n : 0, host_targets->normals ? 12 * n : 0, host_targets->rgb ? 3 * n : 0};
    size_t at[6], bytes = 16;
    for (int i = 0; i < 6; i++) {
        at[i] = bytes;
        bytes += (sizes[i] + 15) & ~(size_t)15;
    }
    HostStage st;
    int rc = st.begin(nullptr, bytes, "tsdf_mesh_render: couldn't allocate %zu bytes for the targets");
    if (rc != TSDF_OK) return rc;
    char *base = static_cast<char *>(st.buf);
    auto part = [&](int i) { return sizes[i] ? base + at[i] : nullptr; };
    const tsdf_render_targets device = {(uint32_t *)part(0), (float *)part(1), (uint16_t *)part(2), (float *)part(3), (float *)part(4), (uint8_t *)part(5)};
    rc = render_handle_on(who, r, mesh, width, height, inv_pose, k, z_near, z_far, flags, &device, nullptr, nullptr);
    void *host[6] = {host_targets->triangle, host_targets->z, host_targets->depth, host_targets->vertices, host_targets->normals, host_targets->rgb};
    if (rc == TSDF_OK)
        for (int i = 0; i < 6; i++)
            if (sizes[i]) st.down(host[i], base + at[i], sizes[i]);
    rc = st.finish(rc, "Mesh render failed");
    if (rc != TSDF_OK) return rc;
    r->pending = 0;   // (the stream has been waited for)
    mesh->pending = 0;
    return render_verdict(who, r, info);
}

}  // extern "C"
