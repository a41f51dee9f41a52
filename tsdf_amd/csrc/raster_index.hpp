// The integer arithmetic of the mesh renderer (include/tsdf_amd.h, "mesh rendering", rules 2 - 4): the snap of a screen
// coordinate to the 1/256 grid, the twice-area, the three edge functions at a pixel centre, the top-left rule and the pixel box of a
// triangle clipped to the image.  mesh_render.hip's kernels use these and nothing else for their decisions.  Everything is formed in 64
// bits: with |X|, |Y| <= 2^28 (kRasterMaxCoordinate) a difference is at most 2^29 and every product stays below 2^58.  Compiles for the
// host alone: tests/cpp/render_host.cpp runs it under the address and undefined-behaviour sanitizers (`make sanitize-render`).
#pragma once

#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace tsdf {

constexpr int kRasterSubpixel = 256;                   // fixed-point units per pixel
constexpr float kRasterMaxScreen = 1048576.0f;         // 2^20: the largest |sx|, |sy| of a usable vertex
constexpr int32_t kRasterMaxCoordinate = 1 << 28;      // ... so the largest |X|, |Y|

// rule 2: a screen coordinate in range (false for NaN), and its fixed-point value
__host__ __device__ inline bool raster_in_range(float s) { return fabsf(s) <= kRasterMaxScreen; }
__host__ __device__ inline int32_t raster_snap(float s) { return (int32_t)rintf(s * 256.0f); }

struct RasterPoint {
    int32_t x, y;
};

// (B - A) x (P - A), z component: positive when P lies to the side of A -> B that +y lies of +x
__host__ __device__ inline int64_t raster_orient(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

// rule 3: the twice-area of (P0, P1, P2)
__host__ __device__ inline int64_t raster_area2(RasterPoint p0, RasterPoint p1, RasterPoint p2) {
    return raster_orient(p0.x, p0.y, p1.x, p1.y, p2.x, p2.y);
}

// Rule 4.  E_k(P) = a_k P.x + b_k P.y + c_k is the edge function opposite corner k, sign-normalised by A2 so that the inside is E_k > 0
// and E_0 + E_1 + E_2 == |A2| at every P; top_left[k] says whether a pixel centre with E_k == 0 belongs to the triangle.
struct RasterEdges {
    int64_t a[3], b[3], c[3];
    int64_t area;        // |A2|
    bool top_left[3];    // a_k > 0, or a_k == 0 and b_k > 0
};

__host__ __device__ inline RasterEdges raster_edges(RasterPoint p0, RasterPoint p1, RasterPoint p2, int64_t area2) {
    const int64_t s = area2 < 0 ? -1 : 1;
    const RasterPoint from[3] = {p1, p2, p0}, to[3] = {p2, p0, p1};
    RasterEdges e;
    for (int k = 0; k < 3; k++) {
        const int64_t ax = from[k].x, ay = from[k].y, bx = to[k].x, by = to[k].y;
        e.a[k] = -s * (by - ay);
        e.b[k] = s * (bx - ax);
        e.c[k] = s * ((by - ay) * ax - (bx - ax) * ay);
        e.top_left[k] = e.a[k] > 0 || (e.a[k] == 0 && e.b[k] > 0);
    }
    e.area = s * area2;
    return e;
}

// E_k at the centre of pixel (i, j), which is the screen point (i, j): P = (256 i, 256 j).  (i, j) lies in the triangle's box, so
// |P| <= 2^28 as well.
__host__ __device__ inline int64_t raster_edge_at(const RasterEdges &e, int k, int64_t i, int64_t j) {
    return e.a[k] * (i * kRasterSubpixel) + e.b[k] * (j * kRasterSubpixel) + e.c[k];
}

__host__ __device__ inline bool raster_covered(const RasterEdges &e, int64_t e0, int64_t e1, int64_t e2) {
    return (e0 > 0 || (e0 == 0 && e.top_left[0])) && (e1 > 0 || (e1 == 0 && e.top_left[1])) && (e2 > 0 || (e2 == 0 && e.top_left[2]));
}

__host__ __device__ inline int64_t raster_floor_div(int64_t v, int64_t d) { return v >= 0 ? v / d : -((-v + d - 1) / d); }
__host__ __device__ inline int64_t raster_ceil_div(int64_t v, int64_t d) { return -raster_floor_div(-v, d); }

// The pixels whose centres lie in the triangle's bounding box and in the image: [x0, x1] x [y0, y1], inclusive; false when there is
// none (a box wholly outside the image, or between two pixel centres).
struct RasterBox {
    uint32_t x0, y0, x1, y1;
};

__host__ __device__ inline bool raster_box(RasterPoint p0, RasterPoint p1, RasterPoint p2, uint32_t width, uint32_t height, RasterBox &box) {
    const int64_t lo_x = p0.x < p1.x ? (p0.x < p2.x ? p0.x : p2.x) : (p1.x < p2.x ? p1.x : p2.x);
    const int64_t hi_x = p0.x > p1.x ? (p0.x > p2.x ? p0.x : p2.x) : (p1.x > p2.x ? p1.x : p2.x);
    const int64_t lo_y = p0.y < p1.y ? (p0.y < p2.y ? p0.y : p2.y) : (p1.y < p2.y ? p1.y : p2.y);
    const int64_t hi_y = p0.y > p1.y ? (p0.y > p2.y ? p0.y : p2.y) : (p1.y > p2.y ? p1.y : p2.y);
    int64_t x0 = raster_ceil_div(lo_x, kRasterSubpixel), x1 = raster_floor_div(hi_x, kRasterSubpixel);
    int64_t y0 = raster_ceil_div(lo_y, kRasterSubpixel), y1 = raster_floor_div(hi_y, kRasterSubpixel);
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > (int64_t)width - 1) x1 = (int64_t)width - 1;
    if (y1 > (int64_t)height - 1) y1 = (int64_t)height - 1;
    if (x0 > x1 || y0 > y1) return false;
    box.x0 = (uint32_t)x0;
    box.y0 = (uint32_t)y0;
    box.x1 = (uint32_t)x1;
    box.y1 = (uint32_t)y1;
    return true;
}

__host__ __device__ inline uint64_t raster_box_pixels(const RasterBox &box) { return (uint64_t)(box.x1 - box.x0 + 1) * (uint64_t)(box.y1 - box.y0 + 1); }

}  // namespace tsdf
