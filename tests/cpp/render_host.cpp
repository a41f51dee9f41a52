// Host-side run of the mesh renderer's integer arithmetic (tsdf_amd/csrc/raster_index.hpp) under the address and undefined-behaviour
// sanitizers (`make sanitize-render`): the snap at the ends of the screen range, the twice-area and the edge functions at the ends of
// the coordinate range (|X|, |Y| = 2^28, where a product formed in 32 bits or a sum past 2^63 is a sanitizer report), boxes wholly
// outside the image and between pixel centres, and brute force over small images: the edge functions sum to |A2| at every pixel, the
// coverage does not depend on which corner comes first or on the winding, two triangles that share an edge cover every centre of their
// quadrilateral exactly once -- centres on the shared edge included -- and a fan round a pixel centre covers every pixel of the image
// once.  Needs no GPU and links nothing of the library.
#include <cstdio>
#include <cstdlib>

#include "raster_index.hpp"

using namespace tsdf;

static int failures = 0;
#define EXPECT(c)                                                   \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("line %d: %s\n", __LINE__, #c);             \
            failures++;                                             \
        }                                                           \
    } while (0)

static bool covers(RasterPoint p0, RasterPoint p1, RasterPoint p2, int64_t i, int64_t j, bool check_sum = true) {
    const int64_t a2 = raster_area2(p0, p1, p2);
    if (a2 == 0) return false;
    const RasterEdges e = raster_edges(p0, p1, p2, a2);
    const int64_t e0 = raster_edge_at(e, 0, i, j), e1 = raster_edge_at(e, 1, i, j), e2 = raster_edge_at(e, 2, i, j);
    if (check_sum) EXPECT(e0 + e1 + e2 == e.area && e.area > 0);
    return raster_covered(e, e0, e1, e2);
}

// the side of A -> B the centre of (i, j) lies on, in 128 bits and written independently of the header
static int side(RasterPoint a, RasterPoint b, int64_t i, int64_t j) {
    const __int128 v = (__int128)(b.x - a.x) * (256 * j - a.y) - (__int128)(b.y - a.y) * (256 * i - a.x);
    return v > 0 ? 1 : (v < 0 ? -1 : 0);
}

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

int main() {
    // the snap: the ends of the screen range, halves go to even
    EXPECT(raster_in_range(1048576.0f) && raster_in_range(-1048576.0f) && !raster_in_range(1048576.125f) && !raster_in_range(NAN) && !raster_in_range(INFINITY));
    EXPECT(raster_snap(1048576.0f) == kRasterMaxCoordinate && raster_snap(-1048576.0f) == -kRasterMaxCoordinate);
    EXPECT(raster_snap(0.001953125f) == 0 && raster_snap(0.005859375f) == 2 && raster_snap(-0.001953125f) == 0 && raster_snap(3.5f) == 896);

    // the ends of the coordinate range: every product in 64 bits, the sum rule holds at the far corners
    const int32_t M = kRasterMaxCoordinate;
    const RasterPoint far[4] = {{-M, -M}, {M, -M}, {M, M}, {-M, M}};
    for (int r = 0; r < 4; r++) {
        const RasterPoint p0 = far[r], p1 = far[(r + 1) % 4], p2 = far[(r + 2) % 4];
        const int64_t a2 = raster_area2(p0, p1, p2);
        EXPECT(a2 == ((int64_t)1 << 58) && raster_area2(p0, p2, p1) == -a2);
        for (int flip = 0; flip < 2; flip++) {
            const RasterEdges e = flip ? raster_edges(p0, p2, p1, -a2) : raster_edges(p0, p1, p2, a2);
            EXPECT(e.area == a2);
            const int64_t ends[3] = {-(M / 256), 0, M / 256};
            for (int64_t i : ends)
                for (int64_t j : ends) EXPECT(raster_edge_at(e, 0, i, j) + raster_edge_at(e, 1, i, j) + raster_edge_at(e, 2, i, j) == a2);
        }
        RasterBox box;
        EXPECT(raster_box(p0, p1, p2, 0xfffffffeu, 1, box) && box.x0 == 0 && box.y0 == 0 && box.x1 == (uint32_t)(M / 256) && box.y1 == 0);
        EXPECT(raster_box(p0, p1, p2, 7, 5, box) && box.x1 == 6 && box.y1 == 4 && raster_box_pixels(box) == 35);
    }
    EXPECT(raster_floor_div(-1, 256) == -1 && raster_floor_div(-256, 256) == -1 && raster_floor_div(-257, 256) == -2 && raster_floor_div(255, 256) == 0);
    EXPECT(raster_ceil_div(-1, 256) == 0 && raster_ceil_div(-256, 256) == -1 && raster_ceil_div(1, 256) == 1 && raster_ceil_div(256, 256) == 1);

    // boxes wholly outside the image, on each side, and between two pixel centres
    {
        RasterBox box;
        const uint32_t W = 8, H = 6;
        EXPECT(!raster_box({-900, 100}, {-300, 100}, {-300, 700}, W, H, box));                // left
        EXPECT(!raster_box({8 * 256 - 255, 100}, {9 * 256, 100}, {9 * 256, 700}, W, H, box));  // right of the last centre
        EXPECT(!raster_box({100, -900}, {700, -900}, {700, -1}, W, H, box));                   // above
        EXPECT(!raster_box({100, 5 * 256 + 1}, {700, 5 * 256 + 1}, {700, M}, W, H, box));      // below
        EXPECT(!raster_box({257, 257}, {511, 257}, {511, 511}, W, H, box));                    // between centres
        EXPECT(raster_box({256, 256}, {512, 256}, {512, 512}, W, H, box) && box.x0 == 1 && box.x1 == 2 && box.y0 == 1 && box.y1 == 2);
        EXPECT(raster_box({-M, -M}, {M, -M}, {M, M}, W, H, box) && box.x0 == 0 && box.y0 == 0 && box.x1 == W - 1 && box.y1 == H - 1);
    }

    // brute force over small images: corners on the quarter-pixel grid round a 9 x 7 image
    const int W = 9, H = 7;
    uint32_t seed = 12345u;
    long on_shared_edge = 0, quads = 0;
    for (int trial = 0; trial < 4000; trial++) {
        RasterPoint q[4];
        for (auto &p : q) {
            p.x = (int32_t)(lcg(seed) >> 16) % (64 * 4 * (W + 2)) / 64 * 64 - 256;   // multiples of 64 in [-256, 256 (W + 1))
            p.y = (int32_t)(lcg(seed) >> 16) % (64 * 4 * (H + 2)) / 64 * 64 - 256;
        }
        if (trial % 2) {   // every other trial: the ends of the cut on pixel centres, so that centres lie on it
            q[0].x = q[0].x / 256 * 256; q[0].y = q[0].y / 256 * 256;
            q[2].x = q[2].x / 256 * 256; q[2].y = q[2].y / 256 * 256;
        }
        // one triangle: rotation and winding do not change the coverage; strictly inside is covered, strictly outside is not
        const int64_t a2 = raster_area2(q[0], q[1], q[2]);
        for (int j = 0; j < H; j++)
            for (int i = 0; i < W; i++) {
                const bool c = covers(q[0], q[1], q[2], i, j);
                EXPECT(c == covers(q[1], q[2], q[0], i, j) && c == covers(q[2], q[0], q[1], i, j) && c == covers(q[0], q[2], q[1], i, j));
                if (a2 != 0) {
                    const int s = a2 > 0 ? 1 : -1;
                    const int s0 = s * side(q[0], q[1], i, j), s1 = s * side(q[1], q[2], i, j), s2 = s * side(q[2], q[0], i, j);
                    if (s0 > 0 && s1 > 0 && s2 > 0) EXPECT(c);
                    if (s0 < 0 || s1 < 0 || s2 < 0) EXPECT(!c);
                    RasterBox box;
                    const bool in_box = raster_box(q[0], q[1], q[2], W, H, box) && (uint32_t)i >= box.x0 && (uint32_t)i <= box.x1 && (uint32_t)j >= box.y0 &&
                                        (uint32_t)j <= box.y1;
                    if (c) EXPECT(in_box);   // the box loses no covered pixel
                }
            }
        // a convex quadrilateral cut along q0 - q2: every centre strictly inside it is covered exactly once
        const int64_t w0 = raster_area2(q[0], q[1], q[2]), w1 = raster_area2(q[1], q[2], q[3]), w2 = raster_area2(q[2], q[3], q[0]),
                      w3 = raster_area2(q[3], q[0], q[1]);
        const bool convex = (w0 > 0 && w1 > 0 && w2 > 0 && w3 > 0) || (w0 < 0 && w1 < 0 && w2 < 0 && w3 < 0);
        if (!convex) continue;
        quads++;
        const int s = w0 > 0 ? 1 : -1;
        for (int j = 0; j < H; j++)
            for (int i = 0; i < W; i++) {
                const int n = (int)covers(q[0], q[1], q[2], i, j, false) + (int)covers(q[0], q[2], q[3], i, j, false);
                EXPECT(n <= 1);
                const bool inside = s * side(q[0], q[1], i, j) > 0 && s * side(q[1], q[2], i, j) > 0 && s * side(q[2], q[3], i, j) > 0 &&
                                    s * side(q[3], q[0], i, j) > 0;
                if (inside) {
                    EXPECT(n == 1);
                    if (side(q[0], q[2], i, j) == 0) on_shared_edge++;
                }
            }
    }
    EXPECT(quads > 0 && on_shared_edge > 0);   // the trials really put centres on shared edges

    // a fan round the pixel centre (4, 3), out to the half-pixel border of the image: every pixel once, the hub included
    {
        const RasterPoint hub = {4 * 256, 3 * 256};
        const RasterPoint rim[8] = {{-128, -128}, {4 * 256, -128}, {W * 256 - 128, -128}, {W * 256 - 128, 3 * 256}, {W * 256 - 128, H * 256 - 128},
                                    {4 * 256, H * 256 - 128}, {-128, H * 256 - 128}, {-128, 3 * 256}};
        for (int j = 0; j < H; j++)
            for (int i = 0; i < W; i++) {
                int n = 0, n_reversed = 0;
                for (int k = 0; k < 8; k++) {
                    n += covers(hub, rim[k], rim[(k + 1) % 8], i, j);
                    n_reversed += covers(hub, rim[(k + 1) % 8], rim[k], i, j);
                }
                EXPECT(n == 1 && n_reversed == 1);
            }
    }

    if (failures) {
        std::printf("render_host: %d failures\n", failures);
        return 1;
    }
    std::printf("render_host: ok (%ld quadrilaterals, %ld centres on shared edges)\n", quads, on_shared_edge);
    return 0;
}
