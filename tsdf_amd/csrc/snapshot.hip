// Sparse snapshots for gfx950 (include/tsdf_amd.h, "sparse snapshot"): the bricks of 8^3 voxels of a whole volume that hold anything
// but the state clear() leaves, taken out of the dense arrays into compact ones and put back.  No reference counterpart.
//
// The value is a unique set of bytes (the header has the definition); the kernels only move words:
//   snapshot_flag_kernel     one workgroup per strip (by, bz) of bricks, lanes along x: every distance, weight and colour word of the
//                            strip is read once, in whole rows; a ballot per row, OR-ed per wave and combined through LDS, gives one
//                            flag per brick
//   mesh_scan<ArrayCounts>   flags -> the list position of every live brick (mesh_scan.hip)
//   snapshot_list_kernel     the ascending id list, and the brick -> list position map restore goes through
//   snapshot_gather_kernel   one workgroup per live brick: the 32-byte rows in 16-byte reads, the compact arrays written contiguously,
//                            packed weights taken out of their z-groups (weights.hip)
//   snapshot_scatter_kernel  one workgroup per four bricks of the grid along x: every dense word written once, the stored brick or the
//                            fill, eight threads to 128 contiguous bytes of a row
// and the rolling volume built on them ("rolling volume"; brick_shift.hpp has its arithmetic, DESIGN.md 32 the reasons):
//   snapshot_scatter_shifted_kernel  the scatter over a grid that need not be the snapshot's, each brick from the brick a shift away
//   snapshot_page_in_kernel  the same rows and z-groups over the snapshot's list: only the stored bricks are written
//   select_flag_kernel, mesh_scan, select_gather_kernel   the entries of a list inside (outside) a box of bricks -> a list of their own
// Every output word has one writer and there are no atomics: the same bytes on every run.
#include <algorithm>

#include "brick_shift.hpp"
#include "common.hpp"
#include "field_sample.hpp"
#include "handle_counters.hpp"
#include "handle_order.hpp"
#include "mesh_handle.hpp"

namespace tsdf {

constexpr uint32_t kSnapBrick = TSDF_SNAPSHOT_BRICK;
constexpr uint32_t kSnapVoxels = kSnapBrick * kSnapBrick * kSnapBrick;
constexpr uint32_t kSnapNone = 0xffffffffu;   // the map's word of a brick that is not stored

struct SnapGrid {
    uint32_t X, Y, Z;
    uint32_t nbx, nby, nbz;
};

// Four consecutive words of a row from x (a multiple of 4) on; words beyond the row are `pad`.  `vec`: the row length is a multiple of
// 4, so the four words are either all inside and 16-byte aligned, or all outside.
__device__ inline void load4(const uint32_t *__restrict__ base, size_t i, uint32_t x, uint32_t X, bool vec, uint32_t pad, uint32_t out[4]) {
    if (vec) {
        const uint4 q = x < X ? *reinterpret_cast<const uint4 *>(base + i) : make_uint4(pad, pad, pad, pad);
        out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) out[k] = x + k < X ? base[i + k] : pad;
}

__device__ inline void store4(uint32_t *__restrict__ base, size_t i, uint32_t x, uint32_t X, bool vec, const uint32_t in[4]) {
    if (vec) {
        if (x < X) *reinterpret_cast<uint4 *>(base + i) = make_uint4(in[0], in[1], in[2], in[3]);
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
        if (x + k < X) base[i + k] = in[k];
}

__global__ __launch_bounds__(256) void snapshot_flag_kernel(const float *__restrict__ dist, const WeightView wv, const uint32_t *__restrict__ colour,
                                                            const SnapGrid g, const uint32_t fill_bits, uint32_t *__restrict__ flags) {
    __shared__ unsigned long long masks[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t by = blockIdx.x, bz = blockIdx.y;
    const size_t xy = (size_t)g.X * g.Y;
    const uint32_t *dbits = reinterpret_cast<const uint32_t *>(dist), *wbits = reinterpret_cast<const uint32_t *>(wv.f32);
    // packed counts: the planes of a dword, the dwords (z-groups) of a brick, and its rows of dwords
    const uint32_t per = wv.mode == 8 ? 4u : 2u, groups = kSnapBrick / per;
    for (uint32_t x0 = 0; x0 < g.X; x0 += 64u) {
        const uint32_t x = x0 + lane;
        bool live = false;
        for (uint32_t r = wave; r < 64u; r += 4u) {
            const uint32_t y = by * kSnapBrick + (r & 7u), z = bz * kSnapBrick + (r >> 3);
            if (x < g.X && y < g.Y && z < g.Z) {
                const size_t i = xy * z + (size_t)g.X * y + x;
                live |= dbits[i] != fill_bits;
                if (colour) live |= colour[i] != 0u;
                if (wv.mode == 0) live |= wbits[i] != 0u;
            }
        }
        if (wv.mode != 0) {
            for (uint32_t r = wave; r < 8u * groups; r += 4u) {
                const uint32_t y = by * kSnapBrick + (r & 7u), z0 = bz * kSnapBrick + (r >> 3) * per;
                if (x < g.X && y < g.Y && z0 < g.Z) {
                    uint32_t word = wv.packed[xy * (z0 / per) + (size_t)g.X * y + x];
                    const uint32_t bits = min(per, g.Z - z0) * (uint32_t)wv.mode;   // (fields of planes beyond the grid say nothing)
                    if (bits < 32u) word &= (1u << bits) - 1u;
                    live |= word != 0u;
                }
            }
        }
        const unsigned long long mask = __ballot(live);
        if (lane == 0) masks[wave] = mask;
        __syncthreads();
        if (threadIdx.x < 8u) {
            const uint32_t bx = (x0 >> 3) + threadIdx.x;
            const unsigned long long m = masks[0] | masks[1] | masks[2] | masks[3];
            if (bx < g.nbx) flags[bx + g.nbx * (by + (size_t)g.nby * bz)] = ((m >> (8u * threadIdx.x)) & 0xffull) ? 1u : 0u;
        }
        __syncthreads();
    }
}

// bases: the scanned flags (the list position of brick b if it is live), total: the scan's first total
__global__ __launch_bounds__(256) void snapshot_list_kernel(const uint32_t *__restrict__ bases, const uint64_t *__restrict__ total, uint32_t n_bricks,
                                                            uint32_t *__restrict__ ids, uint32_t *__restrict__ map) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_bricks) return;
    const uint32_t base = bases[b], next = b + 1u < n_bricks ? bases[b + 1u] : (uint32_t)*total;
    const bool live = next != base;
    map[b] = live ? base : kSnapNone;
    if (live) ids[base] = b;
}

__global__ __launch_bounds__(256) void snapshot_map_kernel(const uint32_t *__restrict__ ids, uint32_t n, uint32_t *__restrict__ map) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) map[ids[i]] = i;
}

// the packed counts of brick (bx, by, bz) -> 512 elements of BITS bits at list position p: a thread per (4 x, y, z-group)
template <int BITS>
__device__ inline void gather_packed(const uint32_t *__restrict__ wp, const SnapGrid &g, uint32_t bx, uint32_t by, uint32_t bz, size_t p,
                                     void *__restrict__ out) {
    constexpr uint32_t kPer = 32 / BITS, kGroups = kSnapBrick / kPer, kMask = BITS == 8 ? 0xffu : 0xffffu;
    const uint32_t t = threadIdx.x;
    if (t >= 16u * kGroups) return;
    const uint32_t half = t & 1u, ly = (t >> 1) & 7u, gi = t >> 4;
    const uint32_t x = bx * kSnapBrick + 4u * half, y = by * kSnapBrick + ly, z0 = bz * kSnapBrick + gi * kPer;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (y < g.Y && z0 < g.Z) load4(wp, (size_t)g.X * g.Y * (z0 / kPer) + (size_t)g.X * y + x, x, g.X, (g.X & 3u) == 0u, 0u, w);
#pragma unroll
    for (uint32_t s = 0; s < kPer; s++) {
        uint32_t v[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) v[k] = z0 + s < g.Z ? (w[k] >> (BITS * s)) & kMask : 0u;
        const size_t e = p * kSnapVoxels + 64u * (gi * kPer + s) + 8u * ly + 4u * half;
        if (BITS == 8) static_cast<uint32_t *>(out)[e >> 2] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        else static_cast<uint2 *>(out)[e >> 2] = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
    }
}

// 128 threads: thread t takes the half t & 1 of row t >> 1 (ly = row & 7, lz = row >> 3)
__global__ __launch_bounds__(128) void snapshot_gather_kernel(const float *__restrict__ dist, const WeightView wv, const uint32_t *__restrict__ colour,
                                                              const SnapGrid g, const uint32_t fill_bits, const uint32_t *__restrict__ ids,
                                                              float *__restrict__ odist, void *__restrict__ oweights, uint32_t *__restrict__ ocolour) {
    const size_t p = blockIdx.x;
    const uint32_t b = ids[p];
    const uint32_t bx = b % g.nbx, by = (b / g.nbx) % g.nby, bz = b / (g.nbx * g.nby);
    const uint32_t half = threadIdx.x & 1u, row = threadIdx.x >> 1;
    const uint32_t x = bx * kSnapBrick + 4u * half, y = by * kSnapBrick + (row & 7u), z = bz * kSnapBrick + (row >> 3);
    const bool vec = (g.X & 3u) == 0u, inside = y < g.Y && z < g.Z;
    const size_t i = inside ? (size_t)g.X * g.Y * z + (size_t)g.X * y + x : 0, o = p * kSnapVoxels + 8u * row + 4u * half;
    uint32_t d[4] = {fill_bits, fill_bits, fill_bits, fill_bits}, c[4] = {0u, 0u, 0u, 0u}, w[4] = {0u, 0u, 0u, 0u};
    if (inside) load4(reinterpret_cast<const uint32_t *>(dist), i, x, g.X, vec, fill_bits, d);
    *reinterpret_cast<uint4 *>(odist + o) = make_uint4(d[0], d[1], d[2], d[3]);
    if (colour) {
        if (inside) load4(colour, i, x, g.X, vec, 0u, c);
        *reinterpret_cast<uint4 *>(ocolour + o) = make_uint4(c[0], c[1], c[2], c[3]);
    }
    if (wv.mode == 0) {
        if (inside) load4(reinterpret_cast<const uint32_t *>(wv.f32), i, x, g.X, vec, 0u, w);
        *reinterpret_cast<uint4 *>(static_cast<uint32_t *>(oweights) + o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else if (wv.mode == 8) {
        gather_packed<8>(wv.packed, g, bx, by, bz, p, oweights);
    } else {
        gather_packed<16>(wv.packed, g, bx, by, bz, p, oweights);
    }
}

// element e of a snapshot's weight array of `sbits`-bit counts
__device__ inline uint32_t snap_count(const void *__restrict__ sweights, int sbits, size_t e) {
    return sbits == 8 ? (uint32_t)static_cast<const uint8_t *>(sweights)[e] : (uint32_t)static_cast<const uint16_t *>(sweights)[e];
}

// the counts of list position p (kSnapNone: zeros) -> the z-groups of brick (bx, by, bz) of a DBITS-bit packed array, by the thread of
// (4 x from 4 half, ly, z-group gi); sbits <= DBITS
template <int DBITS>
__device__ inline void scatter_packed(uint32_t *__restrict__ wp, const SnapGrid &g, uint32_t bx, uint32_t by, uint32_t bz, uint32_t p,
                                      const void *__restrict__ sweights, int sbits, uint32_t half, uint32_t ly, uint32_t gi) {
    constexpr uint32_t kPer = 32 / DBITS;
    const uint32_t x = bx * kSnapBrick + 4u * half, y = by * kSnapBrick + ly, z0 = bz * kSnapBrick + gi * kPer;
    if (y >= g.Y || z0 >= g.Z) return;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (p != kSnapNone) {
#pragma unroll
        for (uint32_t s = 0; s < kPer; s++) {
            if (z0 + s >= g.Z) break;   // (what a snapshot holds beyond the grid is not put into the volume)
            const size_t e = (size_t)p * kSnapVoxels + 64u * (gi * kPer + s) + 8u * ly + 4u * half;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) w[k] |= snap_count(sweights, sbits, e + k) << (DBITS * s);
        }
    }
    store4(wp, (size_t)g.X * g.Y * (z0 / kPer) + (size_t)g.X * y + x, x, g.X, (g.X & 3u) == 0u, w);
}

// One thread's share of brick (bx, by, bz) of the volume -- the half `half` of row `row` (ly = row & 7, lz = row >> 3) and, in the packed
// modes, one dword column of four -- from list position p of the snapshot, or the cleared state for kSnapNone.
// dmode: the volume's weight storage (0 / 8 / 16), sbits: the snapshot's element type (8 / 16 / 32); the host has made dmode hold sbits
// (the pointers are the calling kernel's own __restrict__ arguments; inlined before anything is optimised, so that
// snapshot_scatter_kernel compiles to what it was when this was its body)
__device__ __forceinline__ void scatter_brick(float *dist, float *wf32, uint32_t *wpacked, const int dmode, uint32_t *colour, const SnapGrid &g,
                                     const uint32_t fill_bits, const uint32_t bx, const uint32_t by, const uint32_t bz, const uint32_t p,
                                     const uint32_t half, const uint32_t row, const float *sdist, const void *sweights, const int sbits,
                                     const uint32_t *scolour) {
    const uint32_t x = bx * kSnapBrick + 4u * half, y = by * kSnapBrick + (row & 7u), z = bz * kSnapBrick + (row >> 3);
    const bool vec = (g.X & 3u) == 0u, stored = p != kSnapNone;
    if (y < g.Y && z < g.Z) {
        const size_t i = (size_t)g.X * g.Y * z + (size_t)g.X * y + x, o = (size_t)p * kSnapVoxels + 8u * row + 4u * half;
        uint32_t d[4] = {fill_bits, fill_bits, fill_bits, fill_bits};
        if (stored) {
            const uint4 q = *reinterpret_cast<const uint4 *>(sdist + o);
            d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
        }
        store4(reinterpret_cast<uint32_t *>(dist), i, x, g.X, vec, d);
        if (colour) {
            uint32_t c[4] = {0u, 0u, 0u, 0u};
            if (stored && scolour) {
                const uint4 q = *reinterpret_cast<const uint4 *>(scolour + o);
                c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
            }
            store4(colour, i, x, g.X, vec, c);
        }
        if (dmode == 0) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (stored) {
#pragma unroll
                for (uint32_t k = 0; k < 4; k++)
                    w[k] = sbits == 32 ? static_cast<const uint32_t *>(sweights)[o + k] : __float_as_uint((float)snap_count(sweights, sbits, o + k));
            }
            store4(reinterpret_cast<uint32_t *>(wf32), i, x, g.X, vec, w);
        }
    }
    // packed counts: the threads of the first 8 y x 2 (8-bit) or 4 (16-bit) z-groups, one dword column of four each
    if (dmode == 8 && row < 16u) scatter_packed<8>(wpacked, g, bx, by, bz, p, sweights, sbits, half, row & 7u, row >> 3);
    else if (dmode == 16 && row < 32u) scatter_packed<16>(wpacked, g, bx, by, bz, p, sweights, sbits, half, row & 7u, row >> 3);
}

// A workgroup takes kScatterBricks bricks next to each other along x: thread t the half t & 1 of row t >> 3 (ly = row & 7, lz = row >> 3)
// of brick (t >> 1) & 3, so that eight consecutive threads write 128 contiguous bytes of a dense row.
constexpr uint32_t kScatterBricks = 4;
__global__ __launch_bounds__(512) void snapshot_scatter_kernel(float *__restrict__ dist, float *__restrict__ wf32, uint32_t *__restrict__ wpacked,
                                                               const int dmode, uint32_t *__restrict__ colour, const SnapGrid g,
                                                               const uint32_t fill_bits, const uint32_t *__restrict__ map,
                                                               const float *__restrict__ sdist, const void *__restrict__ sweights, const int sbits,
                                                               const uint32_t *__restrict__ scolour) {
    const uint32_t half = threadIdx.x & 1u, row = threadIdx.x >> 3;
    const uint32_t bx = blockIdx.x * kScatterBricks + ((threadIdx.x >> 1) & (kScatterBricks - 1u)), by = blockIdx.y, bz = blockIdx.z;
    if (bx >= g.nbx) return;
    const uint32_t p = map[bx + g.nbx * (by + (size_t)g.nby * bz)];
    scatter_brick(dist, wf32, wpacked, dmode, colour, g, fill_bits, bx, by, bz, p, half, row, sdist, sweights, sbits, scolour);
}

// The same over the grid g of a volume that need not be the snapshot's: brick bD takes the source brick bD + from (from = -brick_shift,
// from.nb* the snapshot's brick grid, which `map` is indexed by); a brick whose source is outside that grid or not stored is cleared.
// A kernel of its own, so that the launch of tsdf_volume_restore is what it was.
__global__ __launch_bounds__(512) void snapshot_scatter_shifted_kernel(float *__restrict__ dist, float *__restrict__ wf32, uint32_t *__restrict__ wpacked,
                                                                       const int dmode, uint32_t *__restrict__ colour, const SnapGrid g,
                                                                       const uint32_t fill_bits, const uint32_t *__restrict__ map, const BrickShift from,
                                                                       const float *__restrict__ sdist, const void *__restrict__ sweights,
                                                                       const int sbits, const uint32_t *__restrict__ scolour) {
    const uint32_t half = threadIdx.x & 1u, row = threadIdx.x >> 3;
    const uint32_t bx = blockIdx.x * kScatterBricks + ((threadIdx.x >> 1) & (kScatterBricks - 1u)), by = blockIdx.y, bz = blockIdx.z;
    if (bx >= g.nbx) return;
    uint32_t s[3], p = kSnapNone;
    if (brick_moved(from, bx, by, bz, s)) p = map[s[0] + from.nbx * (s[1] + (size_t)from.nby * s[2])];
    scatter_brick(dist, wf32, wpacked, dmode, colour, g, fill_bits, bx, by, bz, p, half, row, sdist, sweights, sbits, scolour);
}

// Paging in (TSDF_RESTORE_KEEP_OTHERS): over the snapshot's list, not over the grid.  A workgroup takes kScatterBricks consecutive list
// positions -- neighbours along x where the list has them -- with the thread layout of the kernels above; brick bS of the snapshot's
// grid (nbx, nby) lands at bS + to (to = brick_shift, to.nb* the volume's brick grid) or, outside it, nowhere.
__global__ __launch_bounds__(512) void snapshot_page_in_kernel(float *__restrict__ dist, float *__restrict__ wf32, uint32_t *__restrict__ wpacked,
                                                               const int dmode, uint32_t *__restrict__ colour, const SnapGrid g,
                                                               const uint32_t *__restrict__ ids, const uint32_t n, const uint32_t nbx, const uint32_t nby,
                                                               const BrickShift to, const float *__restrict__ sdist, const void *__restrict__ sweights,
                                                               const int sbits, const uint32_t *__restrict__ scolour) {
    const uint32_t half = threadIdx.x & 1u, row = threadIdx.x >> 3;
    const uint32_t p = blockIdx.x * kScatterBricks + ((threadIdx.x >> 1) & (kScatterBricks - 1u));
    if (p >= n) return;
    const uint32_t b = ids[p];
    uint32_t d[3];
    if (!brick_moved(to, b % nbx, (b / nbx) % nby, b / (nbx * nby), d)) return;
    scatter_brick(dist, wf32, wpacked, dmode, colour, g, 0u, d[0], d[1], d[2], p, half, row, sdist, sweights, sbits, scolour);
}

// tsdf_snapshot_select: one flag per list entry -- its brick is inside the box, or with `outside` is not
__global__ __launch_bounds__(256) void select_flag_kernel(const uint32_t *__restrict__ ids, const uint32_t n, const uint32_t nbx, const uint32_t nby,
                                                          const BrickBox box, const uint32_t outside, uint32_t *__restrict__ flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = ids[i];
    const bool inside = brick_in_box(box, b % nbx, (b / nbx) % nby, b / (nbx * nby));
    flags[i] = inside != (outside != 0u) ? 1u : 0u;
}

// ... and, the flags scanned into bases (total: the scan's first total), a workgroup per entry of the source list: the id and the
// brick's rows, one uint4 per lane and array; wq: the uint4 words of a brick's weights (32, 64 or 128)
__global__ __launch_bounds__(128) void select_gather_kernel(const uint32_t *__restrict__ bases, const uint64_t *__restrict__ total, const uint32_t n,
                                                            const uint32_t *__restrict__ ids, const uint4 *__restrict__ sdist,
                                                            const uint4 *__restrict__ sweights, const uint4 *__restrict__ scolour, const uint32_t wq,
                                                            uint32_t *__restrict__ oids, uint4 *__restrict__ odist, uint4 *__restrict__ oweights,
                                                            uint4 *__restrict__ ocolour) {
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    const uint32_t base = bases[i], next = i + 1u < n ? bases[i + 1u] : (uint32_t)*total;
    if (next == base) return;
    constexpr uint32_t kQ = kSnapVoxels / 4u;   // the uint4 words of 512 dwords
    if (t == 0) oids[base] = ids[i];
    odist[(size_t)base * kQ + t] = sdist[(size_t)i * kQ + t];
    if (scolour) ocolour[(size_t)base * kQ + t] = scolour[(size_t)i * kQ + t];
    if (t < wq) oweights[(size_t)base * wq + t] = sweights[(size_t)i * wq + t];
}

}  // namespace tsdf

using namespace tsdf;

struct tsdf_snapshot : HandleOrder {
    int filled;             // a snapshot or an upload has gone into the handle
    uint32_t *ids;
    float *dist;
    void *weights;
    uint32_t *colours;
    size_t ids_cap, dist_cap, weights_cap, colours_cap;   // in bricks, floats, bytes, words
    uint32_t *flags;        // per brick of the grid: the live flag, then its list position
    uint32_t *map;          // per brick of the grid: its list position or kSnapNone
    size_t flags_cap, map_cap;
    uint64_t *parts;        // the scan's sums and totals
    size_t parts_cap;       // in words
    uint64_t *total_host;   // pinned: where the count of live bricks lands
    tsdf_snapshot_info info;
};

namespace {

void snapshot_free(tsdf_snapshot *s) {
    s->destroy();
    device_free_all(s->ids, s->dist, s->weights, s->colours, s->flags, s->map, s->parts);
    (void)hipHostFree(s->total_host);
    delete s;
}

// the texts of the handle's stream order (handle_order.hpp)
constexpr const char *kSnapOrder = "snapshot stream order", *kSnapEvent = "snapshot event", *kSnapWait = "snapshot wait";

uint64_t brick_count(const uint32_t size[3], uint32_t nb[3]) {
    for (int a = 0; a < 3; a++) nb[a] = (size[a] + kSnapBrick - 1) / kSnapBrick;
    return (uint64_t)nb[0] * nb[1] * nb[2];
}

uint64_t snapshot_bytes(const tsdf_snapshot_info &i) {
    const uint64_t per_brick = 4u + kSnapVoxels * (4u + i.weight_bits / 8u + ((i.flags & TSDF_SNAPSHOT_COLOUR) ? 4u : 0u));
    return i.n_bricks * per_brick;
}

// the four arrays for what info describes
hipError_t snapshot_reserve(tsdf_snapshot *s) {
    const size_t n = (size_t)s->info.n_bricks;
    hipError_t e = device_reserve(s->ids, s->ids_cap, n);
    if (e == hipSuccess) e = device_reserve(s->dist, s->dist_cap, n * kSnapVoxels);
    if (e == hipSuccess) e = device_reserve_bytes(s->weights, s->weights_cap, n * kSnapVoxels * (s->info.weight_bits / 8u));
    if (e == hipSuccess && (s->info.flags & TSDF_SNAPSHOT_COLOUR)) e = device_reserve(s->colours, s->colours_cap, n * kSnapVoxels);
    return e;
}

int refuse_volume(const tsdf_volume *v, const char *who) {
    TSDF_REQUIRE(!v->slab && v->g.z_store_begin == 0 && v->g.z_store_end == v->g.Z,
                 "%s: a Z-slab volume (tsdf_volume_create_slab) is not supported", who);
    TSDF_REQUIRE(!v->nodes, "%s: the volume has a materialised deformation-node array, which a snapshot does not carry", who);
    return TSDF_OK;
}

// What every restore does before its launch: the volume's storage made to hold the snapshot's, the stream behind the handle, the marks
// of a writer of distances and weights.  keep: the data in the volume stays (TSDF_RESTORE_KEEP_OTHERS), so its bound does too.
int restore_prepare(tsdf_volume *v, const tsdf_snapshot *s, bool keep) {
    const tsdf_snapshot_info &info = s->info;
    // what a writer of distances and weights owes the volume (common.hpp, "THE INVARIANT"): the tightening in flight first, then
    // every flag is rebuilt from everything
    int rc = occupancy_join(v);
    if (rc != TSDF_OK) return rc;
    // the storage: the wider of what the volume has and what the snapshot carries (a pinned volume is fp32 already); widening converts
    // the counts the volume holds
    const uint32_t now = v->wmode == 0 ? 32u : (uint32_t)v->wmode;
    if (info.weight_bits > now) {
        rc = tsdf_volume_set_weight_storage(v, (int)info.weight_bits);
        if (rc != TSDF_OK) return rc;
    }
    if (info.flags & TSDF_SNAPSHOT_COLOUR) {
        rc = tsdf_volume_enable_colour(v, 1);
        if (rc != TSDF_OK) return rc;
    }
    rc = s->join(v->stream, kSnapOrder);
    if (rc != TSDF_OK) return rc;
    v->occ_dirty = 1;
    v->occ_scan_all = 1;
    v->prepared_valid = 0;
    v->weight_bound = keep ? std::max(v->weight_bound, info.weight_bound) : info.weight_bound;
    return TSDF_OK;
}

// tsdf_volume_restore_shifted with a shift of 64 bits (tsdf_volume_shift negates an int32)
int restore_shifted(tsdf_volume *v, const tsdf_snapshot *s, const long long shift[3], uint32_t flags) {
    TSDF_REQUIRE(s->filled, "tsdf_volume_restore_shifted: the handle has never been filled (tsdf_volume_snapshot, tsdf_snapshot_upload)");
    TSDF_REQUIRE((flags & ~(uint32_t)TSDF_RESTORE_KEEP_OTHERS) == 0, "tsdf_volume_restore_shifted: unknown flags %#x", flags);
    int rc = refuse_volume(v, "tsdf_volume_restore_shifted");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(v->device == s->device, "tsdf_volume_restore_shifted: the handle was created on device %d, the volume on device %d", s->device,
                 v->device);
    const bool keep = (flags & TSDF_RESTORE_KEEP_OTHERS) != 0;
    rc = restore_prepare(v, s, keep);
    if (rc != TSDF_OK) return rc;
    const tsdf_snapshot_info &info = s->info;
    const uint32_t size[3] = {v->g.X, v->g.Y, v->g.Z};
    uint32_t nb[3];
    brick_count(size, nb);
    const SnapGrid dg = {size[0], size[1], size[2], nb[0], nb[1], nb[2]};
    uint32_t fill_bits;
    std::memcpy(&fill_bits, &info.fill_distance, sizeof(fill_bits));
    const uint32_t *scolour = (info.flags & TSDF_SNAPSHOT_COLOUR) ? s->colours : nullptr;
    if (keep) {
        // over the list: source brick + shift, inside the volume's grid
        const BrickShift to = {shift[0], shift[1], shift[2], nb[0], nb[1], nb[2]};
        const uint32_t n = (uint32_t)info.n_bricks;
        if (n)
            hipLaunchKernelGGL(snapshot_page_in_kernel, grid_for(n, kScatterBricks), dim3(64 * 2 * kScatterBricks), 0, v->stream, v->dist, v->weight,
                               v->wpacked, v->wmode, v->colour, dg, s->ids, n, info.bricks[0], info.bricks[1], to, s->dist, s->weights,
                               (int)info.weight_bits, scolour);
    } else {
        // over the grid: destination brick - shift, inside the snapshot's grid
        const BrickShift from = {-shift[0], -shift[1], -shift[2], info.bricks[0], info.bricks[1], info.bricks[2]};
        hipLaunchKernelGGL(snapshot_scatter_shifted_kernel, dim3((dg.nbx + kScatterBricks - 1) / kScatterBricks, dg.nby, dg.nbz),
                           dim3(64 * 2 * kScatterBricks), 0, v->stream, v->dist, v->weight, v->wpacked, v->wmode, v->colour, dg, fill_bits, s->map, from,
                           s->dist, s->weights, (int)info.weight_bits, scolour);
    }
    TSDF_HIP(hipGetLastError(), "snapshot shifted scatter kernel failed");
    return s->leave(v->stream, kSnapEvent);
}

// tsdf_snapshot_select on a stream of the caller's choice
int snapshot_select(const tsdf_snapshot *src, const BrickBox &box, uint32_t flags, tsdf_snapshot *dst, hipStream_t stream) {
    TSDF_REQUIRE(dst != src, "tsdf_snapshot_select: dst is src");
    TSDF_REQUIRE(src->filled, "tsdf_snapshot_select: src has never been filled (tsdf_volume_snapshot, tsdf_snapshot_upload)");
    TSDF_REQUIRE((flags & ~(uint32_t)TSDF_SELECT_OUTSIDE) == 0, "tsdf_snapshot_select: unknown flags %#x", flags);
    TSDF_REQUIRE(src->device == dst->device, "tsdf_snapshot_select: src was created on device %d, dst on device %d", src->device, dst->device);
    int rc = src->join(stream, kSnapOrder);
    if (rc == TSDF_OK) rc = dst->join(stream, kSnapOrder);   // (what still reads dst's arrays)
    if (rc != TSDF_OK) return rc;
    dst->filled = 0;
    tsdf_snapshot_info info = src->info;
    const uint32_t n = (uint32_t)info.n_bricks;
    const uint64_t total = (uint64_t)info.bricks[0] * info.bricks[1] * info.bricks[2];
    const uint32_t n_parts = mesh_scan_parts(n);
    hipError_t e = device_reserve(dst->flags, dst->flags_cap, (size_t)n);
    if (e == hipSuccess) e = device_reserve(dst->map, dst->map_cap, (size_t)total);
    if (e == hipSuccess) e = device_reserve(dst->parts, dst->parts_cap, 2 * ((size_t)n_parts + 1));
    if (e != hipSuccess) return hip_fail(e, "snapshot select scratch alloc failed");
    uint64_t *count = dst->parts + 2 * (size_t)n_parts;
    *dst->total_host = 0;
    if (n) {
        hipLaunchKernelGGL(select_flag_kernel, grid_for(n, 256), dim3(256), 0, stream, src->ids, n, info.bricks[0], info.bricks[1], box,
                           flags & TSDF_SELECT_OUTSIDE, dst->flags);
        mesh_scan(ArrayCounts{dst->flags, n, nullptr, 0u}, n_parts, dst->parts, stream);
        TSDF_HIP(hipGetLastError(), "snapshot select flag kernels failed");
        TSDF_HIP(hipMemcpyAsync(dst->total_host, count, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "snapshot select count download");
        TSDF_HIP(hipStreamSynchronize(stream), "snapshot select count");   // the one synchronisation: dst is sized by the count
    }
    info.n_bricks = *dst->total_host;
    info.bytes = snapshot_bytes(info);
    dst->info = info;
    e = snapshot_reserve(dst);
    if (e != hipSuccess) return hip_fail(e, "snapshot select array alloc failed");
    TSDF_HIP(hipMemsetAsync(dst->map, 0xff, (size_t)total * sizeof(uint32_t), stream), "snapshot select map");
    if (info.n_bricks) {
        const bool colour = (info.flags & TSDF_SNAPSHOT_COLOUR) != 0;
        hipLaunchKernelGGL(select_gather_kernel, dim3(n), dim3(128), 0, stream, dst->flags, count, n, src->ids,
                           reinterpret_cast<const uint4 *>(src->dist), static_cast<const uint4 *>(src->weights),
                           colour ? reinterpret_cast<const uint4 *>(src->colours) : nullptr, 4u * info.weight_bits,
                           dst->ids, reinterpret_cast<uint4 *>(dst->dist), static_cast<uint4 *>(dst->weights),
                           colour ? reinterpret_cast<uint4 *>(dst->colours) : nullptr);
        hipLaunchKernelGGL(snapshot_map_kernel, grid_for(info.n_bricks, 256), dim3(256), 0, stream, dst->ids, (uint32_t)info.n_bricks, dst->map);
    }
    TSDF_HIP(hipGetLastError(), "snapshot select gather kernels failed");
    dst->filled = 1;
    rc = src->leave(stream, kSnapEvent);
    return rc == TSDF_OK ? dst->leave(stream, kSnapEvent) : rc;
}

}  // namespace

extern "C" {

int tsdf_snapshot_create(tsdf_snapshot **out) {
    return handle_create(out, "tsdf_snapshot_create", "snapshot alloc failed", [](tsdf_snapshot *s) {
        std::memset(s, 0, sizeof(*s));
        hipError_t e = s->create();
        if (e == hipSuccess) e = hipHostMalloc((void **)&s->total_host, sizeof(uint64_t), hipHostMallocDefault);
        if (e == hipSuccess) *s->total_host = 0;
        return e;
    }, snapshot_free);
}

void tsdf_snapshot_destroy(tsdf_snapshot *s) {
    if (s) snapshot_free(s);
}

int tsdf_volume_snapshot(const tsdf_volume *cv, uint32_t flags, tsdf_snapshot *s) {
    TSDF_REQUIRE(cv && s, "tsdf_volume_snapshot: null argument");
    TSDF_REQUIRE(flags == 0, "tsdf_volume_snapshot: unknown flags %#x", flags);
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);
    const int rcv = refuse_volume(v, "tsdf_volume_snapshot");
    if (rcv != TSDF_OK) return rcv;
    TSDF_REQUIRE(v->device == s->device, "tsdf_volume_snapshot: the handle was created on device %d, the volume on device %d", s->device, v->device);
    const Geom &g = v->g;
    tsdf_snapshot_info info;
    std::memset(&info, 0, sizeof(info));
    info.size[0] = g.X; info.size[1] = g.Y; info.size[2] = g.Z;
    const uint64_t total = brick_count(info.size, info.bricks);
    TSDF_REQUIRE(total > 0 && total < kSnapNone, "tsdf_volume_snapshot: %llu bricks do not fit 32-bit brick ids", (unsigned long long)total);
    info.flags = v->colour ? TSDF_SNAPSHOT_COLOUR : 0u;
    info.weight_bits = v->wmode == 0 ? 32u : (uint32_t)v->wmode;
    info.weight_bound = v->wmode == 0 ? 0u : v->weight_bound;
    info.fill_distance = g.trunc;
    info.voxel_size[0] = g.vs.x; info.voxel_size[1] = g.vs.y; info.voxel_size[2] = g.vs.z;
    info.offset[0] = g.offset.x; info.offset[1] = g.offset.y; info.offset[2] = g.offset.z;
    const int rcj = s->join(v->stream, kSnapOrder);   // what is in flight on the handle
    if (rcj != TSDF_OK) return rcj;
    s->filled = 0;
    const uint32_t n_parts = mesh_scan_parts((uint32_t)total);
    hipError_t e = device_reserve(s->flags, s->flags_cap, (size_t)total);
    if (e == hipSuccess) e = device_reserve(s->map, s->map_cap, (size_t)total);
    if (e == hipSuccess) e = device_reserve(s->parts, s->parts_cap, 2 * ((size_t)n_parts + 1));
    if (e != hipSuccess) return hip_fail(e, "snapshot scratch alloc failed");

    const SnapGrid sg = {g.X, g.Y, g.Z, info.bricks[0], info.bricks[1], info.bricks[2]};
    const WeightView wv = {v->weight, v->wpacked, v->wmode};
    uint32_t fill_bits;
    std::memcpy(&fill_bits, &g.trunc, sizeof(fill_bits));
    hipLaunchKernelGGL(snapshot_flag_kernel, dim3(sg.nby, sg.nbz), dim3(256), 0, v->stream, v->dist, wv, v->colour, sg, fill_bits, s->flags);
    mesh_scan(ArrayCounts{s->flags, (uint32_t)total, nullptr, 0u}, n_parts, s->parts, v->stream);
    TSDF_HIP(hipGetLastError(), "snapshot flag kernels failed");
    TSDF_HIP(hipMemcpyAsync(s->total_host, s->parts + 2 * (size_t)n_parts, sizeof(uint64_t), hipMemcpyDeviceToHost, v->stream), "snapshot count download");
    TSDF_HIP(hipStreamSynchronize(v->stream), "snapshot count");   // the one synchronisation: the arrays are sized by the count
    info.n_bricks = *s->total_host;
    info.bytes = snapshot_bytes(info);
    s->info = info;
    e = snapshot_reserve(s);
    if (e != hipSuccess) return hip_fail(e, "snapshot array alloc failed");
    hipLaunchKernelGGL(snapshot_list_kernel, grid_for(total, 256), dim3(256), 0, v->stream, s->flags, s->parts + 2 * (size_t)n_parts, (uint32_t)total,
                       s->ids, s->map);
    if (info.n_bricks)
        hipLaunchKernelGGL(snapshot_gather_kernel, dim3((uint32_t)info.n_bricks), dim3(128), 0, v->stream, v->dist, wv, v->colour, sg, fill_bits, s->ids,
                           s->dist, s->weights, s->colours);
    TSDF_HIP(hipGetLastError(), "snapshot gather kernels failed");
    s->filled = 1;
    return s->leave(v->stream, kSnapEvent);
}

int tsdf_volume_restore(tsdf_volume *v, const tsdf_snapshot *s) {
    TSDF_REQUIRE(v && s, "tsdf_volume_restore: null argument");
    TSDF_REQUIRE(s->filled, "tsdf_volume_restore: the handle has never been filled (tsdf_volume_snapshot, tsdf_snapshot_upload)");
    const int rcv = refuse_volume(v, "tsdf_volume_restore");
    if (rcv != TSDF_OK) return rcv;
    const tsdf_snapshot_info &info = s->info;
    TSDF_REQUIRE(v->g.X == info.size[0] && v->g.Y == info.size[1] && v->g.Z == info.size[2],
                 "tsdf_volume_restore: the snapshot is of a %u x %u x %u grid, the volume is %u x %u x %u", info.size[0], info.size[1], info.size[2],
                 v->g.X, v->g.Y, v->g.Z);
    TSDF_REQUIRE(v->device == s->device, "tsdf_volume_restore: the handle was created on device %d, the volume on device %d", s->device, v->device);
    const int rc = restore_prepare(v, s, false);
    if (rc != TSDF_OK) return rc;
    const SnapGrid sg = {info.size[0], info.size[1], info.size[2], info.bricks[0], info.bricks[1], info.bricks[2]};
    uint32_t fill_bits;
    std::memcpy(&fill_bits, &info.fill_distance, sizeof(fill_bits));
    hipLaunchKernelGGL(snapshot_scatter_kernel, dim3((sg.nbx + kScatterBricks - 1) / kScatterBricks, sg.nby, sg.nbz), dim3(64 * 2 * kScatterBricks), 0, v->stream, v->dist, v->weight, v->wpacked, v->wmode, v->colour, sg, fill_bits,
                       s->map, s->dist, s->weights, (int)info.weight_bits, (info.flags & TSDF_SNAPSHOT_COLOUR) ? s->colours : nullptr);
    TSDF_HIP(hipGetLastError(), "snapshot scatter kernel failed");
    return s->leave(v->stream, kSnapEvent);   // the handle's arrays are read by what has just been enqueued
}

// ---- rolling volume (include/tsdf_amd.h) ---------------------------------------------------------------------------------------------
int tsdf_volume_restore_shifted(tsdf_volume *v, const tsdf_snapshot *s, const int32_t brick_shift[3], uint32_t flags) {
    TSDF_REQUIRE(v && s && brick_shift, "tsdf_volume_restore_shifted: null argument");
    const long long shift[3] = {brick_shift[0], brick_shift[1], brick_shift[2]};
    return restore_shifted(v, s, shift, flags);
}

int tsdf_snapshot_select(const tsdf_snapshot *src, const int32_t lo[3], const int32_t hi[3], uint32_t flags, tsdf_snapshot *dst) {
    TSDF_REQUIRE(src && lo && hi && dst, "tsdf_snapshot_select: null argument");
    const BrickBox box = {{lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}};
    return snapshot_select(src, box, flags, dst, nullptr);
}

int tsdf_volume_shift(tsdf_volume *v, const int32_t box_shift[3], tsdf_snapshot *work, tsdf_snapshot *leaving) {
    TSDF_REQUIRE(v && box_shift && work, "tsdf_volume_shift: null argument");
    TSDF_REQUIRE(leaving != work, "tsdf_volume_shift: leaving is work");
    int rc = refuse_volume(v, "tsdf_volume_shift");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(v->g.X % kSnapBrick == 0 && v->g.Y % kSnapBrick == 0 && v->g.Z % kSnapBrick == 0,
                 "tsdf_volume_shift: the grid is %u x %u x %u, not a multiple of 8 on every axis: the voxels of a partial brick cut off at the border "
                 "would be lost without appearing in leaving",
                 v->g.X, v->g.Y, v->g.Z);
    TSDF_REQUIRE(!v->classes, "tsdf_volume_shift: classes are enabled on this volume; snapshots do not carry class words, which would stay behind "
                              "while the geometry moves");
    TSDF_REQUIRE(v->device == work->device && (!leaving || v->device == leaving->device),
                 "tsdf_volume_shift: a handle was created on another device than the volume's %d", v->device);
    const bool zero = box_shift[0] == 0 && box_shift[1] == 0 && box_shift[2] == 0;
    if (zero && !leaving) return TSDF_OK;
    rc = tsdf_volume_snapshot(v, 0, work);
    if (rc != TSDF_OK) return rc;
    if (leaving) {
        // (work's offset is the volume's, still the old one; with no shift every brick stays)
        rc = snapshot_select(work, staying_box(box_shift, work->info.bricks), TSDF_SELECT_OUTSIDE, leaving, v->stream);
        if (rc != TSDF_OK) return rc;
    }
    if (zero) return TSDF_OK;
    const long long back[3] = {-(long long)box_shift[0], -(long long)box_shift[1], -(long long)box_shift[2]};
    rc = restore_shifted(v, work, back, 0);
    if (rc != TSDF_OK) return rc;
    const Geom &g = v->g;
    return tsdf_volume_set_offset(v, shifted_offset(g.offset.x, box_shift[0], g.vs.x), shifted_offset(g.offset.y, box_shift[1], g.vs.y),
                                  shifted_offset(g.offset.z, box_shift[2], g.vs.z));
}

int tsdf_snapshot_get_info(const tsdf_snapshot *s, tsdf_snapshot_info *info) {
    TSDF_REQUIRE(s && info, "tsdf_snapshot_get_info: null argument");
    const int rc = s->wait(kSnapWait);
    if (rc != TSDF_OK) return rc;
    *info = s->info;
    return TSDF_OK;
}

int tsdf_snapshot_buffers(const tsdf_snapshot *s, const uint32_t **device_bricks, const float **device_distances, const void **device_weights,
                          const uint32_t **device_colours) {
    TSDF_REQUIRE(s && device_bricks && device_distances && device_weights && device_colours, "tsdf_snapshot_buffers: null argument");
    TSDF_REQUIRE(s->filled, "tsdf_snapshot_buffers: the handle has never been filled (tsdf_volume_snapshot, tsdf_snapshot_upload)");
    const int rc = s->wait(kSnapWait);
    if (rc != TSDF_OK) return rc;
    const bool any = s->info.n_bricks != 0;
    *device_bricks = any ? s->ids : nullptr;
    *device_distances = any ? s->dist : nullptr;
    *device_weights = any ? s->weights : nullptr;
    *device_colours = any && (s->info.flags & TSDF_SNAPSHOT_COLOUR) ? s->colours : nullptr;
    return TSDF_OK;
}

int tsdf_snapshot_download(const tsdf_snapshot *s, uint32_t *host_bricks, float *host_distances, void *host_weights, uint32_t *host_colours) {
    TSDF_REQUIRE(s, "tsdf_snapshot_download: null argument");
    TSDF_REQUIRE(s->filled, "tsdf_snapshot_download: the handle has never been filled (tsdf_volume_snapshot, tsdf_snapshot_upload)");
    const bool colour = (s->info.flags & TSDF_SNAPSHOT_COLOUR) != 0;
    TSDF_REQUIRE(host_bricks && host_distances && host_weights && (host_colours || !colour), "tsdf_snapshot_download: null argument");
    const int rc = s->wait(kSnapWait);
    if (rc != TSDF_OK) return rc;
    const size_t n = (size_t)s->info.n_bricks, nv = n * kSnapVoxels;
    if (n == 0) return TSDF_OK;
    TSDF_HIP(hipMemcpy(host_bricks, s->ids, n * sizeof(uint32_t), hipMemcpyDeviceToHost), "snapshot download");
    TSDF_HIP(hipMemcpy(host_distances, s->dist, nv * sizeof(float), hipMemcpyDeviceToHost), "snapshot download");
    TSDF_HIP(hipMemcpy(host_weights, s->weights, nv * (s->info.weight_bits / 8u), hipMemcpyDeviceToHost), "snapshot download");
    if (colour) TSDF_HIP(hipMemcpy(host_colours, s->colours, nv * sizeof(uint32_t), hipMemcpyDeviceToHost), "snapshot download");
    return TSDF_OK;
}

int tsdf_snapshot_upload(tsdf_snapshot *s, const tsdf_snapshot_info *in, const uint32_t *host_bricks, const float *host_distances,
                         const void *host_weights, const uint32_t *host_colours) {
    TSDF_REQUIRE(s && in, "tsdf_snapshot_upload: null argument");
    // everything is checked on the host before a device is touched
    for (int a = 0; a < 3; a++)
        TSDF_REQUIRE(in->size[a] >= 1 && in->size[a] <= 65535, "tsdf_snapshot_upload: size[%d] = %u is not in 1 .. 65535", a, in->size[a]);
    TSDF_REQUIRE(in->weight_bits == 8 || in->weight_bits == 16 || in->weight_bits == 32, "tsdf_snapshot_upload: weight_bits = %u is not 8, 16 or 32",
                 in->weight_bits);
    TSDF_REQUIRE((in->flags & ~(uint32_t)TSDF_SNAPSHOT_COLOUR) == 0, "tsdf_snapshot_upload: unknown flags %#x", in->flags);
    tsdf_snapshot_info info;
    std::memset(&info, 0, sizeof(info));
    std::memcpy(info.size, in->size, sizeof(info.size));
    const uint64_t total = brick_count(info.size, info.bricks);
    TSDF_REQUIRE(total < kSnapNone, "tsdf_snapshot_upload: %llu bricks do not fit 32-bit brick ids", (unsigned long long)total);
    TSDF_REQUIRE(in->n_bricks <= total, "tsdf_snapshot_upload: n_bricks = %llu, the grid has %llu bricks", (unsigned long long)in->n_bricks,
                 (unsigned long long)total);
    const bool colour = (in->flags & TSDF_SNAPSHOT_COLOUR) != 0;
    const size_t n = (size_t)in->n_bricks, nv = n * kSnapVoxels;
    TSDF_REQUIRE(n == 0 || (host_bricks && host_distances && host_weights && (host_colours || !colour)), "tsdf_snapshot_upload: null array");
    for (size_t i = 0; i < n; i++) {
        TSDF_REQUIRE(host_bricks[i] < total, "tsdf_snapshot_upload: brick id %u at %zu is not below the brick count %llu", host_bricks[i], i,
                     (unsigned long long)total);
        TSDF_REQUIRE(i == 0 || host_bricks[i] > host_bricks[i - 1], "tsdf_snapshot_upload: brick ids are not strictly ascending at %zu", i);
    }
    info.flags = in->flags;
    info.weight_bits = in->weight_bits;
    info.fill_distance = in->fill_distance;
    std::memcpy(info.voxel_size, in->voxel_size, sizeof(info.voxel_size));
    std::memcpy(info.offset, in->offset, sizeof(info.offset));
    info.n_bricks = in->n_bricks;
    uint32_t top = 0;   // counts: the largest in the array, whatever the caller's info says
    if (info.weight_bits == 8)
        for (size_t i = 0; i < nv; i++) top = std::max<uint32_t>(top, static_cast<const uint8_t *>(host_weights)[i]);
    else if (info.weight_bits == 16)
        for (size_t i = 0; i < nv; i++) top = std::max<uint32_t>(top, static_cast<const uint16_t *>(host_weights)[i]);
    info.weight_bound = top;
    info.bytes = snapshot_bytes(info);

    int rc = s->wait(kSnapWait);
    if (rc != TSDF_OK) return rc;
    s->filled = 0;
    s->info = info;
    hipError_t e = snapshot_reserve(s);
    if (e == hipSuccess) e = device_reserve(s->map, s->map_cap, (size_t)total);
    if (e != hipSuccess) return hip_fail(e, "snapshot array alloc failed");
    if (n) {
        TSDF_HIP(hipMemcpy(s->ids, host_bricks, n * sizeof(uint32_t), hipMemcpyHostToDevice), "snapshot upload");
        TSDF_HIP(hipMemcpy(s->dist, host_distances, nv * sizeof(float), hipMemcpyHostToDevice), "snapshot upload");
        TSDF_HIP(hipMemcpy(s->weights, host_weights, nv * (info.weight_bits / 8u), hipMemcpyHostToDevice), "snapshot upload");
        if (colour) TSDF_HIP(hipMemcpy(s->colours, host_colours, nv * sizeof(uint32_t), hipMemcpyHostToDevice), "snapshot upload");
    }
    TSDF_HIP(hipMemsetAsync(s->map, 0xff, (size_t)total * sizeof(uint32_t), nullptr), "snapshot map");
    if (n) hipLaunchKernelGGL(snapshot_map_kernel, grid_for(n, 256), dim3(256), 0, nullptr, s->ids, (uint32_t)n, s->map);
    TSDF_HIP(hipGetLastError(), "snapshot map kernel failed");
    TSDF_HIP(hipStreamSynchronize(nullptr), "snapshot upload");
    s->filled = 1;
    return TSDF_OK;
}

int tsdf_snapshot_scratch_bytes(const tsdf_snapshot *s, uint64_t *bytes) {
    TSDF_REQUIRE(s && bytes, "tsdf_snapshot_scratch_bytes: null argument");
    *bytes = (uint64_t)(s->flags_cap + s->map_cap) * sizeof(uint32_t) + (uint64_t)s->parts_cap * sizeof(uint64_t);
    return TSDF_OK;
}

}  // extern "C"
