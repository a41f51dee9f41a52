// Reachability for gfx950 (include/tsdf_amd.h, "reachability"): the travel cost from seed points through traversable
// voxels in the 10-14-17 chamfer metric without corner cutting, the voxel paths back to the seeds, and the nearest voxel of every
// frontier cluster.  No reference counterpart.  Nothing of a volume, an ESDF or an explorer is written.
//
//   TraversableFlag       TRAVERSABLE per voxel (rule 2), the ballot mask per 64 voxel ids and the count: voxel_set.hpp's flag walk
//   reach_init_kernel     costs to UNREACHED, the per-brick dirty words of both parities to 0
//   reach_seed_kernel     a lane per seed: a plain store of 0 (idempotent); its brick and the bricks that see it dirty for round 0
//   reach_relax_kernel    one round: a workgroup per brick of 8^3 voxels; a dirty brick stages its 10^3 tile (its own voxels and a halo of
//                         one) in LDS, relaxes D(v) = min(D(v), D(u) + c(u, v)) there until a sweep changes nothing, stores what changed
//                         and marks for the next round the bricks that see a changed voxel in their halo
//   reach_stats_kernel    reached voxels, seed voxels and the largest cost: wave, then LDS, then one set of integer atomics a workgroup
//   reach_lookup_kernel   a lane per point
//   reach_paths_kernel    a lane per goal walks to a seed (rule 8): dependent loads, latency-bound by nature
//   reach_rank_kernel     a lane per listed frontier voxel: one 64-bit atomicMin of (cost << 32 | id) into its cluster's row, found by
//   reach_unpack_kernel   a binary search of the table's ascending labels; then the rows as tsdf_reach_cluster
//
// Why the bytes are unique.  The field is the one fixed point of D(v) = min(D(v), D(u) + c(u, v)) over admissible steps with D = 0 at the
// seeds.  Every value any kernel stores is 0 at a seed or a stored value plus a step's cost, so by induction the length of a real path:
// an upper bound of D.  Values only fall.  A brick reads its halo while the owners may be storing: whatever it reads is such an upper
// bound, old or new (a word is one aligned 32-bit store; nothing tears), and an owner that lowers a voxel on its outer layer marks every
// brick that sees the voxel for the NEXT round, which is another launch and reads the stored value.  So nothing rests on a fresh read,
// and when a round marks nothing every brick is at its local fixed point over final halo values: the global one.  The owner of a voxel
// is the only writer of its word in a round: no atomics on the cost array, no float atomics anywhere, no grid-wide barrier, no lane or
// workgroup waits for another, and every loop has a stated bound.
#include "common.hpp"
#include "field_sample.hpp"
#include "voxel_set.hpp"

#ifndef TSDF_REACH_BATCH
#define TSDF_REACH_BATCH 8   // rounds enqueued between two reads of the round words (DESIGN.md 31 has the measurement)
#endif

namespace tsdf {

constexpr uint32_t kUnreached = TSDF_REACH_UNREACHED;
constexpr uint32_t kReachBrick = 8;          // voxels per side of a brick
constexpr uint32_t kReachBatch = TSDF_REACH_BATCH;
constexpr uint32_t kReachMaxBatch = 32;      // round words the handle holds
static_assert(kReachBatch >= 1 && kReachBatch <= kReachMaxBatch, "a batch fits the round words");
constexpr uint64_t kReachMaxPoints = (uint64_t)0x7fffffff * 256;   // what a launch of 256-lane workgroups holds

// The tile of a brick in LDS: 10 planes of 10 rows of 10 words, rows 24 words apart.  A wave owns one 8 x 8 plane of the brick, so the 32
// lanes that share an LDS cycle read four rows of eight consecutive words; 24 words apart they fall on banks 0-7, 24-31, 16-23 and 8-15
// of the 32 a ds_read_b32 sees: conflict-free for every one of the 26 neighbour offsets, which shift all lanes alike.  (10 apart, rows
// 0 and 3 share six banks and every read takes two cycles.)  2400 words, 9600 bytes; with a traversable byte per tile word (2400 bytes) and
// the mark word the workgroup holds 12 KiB of LDS (the compiler reports 12 264 bytes), far from limiting the workgroups a CU holds by its
// wave slots.
constexpr uint32_t kTileRow = 24, kTilePlane = 10 * kTileRow, kTileWords = 10 * kTilePlane;

// the handle's words on the device, mirrored in pinned host memory
struct ReachWords {
    unsigned long long n_traversable, n_reached, n_seed_voxels, max_cost_reached;
    uint32_t round[kReachMaxBatch];   // per round of a batch: the workgroups that marked a brick for the next round
};

struct ReachBricks {
    uint32_t x, y, z, n;   // bricks per axis (whole or partial) and in all
};

inline ReachBricks reach_bricks(const VoxelGrid &g) {
    ReachBricks b = {(g.X + kReachBrick - 1) / kReachBrick, (g.Y + kReachBrick - 1) / kReachBrick, (g.Z + kReachBrick - 1) / kReachBrick, 0};
    b.n = b.x * b.y * b.z;   // (<= 2^32 / 512 whole bricks and the partial ones: far below 2^31)
    return b;
}

// Rule 4 / 7: the voxel of a world point with the geometry's CURRENT offset, every fp32 operation rounded on its own; false for a
// coordinate that is not finite (the comparisons fail) and for an index off the grid (the sides are below 2^16: exact floats).
__device__ inline bool reach_point_voxel(const Geom &g, const float *__restrict__ p, uint32_t &x, uint32_t &y, uint32_t &z) {
    const float fx = floorf((p[0] - g.offset.x) / g.vs.x), fy = floorf((p[1] - g.offset.y) / g.vs.y), fz = floorf((p[2] - g.offset.z) / g.vs.z);
    if (!(fx >= 0.0f && fx < (float)g.X && fy >= 0.0f && fy < (float)g.Y && fz >= 0.0f && fz < (float)g.Z)) return false;
    x = (uint32_t)fx;
    y = (uint32_t)fy;
    z = (uint32_t)fz;
    return true;
}

// neighbour k = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) of the 27 (13: the voxel itself): rule 8's order is ascending k
__host__ __device__ constexpr int nb_dx(int k) { return k % 3 - 1; }
__host__ __device__ constexpr int nb_dy(int k) { return (k / 3) % 3 - 1; }
__host__ __device__ constexpr int nb_dz(int k) { return k / 9 - 1; }
__host__ __device__ constexpr int nb_axes(int k) { return (nb_dx(k) != 0) + (nb_dy(k) != 0) + (nb_dz(k) != 0); }
__host__ __device__ constexpr uint32_t nb_cost(int k) {
    return nb_axes(k) == 1 ? TSDF_REACH_COST_FACE : nb_axes(k) == 2 ? TSDF_REACH_COST_EDGE : TSDF_REACH_COST_CORNER;
}
// the bits (same numbering) of the 2, 4 or 8 voxels a step to neighbour k needs traversable: every w with w_a in {0, d_a} (rule 3)
__host__ __device__ constexpr uint32_t nb_needs(int k) {
    uint32_t m = 0;
    for (int c = 0; c < 2; c++)
        for (int b = 0; b < 2; b++)
            for (int a = 0; a < 2; a++) m |= 1u << ((c * nb_dz(k) + 1) * 9 + (b * nb_dy(k) + 1) * 3 + (a * nb_dx(k) + 1));
    return m;
}
constexpr uint32_t kFaceSteps = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22);

// TRAVERSABLE (rule 2): not occupied -- an unknown voxel only with THROUGH_UNKNOWN -- and, with an ESDF, at least the clearance away from
// the nearest surface.  One counter, into ReachWords::n_traversable; the mask is read by id, never listed.
struct TraversableFlag {
    static constexpr uint32_t kCounts = 1, kListed = 0;
    const float *dist;
    WeightView wv;
    const float *esdf;
    float clearance;
    int through_unknown;
    __device__ uint32_t operator()(uint32_t id, const VoxelGrid &grid) const {
        uint32_t x, y, z;
        grid.split(id, x, y, z);
        bool ok = voxel_observed(wv, (size_t)grid.X * grid.Y, (size_t)grid.X * y + x, z) ? !voxel_occupied(dist, id) : through_unknown != 0;
        if (ok && esdf) ok = esdf[id] >= clearance;   // (false for NaN)
        return ok ? 1u : 0u;
    }
};

__global__ __launch_bounds__(256) void reach_init_kernel(uint32_t *__restrict__ cost, const uint32_t n, uint32_t *__restrict__ dirty,
                                                         const uint32_t n_dirty) {
    const uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;   // four words a lane: one 16-byte store where they all exist
    if (i + 3 < n) *reinterpret_cast<uint4 *>(cost + i) = make_uint4(kUnreached, kUnreached, kUnreached, kUnreached);
    else
        for (uint64_t j = i; j < n; j++) cost[j] = kUnreached;   // bounded: 3 trips
    if (i + 3 < n_dirty) *reinterpret_cast<uint4 *>(dirty + i) = make_uint4(0u, 0u, 0u, 0u);
    else
        for (uint64_t j = i; j < n_dirty; j++) dirty[j] = 0u;
}

__global__ __launch_bounds__(256) void reach_seed_kernel(const Geom g, const ReachBricks nb, const uint64_t n, const float *__restrict__ seeds,
                                                         const uint64_t *__restrict__ mask, uint32_t *__restrict__ cost,
                                                         uint32_t *__restrict__ dirty) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t x, y, z;
    if (!reach_point_voxel(g, seeds + 3 * i, x, y, z)) return;
    const uint32_t id = (z * g.Y + y) * g.X + x;
    if (!mask_bit(mask, id)) return;
    cost[id] = 0u;   // (several seeds in one voxel store the same word)
    // its own brick and, from a voxel on the brick's outer layer, the up to seven others that see it in their halo: the 0 is a changed
    // word to all of them.  Bounded: 27 trips.
    const uint32_t c[3] = {x, y, z}, count[3] = {nb.x, nb.y, nb.z};
    int lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        const uint32_t b = c[k] / kReachBrick, l = c[k] % kReachBrick;
        lo[k] = l == 0u && b > 0u ? -1 : 0;
        hi[k] = l == kReachBrick - 1u && b + 1u < count[k] ? 1 : 0;
    }
    for (int dz = lo[2]; dz <= hi[2]; dz++)
        for (int dy = lo[1]; dy <= hi[1]; dy++)
            for (int dx = lo[0]; dx <= hi[0]; dx++)
                dirty[((z / kReachBrick + dz) * nb.y + (y / kReachBrick + dy)) * nb.x + (x / kReachBrick + dx)] = 1u;
}

// One round.  256 lanes, two voxels of the brick a lane: (lx, ly, lz) and (lx, ly, lz + 4), so a wave owns planes lz and lz + 4.
//   The sweeps are chaotic relaxation inside LDS: a lane reads its neighbours' words while their owners may be lowering them.  Every
//   word is an upper bound that is a real path's length at all times, and the loop ends only after a sweep in which no lane stored: every
//   read of that sweep then saw the words as they are, so each own voxel is at the minimum over its admissible neighbours -- the local
//   fixed point for the staged halo.  Bound: a sweep lowers, at the least, every own voxel whose best path from the halo and the own
//   voxels' staged values has one step more inside the brick than those already final; such a path is simple (costs are positive) and has
//   at most 511 steps among 512 voxels, so 512 sweeps reach the fixed point and one more sees no change: 513 trips.
__global__ __launch_bounds__(256) void reach_relax_kernel(uint32_t *cost, const uint64_t *__restrict__ mask, const VoxelGrid grid,
                                                          const ReachBricks nb, const uint32_t faces_only, const uint32_t cap,
                                                          uint32_t *dirty_now, uint32_t *dirty_next, uint32_t *round_word) {
    __shared__ uint32_t tile[kTileWords];
    __shared__ uint32_t open[kTileWords / 4];   // TRAVERSABLE per tile word, a byte each
    __shared__ uint32_t marks;                   // the neighbour bricks (bit k, as the voxel neighbours) that see a changed voxel
    const uint32_t b = blockIdx.x;
    // nobody writes this round's words but their own bricks, and this one clears its own only behind the barrier below: uniform
    if (dirty_now[b] == 0u) return;
    uint8_t *open8 = reinterpret_cast<uint8_t *>(open);
    const uint32_t bx = b % nb.x, by = (b / nb.x) % nb.y, bz = b / (nb.x * nb.y);
    bool any_open = false;
    for (uint32_t t = threadIdx.x; t < 1000u; t += 256u) {   // bounded: 4 trips
        const uint32_t tx = t % 10u, ty = (t / 10u) % 10u, tz = t / 100u;
        const int64_t gx = (int64_t)bx * kReachBrick + tx - 1, gy = (int64_t)by * kReachBrick + ty - 1, gz = (int64_t)bz * kReachBrick + tz - 1;
        uint32_t c = kUnreached;
        bool o = false;
        if (gx >= 0 && gx < (int64_t)grid.X && gy >= 0 && gy < (int64_t)grid.Y && gz >= 0 && gz < (int64_t)grid.Z) {
            const uint32_t id = (uint32_t)((gz * grid.Y + gy) * grid.X + gx);
            o = mask_bit(mask, id);
            // (a voxel that is not traversable is never stored to: it stays UNREACHED)
            if (o) c = __hip_atomic_load(cost + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const uint32_t at = tz * kTilePlane + ty * kTileRow + tx;
        tile[at] = c;
        open8[at] = o ? 1 : 0;
        any_open |= o && tx >= 1u && tx <= 8u && ty >= 1u && ty <= 8u && tz >= 1u && tz <= 8u;
    }
    if (threadIdx.x == 0) marks = 0u;
    const int some = __syncthreads_or(any_open);
    if (threadIdx.x == 0) dirty_now[b] = 0u;
    if (!some) return;   // (uniform) no traversable voxel of its own: nothing can change here

    const uint32_t lx = threadIdx.x & 7u, ly = (threadIdx.x >> 3) & 7u, lz = threadIdx.x >> 6;
    uint32_t own[2], steps[2], before[2];
    for (int v = 0; v < 2; v++) {
        own[v] = (lz + 4u * v + 1u) * kTilePlane + (ly + 1u) * kTileRow + lx + 1u;
        // the 27 traversable bits around the voxel, then the steps whose 2, 4 or 8 voxels are all set
        uint32_t around = 0;
#pragma unroll
        for (int k = 0; k < 27; k++)
            around |= (uint32_t)open8[(int)own[v] + nb_dz(k) * (int)kTilePlane + nb_dy(k) * (int)kTileRow + nb_dx(k)] << k;
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < 27; k++)
            if (k != 13 && (around & nb_needs(k)) == nb_needs(k)) s |= 1u << k;
        steps[v] = faces_only ? s & kFaceSteps : s;
        before[v] = tile[own[v]];
    }
    for (int sweep = 0; sweep < 513; sweep++) {   // bounded: see above
        bool changed = false;
        for (int v = 0; v < 2; v++) {
            if (steps[v] == 0u) continue;
            const uint32_t cur = __hip_atomic_load(tile + own[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            uint32_t best = cur;
#pragma unroll
            for (int k = 0; k < 27; k++) {
                if (k == 13) continue;
                // No branch on the step's bit: a step that is not admissible reads its neighbour all the same (every one of the 26 lies
                // inside the tile) and turns the word into UNREACHED by an OR.  (Tested bit by bit, the 52 lane masks are loop-invariant,
                // the compiler keeps them in scalar registers across the sweeps, and 50 of those spill.)
                const uint32_t shut = ((steps[v] >> k) & 1u) - 1u;   // 0 where admissible, all ones where not
                const uint32_t d = shut | __hip_atomic_load(tile + ((int)own[v] + nb_dz(k) * (int)kTilePlane + nb_dy(k) * (int)kTileRow + nb_dx(k)),
                                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                // UNREACHED is above every cap; a sum above the cap is dropped before it is formed (no overflow)
                if (d <= cap && nb_cost(k) <= cap - d && d + nb_cost(k) < best) best = d + nb_cost(k);
            }
            if (best < cur) {
                __hip_atomic_store(tile + own[v], best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                changed = true;
            }
        }
        if (!__syncthreads_or(changed)) break;   // (workgroup-uniform)
    }
    // what changed goes back with plain stores -- this brick is the only writer of its words -- and the bricks that see it are marked
    uint32_t mine = 0;
    for (int v = 0; v < 2; v++) {
        const uint32_t now = tile[own[v]];
        if (now == before[v]) continue;
        const uint32_t vz = lz + 4u * v;
        const uint32_t gx = bx * kReachBrick + lx, gy = by * kReachBrick + ly, gz = bz * kReachBrick + vz;   // (inside the grid: it is traversable)
        __hip_atomic_store(cost + ((size_t)gz * grid.Y + gy) * grid.X + gx, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // per axis: this brick (bit 1), the one below if the voxel is in the first layer and it exists, the one above likewise
        const uint32_t mx = 2u | (lx == 0u && bx > 0u ? 1u : 0u) | ((lx == kReachBrick - 1u || gx + 1u == grid.X) && bx + 1u < nb.x ? 4u : 0u);
        const uint32_t my = 2u | (ly == 0u && by > 0u ? 1u : 0u) | ((ly == kReachBrick - 1u || gy + 1u == grid.Y) && by + 1u < nb.y ? 4u : 0u);
        const uint32_t mz = 2u | (vz == 0u && bz > 0u ? 1u : 0u) | ((vz == kReachBrick - 1u || gz + 1u == grid.Z) && bz + 1u < nb.z ? 4u : 0u);
        const uint32_t plane = (my & 1u ? mx : 0u) | (my & 2u ? mx << 3 : 0u) | (my & 4u ? mx << 6 : 0u);
        mine |= (mz & 1u ? plane : 0u) | (mz & 2u ? plane << 9 : 0u) | (mz & 4u ? plane << 18 : 0u);
    }
    mine &= ~(1u << 13);
    if (mine) atomicOr(&marks, mine);
    __syncthreads();
    const uint32_t all = marks;
    if (threadIdx.x < 27u && ((all >> threadIdx.x) & 1u)) {
        const int k = (int)threadIdx.x;
        // (the bit is set only where that brick exists)
        dirty_next[((bz + nb_dz(k)) * nb.y + (by + nb_dy(k))) * nb.x + (bx + nb_dx(k))] = 1u;
    }
    if (threadIdx.x == 0 && all) atomicAdd(round_word, 1u);
}

__global__ __launch_bounds__(256) void reach_stats_kernel(const uint32_t *__restrict__ cost, const uint32_t n, ReachWords *__restrict__ words) {
    constexpr uint32_t kPerLane = 16;   // 4096 voxels a workgroup
    __shared__ uint32_t totals[3];      // reached, seeds, max
    if (threadIdx.x < 3) totals[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * 256 * kPerLane;
    uint32_t reached = 0, seeds = 0, top = 0;
    for (uint32_t k = 0; k < kPerLane; k++) {   // bounded: kPerLane trips
        const uint64_t i = base + (uint64_t)k * 256 + threadIdx.x;
        if (i >= n) break;
        const uint32_t c = cost[i];
        if (c == kUnreached) continue;
        reached++;
        seeds += c == 0u;
        top = max(top, c);
    }
    for (int o = 32; o > 0; o >>= 1) {
        reached += (uint32_t)__shfl_xor(reached, o);
        seeds += (uint32_t)__shfl_xor(seeds, o);
        top = max(top, (uint32_t)__shfl_xor(top, o));
    }
    if ((threadIdx.x & 63u) == 0 && reached) {
        atomicAdd(&totals[0], reached);
        if (seeds) atomicAdd(&totals[1], seeds);
        atomicMax(&totals[2], top);
    }
    __syncthreads();
    if (threadIdx.x == 0 && totals[0]) {
        atomicAdd(&words->n_reached, (unsigned long long)totals[0]);
        if (totals[1]) atomicAdd(&words->n_seed_voxels, (unsigned long long)totals[1]);
        atomicMax(&words->max_cost_reached, (unsigned long long)totals[2]);
    }
}

__global__ __launch_bounds__(256) void reach_lookup_kernel(const Geom g, const uint64_t n, const float *__restrict__ points,
                                                           const uint32_t *__restrict__ cost, uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t x, y, z;
    out[i] = reach_point_voxel(g, points + 3 * i, x, y, z) ? cost[((size_t)z * g.Y + y) * g.X + x] : kUnreached;
}

// A lane per goal.  Every step is a dependent load of up to 26 neighbours: latency-bound by nature, and left so.  Bounded: every step
// lowers the cost by at least 10, so the walk takes at most out(goal) / 10 steps (the outer loop), 26 trips inside.
__global__ __launch_bounds__(256) void reach_paths_kernel(const Geom g, const uint64_t n, const float *__restrict__ goals,
                                                          const uint32_t *__restrict__ cost, const uint64_t *__restrict__ mask,
                                                          const uint32_t faces_only, const uint32_t max_len, uint32_t *__restrict__ lengths,
                                                          uint32_t *__restrict__ rows) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t x, y, z, len = 0;
    if (reach_point_voxel(g, goals + 3 * i, x, y, z)) {
        uint32_t id = (z * g.Y + y) * g.X + x, c = cost[id];
        if (c != kUnreached) {
            uint32_t *row = rows + i * (uint64_t)max_len;
            const uint32_t limit = c / TSDF_REACH_COST_FACE;
            for (uint32_t step = 0;; step++) {
                if (len < max_len) row[len] = id;
                len++;
                if (c == 0u || step >= limit) break;
                bool moved = false;
                for (int k = 0; k < 27 && !moved; k++) {
                    const int dx = nb_dx(k), dy = nb_dy(k), dz = nb_dz(k), axes = (dx != 0) + (dy != 0) + (dz != 0);
                    if (axes == 0 || (faces_only && axes != 1)) continue;
                    const int64_t ux = (int64_t)x + dx, uy = (int64_t)y + dy, uz = (int64_t)z + dz;
                    if (ux < 0 || ux >= (int64_t)g.X || uy < 0 || uy >= (int64_t)g.Y || uz < 0 || uz >= (int64_t)g.Z) continue;
                    const uint32_t uid = (uint32_t)((uz * g.Y + uy) * g.X + ux), cu = cost[uid];
                    const uint32_t ck = axes == 1 ? TSDF_REACH_COST_FACE : axes == 2 ? TSDF_REACH_COST_EDGE : TSDF_REACH_COST_CORNER;
                    if (cu >= c || c - cu != ck) continue;   // (UNREACHED is above every c)
                    // admissible: the 2, 4 or 8 voxels between them (both ends are reached, so traversable)
                    bool ok = true;
                    for (int q = 1; q < 7 && ok; q++) {
                        const int a = q & 1, b2 = (q >> 1) & 1, c2 = q >> 2;
                        if ((a && !dx) || (b2 && !dy) || (c2 && !dz)) continue;
                        ok = mask_bit(mask, (uint32_t)((((int64_t)z + c2 * dz) * g.Y + ((int64_t)y + b2 * dy)) * g.X + ((int64_t)x + a * dx)));
                    }
                    if (!ok) continue;
                    x = (uint32_t)ux;
                    y = (uint32_t)uy;
                    z = (uint32_t)uz;
                    id = uid;
                    c = cu;
                    moved = true;
                }
                if (!moved) break;   // (a reached voxel that is no seed always has such a neighbour)
            }
        }
    }
    lengths[i] = len;
}

// The row of a label in the table's ascending labels; the table's size where the cluster is not listed.  Bounded: 32 trips.
__device__ inline uint32_t reach_row_of(const tsdf_frontier_cluster *__restrict__ table, uint32_t n_rows, uint32_t label) {
    uint32_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (table[mid].label < label) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_rows && table[lo].label == label ? lo : n_rows;
}

// A wave whose lanes all fall into one row -- neighbours in the list are neighbours in the grid -- sends one atomic; a mixed wave one per
// reached lane.  A minimum of integers: order-free.
__global__ __launch_bounds__(256) void reach_rank_kernel(const uint32_t n_list, const uint32_t *__restrict__ list, const uint32_t *__restrict__ labels,
                                                         const tsdf_frontier_cluster *__restrict__ table, const uint32_t n_rows,
                                                         const uint32_t *__restrict__ cost, unsigned long long *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t row = n_rows;
    unsigned long long key = ~0ull;
    if (i < n_list) {
        const uint32_t id = list[i], c = cost[id];
        if (c != kUnreached) {
            row = reach_row_of(table, n_rows, labels[i]);
            key = ((unsigned long long)c << 32) | id;
        }
    }
    const bool live = row < n_rows;
    const uint64_t lives = __ballot(live);
    if (lives == 0ull) return;   // (the whole wave)
    const uint32_t lead = __shfl(row, __ffsll((unsigned long long)lives) - 1);
    if (__ballot(live && row != lead) == 0ull) {
        unsigned long long k = live ? key : ~0ull;
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = ((unsigned long long)(uint32_t)__shfl_xor((uint32_t)(k >> 32), o) << 32) | (uint32_t)__shfl_xor((uint32_t)k, o);
            k = other < k ? other : k;
        }
        if ((threadIdx.x & 63u) == 0) atomicMin(keys + lead, k);
    } else if (live) {
        atomicMin(keys + row, key);
    }
}

__global__ __launch_bounds__(256) void reach_unpack_kernel(const uint32_t n_rows, const tsdf_frontier_cluster *__restrict__ table,
                                                           const unsigned long long *__restrict__ keys, tsdf_reach_cluster *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const unsigned long long k = keys[i];   // (all ones where no member was reached: UNREACHED, 0xFFFFFFFF)
    out[i] = {table[i].label, (uint32_t)(k >> 32), (uint32_t)k, 0u};
}

}  // namespace tsdf

using namespace tsdf;

struct tsdf_reach : HandleOrder {
    int computed;           // the cost array and the mask are a finished computation's of the geometry g
    Geom g;
    uint32_t *cost;         // one word per voxel id
    uint64_t *mask;         // TRAVERSABLE, one bit per voxel id
    uint32_t *dirty;        // per brick, two parities
    unsigned long long *keys;   // ranking: one packed minimum per table row
    size_t cost_cap, mask_cap, dirty_cap, keys_cap;
    CounterBlock<ReachWords> words;   // (handle_counters.hpp)
    tsdf_reach_info info;
};

namespace {

void reach_free(tsdf_reach *s) {
    s->destroy();
    device_free_all(s->cost, s->mask, s->dirty, s->keys);
    s->words.release();
    delete s;
}

// the texts of the handle's stream order (handle_order.hpp)
constexpr const char *kReachOrder = "reach stream order", *kReachEvent = "reach event", *kReachWait = "reach wait";

int reach_computed(const char *who, const tsdf_reach *s) {
    TSDF_REQUIRE(s, "%s: null handle", who);
    TSDF_REQUIRE(s->computed, "%s: the handle has never been computed (tsdf_volume_compute_reach)", who);
    return TSDF_OK;
}

// what both computing entry points refuse, under their own name; *esdf_array: the ESDF's device array (null without one)
int compute_checked(const char *who, const tsdf_volume *v, const tsdf_reach *s, uint64_t n, const float *seeds, uint32_t connectivity,
                    const tsdf_esdf *esdf, float clearance, uint32_t flags, const float **esdf_array) {
    TSDF_REQUIRE(v, "%s: null volume", who);
    TSDF_REQUIRE(s, "%s: null reach handle", who);
    TSDF_REQUIRE(n == 0 || seeds, "%s: null seeds with n = %llu", who, (unsigned long long)n);
    TSDF_REQUIRE(n <= kReachMaxPoints, "%s: %llu seeds are more than a launch holds (%llu)", who, (unsigned long long)n, (unsigned long long)kReachMaxPoints);
    const int rcv = whole_volume_checked(who, v, s->device, "a path's voxels lie in other slabs");
    if (rcv != TSDF_OK) return rcv;
    TSDF_REQUIRE(connectivity == 6u || connectivity == 26u, "%s: connectivity must be 6 or 26, got %u", who, connectivity);
    TSDF_REQUIRE((flags & ~(uint32_t)TSDF_REACH_THROUGH_UNKNOWN) == 0, "%s: unknown flags %#x", who, flags);
    TSDF_REQUIRE(clearance >= 0.0f && clearance < INFINITY, "%s: clearance must be finite and >= 0, got %g", who, (double)clearance);
    TSDF_REQUIRE(esdf || clearance == 0.0f, "%s: a clearance (%g) needs an ESDF handle", who, (double)clearance);
    return esdf_array_checked(who, esdf, v->g, esdf_array);
}

// The whole computation on the volume's stream, seeds on the device; returns when the field is final.
int reach_on(const char *who, tsdf_volume *v, tsdf_reach *s, uint64_t n, const float *seeds, uint32_t connectivity, const float *esdf_array,
             float clearance, uint32_t max_cost, uint32_t flags) {
    hipStream_t stream = v->stream;
    int rc = s->join(stream, kReachOrder);
    if (rc != TSDF_OK) return rc;
    s->computed = 0;
    const VoxelGrid grid = voxel_grid(v->g);
    const ReachBricks nb = reach_bricks(grid);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)grid.n + 63) / 64), n_dirty = 2 * nb.n;
    hipError_t e = device_reserve(s->cost, s->cost_cap, (size_t)grid.n);
    if (e == hipSuccess) e = device_reserve(s->mask, s->mask_cap, (size_t)n_chunks);
    if (e == hipSuccess) e = device_reserve(s->dirty, s->dirty_cap, (size_t)n_dirty);
    if (e != hipSuccess) return hip_fail(e, "reach array alloc failed");
    s->g = v->g;
    std::memset(&s->info, 0, sizeof(s->info));
    geometry_into(s->info, v->g);
    s->info.connectivity = connectivity;
    s->info.flags = flags;
    s->info.clearance = clearance;
    s->info.max_cost = max_cost;
    const uint32_t cap = max_cost ? max_cost : 0xFFFFFFFEu;
    const uint32_t faces_only = connectivity == 6u ? 1u : 0u;

    ReachWords *const words = s->words.dev, *const host_words = s->words.host;
    TSDF_HIP(s->words.reset(stream), "reach counts reset");
    voxel_flag(TraversableFlag{v->dist, {v->weight, v->wpacked, v->wmode}, esdf_array, clearance, (flags & TSDF_REACH_THROUGH_UNKNOWN) ? 1 : 0}, grid,
               n_chunks, s->mask, nullptr, &words->n_traversable, stream);
    hipLaunchKernelGGL(reach_init_kernel, grid_for(((uint64_t)max(grid.n, n_dirty) + 3) / 4, 256), dim3(256), 0, stream, s->cost, grid.n, s->dirty, n_dirty);
    if (n) hipLaunchKernelGGL(reach_seed_kernel, grid_for(n, 256), dim3(256), 0, stream, v->g, nb, n, seeds, s->mask, s->cost, s->dirty);
    TSDF_HIP(hipGetLastError(), "reach setup kernels failed");

    // Rounds in batches: the round words of a batch are zeroed, its launches enqueued, and the words read once through the pinned mirror.
    // A round that marked nothing leaves every later round without a dirty brick, so the first zero word ends the computation.  After
    // round k every voxel whose shortest path crosses at most k brick borders is final, a shortest path has fewer than n_traversable
    // steps, and one more round sees nothing change: rounds <= n_traversable + 1, or the call fails rather than loop.
    uint64_t rounds = 0;
    for (bool final = false; !final;) {
        TSDF_HIP(s->words.reset(words->round, kReachMaxBatch, stream), "reach round words reset");
        for (uint32_t r = 0; r < kReachBatch; r++) {
            const uint64_t k = rounds + r;
            hipLaunchKernelGGL(reach_relax_kernel, dim3(nb.n), dim3(256), 0, stream, s->cost, s->mask, grid, nb, faces_only, cap,
                               s->dirty + (k & 1u) * nb.n, s->dirty + ((k + 1) & 1u) * nb.n, words->round + r);
        }
        TSDF_HIP(hipGetLastError(), "reach relax kernel failed");
        TSDF_HIP(s->words.download(stream), "reach round words download");
        TSDF_HIP(hipStreamSynchronize(stream), "reach rounds");
        s->pending = 0;
        uint32_t used = kReachBatch;
        for (uint32_t r = 0; r < kReachBatch; r++)
            if (host_words->round[r] == 0u) {
                used = r + 1;
                final = true;
                break;
            }
        rounds += used;
        if (!final && rounds > host_words->n_traversable) {
            set_error("%s: %llu rounds have not converged on %llu traversable voxels", who, (unsigned long long)rounds,
                      (unsigned long long)host_words->n_traversable);
            return TSDF_ERR_DEVICE;
        }
    }
    hipLaunchKernelGGL(reach_stats_kernel, grid_for(grid.n, 256 * 16), dim3(256), 0, stream, s->cost, grid.n, words);
    TSDF_HIP(hipGetLastError(), "reach stats kernel failed");
    TSDF_HIP(s->words.download(stream), "reach counts download");
    TSDF_HIP(hipStreamSynchronize(stream), "reach counts");
    s->info.n_traversable = host_words->n_traversable;
    s->info.n_reached = host_words->n_reached;
    s->info.n_seed_voxels = host_words->n_seed_voxels;
    s->info.max_cost_reached = (uint32_t)host_words->max_cost_reached;
    s->info.rounds = rounds;
    s->computed = 1;
    return TSDF_OK;
}

int points_checked(const char *who, const tsdf_reach *s, uint64_t n, const void *points, const void *out) {
    const int rc = reach_computed(who, s);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(n == 0 || points, "%s: null points with n = %llu", who, (unsigned long long)n);
    TSDF_REQUIRE(n == 0 || out, "%s: null output with n = %llu", who, (unsigned long long)n);
    TSDF_REQUIRE(n <= kReachMaxPoints, "%s: %llu points are more than a launch holds (%llu)", who, (unsigned long long)n, (unsigned long long)kReachMaxPoints);
    return TSDF_OK;
}

int paths_checked(const char *who, const tsdf_reach *s, uint64_t n, const void *goals, uint32_t max_len, const void *lengths, const void *rows) {
    const int rc = reach_computed(who, s);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(n == 0 || goals, "%s: null goals with n = %llu", who, (unsigned long long)n);
    TSDF_REQUIRE(n == 0 || max_len > 0, "%s: max_len must be > 0", who);
    TSDF_REQUIRE(n == 0 || (lengths && rows), "%s: null lengths or rows with n = %llu", who, (unsigned long long)n);
    TSDF_REQUIRE(n <= kReachMaxPoints, "%s: %llu goals are more than a launch holds (%llu)", who, (unsigned long long)n, (unsigned long long)kReachMaxPoints);
    return TSDF_OK;
}

// what a ranking reads of the explorer, through its own entry points (they wait for its pending work)
struct RankInput {
    uint32_t n_list, n_rows;
    const uint32_t *list, *labels;
    const tsdf_frontier_cluster *table;
};

int rank_checked(const char *who, const tsdf_reach *s, const tsdf_explorer *ex, const void *out, RankInput *in) {
    int rc = reach_computed(who, s);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(ex, "%s: null explorer handle", who);
    tsdf_explorer_info ei;
    rc = tsdf_explorer_get_info(ex, &ei);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(ei.connectivity != 0u, "%s: the explorer has not been clustered since its last tsdf_volume_find_frontiers (tsdf_explorer_cluster_frontiers)", who);
    TSDF_REQUIRE(same_geometry(geometry_of(ei), s->g), "%s: the explorer holds another geometry (%u x %u x %u, or other voxel sizes or offset) than the reach handle's", who, ei.size[0],
                 ei.size[1], ei.size[2]);
    TSDF_REQUIRE(ei.n_listed_clusters == 0 || out, "%s: null output for %llu clusters", who, (unsigned long long)ei.n_listed_clusters);
    in->n_list = (uint32_t)ei.n_frontiers;
    in->n_rows = (uint32_t)ei.n_listed_clusters;
    rc = tsdf_explorer_frontier_buffers(ex, &in->list, nullptr, nullptr);
    if (rc == TSDF_OK) rc = tsdf_explorer_cluster_buffers(ex, &in->labels, &in->table);
    return rc;
}

int rank_on(tsdf_reach *s, const RankInput &in, tsdf_reach_cluster *out, hipStream_t stream) {
    if (in.n_rows == 0) return TSDF_OK;
    int rc = s->join(stream, kReachOrder);
    if (rc != TSDF_OK) return rc;
    const hipError_t e = device_reserve(s->keys, s->keys_cap, (size_t)in.n_rows);
    if (e != hipSuccess) return hip_fail(e, "reach rank alloc failed");
    TSDF_HIP(hipMemsetAsync(s->keys, 0xff, (size_t)in.n_rows * sizeof(unsigned long long), stream), "reach rank reset");
    hipLaunchKernelGGL(reach_rank_kernel, grid_for(in.n_list, 256), dim3(256), 0, stream, in.n_list, in.list, in.labels, in.table, in.n_rows, s->cost, s->keys);
    hipLaunchKernelGGL(reach_unpack_kernel, grid_for(in.n_rows, 256), dim3(256), 0, stream, in.n_rows, in.table, s->keys, out);
    TSDF_HIP(hipGetLastError(), "reach rank kernels failed");
    return s->leave(stream, kReachEvent);
}

}  // namespace

extern "C" {

int tsdf_reach_create(tsdf_reach **out) {
    return handle_create(out, "tsdf_reach_create", "reach alloc failed", [](tsdf_reach *s) {
        std::memset(s, 0, sizeof(*s));
        const hipError_t e = s->create();
        return e == hipSuccess ? s->words.create() : e;
    }, reach_free);
}

void tsdf_reach_destroy(tsdf_reach *s) {
    if (s) reach_free(s);
}

int tsdf_volume_compute_reach_device(const tsdf_volume *cv, uint64_t n, const float *device_seeds, uint32_t connectivity, const tsdf_esdf *esdf,
                                     float clearance, uint32_t max_cost, uint32_t flags, tsdf_reach *s) {
    const float *esdf_array = nullptr;
    const int rc = compute_checked("tsdf_volume_compute_reach_device", cv, s, n, device_seeds, connectivity, esdf, clearance, flags, &esdf_array);
    if (rc != TSDF_OK) return rc;
    return reach_on("tsdf_volume_compute_reach_device", const_cast<tsdf_volume *>(cv), s, n, device_seeds, connectivity, esdf_array, clearance,
                    max_cost, flags);
}

int tsdf_volume_compute_reach(const tsdf_volume *cv, uint64_t n, const float *host_seeds, uint32_t connectivity, const tsdf_esdf *esdf,
                              float clearance, uint32_t max_cost, uint32_t flags, tsdf_reach *s) {
    const float *esdf_array = nullptr;
    const int rc0 = compute_checked("tsdf_volume_compute_reach", cv, s, n, host_seeds, connectivity, esdf, clearance, flags, &esdf_array);
    if (rc0 != TSDF_OK) return rc0;
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);
    const char *const who = "tsdf_volume_compute_reach";
    if (n == 0) return reach_on(who, v, s, 0, nullptr, connectivity, esdf_array, clearance, max_cost, flags);
    HostStage st;
    int rc = st.begin(v->stream, 3 * (size_t)n * sizeof(float), "tsdf_volume_compute_reach: couldn't allocate %zu bytes for the seeds");
    if (rc != TSDF_OK) return rc;
    st.up(st.buf, host_seeds, 3 * (size_t)n * sizeof(float));
    if (st.ok()) rc = reach_on(who, v, s, n, static_cast<const float *>(st.buf), connectivity, esdf_array, clearance, max_cost, flags);
    return st.finish(rc, "Reach computation failed");
}

int tsdf_reach_get_info(const tsdf_reach *s, tsdf_reach_info *info) {
    TSDF_REQUIRE(s && info, "tsdf_reach_get_info: null argument");
    *info = s->info;
    return TSDF_OK;
}

int tsdf_reach_buffer(const tsdf_reach *s, const uint32_t **device_costs) {
    TSDF_REQUIRE(s && device_costs, "tsdf_reach_buffer: null argument");
    const int rc = s->wait(kReachWait);
    if (rc != TSDF_OK) return rc;
    *device_costs = s->computed ? s->cost : nullptr;
    return TSDF_OK;
}

int tsdf_reach_download(const tsdf_reach *s, uint32_t *host_costs) {
    TSDF_REQUIRE(s && host_costs, "tsdf_reach_download: null argument");
    TSDF_REQUIRE(s->computed, "tsdf_reach_download: the handle has never been computed (tsdf_volume_compute_reach)");
    const int rc = s->wait(kReachWait);
    if (rc != TSDF_OK) return rc;
    const size_t n = (size_t)s->g.X * s->g.Y * s->g.Z;
    if (n) TSDF_HIP(hipMemcpy(host_costs, s->cost, n * sizeof(uint32_t), hipMemcpyDeviceToHost), "reach download");
    return TSDF_OK;
}

int tsdf_reach_scratch_bytes(const tsdf_reach *s, uint64_t *bytes) {
    TSDF_REQUIRE(s && bytes, "tsdf_reach_scratch_bytes: null argument");
    *bytes = (uint64_t)s->mask_cap * sizeof(uint64_t) + (uint64_t)s->dirty_cap * sizeof(uint32_t) + (uint64_t)s->keys_cap * sizeof(unsigned long long) +
             s->words.device_bytes();
    return TSDF_OK;
}

int tsdf_reach_lookup_device(const tsdf_reach *s, uint64_t n, const float *device_points, uint32_t *device_costs, void *hip_stream) {
    int rc = points_checked("tsdf_reach_lookup_device", s, n, device_points, device_costs);
    if (rc != TSDF_OK) return rc;
    if (n == 0) return TSDF_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    rc = s->join(stream, kReachOrder);
    if (rc != TSDF_OK) return rc;
    hipLaunchKernelGGL(reach_lookup_kernel, grid_for(n, 256), dim3(256), 0, stream, s->g, n, device_points, s->cost, device_costs);
    TSDF_HIP(hipGetLastError(), "reach lookup kernel failed");
    return s->leave(stream, kReachEvent);
}

int tsdf_reach_lookup(const tsdf_reach *s, uint64_t n, const float *host_points, uint32_t *host_costs) {
    const int rc0 = points_checked("tsdf_reach_lookup", s, n, host_points, host_costs);
    if (rc0 != TSDF_OK) return rc0;
    if (n == 0) return TSDF_OK;
    const size_t fn = (size_t)n;
    HostStage st;
    int rc = st.begin(nullptr, 4 * fn * sizeof(float), "tsdf_reach_lookup: couldn't allocate %zu bytes for the points and results");
    if (rc != TSDF_OK) return rc;
    float *const buf = static_cast<float *>(st.buf);
    uint32_t *const out = static_cast<uint32_t *>(st.buf) + 3 * fn;
    st.up(buf, host_points, 3 * fn * sizeof(float));
    if (st.ok()) rc = tsdf_reach_lookup_device(s, n, buf, out, nullptr);
    if (rc == TSDF_OK) st.down(host_costs, out, fn * sizeof(uint32_t));
    return st.finish(rc, "Reach lookup failed");
}

int tsdf_reach_paths_device(const tsdf_reach *s, uint64_t n, const float *device_goals, uint32_t max_len, uint32_t *device_lengths,
                            uint32_t *device_rows, void *hip_stream) {
    int rc = paths_checked("tsdf_reach_paths_device", s, n, device_goals, max_len, device_lengths, device_rows);
    if (rc != TSDF_OK) return rc;
    if (n == 0) return TSDF_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    rc = s->join(stream, kReachOrder);
    if (rc != TSDF_OK) return rc;
    hipLaunchKernelGGL(reach_paths_kernel, grid_for(n, 256), dim3(256), 0, stream, s->g, n, device_goals, s->cost, s->mask,
                       s->info.connectivity == 6u ? 1u : 0u, max_len, device_lengths, device_rows);
    TSDF_HIP(hipGetLastError(), "reach paths kernel failed");
    return s->leave(stream, kReachEvent);
}

int tsdf_reach_paths(const tsdf_reach *s, uint64_t n, const float *host_goals, uint32_t max_len, uint32_t *host_lengths, uint32_t *host_rows) {
    const int rc0 = paths_checked("tsdf_reach_paths", s, n, host_goals, max_len, host_lengths, host_rows);
    if (rc0 != TSDF_OK) return rc0;
    if (n == 0) return TSDF_OK;
    // one allocation: goals (3n floats), lengths (n words), rows (n * max_len words, uploaded first: what a path does not reach stays)
    const size_t fn = (size_t)n, row_words = fn * max_len;
    HostStage st;
    int rc = st.begin(nullptr, (4 * fn + row_words) * sizeof(uint32_t), "tsdf_reach_paths: couldn't allocate %zu bytes for the goals and paths");
    if (rc != TSDF_OK) return rc;
    float *const buf = static_cast<float *>(st.buf);
    uint32_t *const lengths = static_cast<uint32_t *>(st.buf) + 3 * fn, *const rows = lengths + fn;
    st.up(buf, host_goals, 3 * fn * sizeof(float));
    st.up(rows, host_rows, row_words * sizeof(uint32_t));
    if (st.ok()) rc = tsdf_reach_paths_device(s, n, buf, max_len, lengths, rows, nullptr);
    if (rc == TSDF_OK) {
        st.down(host_lengths, lengths, fn * sizeof(uint32_t));
        st.down(host_rows, rows, row_words * sizeof(uint32_t));
    }
    return st.finish(rc, "Reach paths failed");
}

int tsdf_reach_rank_frontiers_device(tsdf_reach *s, const tsdf_explorer *explorer, tsdf_reach_cluster *device_rows, void *hip_stream) {
    RankInput in;
    const int rc = rank_checked("tsdf_reach_rank_frontiers_device", s, explorer, device_rows, &in);
    if (rc != TSDF_OK) return rc;
    return rank_on(s, in, device_rows, (hipStream_t)hip_stream);
}

int tsdf_reach_rank_frontiers(tsdf_reach *s, const tsdf_explorer *explorer, tsdf_reach_cluster *host_rows) {
    RankInput in;
    const int rc0 = rank_checked("tsdf_reach_rank_frontiers", s, explorer, host_rows, &in);
    if (rc0 != TSDF_OK) return rc0;
    if (in.n_rows == 0) return TSDF_OK;
    HostStage st;
    int rc = st.begin(nullptr, (size_t)in.n_rows * sizeof(tsdf_reach_cluster), "tsdf_reach_rank_frontiers: couldn't allocate %zu bytes for the rows");
    if (rc != TSDF_OK) return rc;
    rc = rank_on(s, in, static_cast<tsdf_reach_cluster *>(st.buf), nullptr);
    if (rc == TSDF_OK) st.down(host_rows, st.buf, (size_t)in.n_rows * sizeof(tsdf_reach_cluster));
    return st.finish(rc, "Reach ranking failed");
}

}  // extern "C"
