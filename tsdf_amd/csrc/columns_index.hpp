// The cell and band arithmetic of the column maps (include/tsdf_amd.h, "column maps", rules 2 - 3): which two axes span the
// map, which voxel is step p of a cell's column, forward or reversed, the strides of a walk in voxel ids, and U * V * L in 64 bits.
// columns.hip's kernels and its argument checks use these and nothing else for their indices.  Compiles for the host alone:
// tests/cpp/columns_host.cpp runs it under the address and undefined-behaviour sanitizers (`make sanitize-columns`).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace tsdf {

struct ColumnsShape {
    uint32_t N[3];       // the grid, x y z
    uint32_t axis;       // the axis reduced
    uint32_t au, av;     // the map's axes, ascending: the two others
    uint32_t U, V;       // the map: N[au] x N[av] cells, cell (u, v) has index v * U + u
    uint32_t lo, hi;     // the band on `axis`, hi resolved: 0 <= lo < hi <= N[axis]
    uint32_t L;          // hi - lo
    uint32_t reversed;   // 1: c_p has axis index hi - 1 - p
};

// the longest axis a map takes: top and bottom are int32
constexpr uint32_t kColumnsMaxAxis = 0x7fffffffu;

__host__ __device__ inline void columns_map_axes(uint32_t axis, uint32_t &au, uint32_t &av) {
    au = axis == 0 ? 1u : 0u;
    av = axis == 2 ? 1u : 2u;
}

// The shape of a projection, or false for what rule 8 refuses: axis > 2, lo >= hi after hi == 0 became N[axis], hi > N[axis], an axis
// longer than kColumnsMaxAxis, an empty grid.
inline bool columns_shape(const uint32_t N[3], uint32_t axis, uint32_t lo, uint32_t hi, bool reversed, ColumnsShape &s) {
    if (axis > 2 || N[0] == 0 || N[1] == 0 || N[2] == 0 || N[axis] > kColumnsMaxAxis) return false;
    if (hi == 0) hi = N[axis];
    if (lo >= hi || hi > N[axis]) return false;
    s.N[0] = N[0]; s.N[1] = N[1]; s.N[2] = N[2];
    s.axis = axis;
    columns_map_axes(axis, s.au, s.av);
    s.U = N[s.au];
    s.V = N[s.av];
    s.lo = lo;
    s.hi = hi;
    s.L = hi - lo;
    s.reversed = reversed ? 1u : 0u;
    return true;
}

__host__ __device__ inline uint64_t columns_cells(const ColumnsShape &s) { return (uint64_t)s.U * s.V; }
// the voxels a projection reads, U * V * L: what the totals of the three states sum to
__host__ __device__ inline uint64_t columns_voxels(const ColumnsShape &s) { return (uint64_t)s.U * s.V * s.L; }

// the index on `axis` of step p of a column, p < L ("up" is increasing p)
__host__ __device__ inline uint32_t columns_axis_index(const ColumnsShape &s, uint32_t p) { return s.reversed ? s.hi - 1u - p : s.lo + p; }

// voxel c_p of cell (u, v)
__host__ __device__ inline void columns_voxel(const ColumnsShape &s, uint32_t u, uint32_t v, uint32_t p, uint32_t &x, uint32_t &y, uint32_t &z) {
    const uint32_t a = columns_axis_index(s, p);
    x = s.axis == 0 ? a : u;
    y = s.axis == 0 ? u : s.axis == 1 ? a : v;
    z = s.axis == 2 ? a : v;
}

__host__ __device__ inline uint64_t columns_voxel_id(const ColumnsShape &s, uint32_t x, uint32_t y, uint32_t z) {
    return ((uint64_t)z * s.N[1] + y) * s.N[0] + x;
}

// A walk in strides: c_p of a cell is at in-plane index (x + X y) ip0 + p * ip_step in plane z0 + p * z_step.  One of the two steps is
// zero; a reversed walk has the other negative.  |ip_step| <= X, |z_step| <= 1: products with p < 2^31 fit 64 bits by far.
struct ColumnsWalk {
    int64_t ip0, ip_step;
    int64_t z0, z_step;
};

__host__ __device__ inline ColumnsWalk columns_walk(const ColumnsShape &s, uint32_t u, uint32_t v) {
    uint32_t x, y, z;
    columns_voxel(s, u, v, 0, x, y, z);
    const int64_t dir = s.reversed ? -1 : 1;
    ColumnsWalk w;
    w.ip0 = (int64_t)s.N[0] * y + x;
    w.z0 = z;
    w.ip_step = s.axis == 0 ? dir : s.axis == 1 ? dir * (int64_t)s.N[0] : 0;
    w.z_step = s.axis == 2 ? dir : 0;
    return w;
}

// The walk goes in groups of kColumnsGroup steps: group k holds the steps p = 4 k - pad + t, t = 0 .. 3, of which those in [0, L) exist.
// pad = 0 begins the first group at c_0.  A walk along z over packed weights (align_z) is padded so that its groups are aligned with the
// packed dwords, which hold 4 (8-bit) or 2 (16-bit) consecutive z: then z >> 2 is the same for every existing step of a group, and
// z >> 1 for those at t = 0, 1 and for those at t = 2, 3.
constexpr uint32_t kColumnsGroup = 4;

__host__ __device__ inline uint32_t columns_group_pad(const ColumnsShape &s, bool align_z) {
    if (!align_z || s.axis != 2) return 0;
    return s.reversed ? 3u - ((s.hi - 1u) & 3u) : (s.lo & 3u);
}

// (L + pad <= 2^31 + 2)
__host__ __device__ inline uint32_t columns_groups(const ColumnsShape &s, uint32_t pad) {
    return (uint32_t)(((uint64_t)s.L + pad + (kColumnsGroup - 1)) / kColumnsGroup);
}

}  // namespace tsdf
