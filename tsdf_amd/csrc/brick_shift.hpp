// The brick arithmetic of the rolling volume (include/tsdf_amd.h, "rolling volume"; snapshot.hip): where a brick lands under a shift by
// whole bricks, which bricks a box holds, which stay when the box of a volume moves, and the offset after the move.  Shifts are any
// int32; everything is formed in 64 bits, so nothing wraps.  Host and device; includes nothing of the library
// (tests/cpp/rolling_host.cpp runs it under the host sanitizers).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace tsdf {

// a shift per axis and the brick grid that the shifted coordinates must fall into
struct BrickShift {
    long long x, y, z;
    uint32_t nbx, nby, nbz;
};

// brick (bx, by, bz) + shift -> out, false if that is outside the grid on some axis
__host__ __device__ inline bool brick_moved(const BrickShift &s, uint32_t bx, uint32_t by, uint32_t bz, uint32_t out[3]) {
    const long long x = (long long)bx + s.x, y = (long long)by + s.y, z = (long long)bz + s.z;
    if (x < 0 || x >= (long long)s.nbx || y < 0 || y >= (long long)s.nby || z < 0 || z >= (long long)s.nbz) return false;
    out[0] = (uint32_t)x; out[1] = (uint32_t)y; out[2] = (uint32_t)z;
    return true;
}

// the box [lo, hi) of brick coordinates
struct BrickBox {
    int32_t lo[3], hi[3];
};

__host__ __device__ inline bool brick_in_box(const BrickBox &b, uint32_t bx, uint32_t by, uint32_t bz) {
    const long long c[3] = {(long long)bx, (long long)by, (long long)bz};
    for (int a = 0; a < 3; a++)
        if (c[a] < (long long)b.lo[a] || c[a] >= (long long)b.hi[a]) return false;
    return true;
}

// The bricks b of a grid of nb bricks that stay when its box moves by `shift`: b - shift in [0, nb), the box [shift, shift + nb).  Brick
// coordinates are below 2^13, so clamping the upper end to INT32_MAX loses nothing.
inline BrickBox staying_box(const int32_t shift[3], const uint32_t nb[3]) {
    BrickBox b;
    for (int a = 0; a < 3; a++) {
        const long long hi = (long long)shift[a] + (long long)nb[a];
        b.lo[a] = shift[a];
        b.hi[a] = hi > (long long)INT32_MAX ? INT32_MAX : (int32_t)hi;
    }
    return b;
}

// offset + (float)(8 shift) voxel_size in fp32, each operation rounding on its own (the product of 8 and any int32 is exact in 64 bits)
inline float shifted_offset(float offset, int32_t shift, float voxel_size) {
    const float bricks = (float)(8 * (long long)shift);
    const float move = bricks * voxel_size;
    return offset + move;
}

}  // namespace tsdf
