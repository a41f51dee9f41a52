// Ray integration for gfx950: fuse an unorganised set of rays -- a LiDAR scan, a fisheye depth sensor, a point cloud with its sensor
// position -- into the volume (include/tsdf_amd.h, "ray integration").  No reference counterpart: the reference's volume
// is filled from pinhole depth frames, each voxel projected into the image.  A ray set has no projection to invert, so this is the one
// writer of the field that scatters: a lane walks its ray through the grid and leaves an observation in every voxel it crosses.
//
// Two launches on the volume's stream:
//   - rays_scatter_kernel: one lane per ray, rules 1-6 of the header (rays_walk.hpp).  Per observed voxel ONE 64-bit integer atomicAdd of
//     (1 << 40) + q into the voxel's zeroed scratch word: the count in the top 24 bits, the two's-complement sum of the quantised
//     observations in the low 40 (n <= 2^23 rays, |q| <= 2^15: the sum stays below 2^38 and never reaches the count).  Integer adds
//     commute: the word, and so every bit of the result, is the same whatever order the rays arrive in.  No float atomic anywhere.
//     The lane also marks the integrate brick (64 x 4 x 32 voxels) of the voxel with a plain byte store -- racing stores of the same 1
//     -- once per brick it enters, not once per voxel;
//   - rays_apply_kernel: one workgroup per integrate brick, of fuse_kernel's shape (64 x 4 lanes, lane <-> (x, y), the walk along z one
//     packed weight dword at a time so that counts are stored as whole dwords).  An unmarked brick leaves at once (one byte read; a
//     compact list as fuse_cull_kernel builds would save 16 384 empty workgroups at 512^3 and cost a launch).  A marked one decodes
//     its scratch words, blends (rule 8), stores distance and weight and puts the zero back into every word and into its mark: the
//     scratch is all zero again when the call ends.
//
// The coloured call (tsdf_integrate_rays_colour*, rules 9-12 of the header) is the plain call plus a colour update, in kernels of its own:
//   - rays_scatter_colour_kernel: rays_scatter_kernel, and for an observation whose unclamped sdf is <= trunc two further 64-bit integer
//     atomicAdds into the voxel's pair of words in the colour scratch: (1 << 40) + R and (G << 32) + B;
//   - rays_colour_apply_kernel: rays_apply_kernel's shape, launched BEFORE it (it reads the marks and leaves them to rays_apply_kernel):
//     the mean rounded half up per channel, the depth path's blend as one whole-dword read-modify-write of the colour word, zero back
//     into both scratch words.
#include <algorithm>

#include "band_pass.hpp"
#include "field_sample.hpp"
#include "rays_walk.hpp"

namespace tsdf {

constexpr uint64_t kRaysMax = (uint64_t)1 << 23;
constexpr int kRaysCountShift = 40;
constexpr size_t kRaysHeader = 16;   // {updated voxels (u64), pad}

__global__ __launch_bounds__(256) void rays_scatter_kernel(const Geom g, const uint64_t n_rays, const float *__restrict__ origins,
                                                           const uint32_t origin_per_ray, const float *__restrict__ points,
                                                           const float min_range, const float max_range, const int band_only,
                                                           unsigned long long *__restrict__ acc, uint8_t *__restrict__ marks,
                                                           const uint32_t bricks_x, const uint32_t bricks_y) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rays) return;
    const float *const op = origins + (origin_per_ray ? 3 * i : 0);
    const float ox = op[0], oy = op[1], oz = op[2];
    const float px = points[3 * i + 0], py = points[3 * i + 1], pz = points[3 * i + 2];
    const size_t row = g.X, plane = (size_t)g.X * g.Y;
    uint32_t last_brick = 0xffffffffu;
    rays_walk(g, ox, oy, oz, px, py, pz, min_range, max_range, band_only, [&](int ix, int iy, int iz, int q) {
        atomicAdd(&acc[plane * (size_t)iz + row * (size_t)iy + (size_t)ix], (1ull << kRaysCountShift) + (unsigned long long)(long long)q);
        const uint32_t brick = ((uint32_t)iz / kIntBrickZ * bricks_y + (uint32_t)iy / kIntBrickY) * bricks_x + (uint32_t)ix / kIntBrickX;
        if (brick != last_brick) {
            marks[brick] = 1;
            last_brick = brick;
        }
    });
}

// rays_scatter_kernel with the colour sums of rules 9 and 10.  col holds two words per voxel: A = count << 40 | sum of R, B = sum of G <<
// 32 | sum of B.  n <= 2^23 rays and channels <= 255: every sum stays below 2^31 and the count below 2^24, so the sum of R (40 bits of
// room) never reaches the count and the sum of B (32 bits) never reaches the sum of G.  No atomic's value is used.
__global__ __launch_bounds__(256) void rays_scatter_colour_kernel(const Geom g, const uint64_t n_rays, const float *__restrict__ origins,
                                                                  const uint32_t origin_per_ray, const float *__restrict__ points,
                                                                  const uint8_t *__restrict__ rgb, const float min_range,
                                                                  const float max_range, const int band_only,
                                                                  unsigned long long *__restrict__ acc, unsigned long long *__restrict__ col,
                                                                  uint8_t *__restrict__ marks, const uint32_t bricks_x,
                                                                  const uint32_t bricks_y) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rays) return;
    const float *const op = origins + (origin_per_ray ? 3 * i : 0);
    const float ox = op[0], oy = op[1], oz = op[2];
    const float px = points[3 * i + 0], py = points[3 * i + 1], pz = points[3 * i + 2];
    const unsigned long long word_a = (1ull << kRaysCountShift) + rgb[3 * i + 0];
    const unsigned long long word_b = ((unsigned long long)rgb[3 * i + 1] << 32) + rgb[3 * i + 2];
    const size_t row = g.X, plane = (size_t)g.X * g.Y;
    const float trunc = g.trunc;
    uint32_t last_brick = 0xffffffffu;
    rays_walk_sdf(g, ox, oy, oz, px, py, pz, min_range, max_range, band_only, [&](int ix, int iy, int iz, int q, float sdf) {
        const size_t at = plane * (size_t)iz + row * (size_t)iy + (size_t)ix;
        atomicAdd(&acc[at], (1ull << kRaysCountShift) + (unsigned long long)(long long)q);
        // rule 9: the band of the depth path, on the unclamped sdf (q == 32768 is also reached by rounding from below trunc)
        if (sdf <= trunc) {
            atomicAdd(&col[2 * at + 0], word_a);
            atomicAdd(&col[2 * at + 1], word_b);
        }
        const uint32_t brick = ((uint32_t)iz / kIntBrickZ * bricks_y + (uint32_t)iy / kIntBrickY) * bricks_x + (uint32_t)ix / kIntBrickX;
        if (brick != last_brick) {
            marks[brick] = 1;
            last_brick = brick;
        }
    });
}

// the mean of a channel rounded half up, (2 * sum + count) / (2 * count) of rule 11, in 32 bits: sum < 2^31 and count < 2^24, so
// floor(sum / count) and the doubled remainder fit, and floor(sum / count + 1/2) = floor(sum / count) + (2 * remainder >= count)
__device__ inline uint32_t rays_colour_mean(uint32_t sum, uint32_t count) {
    const uint32_t quot = sum / count, rem = sum - quot * count;
    return quot + (2u * rem >= count ? 1u : 0u);
}

// One workgroup per integrate brick, 64 x 4 lanes, lane <-> (x, y), z walked; runs before rays_apply_kernel, which clears the marks.
__global__ __launch_bounds__(256) void rays_colour_apply_kernel(uint32_t *__restrict__ colour, const Geom g, const uint32_t bricks_x,
                                                                const uint32_t bricks_y, ulonglong2 *__restrict__ col,
                                                                const uint8_t *__restrict__ marks) {
    const uint32_t b = blockIdx.x;
    if (!marks[b]) return;   // (the whole workgroup reads the same byte)
    const uint32_t bx = b % bricks_x, by = (b / bricks_x) % bricks_y, bz = b / (bricks_x * bricks_y);
    const uint32_t x = bx * kIntBrickX + threadIdx.x, y = by * kIntBrickY + threadIdx.y;
    if (x >= g.X || y >= g.Y) return;
    const size_t xy = (size_t)g.X * g.Y;
    const uint32_t z_end = min((bz + 1u) * kIntBrickZ, g.Z);
    size_t at = xy * (bz * kIntBrickZ) + (size_t)g.X * y + x;
    for (uint32_t z = bz * kIntBrickZ; z < z_end; z++, at += xy) {
        const ulonglong2 ab = col[at];
        if (!ab.x) continue;   // (a colour observation counts in A: no count, no sums)
        col[at] = make_ulonglong2(0ull, 0ull);
        const uint32_t count = (uint32_t)(ab.x >> kRaysCountShift);
        const uint32_t mr = rays_colour_mean((uint32_t)ab.x, count);   // (the sum of R is below 2^31: the low dword holds it)
        const uint32_t mg = rays_colour_mean((uint32_t)(ab.y >> 32), count), mb = rays_colour_mean((uint32_t)ab.y, count);
        colour[at] = colour_blend(colour[at], mr, mg, mb);   // rule 12: the blend of tsdf_integrate_colour (band_pass.hpp)
    }
}

// DW: bits per weight, 0 = fp32.  One workgroup per integrate brick, 64 x 4 lanes, lane <-> (x, y).
template <int DW>
__global__ __launch_bounds__(256) void rays_apply_kernel(float *__restrict__ dist, void *__restrict__ weight, const Geom g, const uint32_t cap,
                                                         const uint32_t bricks_x, const uint32_t bricks_y,
                                                         unsigned long long *__restrict__ acc, uint8_t *__restrict__ marks,
                                                         unsigned long long *__restrict__ updated) {
    const uint32_t b = blockIdx.x;
    if (!marks[b]) return;   // (the whole workgroup reads the same byte)
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) marks[b] = 0;
    constexpr uint32_t kPer = DW == 0 ? 1u : 32u / DW, kMask = DW == 8 ? 0xffu : 0xffffu;
    const uint32_t bx = b % bricks_x, by = (b / bricks_x) % bricks_y, bz = b / (bricks_x * bricks_y);
    const uint32_t x = bx * kIntBrickX + threadIdx.x, y = by * kIntBrickY + threadIdx.y;
    uint32_t n_updated = 0;
    if (x < g.X && y < g.Y) {
        const size_t xy = (size_t)g.X * g.Y, in_plane = (size_t)g.X * y + x;
        const double scale = (double)g.trunc * (1.0 / 32768.0);
        const float capf = (float)cap;
        const uint32_t z_end = min((bz + 1u) * kIntBrickZ, g.Z);
        for (uint32_t zw = bz * kIntBrickZ; zw < z_end; zw += kPer) {
            // the dword of planes zw .. zw + kPer - 1 (fp32: the weight itself), loaded with the first voxel that needs it
            uint32_t *const wp = reinterpret_cast<uint32_t *>(weight) + (xy * (zw / kPer) + in_plane);
            uint32_t word = 0;
            bool loaded = false;
#pragma unroll
            for (uint32_t j = 0; j < kPer; j++) {
                const uint32_t z = zw + j;
                if (z >= z_end) break;
                const size_t at = xy * z + in_plane;
                const unsigned long long packed = acc[at];
                if (!packed) continue;
                acc[at] = 0;
                // the low 40 bits sign-extended are the sum; what is left is the count
                const long long sum = (long long)(packed << (64 - kRaysCountShift)) >> (64 - kRaysCountShift);
                const unsigned long long count = (packed - (unsigned long long)sum) >> kRaysCountShift;
                const float m = (float)(((double)sum / (double)count) * scale);
                if (!loaded) {
                    word = *wp;
                    loaded = true;
                }
                const uint32_t shift = DW * j;
                const float w = DW == 0 ? __uint_as_float(word) : (float)((word >> shift) & kMask);
                const float d = dist[at];
                const float wn = w + 1.0f;
                dist[at] = ((d * w) + m) / wn;
                const float stored = (cap && wn > capf) ? capf : wn;
                if (DW == 0) word = __float_as_uint(stored);
                else word = (word & ~(kMask << shift)) | ((uint32_t)stored << shift);   // (a count the field holds: weights_make_room made room)
                n_updated++;
            }
            if (loaded) *wp = word;
        }
    }
    for (int o = 32; o > 0; o >>= 1) n_updated += __shfl_down(n_updated, o);
    if (threadIdx.x == 0 && n_updated) atomicAdd(updated, (unsigned long long)n_updated);
}

struct RaysScratch {
    unsigned long long *updated;
    uint8_t *marks;
    unsigned long long *acc;
    uint32_t bricks_x, bricks_y;
    size_t n_bricks;
};

// the header, the brick marks (padded to 8 bytes), the accumulators: allocated zeroed (on the volume's stream), and left zeroed by every call
static int rays_scratch(tsdf_volume *v, RaysScratch &s) {
    const Geom &g = v->g;
    s.bricks_x = (g.X + kIntBrickX - 1) / kIntBrickX;
    s.bricks_y = (g.Y + kIntBrickY - 1) / kIntBrickY;
    s.n_bricks = (size_t)s.bricks_x * s.bricks_y * ((g.Z + kIntBrickZ - 1) / kIntBrickZ);
    TSDF_REQUIRE(s.n_bricks < ((size_t)1 << 31), "tsdf_integrate_rays: the grid is too large");
    const size_t marks_bytes = (s.n_bricks + 7) & ~(size_t)7, bytes = kRaysHeader + marks_bytes + v->resident_voxels() * sizeof(unsigned long long);
    if (v->rays_scratch_cap != bytes) {
        if (v->rays_scratch) {
            TSDF_HIP(hipStreamSynchronize(v->stream), "ray integration scratch");
            device_release(v->rays_scratch, v->rays_scratch_cap);
        }
        if (hipMalloc(&v->rays_scratch, bytes) != hipSuccess) {
            (void)hipGetLastError();
            v->rays_scratch = nullptr;
            set_error("tsdf_integrate_rays: couldn't allocate the %zu bytes of scratch (8 per voxel)", bytes);
            return TSDF_ERR_NOMEM;
        }
        v->rays_scratch_cap = bytes;
        TSDF_HIP(hipMemsetAsync(v->rays_scratch, 0, bytes, v->stream), "ray integration scratch");
    }
    uint8_t *const base = static_cast<uint8_t *>(v->rays_scratch);
    s.updated = reinterpret_cast<unsigned long long *>(base);
    s.marks = base + kRaysHeader;
    s.acc = reinterpret_cast<unsigned long long *>(base + kRaysHeader + marks_bytes);
    return TSDF_OK;
}

// the colour accumulators of a coloured call, 16 bytes per voxel: allocated zeroed by the first such call, left zeroed by every call
static int rays_colour_scratch(tsdf_volume *v, unsigned long long *&col) {
    const size_t bytes = v->resident_voxels() * 2 * sizeof(unsigned long long);
    if (v->rays_colour_scratch_cap != bytes) {
        if (v->rays_colour_scratch) {
            TSDF_HIP(hipStreamSynchronize(v->stream), "ray integration colour scratch");
            device_release(v->rays_colour_scratch, v->rays_colour_scratch_cap);
        }
        if (hipMalloc(&v->rays_colour_scratch, bytes) != hipSuccess) {
            (void)hipGetLastError();
            v->rays_colour_scratch = nullptr;
            set_error("tsdf_integrate_rays_colour: couldn't allocate the %zu bytes of colour scratch (16 per voxel)", bytes);
            return TSDF_ERR_NOMEM;
        }
        v->rays_colour_scratch_cap = bytes;
        TSDF_HIP(hipMemsetAsync(v->rays_colour_scratch, 0, bytes, v->stream), "ray integration colour scratch");
    }
    col = static_cast<unsigned long long *>(v->rays_colour_scratch);
    return TSDF_OK;
}

// everything that is refused, before anything is touched
static int rays_check(const tsdf_volume *v, uint64_t n, const float *origins, uint64_t n_origins, const float *points, int flags) {
    TSDF_REQUIRE(v, "tsdf_integrate_rays: null volume");
    TSDF_REQUIRE((flags & ~TSDF_RAYS_BAND_ONLY) == 0, "tsdf_integrate_rays: unknown flag bits (0x%x)", (unsigned)flags);
    TSDF_REQUIRE(n_origins == 1 || n_origins == n, "tsdf_integrate_rays: %llu origins for %llu rays (one for all, or one each)",
                 (unsigned long long)n_origins, (unsigned long long)n);
    TSDF_REQUIRE(n <= kRaysMax, "tsdf_integrate_rays: %llu rays in one call (at most 2^23: split the set)", (unsigned long long)n);
    TSDF_REQUIRE(n == 0 || (origins && points), "tsdf_integrate_rays: null origins or points");
    const int rc = field_refuse_slab(v, "tsdf_integrate_rays");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(!v->nodes, "tsdf_integrate_rays: the volume has a materialised deformation-node array: voxel centres must be the implicit grid");
    return TSDF_OK;
}

// the coloured call refuses that, and a volume without colour or rays without colours
static int rays_colour_check(const tsdf_volume *v, uint64_t n, const float *origins, uint64_t n_origins, const float *points,
                             const uint8_t *rgb, int flags) {
    const int rc = rays_check(v, n, origins, n_origins, points, flags);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(v->colour, "tsdf_integrate_rays_colour: colour is not enabled on this volume (tsdf_volume_enable_colour)");
    TSDF_REQUIRE(n == 0 || rgb, "tsdf_integrate_rays_colour: null rgb");
    return TSDF_OK;
}

// The launches of one call on the volume's stream; the arguments have passed rays_check (rays_colour_check with rgb), n > 0.  rgb ==
// nullptr is the plain call: it neither allocates nor touches the colour scratch.
static int rays_integrate(tsdf_volume *v, uint64_t n, const float *device_origins, uint64_t n_origins, const float *device_points,
                          const uint8_t *device_rgb, float min_range, float max_range, int flags, uint64_t *updated_voxels) {
    // the apply kernel writes distances: a tightening of the ray caster's flags still running on another stream comes first
    int rc = occupancy_join(v);
    if (rc != TSDF_OK) return rc;
    RaysScratch s;
    rc = rays_scratch(v, s);
    if (rc != TSDF_OK) return rc;
    unsigned long long *col = nullptr;
    if (device_rgb) {
        rc = rays_colour_scratch(v, col);
        if (rc != TSDF_OK) return rc;
    }
    // room for one more count, as before a depth frame (weights.hip)
    if (v->wmode != 0) {
        rc = weights_make_room(v);
        if (rc != TSDF_OK) return rc;
    }
    TSDF_HIP(hipMemsetAsync(s.updated, 0, sizeof(unsigned long long), v->stream), "ray integration: reset");
    const dim3 rays_grid((unsigned)((n + 255) / 256));
    const uint32_t origin_per_ray = n_origins == n && n > 1 ? 1u : 0u;
    const int band_only = (flags & TSDF_RAYS_BAND_ONLY) ? 1 : 0;
    if (device_rgb)
        hipLaunchKernelGGL(rays_scatter_colour_kernel, rays_grid, dim3(256), 0, v->stream, v->g, n, device_origins, origin_per_ray,
                           device_points, device_rgb, min_range, max_range, band_only, s.acc, col, s.marks, s.bricks_x, s.bricks_y);
    else
        hipLaunchKernelGGL(rays_scatter_kernel, rays_grid, dim3(256), 0, v->stream, v->g, n, device_origins, origin_per_ray, device_points,
                           min_range, max_range, band_only, s.acc, s.marks, s.bricks_x, s.bricks_y);
    TSDF_HIP(hipGetLastError(), "Ray scatter kernel failed");
    const dim3 grid((unsigned)s.n_bricks), block(kIntBrickX, kIntBrickY);
    if (device_rgb) {
        hipLaunchKernelGGL(rays_colour_apply_kernel, grid, block, 0, v->stream, v->colour, v->g, s.bricks_x, s.bricks_y,
                           reinterpret_cast<ulonglong2 *>(col), s.marks);
        TSDF_HIP(hipGetLastError(), "Ray colour apply kernel failed");
    }
#define LAUNCH(DW)                                                                                                                        \
    hipLaunchKernelGGL((rays_apply_kernel<DW>), grid, block, 0, v->stream, v->dist, DW == 0 ? (void *)v->weight : (void *)v->wpacked, v->g, \
                       v->weight_cap, s.bricks_x, s.bricks_y, s.acc, s.marks, s.updated)
    if (v->wmode == 0) LAUNCH(0);
    else if (v->wmode == 8) LAUNCH(8);
    else LAUNCH(16);
#undef LAUNCH
    TSDF_HIP(hipGetLastError(), "Ray apply kernel failed");
    // (with a cap a count at or above it never grows: integrate.hip)
    if (v->wmode != 0 && (!v->weight_cap || v->weight_bound < v->weight_cap)) v->weight_bound++;
    // the ray caster's summary: the route of a writer that does not keep the touched / fine invariant (tsdf_volume_mark_dirty)
    v->occ_dirty = 1;
    v->occ_scan_all = 1;
    if (updated_voxels) {
        unsigned long long count = 0;
        TSDF_HIP(hipMemcpyAsync(&count, s.updated, sizeof(count), hipMemcpyDeviceToHost, v->stream), "ray integration: count");
        TSDF_HIP(hipStreamSynchronize(v->stream), "ray integration: count");
        *updated_voxels = count;
    }
    return TSDF_OK;
}

// The host variants: the rays (and their colours, host_rgb != nullptr) through one device buffer, blocking.  Checked by the caller, n > 0.
static int rays_integrate_host(tsdf_volume *v, uint64_t n, const float *host_origins, uint64_t n_origins, const float *host_points,
                               const uint8_t *host_rgb, float min_range, float max_range, int flags, uint64_t *updated_voxels) {
    // one allocation: the origins, then the points, then the colours
    const size_t fo = 3 * (size_t)n_origins, fp = 3 * (size_t)n, bytes = (fo + fp) * sizeof(float) + (host_rgb ? 3 * (size_t)n : 0);
    HostStage st;
    int rc = st.begin(v->stream, bytes, "tsdf_integrate_rays: couldn't allocate %zu bytes for the rays");
    if (rc != TSDF_OK) return rc;
    float *const buf = static_cast<float *>(st.buf);
    uint8_t *const rgb = host_rgb ? reinterpret_cast<uint8_t *>(buf + fo + fp) : nullptr;
    st.up(buf, host_origins, fo * sizeof(float));
    st.up(buf + fo, host_points, fp * sizeof(float));
    if (rgb) st.up(rgb, host_rgb, 3 * (size_t)n);
    uint64_t updated = 0;
    if (st.ok()) rc = rays_integrate(v, n, buf, n_origins, buf + fo, rgb, min_range, max_range, flags, updated_voxels ? &updated : nullptr);
    rc = st.finish(rc, "Ray integration failed");
    if (rc == TSDF_OK && updated_voxels) *updated_voxels = updated;
    return rc;
}

}  // namespace tsdf

using namespace tsdf;

extern "C" {

int tsdf_integrate_rays_device(tsdf_volume *v, uint64_t n, const float *device_origins, uint64_t n_origins, const float *device_points,
                               float min_range, float max_range, int flags, uint64_t *updated_voxels) {
    const int rc = rays_check(v, n, device_origins, n_origins, device_points, flags);
    if (rc != TSDF_OK) return rc;
    if (n == 0) {
        if (updated_voxels) *updated_voxels = 0;
        return TSDF_OK;
    }
    return rays_integrate(v, n, device_origins, n_origins, device_points, nullptr, min_range, max_range, flags, updated_voxels);
}

int tsdf_integrate_rays(tsdf_volume *v, uint64_t n, const float *host_origins, uint64_t n_origins, const float *host_points,
                        float min_range, float max_range, int flags, uint64_t *updated_voxels) {
    const int rc = rays_check(v, n, host_origins, n_origins, host_points, flags);
    if (rc != TSDF_OK) return rc;
    if (n == 0) {
        if (updated_voxels) *updated_voxels = 0;
        return TSDF_OK;
    }
    return rays_integrate_host(v, n, host_origins, n_origins, host_points, nullptr, min_range, max_range, flags, updated_voxels);
}

int tsdf_integrate_rays_colour_device(tsdf_volume *v, uint64_t n, const float *device_origins, uint64_t n_origins,
                                      const float *device_points, const uint8_t *device_rgb, float min_range, float max_range, int flags,
                                      uint64_t *updated_voxels) {
    const int rc = rays_colour_check(v, n, device_origins, n_origins, device_points, device_rgb, flags);
    if (rc != TSDF_OK) return rc;
    if (n == 0) {
        if (updated_voxels) *updated_voxels = 0;
        return TSDF_OK;
    }
    return rays_integrate(v, n, device_origins, n_origins, device_points, device_rgb, min_range, max_range, flags, updated_voxels);
}

int tsdf_integrate_rays_colour(tsdf_volume *v, uint64_t n, const float *host_origins, uint64_t n_origins, const float *host_points,
                               const uint8_t *host_rgb, float min_range, float max_range, int flags, uint64_t *updated_voxels) {
    const int rc = rays_colour_check(v, n, host_origins, n_origins, host_points, host_rgb, flags);
    if (rc != TSDF_OK) return rc;
    if (n == 0) {
        if (updated_voxels) *updated_voxels = 0;
        return TSDF_OK;
    }
    return rays_integrate_host(v, n, host_origins, n_origins, host_points, host_rgb, min_range, max_range, flags, updated_voxels);
}

int tsdf_volume_ray_scratch_bytes(const tsdf_volume *v, uint64_t *bytes) {
    TSDF_REQUIRE(v && bytes, "tsdf_volume_ray_scratch_bytes: null argument");
    *bytes = (uint64_t)v->rays_scratch_cap + (uint64_t)v->rays_colour_scratch_cap;
    return TSDF_OK;
}

int tsdf_volume_release_ray_scratch(tsdf_volume *v) {
    TSDF_REQUIRE(v, "tsdf_volume_release_ray_scratch: null volume");
    if (!v->rays_scratch && !v->rays_colour_scratch) return TSDF_OK;
    TSDF_HIP(hipStreamSynchronize(v->stream), "ray integration scratch");
    device_release(v->rays_scratch, v->rays_scratch_cap);
    device_release(v->rays_colour_scratch, v->rays_colour_scratch_cap);
    return TSDF_OK;
}

}  // extern "C"
