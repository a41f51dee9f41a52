// Volume fusion for gfx950: resample one volume's field onto another volume's grid through a rigid transform and blend it in
// (include/tsdf_amd.h, "volume fusion").  No reference counterpart: the reference's volume is filled from depth frames only.
//
// Three launches on the destination's stream:
//   - fuse_summary_kernel: one byte per 8^3 brick of the SOURCE, "some weight here is > 0", from one pass over the source's weights
//     (1 B a voxel in packed storage);
//   - fuse_cull_kernel: one thread per destination brick of integrate's shape (64 x 4 x 32, lane <-> x).  The centres of the brick's
//     eight corner voxels go through the transform in double; every voxel centre of the brick is a convex combination of them, so the
//     source voxel of every lane lies in their bounding box -- grown by the fp32 rounding of the main kernel's own expression, by one
//     voxel for the taps and one for the rounding of the division by the voxel edge.  A brick whose box holds no set summary byte is
//     dropped: every voxel of it would fail the "all eight tap weights > 0" test.  The others go into a compact list;
//   - fuse_kernel: one workgroup per listed brick, a lane per (x, y) walking the brick's z planes one packed weight dword (four, two or
//     one plane) at a time, so that counts are stored as whole dwords the way integrate stores them.  Per voxel: centre, transform,
//     the source's voxel and its weight (most lanes of a shell leave here), the eight tap weights, the ray cast's own trilinear()
//     (field_sample.hpp), clamp, blend.  The division is the IEEE one in all three storages: the kernel waits on its gathers, not
//     on its arithmetic (LABNOTES.md, "volume fusion").
// The destination's occupancy summary is handed over the way tsdf_volume_mark_dirty does it (occ_dirty + occ_scan_all).
#include "common.hpp"
#include "field_sample.hpp"

namespace tsdf {

constexpr int kSumBrick = 8, kSumShift = 3;   // the source summary's brick
constexpr uint32_t kCullBoxLimit = 4096;      // summary bytes a destination brick may look at; a larger box keeps the brick unseen

struct FuseMat {
    float m[16];   // column-major dst -> src, rows 0-2 used
};

// ---- source summary ------------------------------------------------------------------------------------------------------------
// one thread per weight dword (packed: PER planes of one (x, y)) or per weight (fp32): a byte store where something is > 0.  Several
// lanes may store the same 1 into one byte; nobody reads it before the launch ends.
template <int BITS>
__global__ __launch_bounds__(256) void fuse_summary_kernel(const WeightView wv, const uint32_t X, const uint32_t Y, const uint32_t Z,
                                                           const uint32_t sbx, const uint32_t sby, uint8_t *__restrict__ summary) {
    constexpr uint32_t kPer = BITS == 0 ? 1u : 32u / BITS;
    const size_t xy = (size_t)X * Y, n = xy * ((Z + kPer - 1) / kPer);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const bool some = BITS == 0 ? wv.f32[i] > 0.0f : wv.packed[i] != 0u;
        if (!some) continue;
        const size_t grp = i / xy, in_plane = i - grp * xy;
        const uint32_t y = (uint32_t)(in_plane / X), x = (uint32_t)(in_plane - (size_t)y * X), z = (uint32_t)grp * kPer;
        summary[((size_t)(z >> kSumShift) * sby + (y >> kSumShift)) * sbx + (x >> kSumShift)] = 1;
    }
}

// fp32 source weights: stats[0] |= 1 when one is not an integer in [0, 65535] (weights.hip's rule for "a count"), stats[1] = the
// largest count
__global__ __launch_bounds__(256) void fuse_survey_kernel(const float *__restrict__ w, size_t n, uint32_t *__restrict__ stats) {
    uint32_t bad = 0, top = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float x = w[i];
        const bool ok = x >= 0.0f && x <= 65535.0f && x == truncf(x) && __float_as_uint(x) != 0x80000000u;
        bad |= ok ? 0u : 1u;
        if (ok) top = max(top, (uint32_t)x);
    }
    for (int o = 32; o > 0; o >>= 1) {
        bad |= (uint32_t)__shfl_down((int)bad, o);
        top = max(top, (uint32_t)__shfl_down((int)top, o));
    }
    if ((threadIdx.x & 63u) == 0) {
        if (bad) atomicOr(&stats[0], 1u);
        if (top) atomicMax(&stats[1], top);
    }
}

// ---- cull ------------------------------------------------------------------------------------------------------------------------
struct FuseBricks {
    uint32_t nx, ny, nz;      // destination bricks per axis (kIntBrickX x kIntBrickY x kIntBrickZ voxels)
    uint32_t sbx, sby, sbz;   // summary bricks per axis of the source
};

__global__ __launch_bounds__(256) void fuse_cull_kernel(const Geom dg, const Geom sg, const FuseMat fm, const FuseBricks fb,
                                                        const uint8_t *__restrict__ summary, uint32_t *__restrict__ list,
                                                        uint32_t *__restrict__ count) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= fb.nx * fb.ny * fb.nz) return;
    const uint32_t bx = b % fb.nx, by = (b / fb.nx) % fb.ny, bz = b / (fb.nx * fb.ny);
    const uint32_t v0[3] = {bx * kIntBrickX, by * kIntBrickY, bz * kIntBrickZ};
    const uint32_t v1[3] = {min(v0[0] + kIntBrickX, dg.X) - 1u, min(v0[1] + kIntBrickY, dg.Y) - 1u, min(v0[2] + kIntBrickZ, dg.Z) - 1u};
    const double vs[3] = {dg.vs.x, dg.vs.y, dg.vs.z}, off[3] = {dg.offset.x, dg.offset.y, dg.offset.z};
    const double so[3] = {sg.offset.x, sg.offset.y, sg.offset.z}, svs[3] = {sg.vs.x, sg.vs.y, sg.vs.z};
    const uint32_t sdim[3] = {sg.X, sg.Y, sg.Z};
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, mag[3] = {0.0, 0.0, 0.0};
    for (int corner = 0; corner < 8; corner++) {
        double c[3];
        for (int a = 0; a < 3; a++) c[a] = ((double)((corner >> a) & 1 ? v1[a] : v0[a]) + 0.5) * vs[a] + off[a];
        for (int r = 0; r < 3; r++) {
            const double t0 = (double)fm.m[r] * c[0], t1 = (double)fm.m[4 + r] * c[1], t2 = (double)fm.m[8 + r] * c[2], t3 = fm.m[12 + r];
            const double q = (t0 + t1 + t2 + t3) - so[r];
            lo[r] = fmin(lo[r], q);
            hi[r] = fmax(hi[r], q);
            // what the fp32 evaluation of the same expression works with: each of its seven roundings is below 2^-24 of this
            mag[r] = fmax(mag[r], fabs(t0) + fabs(t1) + fabs(t2) + fabs(t3) + fabs(so[r]) + fabs(off[0] * fm.m[r]) + fabs(off[1] * fm.m[4 + r]) +
                                      fabs(off[2] * fm.m[8 + r]));
        }
    }
    bool keep = false, look = true;
    int k0[3], k1[3];
    for (int r = 0; r < 3; r++) {
        const double slack = mag[r] * 0x1p-19;   // 32 roundings' worth
        // the lane's voxel floor(q / vs) (+-1 for the fp32 quotient), its taps one voxel either side
        const double a = floor((lo[r] - slack) / svs[r]) - 2.0, z = floor((hi[r] + slack) / svs[r]) + 2.0;
        if (!(a == a && z == z && fabs(a) < 1.0e9 && fabs(z) < 1.0e9)) {   // not finite, or beyond an int: no statement about the box
            keep = true;
            look = false;
            break;
        }
        k0[r] = max((int)a, 0);
        k1[r] = min((int)z, (int)sdim[r] - 1);
        if (k0[r] > k1[r]) look = false;   // wholly outside the source: no lane has a valid point (keep stays false)
    }
    if (look) {
        for (int r = 0; r < 3; r++) {
            k0[r] >>= kSumShift;
            k1[r] >>= kSumShift;
        }
        const uint32_t cells = (uint32_t)(k1[0] - k0[0] + 1) * (uint32_t)(k1[1] - k0[1] + 1) * (uint32_t)(k1[2] - k0[2] + 1);
        if (cells > kCullBoxLimit) keep = true;
        else
            for (int z = k0[2]; z <= k1[2] && !keep; z++)
                for (int y = k0[1]; y <= k1[1] && !keep; y++)
                    for (int x = k0[0]; x <= k1[0]; x++)
                        if (summary[((size_t)z * fb.sby + y) * fb.sbx + x]) {
                            keep = true;
                            break;
                        }
    }
    if (keep) list[atomicAdd(count, 1u)] = b;
}

// ---- the main kernel ---------------------------------------------------------------------------------------------------------------
// What the source says at q (valid): false = the voxel is skipped.  s: the sample, ws: the weight of the voxel q lies in.
template <bool FASTDIV>
__device__ inline bool fuse_source(float qx, float qy, float qz, const FieldView &src, float &s, float &ws) {
    const WeightView &wv = src.wv;
    const Geom &sg = src.g;
    const TriConst &tc = src.tc;
    int vx, vy, vz;
    if (!field_voxel<FASTDIV>(src, qx, qy, qz, vx, vy, vz)) return false;   // (the sample would be NaN)
    const size_t xy = tc.plane;
    ws = field_voxel_weight(src, vx, vy, vz);
    if (!(ws > 0.0f)) return false;   // one of the eight taps: a shell's empty space leaves here
    // trilinear's lower corner and tap clamping, the same expressions
    const float ccx = (vx + 0.5f) * sg.vs.x + 0.0f;
    const float ccy = (vy + 0.5f) * sg.vs.y + 0.0f;
    const float ccz = (vz + 0.5f) * sg.vs.z + 0.0f;
    const uint32_t lx = (uint32_t)max((qx < ccx) ? vx - 1 : vx, 0);
    const uint32_t ly = (uint32_t)max((qy < ccy) ? vy - 1 : vy, 0);
    const uint32_t lz = (uint32_t)max((qz < ccz) ? vz - 1 : vz, 0);
    const uint32_t hx = (lx + 1 < sg.X) ? lx + 1 : lx, hy = (ly + 1 < sg.Y) ? ly + 1 : ly, hz = (lz + 1 < sg.Z) ? lz + 1 : lz;
    const size_t r0 = (size_t)tc.row * ly, r1 = (size_t)tc.row * hy;
    const bool all = weight_at(wv, xy, r0 + lx, lz) > 0.0f && weight_at(wv, xy, r0 + lx, hz) > 0.0f &&
                     weight_at(wv, xy, r1 + lx, lz) > 0.0f && weight_at(wv, xy, r1 + lx, hz) > 0.0f &&
                     weight_at(wv, xy, r0 + hx, lz) > 0.0f && weight_at(wv, xy, r0 + hx, hz) > 0.0f &&
                     weight_at(wv, xy, r1 + hx, lz) > 0.0f && weight_at(wv, xy, r1 + hx, hz) > 0.0f;
    if (!all) return false;
    s = field_distance<FASTDIV>(src, qx, qy, qz);
    return !(s != s);
}

// DW: bits per destination weight, 0 = fp32.  One workgroup per listed brick, 64 x 4 lanes, lane <-> (x, y); the walk along z goes one
// weight dword at a time.
template <int DW, bool FASTDIV>
__global__ __launch_bounds__(256) void fuse_kernel(float *__restrict__ ddist, void *__restrict__ dweight, const Geom dg,
                                                   const FieldView src, const FuseMat fm, const uint32_t cap, const uint32_t bricks_x,
                                                   const uint32_t bricks_y,
                                                   const uint32_t *__restrict__ list, const uint32_t *__restrict__ count,
                                                   unsigned long long *__restrict__ fused) {
    if (blockIdx.x >= *count) return;
    constexpr uint32_t kPer = DW == 0 ? 1u : 32u / DW, kMask = DW == 8 ? 0xffu : 0xffffu;
    const uint32_t b = list[blockIdx.x];
    const uint32_t bx = b % bricks_x, by = (b / bricks_x) % bricks_y, bz = b / (bricks_x * bricks_y);
    const uint32_t x = bx * kIntBrickX + threadIdx.x, y = by * kIntBrickY + threadIdx.y;
    const bool active = x < dg.X && y < dg.Y;
    uint32_t n_fused = 0;
    if (active) {
        const float *m = fm.m;
        const size_t xy = (size_t)dg.X * dg.Y, in_plane = (size_t)dg.X * y + x;
        const float cx = ((x + 0.5f) * dg.vs.x) + dg.offset.x, cy = ((y + 0.5f) * dg.vs.y) + dg.offset.y;
        // the z-independent part of each row, in the stated order: (m0 cx + m4 cy) + m8 cz) + m12
        const float rx = m[0] * cx + m[4] * cy, ry = m[1] * cx + m[5] * cy, rz = m[2] * cx + m[6] * cy;
        const float capf = (float)cap;
        const uint32_t z_end = min((bz + 1u) * kIntBrickZ, dg.Z);
        for (uint32_t zw = bz * kIntBrickZ; zw < z_end; zw += kPer) {
            // the dword of planes zw .. zw + kPer - 1 (fp32: the weight itself), loaded with the first voxel that needs it
            uint32_t *const wp = reinterpret_cast<uint32_t *>(dweight) + (xy * (zw / kPer) + in_plane);
            uint32_t word = 0;
            bool loaded = false;
#pragma unroll
            for (uint32_t j = 0; j < kPer; j++) {
                const uint32_t z = zw + j;
                if (z >= z_end) break;
                const float cz = ((z + 0.5f) * dg.vs.z) + dg.offset.z;
                const float px = (rx + m[8] * cz) + m[12], py = (ry + m[9] * cz) + m[13], pz = (rz + m[10] * cz) + m[14];
                const float qx = px - src.g.offset.x, qy = py - src.g.offset.y, qz = pz - src.g.offset.z;
                if (!field_valid(src, qx, qy, qz)) continue;
                float s, ws;
                if (!fuse_source<FASTDIV>(qx, qy, qz, src, s, ws)) continue;
                s = fminf(fmaxf(s, -dg.trunc), dg.trunc);
                if (!loaded) {
                    word = *wp;
                    loaded = true;
                }
                const uint32_t shift = DW * j;
                const float w = DW == 0 ? __uint_as_float(word) : (float)((word >> shift) & kMask);
                const size_t at = xy * z + in_plane;
                const float d = ddist[at];
                const float wn = w + ws;
                ddist[at] = ((d * w) + (s * ws)) / wn;
                const float stored = (cap && wn > capf) ? capf : wn;
                if (DW == 0) word = __float_as_uint(stored);
                else word = (word & ~(kMask << shift)) | ((uint32_t)stored << shift);   // (a count the field holds: tsdf_volume_fuse made room)
                n_fused++;
            }
            if (loaded) *wp = word;
        }
    }
    for (int o = 32; o > 0; o >>= 1) n_fused += __shfl_down(n_fused, o);
    if (threadIdx.x == 0 && n_fused) atomicAdd(fused, (unsigned long long)n_fused);
}

// what: "tsdf_volume_fuse: the destination" / "... the source"
static int fuse_check(const tsdf_volume *v, const char *what) {
    const int rc = field_refuse_slab(v, what);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(!v->nodes, "%s has a materialised deformation-node array: voxel centres must be the implicit grid", what);
    return TSDF_OK;
}

// header {fused voxels (u64), list length, pad}, the brick list, the source summary
static int fuse_scratch(tsdf_volume *dst, size_t bytes) {
    if (dst->fuse_scratch_cap >= bytes) return TSDF_OK;
    if (dst->fuse_scratch) TSDF_HIP(hipStreamSynchronize(dst->stream), "fuse scratch");   // (launches that read it may be in flight)
    TSDF_HIP(device_reserve_bytes(dst->fuse_scratch, dst->fuse_scratch_cap, bytes), "Couldn't allocate the scratch of tsdf_volume_fuse");
    return TSDF_OK;
}

}  // namespace tsdf

using namespace tsdf;

extern "C" int tsdf_volume_fuse(tsdf_volume *dst, const tsdf_volume *src, const float dst_to_src[16], uint64_t *fused_voxels) {
    TSDF_REQUIRE(dst && src && dst_to_src, "tsdf_volume_fuse: null argument");
    TSDF_REQUIRE(dst != src, "tsdf_volume_fuse: a volume cannot be fused into itself");
    TSDF_REQUIRE(dst->device == src->device, "tsdf_volume_fuse: the volumes are on different devices (%d and %d)", dst->device, src->device);
    int rc = fuse_check(dst, "tsdf_volume_fuse: the destination");
    if (rc == TSDF_OK) rc = fuse_check(src, "tsdf_volume_fuse: the source");
    if (rc != TSDF_OK) return rc;
    FuseMat fm;
    std::memcpy(fm.m, dst_to_src, sizeof(fm.m));
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 3; r++)
            TSDF_REQUIRE(fm.m[4 * c + r] - fm.m[4 * c + r] == 0.0f, "tsdf_volume_fuse: dst_to_src has a non-finite entry (row %d, column %d)", r, c);

    // dst's stream waits for what src's has enqueued, and for a tightening of dst's flags running elsewhere
    if (src->stream != dst->stream) {
        hipEvent_t done = nullptr;
        TSDF_HIP(hipEventCreateWithFlags(&done, stream_order_event_flags()), "fuse: event");
        hipError_t e = hipEventRecord(done, src->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(dst->stream, done, 0);
        (void)hipEventDestroy(done);   // (released once it has completed)
        if (e != hipSuccess) return hip_fail(e, "fuse: wait for the source's stream");
    }
    rc = occupancy_join(dst);
    if (rc != TSDF_OK) return rc;

    const FuseBricks fb = {(dst->g.X + kIntBrickX - 1) / kIntBrickX, (dst->g.Y + kIntBrickY - 1) / kIntBrickY, (dst->g.Z + kIntBrickZ - 1) / kIntBrickZ,
                           (src->g.X + kSumBrick - 1) / kSumBrick, (src->g.Y + kSumBrick - 1) / kSumBrick, (src->g.Z + kSumBrick - 1) / kSumBrick};
    const size_t n_bricks = (size_t)fb.nx * fb.ny * fb.nz, n_summary = (size_t)fb.sbx * fb.sby * fb.sbz;
    TSDF_REQUIRE(n_bricks < ((size_t)1 << 31), "tsdf_volume_fuse: the destination grid is too large");
    constexpr size_t kHeader = 16;
    rc = fuse_scratch(dst, kHeader + n_bricks * sizeof(uint32_t) + n_summary);
    if (rc != TSDF_OK) return rc;
    uint8_t *const base = static_cast<uint8_t *>(dst->fuse_scratch);
    unsigned long long *const fused = reinterpret_cast<unsigned long long *>(base);
    uint32_t *const count = reinterpret_cast<uint32_t *>(base + 8), *const list = reinterpret_cast<uint32_t *>(base + kHeader);
    uint8_t *const summary = base + kHeader + n_bricks * sizeof(uint32_t);
    TSDF_HIP(hipMemsetAsync(base, 0, kHeader, dst->stream), "fuse: reset");
    TSDF_HIP(hipMemsetAsync(summary, 0, n_summary, dst->stream), "fuse: reset");

    // the largest source weight, and whether the source's weights are counts at all
    uint32_t src_top = src->weight_bound;
    bool counts = true;
    if (src->wmode == 0 && dst->wmode != 0) {
        uint32_t stats[2] = {0, 0};
        TSDF_HIP(hipMemsetAsync(count, 0, sizeof(stats), dst->stream), "fuse: survey");   // (count and the pad word: reset again below)
        hipLaunchKernelGGL(fuse_survey_kernel, dim3(2048), dim3(256), 0, dst->stream, src->weight, src->resident_voxels(), count);
        TSDF_HIP(hipGetLastError(), "fuse: survey");
        TSDF_HIP(hipMemcpyAsync(stats, count, sizeof(stats), hipMemcpyDeviceToHost, dst->stream), "fuse: survey");
        TSDF_HIP(hipStreamSynchronize(dst->stream), "fuse: survey");
        TSDF_HIP(hipMemsetAsync(count, 0, sizeof(stats), dst->stream), "fuse: survey");
        counts = stats[0] == 0;
        src_top = stats[1];
    }
    // room in dst's storage: counts stay counts (8 -> 16 -> fp32) unless the source's weights are none
    const int mode_before = dst->wmode;
    if (dst->wmode != 0) {
        const uint64_t need = (uint64_t)dst->weight_bound + src_top;
        const bool cap_fits = dst->weight_cap && (dst->wmode == 16 || dst->weight_cap <= 255u);
        if (!counts) rc = tsdf_volume_set_weight_storage(dst, 32);
        else if (!cap_fits) {
            if (need > 65535u) rc = tsdf_volume_set_weight_storage(dst, 32);
            else if (need > 255u && dst->wmode == 8) rc = tsdf_volume_set_weight_storage(dst, 16);
        }
        if (rc != TSDF_OK) return rc;
        const uint64_t stored = dst->weight_cap ? std::min<uint64_t>(need, dst->weight_cap) : need;
        dst->weight_bound = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(dst->weight_bound, stored), 0xffffffffu);
    }
    if (dst->wmode != mode_before) dst->prepared_valid = 0;   // (a brick list prepared ahead came with the old storage)

    const FieldView sv = make_field_view(src);
    {
        const size_t per = src->wmode == 0 ? 1 : 32 / src->wmode;
        const size_t n = (size_t)src->g.X * src->g.Y * ((src->g.Z + per - 1) / per);
        const dim3 grid((unsigned)std::min<size_t>((n + 255) / 256, 8192));
        if (src->wmode == 0) hipLaunchKernelGGL(fuse_summary_kernel<0>, grid, dim3(256), 0, dst->stream, sv.wv, src->g.X, src->g.Y, src->g.Z, fb.sbx, fb.sby, summary);
        else if (src->wmode == 8) hipLaunchKernelGGL(fuse_summary_kernel<8>, grid, dim3(256), 0, dst->stream, sv.wv, src->g.X, src->g.Y, src->g.Z, fb.sbx, fb.sby, summary);
        else hipLaunchKernelGGL(fuse_summary_kernel<16>, grid, dim3(256), 0, dst->stream, sv.wv, src->g.X, src->g.Y, src->g.Z, fb.sbx, fb.sby, summary);
        TSDF_HIP(hipGetLastError(), "fuse: source summary");
    }
    hipLaunchKernelGGL(fuse_cull_kernel, dim3((unsigned)((n_bricks + 255) / 256)), dim3(256), 0, dst->stream, dst->g, src->g, fm, fb, summary, list, count);
    TSDF_HIP(hipGetLastError(), "fuse: cull");

    const dim3 grid((unsigned)n_bricks), block(kIntBrickX, kIntBrickY);
#define LAUNCH(DW, FD)                                                                                                                  \
    hipLaunchKernelGGL((fuse_kernel<DW, FD>), grid, block, 0, dst->stream, dst->dist, DW == 0 ? (void *)dst->weight : (void *)dst->wpacked, dst->g, \
                       sv, fm, dst->weight_cap, fb.nx, fb.ny, list, count, fused)
    if (dst->wmode == 0) {
        if (src->fast_div) LAUNCH(0, true); else LAUNCH(0, false);
    } else if (dst->wmode == 8) {
        if (src->fast_div) LAUNCH(8, true); else LAUNCH(8, false);
    } else {
        if (src->fast_div) LAUNCH(16, true); else LAUNCH(16, false);
    }
#undef LAUNCH
    TSDF_HIP(hipGetLastError(), "Fuse kernel failed");
    // the ray caster's summary: the route of a writer that does not keep the touched / fine invariant (tsdf_volume_mark_dirty)
    dst->occ_dirty = 1;
    dst->occ_scan_all = 1;
    dst->fuse_bricks_total = (uint32_t)n_bricks;
    if (fused_voxels) {
        unsigned long long n = 0;
        TSDF_HIP(hipMemcpyAsync(&n, fused, sizeof(n), hipMemcpyDeviceToHost, dst->stream), "fuse: count");
        TSDF_HIP(hipStreamSynchronize(dst->stream), "fuse: count");
        *fused_voxels = n;
    }
    return TSDF_OK;
}

extern "C" int tsdf_volume_last_fuse_bricks(const tsdf_volume *dst, uint32_t *listed_bricks, uint32_t *total_bricks) {
    TSDF_REQUIRE(dst && listed_bricks && total_bricks, "tsdf_volume_last_fuse_bricks: null argument");
    *listed_bricks = *total_bricks = 0;
    if (!dst->fuse_scratch || !dst->fuse_bricks_total) return TSDF_OK;   // no fuse yet
    TSDF_HIP(hipMemcpyAsync(listed_bricks, static_cast<const uint8_t *>(dst->fuse_scratch) + 8, sizeof(uint32_t), hipMemcpyDeviceToHost, dst->stream),
             "fuse: list length");
    TSDF_HIP(hipStreamSynchronize(dst->stream), "fuse: list length");
    *total_bricks = dst->fuse_bricks_total;
    return TSDF_OK;
}
