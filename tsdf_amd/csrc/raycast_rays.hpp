// Ray queries (include/tsdf_amd.h, "ray queries"): the march of process_ray (src/RayCaster/GPURaycaster.cu:265-377) for rays the caller
// gives -- an origin and a direction each, used as given -- instead of the rays of a pinhole image.  (Included by raycast.hip inside
// namespace tsdf, behind raycast_march.hpp: compute_near_and_far_t, ray_from_near, set_ray / SkipCtx, process_sample, refine_t /
// hit_point are the image cast's own, unchanged, so a ray given a pixel's origin and direction computes that pixel's vertex with the
// very same expressions; the unit gradient at the hit is field_sample.hpp's, the one the field queries return.)
//   cast_rays_kernel   one lane per ray, 256-thread workgroups, the whole table T[0..4402] in LDS, process_sample per pass
// Nothing of the image cast's state is read or written: no best[] words, no tail queue, no cell list, no learnt order, no entry bound.
// Rays are marched in the order given; a wave is as long as its longest ray (no lane refill: LABNOTES.md, "ray queries").

// What a ray query needs of RayParams: the box, the ownership words of a whole volume, the interpolation constants.
static RayParams make_ray_query_params(const tsdf_volume *v) {
    RayParams rp;
    memset(&rp, 0, sizeof(rp));
    const Geom &g = v->g;
    rp.space_min = g.offset;
    rp.space_max = {g.offset.x + g.phys.x, g.offset.y + g.phys.y, g.offset.z + g.phys.z};
    rp.own_lo = v->z_begin;
    rp.own_hi = v->z_end;
    rp.tc = make_tri_const(g);
    return rp;
}

// Ray i: origin o = origins[i], direction d = directions[i] (not normalised: Q6).
//   decreed misses, before any march: a non-finite component of o or d, d == (+-0, +-0, +-0), a NaN t_max[i];
//   the march: the ray/box test, start = ((near_t * d) + o) - space_min, samples at T[k] for k < k_end (the smallest k >= 1 with
//     T[k] >= max_t, at most 4402), the first sample <= 0 refined with previous_tsdf == trunc (Q7);
//   t = near_t + th; with t_max given the hit counts only if t <= t_max[i].
// Range limit, early: a hit at sample k refines to th >= T[k] - step (the fraction previous / (previous - tsdf) lies in [0, 1] for
// tsdf < 0 and trunc > 0; th == T[k] for tsdf == 0), up to two roundings of a few ulp of T[k].  So a sample with
// T[k] > (t_max - near_t) + 4 step + 1e-5 (|t_max| + |near_t|) gives near_t + th > t_max by more than 2 steps -- far above the
// rounding of the subtraction, of th and of the final add (2^-24 relative each) -- and is rejected whatever its value: the march ends
// at the first such k, as if it were k_end.  Samples before it are evaluated as without the limit.
template <bool FASTDIV, bool NORMALS>
__global__ __launch_bounds__(256) void cast_rays_kernel(const FieldView f, const RayParams rp, const OccGrid occ,
                                                        const float *__restrict__ t_table, const uint64_t n,
                                                        const float *__restrict__ origins, const float *__restrict__ directions,
                                                        const float *__restrict__ t_max, float *__restrict__ out_points,
                                                        float *__restrict__ out_t, float *__restrict__ out_normals) {
    __shared__ float Ts[kTableLen];
    for (int i = (int)threadIdx.x; i < kTableLen; i += 256) Ts[i] = t_table[i];
    __syncthreads();
    const Geom &g = f.g;
    const float step_size = Ts[1];   // = (float)((double)trunc * 0.05), :324
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n;

    F3 o = {0.0f, 0.0f, 0.0f}, d = {0.0f, 0.0f, 0.0f};
    float limit = INFINITY;
    if (live) {
        o = {origins[3 * i + 0], origins[3 * i + 1], origins[3 * i + 2]};
        d = {directions[3 * i + 0], directions[3 * i + 1], directions[3 * i + 2]};
        if (t_max) limit = t_max[i];
    }
    const bool finite = fabsf(o.x) < INFINITY && fabsf(o.y) < INFINITY && fabsf(o.z) < INFINITY && fabsf(d.x) < INFINITY &&
                        fabsf(d.y) < INFINITY && fabsf(d.z) < INFINITY;   // (false for NaN)
    const bool decreed = !finite || (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) || limit != limit;

    float near_t = 0.0f, far_t = 0.0f;
    const bool intersects = live && !decreed && compute_near_and_far_t(o, d, rp.space_min, rp.space_max, near_t, far_t);
    RayParams own = rp;   // (ray_from_near reads the origin and space_min: this lane's origin in a copy of its own)
    own.origin = o;
    const RayState ray = ray_from_near(d, near_t, own);
    const float max_t = far_t - near_t;

    // samples 0 .. k_end-1 are evaluated unless one of them is <= 0: the smallest k in [1, 4402] with T[k] >= max_t (4402 when there
    // is none, a NaN max_t included: setup_ray), or with T[k] beyond what the range limit can still accept
    int k_end = 0;
    if (intersects) {
        float bound = max_t;
        if (g.trunc > 0.0f) {
            const float reach = ((limit - near_t) + 4.0f * step_size) + 1.0e-5f * (fabsf(limit) + fabsf(near_t));
            if (reach < max_t) bound = reach;   // (false for a NaN or infinite reach, and max_t stays what it is when it is NaN)
        }
        int lo = 1, hi = kMaxSamples;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (Ts[mid] >= bound) hi = mid; else lo = mid + 1;
        }
        k_end = lo;
    }

    SkipCtx sc = make_skip_ctx(g, step_size);
    set_ray<true>(sc, ray, step_size, g);   // (skipping switches itself off for a ray whose step exceeds a quarter voxel)
    BrickCache bc = {0, 0, false};
    SampleWork work = {0, 0, 0, 0};
    int k = k_end > 0 ? 0 : kDone;   // next sample of this lane's ray (kDone when finished)
    float th = NAN;
    bool hit = false;
    // every pass is the same straight-line work for all lanes; a wave leaves when all its lanes are done
    while (__ballot(k != kDone) != 0ull) {
        if (k != kDone) {
            const float t = Ts[k];
            int jump, ahead;
            const float tsdf = process_sample<false, false, FASTDIV>(t, k, ray, sc, bc, f.dist, g, rp.tc, rp, occ, nullptr, work, jump, ahead);
            if (jump > 0) {
                k += jump;
            } else if (tsdf <= 0) {
                th = refine_t(t, tsdf, g.trunc, step_size);   // previous_tsdf == trunc (Q7)
                hit = true;
                k = kDone;
            } else {
                k += 1 + (tsdf > 0 ? ahead : 0);   // positive (or NaN): the reference steps on
            }
            if (k != kDone && k >= k_end) k = kDone;
        }
    }

    float ix = NAN, iy = NAN, iz = NAN, t_hit = NAN;
    if (hit) {
        t_hit = near_t + th;
        if (t_max && !(t_hit <= limit)) {
            hit = false;
            t_hit = NAN;
        } else {
            hit_point(th, ray, rp, ix, iy, iz);
        }
    }
    float nx = NAN, ny = NAN, nz = NAN;
    if (NORMALS && hit) {
        // tsdf_volume_sample_field_device(..., TSDF_FIELD_UNIT_GRADIENT) at the hit point (field.hip: field_sample_kernel)
        const FieldStencil s = field_stencil(f, ix - g.offset.x, iy - g.offset.y, iz - g.offset.z);
        if (field_stencil_valid(f, s)) {
            float gx, gy, gz;
            field_gradient<FASTDIV>(f, s, gx, gy, gz);
            const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
            if (len > 0.0f) {   // (false for NaN)
                nx = gx / len;
                ny = gy / len;
                nz = gz / len;
            }
        }
    }
    if (!live) return;
    if (out_points) {
        out_points[3 * i + 0] = ix;
        out_points[3 * i + 1] = iy;
        out_points[3 * i + 2] = iz;
    }
    if (out_t) out_t[i] = t_hit;
    if (NORMALS) {
        out_normals[3 * i + 0] = nx;
        out_normals[3 * i + 1] = ny;
        out_normals[3 * i + 2] = nz;
    }
}

static int count_after_bulk_change(tsdf_volume *v);   // raycast.hip, below the cell-parallel cast

static int cast_rays_check(const tsdf_volume *v, uint64_t n, const float *origins, const float *directions, const float *points,
                           const float *t, const float *normals) {
    TSDF_REQUIRE(v, "tsdf_volume_cast_rays: null volume");
    const int rc = field_refuse_slab(v, "tsdf_volume_cast_rays");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(points || t || normals, "tsdf_volume_cast_rays: no output asked for (all three are NULL)");
    TSDF_REQUIRE(n == 0 || (origins && directions), "tsdf_volume_cast_rays: null origins or directions");
    TSDF_REQUIRE(n <= 0x7FFFFFFFull * 256u, "tsdf_volume_cast_rays: too many rays");   // (n itself: n + 255 wraps for n near 2^64)
    return TSDF_OK;
}

// the launch on the volume's stream; v has passed cast_rays_check, n > 0
static int cast_rays(tsdf_volume *v, uint64_t n, const float *origins, const float *directions, const float *t_max, float *points,
                     float *t, float *normals) {
    // The occupancy the march skips by, as the image cast refreshes it.  After a bulk change of the distances the image cast also counts
    // the flagged bricks for its choice of kernels (count_after_bulk_change) before the flags stop being dirty: done here in its place,
    // so the next image cast chooses as it would have without this query.
    int rc = count_after_bulk_change(v);
    if (rc != TSDF_OK) return rc;
    rc = occupancy_refresh(v);
    if (rc != TSDF_OK) return rc;
    const RayParams rp = make_ray_query_params(v);
    const FieldView f = make_field_view(v);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (v->fast_div) {
        if (normals) hipLaunchKernelGGL((cast_rays_kernel<true, true>), grid, block, 0, v->stream, f, rp, v->occ, v->t_table, n, origins, directions, t_max, points, t, normals);
        else hipLaunchKernelGGL((cast_rays_kernel<true, false>), grid, block, 0, v->stream, f, rp, v->occ, v->t_table, n, origins, directions, t_max, points, t, normals);
    } else {
        if (normals) hipLaunchKernelGGL((cast_rays_kernel<false, true>), grid, block, 0, v->stream, f, rp, v->occ, v->t_table, n, origins, directions, t_max, points, t, normals);
        else hipLaunchKernelGGL((cast_rays_kernel<false, false>), grid, block, 0, v->stream, f, rp, v->occ, v->t_table, n, origins, directions, t_max, points, t, normals);
    }
    TSDF_HIP(hipGetLastError(), "Ray query kernel failed");
    return TSDF_OK;
}

// ---- colour at the hits (tsdf_volume_cast_rays_colour*) ---------------------------------------------------------------------------------
// One thread per ray, behind cast_rays_kernel on the same stream: q = points[i] - offset (the current offset: the ray frame, the one
// coloured ray integration writes in); the voxel a field query reports the weight of, its {r, g, b} if its n > 0; (0, 0, 0) on a miss
// (a NaN point is not valid), for an invalid q, where an index reaches the size, and for n == 0.
template <bool FASTDIV>
__global__ __launch_bounds__(256) void cast_rays_colour_kernel(const FieldView f, const uint32_t *__restrict__ colour, const uint64_t n_rays,
                                                               const float *__restrict__ points, uint8_t *__restrict__ rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rays) return;
    const float x = points[3 * i + 0] - f.g.offset.x, y = points[3 * i + 1] - f.g.offset.y, z = points[3 * i + 2] - f.g.offset.z;
    uint32_t c = 0;
    int vx, vy, vz;
    if (field_valid(f, x, y, z) && field_voxel<FASTDIV>(f, x, y, z, vx, vy, vz)) {
        const uint32_t w = colour[(size_t)f.tc.plane * (uint32_t)vz + (size_t)f.tc.row * (uint32_t)vy + (uint32_t)vx];
        if (w >> 24) c = w;
    }
    rgb[3 * i + 0] = (uint8_t)c;
    rgb[3 * i + 1] = (uint8_t)(c >> 8);
    rgb[3 * i + 2] = (uint8_t)(c >> 16);
}

static int cast_rays_colour_check(const tsdf_volume *v, uint64_t n, const float *origins, const float *directions, const float *points,
                                  const float *t, const float *normals, const uint8_t *rgb) {
    const int rc = cast_rays_check(v, n, origins, directions, points, t, normals);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(v->colour, "tsdf_volume_cast_rays_colour: colour is not enabled on this volume (tsdf_volume_enable_colour)");
    TSDF_REQUIRE(rgb, "tsdf_volume_cast_rays_colour: null rgb");
    TSDF_REQUIRE(points, "tsdf_volume_cast_rays_colour: null points (the colour is sampled at them)");
    return TSDF_OK;
}

// the sample of n hit points on the volume's stream; v has passed cast_rays_colour_check, n > 0
static int cast_rays_colour(const tsdf_volume *v, uint64_t n, const float *points, uint8_t *rgb) {
    const FieldView f = make_field_view(v);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (v->fast_div) hipLaunchKernelGGL(cast_rays_colour_kernel<true>, grid, block, 0, v->stream, f, v->colour, n, points, rgb);
    else hipLaunchKernelGGL(cast_rays_colour_kernel<false>, grid, block, 0, v->stream, f, v->colour, n, points, rgb);
    TSDF_HIP(hipGetLastError(), "Ray query colour kernel failed");
    return TSDF_OK;
}
