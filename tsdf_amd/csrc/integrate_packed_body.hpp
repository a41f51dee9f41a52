// The body of integrate_packed_kernel and integrate_packed_colour_kernel (integrate_packed.hip), included inside each of the two:
// not a header.  The including kernel declares `tile`, `plane_lds`, `constexpr bool COLOUR`, `colour`, `rgb`, `constexpr bool CAPPED`, `cap`,
// `constexpr bool REMOVE` (integrate_packed_remove_kernel: the frame is taken back out, include/tsdf_amd.h "de-integration").  (A body shared
// through an inlined device function compiled to other instructions for the plain kernel than the body written inside it.)
    constexpr int kPlanesPerWord = 32 / WBITS, kWords = kBatchZ / kPlanesPerWord;
    static_assert(kBatchZ == 4 && (WBITS == 8 || WBITS == 16), "a batch is two pairs of planes");
    const uint32_t tid = threadIdx.y * kTileX + threadIdx.x;
    const uint32_t n_active = *count;
    const size_t plane = (size_t)g.X * g.Y;
    const float neg_trunc = -g.trunc;
    // see round_quotients (integrate.hip): thr = 4e-7 * (max(width, height) + 2); the float just below 1/2 - thr
    const float round_near_half = __uint_as_float(__float_as_uint(0.5f - 4.0e-7f * ((float)max(width, height) + 2.0f)) - 1u);
    const uint32_t planes_resident = g.z_store_end - g.z_store_begin;
    uint32_t updated = 0, stores = 0;   // (COUNT: voxels updated, distances stored)

    // One brick per workgroup (launch_integrate sizes the grid to the whole brick grid; workgroups beyond the list leave at once).  No loop
    // over bricks: what the prologue needs of the kernel's arguments is dead once the planes are walked, which the scalar register
    // file needs (with a loop around it the compiler kept it all live and spilled scalars into vector lanes: a v_readlane per use).
    {
        // The list's length first (the same word for every workgroup: a scalar-cache hit; the many workgroups beyond the list -- nine in ten
        // at 1024^3 -- leave here without touching memory), then the list entry, its box and the brick's coordinates in ONE scalar round
        // trip: all three are needed here, in scalar registers -- left alone the compiler spreads them over three dependent trips to L2
        // (the coordinates, the entry inside the `touched` store's branch, the box) in front of the tile's pixels.
        const uint32_t i = blockIdx.x;
        if (i >= n_active) return;
        const uint32_t b = list[i];
        const uint4 box = boxes[i];
        const uint2 co = coords[i];   // the brick's coordinates as the cull kernel had them (three divisions by run-time extents otherwise)
        asm volatile("" :: "s"(b), "s"(box.x), "s"(box.y), "s"(box.z), "s"(box.w), "s"(co.x), "s"(co.y));
#ifdef TSDF_DIAGNOSTICS
        const uint32_t bx = b % bg.nx, by = (b / bg.nx) % bg.ny, bz = b / (bg.nx * bg.ny);   // (the diagnostics may have re-sorted list and boxes on the host)
        (void)co;
#else
        const uint32_t bx = co.x & 0xffffu, by = co.x >> 16, bz = co.y;
#endif
        const uint32_t vx = bx * kTileX + threadIdx.x;
        const uint32_t vy = by * kTileY + threadIdx.y;
        const uint32_t z0 = g.z_store_begin + bz * kChunkZ;
        const uint32_t z_extra = bz + 1 == bg.nz ? bg.z_extra : 0u;
        const uint32_t z1 = min(z0 + kChunkZ + z_extra, g.z_store_end);  // exclusive
        // The tile: image columns box.x - lead .. box.x + box.z + lead - 1, rows box.y - 1 .. box.y + box.w; everything outside the
        // box itself is written as 0 (the ring).  The box holds every pixel a voxel of this brick can project to and lies inside the
        // image (brick_cull_kernel), so a voxel that misses the box fails the reference's frustum test (:349): its look-up, clamped
        // onto the ring, finds depth 0 = no update (:355).
        const uint32_t lead = bg.pair_loads ? 2u : 1u;
        const uint32_t pitch = box.z + 2u * lead, rows = box.w + 2u;
        const bool staged = box.z != 0 && pitch * rows <= (uint32_t)kTilePixels;
        if (tid < (uint32_t)(kChunkZ + kBatchZ)) {
            // z-only terms of the projection (brick_cull_kernel's side job), two planes side by side; planes this brick does not
            // hold get a NaN depth term: their voxels then compare false everywhere below
            const uint32_t p = z0 - g.z_store_begin + tid;
            float4 pc = make_float4(0.f, 0.f, 0.f, NAN);
            if (p < planes_resident + kBatchZ) pc = plane_const[p];
            if (z0 + tid >= z1) pc.w = NAN;
            float *dst = plane_lds + (tid >> 1) * kPairFloats + (tid & 1u);
            dst[0] = pc.x; dst[2] = pc.y; dst[4] = pc.z; dst[6] = pc.w;
        }
        if (staged) {
            constexpr uint32_t kStageBatch = 8;   // look-ups requested before the first is waited for
            if (bg.pair_loads) {
                // (even image width, 4-byte aligned image; the cull kernel has made box.x and box.z even: a lane takes two pixels)
                const uint32_t half = pitch >> 1, total2 = half * rows;
                const uint32_t *depth2 = reinterpret_cast<const uint32_t *>(depth);
                uint32_t *tile2 = reinterpret_cast<uint32_t *>(tile);
                // pair index of tile slot (0, 0) -- may lie before the image (box.y == 0 or box.x == 0); the clamped slots below do not
                const int64_t org2 = (((int64_t)box.y - 1) * (int64_t)width + (int64_t)box.x - 2) / 2;
                // slot p = tid + 256 u of the tile as (row, pair): one division per thread, then steps of 256 slots = (dq rows, dr pairs)
                // (eight divisions by `half` per batch, twice, were a quarter of the prologue's instructions)
                const uint32_t dq = (kTileX * kTileY) / half, dr = (kTileX * kTileY) - dq * half;
                uint32_t ty_ = tid / half, tx_ = tid - ty_ * half;
                for (uint32_t p0 = tid; p0 < total2; p0 += kTileX * kTileY * kStageBatch) {
                    uint32_t px[kStageBatch], row_[kStageBatch], col_[kStageBatch];
#pragma unroll
                    for (uint32_t u = 0; u < kStageBatch; u++) {
                        row_[u] = ty_; col_[u] = tx_;
                        const uint32_t cy = min(max(ty_, 1u), rows - 2u), cx2 = min(max(tx_, 1u), half - 2u);   // (inside the box, whatever the slot)
                        px[u] = depth2[org2 + (int64_t)cy * (int64_t)(width >> 1) + (int64_t)cx2];
                        tx_ += dr; ty_ += dq;
                        if (tx_ >= half) { tx_ -= half; ty_ += 1u; }
                    }
#pragma unroll
                    for (uint32_t u = 0; u < kStageBatch; u++) {
                        const uint32_t p = p0 + u * (kTileX * kTileY);
                        const bool ring = row_[u] == 0u || row_[u] == rows - 1u || col_[u] == 0u || col_[u] == half - 1u;
                        if (p < total2) tile2[p] = ring ? 0u : px[u];
                    }
                }
            } else {
                const uint32_t total = pitch * rows;
                for (uint32_t p0 = tid; p0 < total; p0 += kTileX * kTileY * kStageBatch) {
                    uint16_t px[kStageBatch];
#pragma unroll
                    for (uint32_t u = 0; u < kStageBatch; u++) {
                        const uint32_t p = min(p0 + u * (kTileX * kTileY), total - 1u);
                        const uint32_t ty = p / pitch, tx = p - ty * pitch;
                        const uint32_t cy = min(max(ty, 1u), rows - 2u), cx = min(max(tx, 1u), pitch - 2u);
                        px[u] = depth[(size_t)(box.y + cy - 1u) * width + (box.x + cx - 1u)];
                    }
#pragma unroll
                    for (uint32_t u = 0; u < kStageBatch; u++) {
                        const uint32_t p = p0 + u * (kTileX * kTileY);
                        const uint32_t ty = p / pitch, tx = p - ty * pitch;
                        const bool ring = ty == 0u || ty == rows - 1u || tx == 0u || tx == pitch - 1u;
                        if (p < total) tile[p] = ring ? (uint16_t)0 : px[u];
                    }
                }
            }
        }
        // (the per-lane constants of the walk are formed while the tile's pixels are on their way, in front of the barrier)

        // distance / weight addressing: one buffer descriptor per array based at this brick's first row (scalar registers), the plane as
        // the instruction's scalar byte offset, one 32-bit lane offset in bytes: no address arithmetic on the vector unit (the flat
        // form cost a 64-bit vector add per access).  launch_integrate keeps grids whose 36 planes pass 2^31 bytes on the fp32 kernel.
        const size_t brick_base = plane * (z0 - g.z_store_begin) + (size_t)g.X * (by * kTileY) + (size_t)bx * kTileX;
        const size_t wbrick_base = plane * ((z0 - g.z_store_begin) / kPlanesPerWord) + (size_t)g.X * (by * kTileY) + (size_t)bx * kTileX;
        const __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(dist + brick_base, 0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(wpk + wbrick_base, 0, 0x7fffffff, 0x00020000);
        const uint32_t plane_bytes = (uint32_t)plane * 4u;
        const uint32_t lane_off4 = (threadIdx.y * g.X + threadIdx.x) * 4u;
        auto dsoff = [&](uint32_t zrel) { return plane_bytes * zrel; };                       // plane z0 + zrel of the distances
        auto wsoff = [&](uint32_t zrel) { return plane_bytes * (zrel / kPlanesPerWord); };   // the word holding plane z0 + zrel (z0 - z_store_begin is a multiple of 32)
        // (COLOUR) a colour word has the index of its distance: the same brick base, plane and lane offsets -- as a scalar base + a
        // 32-bit lane offset, like the frame's bytes below (2 scalar registers where a descriptor takes 4: the scalar file is full)
        char *const cbase = reinterpret_cast<char *>(colour + (COLOUR ? brick_base : 0));
        auto cword = [&](uint32_t zrel) { return reinterpret_cast<uint32_t *>(cbase + (lane_off4 + dsoff(zrel))); };

        // voxel centre, x and y parts: initialise_deformation (src/TSDF/TSDFVolume.cu:783-784) then integrate_kernel's
        // offset + translation (:343); partial row sums of inv_pose * (c, 1): the reference evaluates ((m_i1 x + m_i2 y) + m_i3 z) + m_i4
        const float cx = ((((int)vx + 0.5f) * g.vs.x) + g.offset_clear.x) + g.offset.x;
        const float cy = ((((int)vy + 0.5f) * g.vs.y) + g.offset_clear.y) + g.offset.y;
        const float r1 = ip.m11 * cx + ip.m12 * cy;
        const float r2 = ip.m21 * cx + ip.m22 * cy;
        float r3 = ip.m31 * cx + ip.m32 * cy;
        if (vx >= g.X) r3 = NAN;   // lanes past the grid's x edge stay in (the marks at the end are made by the wave's first lanes): NaN depth, no update
        uint32_t low_lo = 0, low_hi = 0;   // bit o: my voxel of plane z0 + o got a distance that is not safely positive
        bool wrote = false;                 // my lane stored a distance (a lane mask: scalar registers)
        // (see integrate_kernel: voxels a boundary brick depends on are held to the stricter "flat" test)
        const bool rim_xy = occ.in_rim_zone(vx, occ.nbx) || occ.in_rim_zone(vy, occ.nby);
        const float flat_lo_open = __uint_as_float(__float_as_uint(occ.flat_lo) - 1u);
        const float mark_lo = rim_xy ? flat_lo_open : occ.tau, mark_hi = rim_xy ? occ.flat_hi : INFINITY;
        // look-up constants (exact small integers in fp32): byte address in the tile = fy * (2 pitch) + fx2,
        // fx2 = clamp(2 rx - 2 (box.x - lead)), fy = clamp(ry - (box.y - 1))
        // (depth_pad: image column x at padded column x + 1, row y at y + 1, pitch width + 2)
        const float x_org2 = staged ? -2.0f * (float)((int)box.x - (int)lead) : 2.0f, y_org = staged ? -(float)((int)box.y - 1) : 1.0f;
        const float fx2_lo = staged ? 2.0f * (float)(lead - 1u) : 0.0f, fx2_hi = staged ? 2.0f * (float)(lead + box.z) : 2.0f * (float)(width + 1u);
        const float fy_hi = staged ? (float)(box.w + 1u) : (float)(height + 1u);
        const float pitch2 = 2.0f * (float)(staged ? pitch : width + 2u);

        __syncthreads();
        if (vy >= g.Y) return;   // (a whole wave)
        // The walk over the brick's planes exists twice in the kernel, once per kind of look-up (a workgroup takes one): with both
        // kinds in one body every LDS read after the join waited for all outstanding memory loads -- the compiler cannot tell which
        // branch filled the destination registers -- and the batches stopped overlapping.
        auto walk = [&](auto staged_c) {
        constexpr bool kStaged = decltype(staged_c)::value;
        auto project_and_load = [&](const uint32_t o, bool (&upd_)[kBatchZ], float (&tsdf_)[kBatchZ], float (&pd_)[kBatchZ], uint32_t (&pw_)[kWords],
                                    uint32_t (&pix_)[kBatchZ]) {
            // o = first plane of the batch relative to z0 (a multiple of 4)
            f2 rx_[2], ry_[2], camz_[2];
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const float *pl = plane_lds + ((o >> 1) + p) * kPairFloats;
                const f2 a2 = *reinterpret_cast<const f2 *>(pl + 2), b2 = *reinterpret_cast<const f2 *>(pl + 4), c2 = *reinterpret_cast<const f2 *>(pl + 6);
                // world_to_pixel (src/Utilities/cuda_coordinate_transforms.cu:10-30), standard camera: the 0 * x terms dropped
                const f2 camx = (f2{r1, r1} + a2) + f2{ip.m14, ip.m14};
                const f2 camy = (f2{r2, r2} + b2) + f2{ip.m24, ip.m24};
                const f2 camz = (f2{r3, r3} + c2) + f2{ip.m34, ip.m34};
                const f2 imx = f2{k.m11, k.m11} * camx + f2{k.m13, k.m13} * camz;
                const f2 imy = f2{k.m22, k.m22} * camy + f2{k.m23, k.m23} * camz;
                const f2 rc = f2{__builtin_amdgcn_rcpf(camz.x), __builtin_amdgcn_rcpf(camz.y)};
                const f2 qx = imx * rc, qy = imy * rc;
                f2 rx = f2{__builtin_rintf(qx.x), __builtin_rintf(qx.y)}, ry = f2{__builtin_rintf(qy.x), __builtin_rintf(qy.y)};
                const f2 dx = qx - rx, dy = qy - ry;
                // round_quotients' test (integrate.hip), once for the two planes: every |q - r| < 1/2 - thr, none NaN; otherwise this
                // lane redoes them with the IEEE divisions and roundf of the reference (:25-26), NaN -> 0 as the target's float -> int
                // conversion does
                const float near = max3_abs_keep_nan(max3_abs_keep_nan(0.0f, dx.x, dx.y), dy.x, dy.y);
                if (!(near < round_near_half)) {
                    rx.x = roundf(imx.x / camz.x); ry.x = roundf(imy.x / camz.x);
                    rx.y = roundf(imx.y / camz.y); ry.y = roundf(imy.y / camz.y);
                    if (rx.x != rx.x) rx.x = 0.0f;
                    if (ry.x != ry.x) ry.x = 0.0f;
                    if (rx.y != rx.y) rx.y = 0.0f;
                    if (ry.y != ry.y) ry.y = 0.0f;
                }
                rx_[p] = rx; ry_[p] = ry; camz_[p] = camz;
            }
            // look-up: the brick's tile in LDS, or -- no tile: the box is unknown (the brick straddles the camera plane) or too big --
            // the whole image inside its own ring of zeros in memory (depth_pad); same address arithmetic, other constants
            uint32_t d_[kBatchZ];   // depth of the voxel's pixel, 0 = none
#pragma unroll
            for (int p = 0; p < 2; p++) {
                f2 fx2 = __builtin_elementwise_fma(rx_[p], f2{2.0f, 2.0f}, f2{x_org2, x_org2});   // (exact: integers; huge or infinite values are clamped next)
                f2 fy = ry_[p] + f2{y_org, y_org};
                fx2.x = med3(fx2.x, fx2_lo, fx2_hi); fx2.y = med3(fx2.y, fx2_lo, fx2_hi);
                fy.x = med3(fy.x, 0.0f, fy_hi); fy.y = med3(fy.y, 0.0f, fy_hi);
                const f2 addr = __builtin_elementwise_fma(fy, f2{pitch2, pitch2}, fx2);           // (exact: < 2^24)
                if (kStaged) {
                    d_[2 * p] = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(tile) + (uint32_t)addr.x);
                    d_[2 * p + 1] = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(tile) + (uint32_t)addr.y);
                } else {
                    d_[2 * p] = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(depth_pad) + (uint32_t)addr.x);
                    d_[2 * p + 1] = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(depth_pad) + (uint32_t)addr.y);
                }
            }
            bool any = false;
#pragma unroll
            for (int j = 0; j < kBatchZ; j++) {
                // pixel_to_camera(...).z == depth, world_to_camera(...).z == camz for the standard camera (cuda_coordinate_transforms.cu:108-146)
                const float camz = (j & 1) ? camz_[j >> 1].y : camz_[j >> 1].x;
                const float sdf = (float)d_[j] - camz;
                // depth > 0 (:355) and sdf >= -trunc (:366); NaN camz (planes / lanes past the grid): false
                const bool update = d_[j] != 0 && sdf >= neg_trunc;
                // (sdf > 0) ? min(sdf, trunc) : sdf  ==  min(sdf, trunc)   (trunc > 0, sdf not NaN under `update`)
                upd_[j] = update;
                asm("v_min_f32 %0, %1, %2" : "=v"(tsdf_[j]) : "s"(g.trunc), "v"(sdf));   // (the plain instruction: fminf would first canonicalise both operands)
                if constexpr (COLOUR) {
                    // band_pass_kernel's set: the voxels updated, without free space -- on the sdf itself, not the blend's min(sdf, trunc).
                    // Its pixel is the look-up's: d != 0 means the look-up was not clamped onto the ring, so (rx, ry) lies in the image.
                    // pix_ = kNoPixel outside the set (a vector register, not one more lane mask: the scalar file is full).
                    pix_[j] = kNoPixel;
                    if (update && sdf <= g.trunc) {
                        const float rx = (j & 1) ? rx_[j >> 1].y : rx_[j >> 1].x, ry = (j & 1) ? ry_[j >> 1].y : ry_[j >> 1].x;
                        pix_[j] = (uint32_t)cvt_i32_sat(ry) * width + (uint32_t)cvt_i32_sat(rx);
                    }
                }
                if (update DIAG_NOLOAD) pd_[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(drsrc, lane_off4, dsoff(o + j), 0));
                any = any || update;
                if (kPlanesPerWord == 2 && (j & 1)) {
                    pw_[j >> 1] = 0u;
                    if (any DIAG_NOLOAD) pw_[j >> 1] = __builtin_amdgcn_raw_buffer_load_b32(wrsrc, lane_off4, wsoff(o + j - 1), 0);
                    any = false;
                }
            }
            if (kPlanesPerWord == 4) {
                pw_[0] = 0u;
                if (any DIAG_NOLOAD) pw_[0] = __builtin_amdgcn_raw_buffer_load_b32(wrsrc, lane_off4, wsoff(o), 0);
            }
        };
        auto blend_and_store = [&](const uint32_t o, const bool (&upd_)[kBatchZ], const float (&tsdf_)[kBatchZ], const float (&pd_)[kBatchZ], const uint32_t (&pw_)[kWords],
                                   const uint32_t (&pix_)[kBatchZ]) {
            // (COLOUR) the batch's colour words and pixels are asked for first; the distance blend below runs while they come
            uint32_t cw_[kBatchZ], c0_[kBatchZ], c1_[kBatchZ], c2_[kBatchZ];
            if constexpr (COLOUR) {
#pragma unroll
                for (int j = 0; j < kBatchZ; j++) {
                    if (pix_[j] != kNoPixel) {
                        // (launch_integrate keeps frames of 2^31 bytes and more on the separate pass)
                        const uint8_t *c = rgb + 3u * pix_[j];
                        cw_[j] = *cword(o + j);
                        c0_[j] = c[0];
                        c1_[j] = c[1];
                        c2_[j] = c[2];
                    }
                }
            }
            const uint32_t zb = z0 + o;
            // (uniform) a batch with a plane in the z part of the rim zone takes the flat test on every lane
            const bool z_rim = zb < (uint32_t)(kBrick + kBrickGrow) || zb + (uint32_t)kBatchZ - 1u + (uint32_t)kBrickGrow >= (uint32_t)kBrick * (occ.nbz - 1u);
            const float lo = z_rim ? flat_lo_open : mark_lo, hi = z_rim ? occ.flat_hi : mark_hi;
            uint32_t nw_[kWords];
#pragma unroll
            for (int w = 0; w < kWords; w++) nw_[w] = pw_[w];
#pragma unroll
            for (int j = 0; j < kBatchZ; j++) {
                if (upd_[j]) {
                    constexpr uint32_t kMask = WBITS == 8 ? 0xffu : 0xffffu;
                    const int w = j / kPlanesPerWord, s = (j % kPlanesPerWord) * WBITS;
                    if constexpr (REMOVE) {
                        // de-integration: a voxel whose count is 0 (never fused, or already taken out) is left alone; the others get
                        // ((D w) - tsdf) / (w - 1), or the cleared state (+trunc, 0) when this was their only frame.  The count goes down
                        // in its own field: it is at least 1, so nothing is borrowed from the neighbour.
                        const uint32_t c = (pw_[w] >> s) & kMask;
                        if (c >= 1u) {
                            float prior_weight = (float)c;
                            asm("" : "+v"(prior_weight));   // (opaque, as in the blend below)
                            const float new_weight = prior_weight - 1.0f;
                            float new_distance = g.trunc;
                            if (new_weight > 0.0f) new_distance = div_by_count((pd_[j] * prior_weight) - (tsdf_[j] * 1.0f), new_weight);
                            nw_[w] -= 1u << s;
                            if (__float_as_uint(new_distance) != __float_as_uint(pd_[j])) {   // (only a distance whose bits change is stored)
                                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(new_distance), drsrc, lane_off4, dsoff(o + j), 0);
                                wrote = true;
                                if (COUNT) stores++;
                            }
                            if (!(new_distance > lo) || new_distance > hi) {   // (the blend's test: a removal can pull a distance down)
                                const uint32_t o_ = o + j;
                                if (o_ < 32u) low_lo |= 1u << o_; else low_hi |= 1u << (o_ - 32u);
                            }
                            if (COUNT) updated++;
                        }
                    } else {
                    float prior_weight = (float)((pw_[w] >> s) & kMask);
                    asm("" : "+v"(prior_weight));   // (opaque: the compiler otherwise forms count + 1 in integers and converts a second time)
                    const float new_weight = prior_weight + 1.0f;                                                   // :375-376
                    const float new_distance = div_by_count((pd_[j] * prior_weight) + (tsdf_[j] * 1.0f), new_weight);   // :381
                    if constexpr (CAPPED) {
                        // the stored count is min(count + 1, cap) -- the divisor above stays count + 1 -- as a signed step of this field
                        // alone: 0 at the cap, negative for a count found above it; every field stays inside its bits, so no carry or borrow
                        const uint32_t c = (pw_[w] >> s) & kMask;
                        nw_[w] += (min(c + 1u, cap) - c) << s;
                    } else
                    nw_[w] += 1u << s;   // (the caller has made room: weights.hip, weights_make_room)
                    // The distance is stored only when its bits change: a voxel that has only seen free space holds +trunc, and the
                    // blend (D w + trunc) / (w + 1) gives +trunc back bit for bit at most counts (it moves at 6, 7, 9, 12, 22, 25, ...),
                    // so most stores in front of the surface would write what memory holds.  Bits, not floats: -0 / +0 and NaN
                    // payloads stay as the blend leaves them.
                    if (__float_as_uint(new_distance) != __float_as_uint(pd_[j]) DIAG_NOSTORE_D) {
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(new_distance), drsrc, lane_off4, dsoff(o + j), 0);
                        wrote = true;
                        if (COUNT) stores++;
                    }
                    if (!(new_distance > lo) || new_distance > hi) {   // not safely positive (rim zone: not flat): remember the plane
                        const uint32_t o_ = o + j;
                        if (o_ < 32u) low_lo |= 1u << o_; else low_hi |= 1u << (o_ - 32u);
                    }
                    if (COUNT) updated++;
                    }
                }
            }
#pragma unroll
            for (int w = 0; w < kWords; w++)
                if (nw_[w] != pw_[w] DIAG_NOSTORE_W) __builtin_amdgcn_raw_buffer_store_b32(nw_[w], wrsrc, lane_off4, wsoff(o + w * kPlanesPerWord), 0);
            if constexpr (COLOUR) {
#pragma unroll
                for (int j = 0; j < kBatchZ; j++) {
                    if (pix_[j] != kNoPixel) *cword(o + j) = colour_blend(cw_[j], c0_[j], c1_[j], c2_[j]);
                }
            }
        };
        static_assert(kChunkZ % (2 * kBatchZ) == 0, "the pipeline alternates two register sets");
        float tsdf_a[kBatchZ], pd_a[kBatchZ], tsdf_b[kBatchZ], pd_b[kBatchZ];
        uint32_t pw_a[kWords], pw_b[kWords];
        bool upd_a[kBatchZ], upd_b[kBatchZ];   // (lane masks in scalar registers)
        uint32_t pix_a[kBatchZ], pix_b[kBatchZ];   // (COLOUR only)
#if TSDF_PACKED_PIPELINE
        project_and_load(0, upd_a, tsdf_a, pd_a, pw_a, pix_a);
#pragma unroll
        for (uint32_t o = 0; o < (uint32_t)kChunkZ; o += 2 * kBatchZ) {
            // (batches past z1 -- the last bricks of a grid whose depth is not a multiple of kChunkZ -- are all NaN planes)
            project_and_load(o + kBatchZ, upd_b, tsdf_b, pd_b, pw_b, pix_b);
            blend_and_store(o, upd_a, tsdf_a, pd_a, pw_a, pix_a);
            if (o + 2 * kBatchZ < (uint32_t)kChunkZ) project_and_load(o + 2 * kBatchZ, upd_a, tsdf_a, pd_a, pw_a, pix_a);
            blend_and_store(o + kBatchZ, upd_b, tsdf_b, pd_b, pw_b, pix_b);
        }
#else
        // (A/B of round 6: one register set, a batch's loads waited for before its blend: more waves per SIMD hide the round trip instead)
        (void)tsdf_b; (void)pd_b; (void)pw_b; (void)upd_b; (void)pix_b;
#pragma unroll
        for (uint32_t o = 0; o < (uint32_t)kChunkZ; o += kBatchZ) {
            project_and_load(o, upd_a, tsdf_a, pd_a, pw_a, pix_a);
            blend_and_store(o, upd_a, tsdf_a, pd_a, pw_a, pix_a);
        }
#endif
        if (z_extra != 0) {   // (uniform; after the pipeline, not inside it)
            project_and_load(kChunkZ, upd_a, tsdf_a, pd_a, pw_a, pix_a);
            blend_and_store(kChunkZ, upd_a, tsdf_a, pd_a, pw_a, pix_a);
        }
        };
        if (staged) walk(std::true_type{}); else walk(std::false_type{});
        if (__any((low_lo | low_hi) != 0u))
            mark_low_voxels(occ, low_lo, low_hi, (bx * kTileX) >> kBrickShift, __builtin_amdgcn_readfirstlane(vy), z0, z0, z1 - 1u, threadIdx.x);
        // for the next occupancy rebuild (volume.hip): this brick's distances have changed.  A brick whose every store was skipped
        // holds the bits it held, so the summary bits of its last scan still describe it and it is left unmarked.
        if (__any(wrote) && threadIdx.x == 0) touched[b] = 1;
    }
    if (COUNT) {   // (waves that left early counted nothing)
        for (int o = 32; o > 0; o >>= 1) updated += __shfl_down(updated, o);
        for (int o = 32; o > 0; o >>= 1) stores += __shfl_down(stores, o);
        if ((threadIdx.x & 63u) == 0 && updated) atomicAdd(counter, (unsigned long long)updated);
        if ((threadIdx.x & 63u) == 0 && stores) atomicAdd(counter + kCounterStores, (unsigned long long)stores);
    }
