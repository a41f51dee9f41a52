// The body of integrate_kernel and integrate_capped_kernel (integrate.hip), included inside each of the two: not a header (see
// integrate_packed_body.hpp).  The including kernel declares `constexpr bool CAPPED`, `capf`, the weight cap as a float, and
// `constexpr bool REMOVE` (integrate_remove_kernel: the frame is taken back out, include/tsdf_amd.h "de-integration") and
// `constexpr bool WEIGHTED` with `pweight` (integrate_weighted_kernel: one weight per pixel of the frame, include/tsdf_amd.h "weighted
// integration"; the other kernels declare it false and never read the pointer).
    // Depth tile of the current brick: the pixel box the cull kernel derived for it, staged once per brick with
    // coalesced row loads; the per-voxel depth look-ups then read LDS instead of gathering from L2.
    __shared__ uint16_t tile[kTilePixels + 2];  // [kTilePixels] stays 0: where look-ups that miss the box are pointed
    __shared__ float4 plane_lds[kChunkZ + kBatchZ];  // this brick's rows of plane_const
    const uint32_t tid = threadIdx.y * kTileX + threadIdx.x;
    const uint32_t n_active = DEFORM ? bg.nx * bg.ny * bg.nz : *count;  // custom nodes: every brick
    const size_t plane = (size_t)g.X * g.Y;
    const float neg_trunc = -g.trunc;
    const float fwidth = (float)width, fheight = (float)height;
    // see round_quotients: thr = 4e-7 * (max(width, height) + 2); the float just below 1/2 - thr
    const float round_near_half = __uint_as_float(__float_as_uint(0.5f - 4.0e-7f * ((float)max(width, height) + 2.0f)) - 1u);   // (positive: one ulp down)
    uint32_t updated = 0, stores = 0;   // (COUNT: voxels updated, distances stored)
    // a batch's prior weights; WEIGHTED: behind them, the weights of the voxels' pixels (pw_[kBatchZ + j] goes with plane j)
    constexpr int kWeightSlots = WEIGHTED ? 2 * kBatchZ : kBatchZ;

    for (uint32_t i = blockIdx.x; i < n_active; i += gridDim.x) {
        const unsigned long long dbg_t0 = (!COUNT && counter) ? wall_clock64() : 0ull;   // (diagnostics, TSDF_DEBUG_BRICKS=3: per-brick clocks)
        const uint32_t b = DEFORM ? i : list[i];
        const uint32_t bx = b % bg.nx, by = (b / bg.nx) % bg.ny, bz = b / (bg.nx * bg.ny);
        const uint32_t vx = bx * kTileX + threadIdx.x;
        const uint32_t vy = by * kTileY + threadIdx.y;
        const uint32_t z0 = g.z_store_begin + bz * kChunkZ;
        const uint32_t z_extra = bz + 1 == bg.nz ? bg.z_extra : 0u;
        const uint32_t z1 = min(z0 + kChunkZ + z_extra, g.z_store_end);  // exclusive
        // stage the brick's pixel box (whole workgroup; falls back to global gathers when it is unknown or too big)
        uint4 box = make_uint4(0, 0, 0, 0);
        if (!DEFORM) box = boxes[i];
        const uint32_t pitch = (box.z + 1u) & ~1u;  // even, so a row starts on a 4-byte boundary
        const bool staged = box.z != 0 && pitch * box.w <= (uint32_t)kTilePixels;
        __syncthreads();  // the previous brick's look-ups are done
        if (!DEFORM && tid < (uint32_t)(kChunkZ + kBatchZ)) {
            const uint32_t p = z0 - g.z_store_begin + tid;   // (plane_const is padded by kBatchZ rows)
            if (p < g.z_store_end - g.z_store_begin + kBatchZ) plane_lds[tid] = plane_const[p];
        }
        if (tid == 0) tile[kTilePixels] = 0;
        if (staged) {
            // kStageBatch look-ups are requested before the first is waited for (a loop of single look-ups is one memory round
            // trip after the other: ~16 of them per brick).  No branch inside a batch: slots past the end re-read the last pixel
            // and are not written.
            constexpr uint32_t kStageBatch = 8;
            const uint32_t total = pitch * box.w;
            if (bg.pair_loads) {
                // (even image width, 4-byte aligned image: the cull kernel has made box.x and box.z even, a lane takes two pixels)
                const uint32_t half = pitch >> 1, total2 = half * box.w;
                const uint32_t *depth2 = reinterpret_cast<const uint32_t *>(depth);
                uint32_t *tile2 = reinterpret_cast<uint32_t *>(tile);
                for (uint32_t p0 = tid; p0 < total2; p0 += kTileX * kTileY * kStageBatch) {
                    uint32_t px[kStageBatch];
#pragma unroll
                    for (uint32_t u = 0; u < kStageBatch; u++) {
                        const uint32_t p = min(p0 + u * (kTileX * kTileY), total2 - 1u);
                        const uint32_t ty = p / half, tx2 = p - ty * half;
                        px[u] = depth2[(((size_t)(box.y + ty) * width + box.x) >> 1) + tx2];
                    }
#pragma unroll
                    for (uint32_t u = 0; u < kStageBatch; u++) {
                        const uint32_t p = p0 + u * (kTileX * kTileY);
                        if (p < total2) tile2[p] = px[u];
                    }
                }
            } else
            for (uint32_t p0 = tid; p0 < total; p0 += kTileX * kTileY * kStageBatch) {
                uint16_t px[kStageBatch];
#pragma unroll
                for (uint32_t u = 0; u < kStageBatch; u++) {
                    const uint32_t p = min(p0 + u * (kTileX * kTileY), total - 1u);
                    const uint32_t ty = p / pitch, tx = min(p - ty * pitch, box.z - 1u);
                    px[u] = depth[(size_t)(box.y + ty) * width + (box.x + tx)];
                }
#pragma unroll
                for (uint32_t u = 0; u < kStageBatch; u++) {
                    const uint32_t p = p0 + u * (kTileX * kTileY);
                    const uint32_t ty = p / pitch, tx = p - ty * pitch;
                    if (p < total) tile[p] = (tx < box.z) ? px[u] : (uint16_t)0;
                }
            }
        }
        __syncthreads();
        if (vy >= g.Y) continue;   // (a whole wave)
        const bool lane_ok = vx < g.X;   // lanes past the grid's x edge stay in (the marks at the end of the brick are made by the wave's first lanes): they update nothing

        size_t idx = plane * (z0 - g.z_store_begin) + (size_t)g.X * vy + vx;  // (custom nodes only)
        // distance / weight addressing: a wave-uniform base per plane (scalar registers) + one 32-bit lane offset that
        // is the same for every plane, so the per-voxel loads and stores need no address arithmetic on the vector unit
        const size_t brick_base = plane * (z0 - g.z_store_begin) + (size_t)g.X * (by * kTileY) + (size_t)bx * kTileX;
        const uint32_t lane_off = threadIdx.y * g.X + threadIdx.x;

        // voxel centre, x and y parts: initialise_deformation (src/TSDF/TSDFVolume.cu:783-784) then
        // integrate_kernel's offset + translation (:343)
        float cx = 0.f, cy = 0.f;
        // partial row sums of inv_pose * (c,1): the reference evaluates ((m_i1*x + m_i2*y) + m_i3*z) + m_i4
        float r1 = 0.f, r2 = 0.f, r3 = 0.f, r4 = 0.f;
        float r4_[kBatchZ] = {};
        uint32_t low_lo = 0, low_hi = 0;   // bit o: my voxel of plane z0 + o got a distance that is not safely positive
        bool wrote = false;                 // my lane stored a distance of this brick
        // Voxels a brick at the grid boundary depends on are held to the stricter test of those bricks (flat, not just positive:
        // OccGrid).  Both tests are "not (d > lo) or d > hi" with per-lane bounds: (tau, +inf) inside, (the float below flat_lo,
        // flat_hi) for lanes in the x / y part of the rim zone; the planes of the z part are picked per batch of planes below.
        const bool rim_xy = occ.in_rim_zone(vx, occ.nbx) || occ.in_rim_zone(vy, occ.nby);
        const float flat_lo_open = __uint_as_float(__float_as_uint(occ.flat_lo) - 1u);   // d >= flat_lo  <=>  d > this  (flat_lo > 0, normal)
        const float mark_lo = rim_xy ? flat_lo_open : occ.tau, mark_hi = rim_xy ? occ.flat_hi : INFINITY;
        if (!DEFORM) {
            cx = ((((int)vx + 0.5f) * g.vs.x) + g.offset_clear.x) + g.offset.x;
            cy = ((((int)vy + 0.5f) * g.vs.y) + g.offset_clear.y) + g.offset.y;
            r1 = ip.m11 * cx + ip.m12 * cy;
            r2 = ip.m21 * cx + ip.m22 * cy;
            r3 = ip.m31 * cx + ip.m32 * cy;
            r4 = ip.m41 * cx + ip.m42 * cy;
        }

        // The planes of the brick are processed kBatchZ at a time in three passes -- project + gather depth,
        // decide + load distance/weight, blend + store -- so that the depth gathers of a batch, and then its
        // HBM loads, are all in flight together instead of one dependent chain per plane.  The batches are software
        // pipelined: the loads of batch b+1 are issued before batch b is blended and stored, so that there is always a
        // batch of loads in flight (two register sets, used alternately).
        auto project_and_load = [&](const uint32_t zb, float (&tsdf_)[kBatchZ], float (&pw_)[kWeightSlots], float (&pd_)[kBatchZ]) {
            const size_t idx_b = idx + plane * (size_t)(zb - z0);
            float camz_[kBatchZ], cz_[kBatchZ];
            int px_[kBatchZ], py_[kBatchZ];
            uint32_t d_[kBatchZ];  // depth of the voxel's pixel, 0 = none
            bool act[kBatchZ];
#pragma unroll
            for (int j = 0; j < kBatchZ; j++) {
                const uint32_t vz = zb + j;
                act[j] = vz < z1 && lane_ok;
                float cz = 0.f;
                if (DEFORM) {
                    // (custom nodes: x/y parts differ per voxel)
                    cz = 0.f;
                    if (act[j]) {
                        const tsdf_deformation_node &nd = nodes[idx_b + plane * j];
                        cx = nd.translation[0] + g.offset.x;
                        cy = nd.translation[1] + g.offset.y;
                        cz = nd.translation[2] + g.offset.z;
                    }
                    r1 = ip.m11 * cx + ip.m12 * cy;
                    r2 = ip.m21 * cx + ip.m22 * cy;
                    r3 = ip.m31 * cx + ip.m32 * cy;
                    r4 = ip.m41 * cx + ip.m42 * cy;
                }
                // world_to_pixel (src/Utilities/cuda_coordinate_transforms.cu:10-30)
                float camx, camy, camz;
                if (DEFORM) {
                    camx = (r1 + ip.m13 * cz) + ip.m14;
                    camy = (r2 + ip.m23 * cz) + ip.m24;
                    camz = (r3 + ip.m33 * cz) + ip.m34;
                } else {
                    const float4 pc = plane_lds[vz - z0];
                    cz = pc.x;
                    camx = (r1 + pc.y) + ip.m14;
                    camy = (r2 + pc.z) + ip.m24;
                    camz = (r3 + pc.w) + ip.m34;
                }
                cz_[j] = cz;
                camz_[j] = camz;
                const float imx = STD ? k.m11 * camx + k.m13 * camz : k.m11 * camx + k.m12 * camy + k.m13 * camz;
                const float imy = STD ? k.m22 * camy + k.m23 * camz : k.m21 * camx + k.m22 * camy + k.m23 * camz;
                const float imz = STD ? camz : k.m31 * camx + k.m32 * camy + k.m33 * camz;
                // pixel = (int)round(q) with the target's conversion (NaN -> 0, saturating); the frustum test (:349) is
                // done on the rounded floats, which order exactly like the saturated ints
                float rx, ry;
                round_quotients(imx, imy, imz, round_near_half, rx, ry);
                // (the hardware conversion saturates: anything beyond the int range is off the image either way)
                px_[j] = cvt_i32_sat(rx);
                py_[j] = cvt_i32_sat(ry);
                // The brick's pixel box (cull kernel) holds every pixel a voxel of this brick can map to, and it lies
                // inside the image: a pixel in the box passes the frustum test.  The LDS read is unconditional (a slot
                // holding 0 when outside) and the global gather a separate, rare branch, so that neither turns into a generic
                // load that would have to be waited for plane by plane.
                const uint32_t tx = (uint32_t)px_[j] - box.x, ty = (uint32_t)py_[j] - box.y;
                const bool in_box = act[j] && staged && tx < box.z && ty < box.w;
                d_[j] = tile[in_box ? __umul24(ty, pitch) + tx : (uint32_t)kTilePixels];   // (in the box both factors are < 2^13: 24-bit multiply, full rate)
                if (act[j] && !in_box && rx >= 0.0f && rx < fwidth && ry >= 0.0f && ry < fheight)
                    d_[j] = depth[(uint32_t)py_[j] * width + (uint32_t)px_[j]];
                if (DEFORM) {  // keep the per-voxel row sums for pass 2
                    r4_[j] = r4;
                }
            }
            // tsdf_[j] is NaN for a voxel this frame does not update
#pragma unroll
            for (int j = 0; j < kBatchZ; j++) {
                // pixel_to_camera(...).z (cuda_coordinate_transforms.cu:132-146)
                float surf_z, voxel_cam_z;
                if (STD) {
                    surf_z = (float)d_[j];
                    voxel_cam_z = camz_[j];
                } else {
                    const float ipz = kinv.m31 * px_[j] + kinv.m32 * py_[j] + kinv.m33;
                    const float scale = (float)d_[j] / ipz;
                    surf_z = ipz * scale;
                    // world_to_camera(...).z (cuda_coordinate_transforms.cu:108-121): same numerator as camz
                    const float w = ((DEFORM ? r4_[j] : r4) + ip.m43 * cz_[j]) + ip.m44;
                    voxel_cam_z = camz_[j] / w;
                }
                const float sdf = surf_z - voxel_cam_z;
                // depth > 0 (:355; also false for planes past the brick and pixels off the image) and sdf >= -trunc (:366)
                const bool update = d_[j] != 0 && sdf >= neg_trunc;
                // (sdf > 0) ? min(sdf, trunc) : sdf  ==  sdf < trunc ? sdf : trunc   (trunc > 0)
                tsdf_[j] = update ? (sdf < g.trunc ? sdf : g.trunc) : NAN;
                pw_[j] = pd_[j] = 0.f;
                if constexpr (WEIGHTED) pw_[kBatchZ + j] = 0.f;
                if (update) {
                    const size_t pb = brick_base + plane * (size_t)(zb - z0 + j);
                    pw_[j] = (weight + pb)[lane_off];
                    pd_[j] = (dist + pb)[lane_off];
                    // the pixel's weight, gathered beside the two loads above (a depth > 0 was read at this pixel: it lies in the image)
                    if constexpr (WEIGHTED) pw_[kBatchZ + j] = pweight[(uint32_t)py_[j] * width + (uint32_t)px_[j]];
                }
            }
        };
        auto blend_and_store = [&](const uint32_t zb, const float (&tsdf_)[kBatchZ], const float (&pw_)[kWeightSlots], const float (&pd_)[kBatchZ]) {
            // (uniform) a batch with a plane in the z part of the rim zone -- z < 6 or z >= 4 (nbz - 1) - 2 -- takes the flat test on every lane
            const bool z_rim = zb < (uint32_t)(kBrick + kBrickGrow) || zb + (uint32_t)kBatchZ - 1u + (uint32_t)kBrickGrow >= (uint32_t)kBrick * (occ.nbz - 1u);
            const float lo = z_rim ? flat_lo_open : mark_lo, hi = z_rim ? occ.flat_hi : mark_hi;
#pragma unroll
            for (int j = 0; j < kBatchZ; j++) {
                if (tsdf_[j] == tsdf_[j]) {
                    if constexpr (REMOVE) {
                        // de-integration: !(w >= 1) -- never fused, already taken out, a NaN -- is left alone; w - 1 > 0 inverts the blend,
                        // otherwise (w == 1) the voxel returns to the cleared state
                        if (pw_[j] >= 1.0f) {
                            const float new_weight = pw_[j] - 1.0f;
                            const float new_distance = new_weight > 0.0f ? ((pd_[j] * pw_[j]) - (tsdf_[j] * 1.0f)) / new_weight : g.trunc;
                            const size_t pb = brick_base + plane * (size_t)(zb - z0 + j);
                            (weight + pb)[lane_off] = new_weight;   // (+0 when it is not > 0)
                            if (__float_as_uint(new_distance) != __float_as_uint(pd_[j])) {
                                (dist + pb)[lane_off] = new_distance;
                                wrote = true;
                                if (COUNT) stores++;
                            }
                            if (!(new_distance > lo) || new_distance > hi) {
                                const uint32_t o_ = zb + j - z0;
                                if (o_ < 32u) low_lo |= 1u << o_; else low_hi |= 1u << (o_ - 32u);
                            }
                            if (COUNT) updated++;
                        }
                    } else {
                    float current_weight = 1.0f;   // (the reference's name for it, src/TSDF/TSDFVolume.cu:375)
                    if constexpr (WEIGHTED) current_weight = pw_[kBatchZ + j];
                    const float new_weight = pw_[j] + current_weight;
                    const float new_distance = ((pd_[j] * pw_[j]) + (tsdf_[j] * current_weight)) / new_weight;
                    const size_t pb = brick_base + plane * (size_t)(zb - z0 + j);
                    if constexpr (CAPPED) {
                        // only the stored weight is clamped, never the divisor (include/tsdf_amd.h, "weight cap"); the comparison keeps
                        // a NaN weight NaN.  A weight that sits at the cap comes out with the bits it had and is not written back.
                        const float stored_weight = new_weight > capf ? capf : new_weight;
                        if (__float_as_uint(stored_weight) != __float_as_uint(pw_[j])) (weight + pb)[lane_off] = stored_weight;
                    } else
                    (weight + pb)[lane_off] = new_weight;
                    // only a distance whose bits change is stored (integrate_packed.hip: free space keeps +trunc at most counts)
                    if (__float_as_uint(new_distance) != __float_as_uint(pd_[j])) {
                        (dist + pb)[lane_off] = new_distance;
                        wrote = true;
                        if (COUNT) stores++;
                    }
                    if (!(new_distance > lo) || new_distance > hi) {   // not safely positive (rim zone: not flat): remember the plane, the bricks are marked when this one is done
                        const uint32_t o_ = zb + j - z0;
                        if (o_ < 32u) low_lo |= 1u << o_; else low_hi |= 1u << (o_ - 32u);
                    }
                    if (COUNT) updated++;
                    }
                }
            }
        };
        static_assert(kChunkZ % (2 * kBatchZ) == 0, "the pipeline alternates two register sets");
        float tsdf_a[kBatchZ], pw_a[kWeightSlots], pd_a[kBatchZ], tsdf_b[kBatchZ], pw_b[kWeightSlots], pd_b[kBatchZ];
        project_and_load(z0, tsdf_a, pw_a, pd_a);
#pragma unroll
        for (uint32_t o = 0; o < (uint32_t)kChunkZ; o += 2 * kBatchZ) {
            // (batches past z1 -- the last bricks of a grid whose depth is not a multiple of kChunkZ -- are all inactive)
            project_and_load(z0 + o + kBatchZ, tsdf_b, pw_b, pd_b);
            blend_and_store(z0 + o, tsdf_a, pw_a, pd_a);
            if (o + 2 * kBatchZ < (uint32_t)kChunkZ) project_and_load(z0 + o + 2 * kBatchZ, tsdf_a, pw_a, pd_a);
            blend_and_store(z0 + o + kBatchZ, tsdf_b, pw_b, pd_b);
        }
        if (z_extra != 0) {   // (uniform; after the pipeline, not inside it)
            project_and_load(z0 + kChunkZ, tsdf_a, pw_a, pd_a);
            blend_and_store(z0 + kChunkZ, tsdf_a, pw_a, pd_a);
        }
        if (__any((low_lo | low_hi) != 0u))
            mark_low_voxels(occ, low_lo, low_hi, (bx * kTileX) >> kBrickShift, __builtin_amdgcn_readfirstlane(vy), z0, z0, z1 - 1u, threadIdx.x);
        // for the next occupancy rebuild (volume.hip): this brick's distances have changed (a brick with every store skipped is not)
        if (__any(wrote) && threadIdx.x == 0) touched[b] = 1;
        if (!COUNT && counter && tid == 0) { counter[2 * i] = dbg_t0; counter[2 * i + 1] = wall_clock64(); }
    }
    if (COUNT) {
        // wave reduction then one atomic per wave
        for (int o = 32; o > 0; o >>= 1) updated += __shfl_down(updated, o);
        for (int o = 32; o > 0; o >>= 1) stores += __shfl_down(stores, o);
        if ((threadIdx.x & 63u) == 0 && updated) atomicAdd(counter, (unsigned long long)updated);
        if ((threadIdx.x & 63u) == 0 && stores) atomicAdd(counter + kCounterStores, (unsigned long long)stores);
    }
