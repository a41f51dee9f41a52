// What the two stable compactions of an indexed mesh share (mesh_components.hip: the components filter; mesh_simplify.hip: vertex
// clustering): keep counts per 64 vertices and per 64 triples turned into bases by a chunk scan in the shape of mesh_scan_*_kernel
// (mesh.hip), and the stream order of a handle.  The kernels are static: each of the two translation units carries its own copy.
#pragma once

#include "common.hpp"
#include "mesh_handle.hpp"

namespace tsdf {

__device__ inline uint32_t keep_inclusive_sum(uint32_t v, uint32_t lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(v, o);
        if ((int)lane >= o) v += up;
    }
    return v;
}

// The two exclusive scans, in the shape of mesh_scan_*_kernel (mesh.hip), over two arrays of their own lengths.
// part[2 p], part[2 p + 1]: the sums of workgroup p's 1024 chunks
static __global__ __launch_bounds__(1024) void components_scan_sums_kernel(const uint32_t *__restrict__ v_base, uint32_t v_chunks, const uint32_t *__restrict__ t_base,
                                                                    uint32_t t_chunks, uint64_t *__restrict__ part) {
    __shared__ uint32_t sv[16], st[16];
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t v = keep_inclusive_sum(i < v_chunks ? v_base[i] : 0u, lane);
    const uint32_t t = keep_inclusive_sum(i < t_chunks ? t_base[i] : 0u, lane);
    if (lane == 63) {
        sv[wave] = v;
        st[wave] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0, c = 0;
        for (int w = 0; w < 16; w++) {
            a += sv[w];
            c += st[w];
        }
        part[2 * blockIdx.x] = a;
        part[2 * blockIdx.x + 1] = c;
    }
}

// In place, one workgroup: part[2 p], part[2 p + 1] = the sums of the parts before p; part[2 n_parts], [2 n_parts + 1] = the totals.
static __global__ __launch_bounds__(1024) void components_scan_parts_kernel(uint64_t *__restrict__ part, uint32_t n_parts) {
    __shared__ uint64_t wave_sum[2][16];
    __shared__ uint64_t carry[2];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < 2) carry[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t first = 0; first < n_parts; first += 1024) {
        const uint32_t i = first + threadIdx.x;
        uint64_t v[2], incl[2];
        for (int k = 0; k < 2; k++) {
            v[k] = i < n_parts ? part[2 * (size_t)i + k] : 0;
            incl[k] = v[k];
            for (int o = 1; o < 64; o <<= 1) {
                const uint64_t up = __shfl_up(incl[k], o);
                if ((int)lane >= o) incl[k] += up;
            }
            if (lane == 63) wave_sum[k][wave] = incl[k];
        }
        __syncthreads();
        uint64_t before[2];
        for (int k = 0; k < 2; k++) {
            before[k] = carry[k];
            for (uint32_t w = 0; w < wave; w++) before[k] += wave_sum[k][w];
            if (i < n_parts) part[2 * (size_t)i + k] = before[k] + incl[k] - v[k];
        }
        __syncthreads();
        if (threadIdx.x == 1023) {
            carry[0] = before[0] + incl[0];
            carry[1] = before[1] + incl[1];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) part[2 * (size_t)n_parts + threadIdx.x] = carry[threadIdx.x];
}

// counts -> bases (the totals are at most the source's counts, which fit 32 bits)
static __global__ __launch_bounds__(1024) void components_scan_apply_kernel(uint32_t *__restrict__ v_base, uint32_t v_chunks, uint32_t *__restrict__ t_base,
                                                                     uint32_t t_chunks, const uint64_t *__restrict__ part) {
    __shared__ uint32_t sv[16], st[16];
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t v = i < v_chunks ? v_base[i] : 0u, t = i < t_chunks ? t_base[i] : 0u;
    const uint32_t iv = keep_inclusive_sum(v, lane), it = keep_inclusive_sum(t, lane);
    if (lane == 63) {
        sv[wave] = iv;
        st[wave] = it;
    }
    __syncthreads();
    uint32_t bv = (uint32_t)part[2 * blockIdx.x], bt = (uint32_t)part[2 * blockIdx.x + 1];
    for (uint32_t w = 0; w < wave; w++) {
        bv += sv[w];
        bt += st[w];
    }
    if (i < v_chunks) v_base[i] = bv + iv - v;
    if (i < t_chunks) t_base[i] = bt + it - t;
}

// where a kept vertex goes: its chunk's base plus the kept vertices below it
__device__ inline uint32_t compact_index(const uint64_t *__restrict__ v_mask, const uint32_t *__restrict__ v_base, uint32_t v) {
    return v_base[v >> 6] + (uint32_t)__popcll(v_mask[v >> 6] & ((1ull << (v & 63u)) - 1));
}

inline dim3 grid_for(uint64_t n, uint32_t per_block) { return dim3((uint32_t)((n + per_block - 1) / per_block)); }

// the stream waits for what is in flight on the handle
inline int mesh_join(tsdf_mesh *m, hipStream_t stream) {
    if (m->pending) TSDF_HIP(hipStreamWaitEvent(stream, m->done, 0), "mesh stream order");
    return TSDF_OK;
}

inline int mesh_leave(tsdf_mesh *m, hipStream_t stream) {
    TSDF_HIP(hipEventRecord(m->done, stream), "mesh event");
    m->pending = 1;
    return TSDF_OK;
}

}  // namespace tsdf
