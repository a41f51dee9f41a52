// The chunk scan of the mesh operations: two exclusive scans at once over per-chunk counts, 1024 chunks a workgroup,
// then the workgroups' sums.  The counts are read, and the bases written in their place, through ChunkCounts (the records of an
// extraction) or ArrayCounts (the keep counts of a compaction, the row lengths of a smoothing): mesh_handle.hpp.
//   mesh_scan_sums_kernel    part[2 p], part[2 p + 1]: the sums of workgroup p's 1024 chunks
//   mesh_scan_parts_kernel   in place, one workgroup: the sums of the parts before p; the two totals behind them
//   mesh_scan_apply_kernel   counts -> bases
// No atomics, every output word has one writer.
#include "common.hpp"
#include "mesh_device.hpp"
#include "mesh_handle.hpp"

namespace tsdf {

template <typename Counts>
__global__ __launch_bounds__(1024) void mesh_scan_sums_kernel(const Counts counts, uint64_t *__restrict__ part) {
    __shared__ uint32_t sa[16], sb[16];
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t a = wave_inclusive_sum(counts.first(i), lane);
    const uint32_t b = wave_inclusive_sum(counts.second(i), lane);
    if (lane == 63) {
        sa[wave] = a;
        sb[wave] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t ta = 0, tb = 0;
        for (int w = 0; w < 16; w++) {
            ta += sa[w];
            tb += sb[w];
        }
        part[2 * blockIdx.x] = ta;
        part[2 * blockIdx.x + 1] = tb;
    }
}

// In place, one workgroup: part[2 p], part[2 p + 1] = the sums of the parts before p; part[2 n_parts], [2 n_parts + 1] = the totals.
__global__ __launch_bounds__(1024) void mesh_scan_parts_kernel(uint64_t *__restrict__ part, uint32_t n_parts) {
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

// (An extraction's totals above 2^32 - 1 wrap here; its host refuses them before anything reads a base.  The other totals are at most
// their source's counts, which fit 32 bits.)
template <typename Counts>
__global__ __launch_bounds__(1024) void mesh_scan_apply_kernel(const Counts counts, const uint64_t *__restrict__ part) {
    __shared__ uint32_t sa[16], sb[16];
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t a = counts.first(i), b = counts.second(i);
    const uint32_t ia = wave_inclusive_sum(a, lane), ib = wave_inclusive_sum(b, lane);
    if (lane == 63) {
        sa[wave] = ia;
        sb[wave] = ib;
    }
    __syncthreads();
    uint32_t ba = (uint32_t)part[2 * blockIdx.x], bb = (uint32_t)part[2 * blockIdx.x + 1];
    for (uint32_t w = 0; w < wave; w++) {
        ba += sa[w];
        bb += sb[w];
    }
    counts.store(i, ba + ia - a, bb + ib - b);
}

// (the caller's hipGetLastError behind its own launches covers these)
template <typename Counts>
void mesh_scan(const Counts counts, uint32_t n_parts, uint64_t *parts, hipStream_t stream) {
    hipLaunchKernelGGL(mesh_scan_sums_kernel<Counts>, dim3(n_parts), dim3(1024), 0, stream, counts, parts);
    hipLaunchKernelGGL(mesh_scan_parts_kernel, dim3(1), dim3(1024), 0, stream, parts, n_parts);
    hipLaunchKernelGGL(mesh_scan_apply_kernel<Counts>, dim3(n_parts), dim3(1024), 0, stream, counts, parts);
}

template void mesh_scan<ChunkCounts>(ChunkCounts, uint32_t, uint64_t *, hipStream_t);
template void mesh_scan<ArrayCounts>(ArrayCounts, uint32_t, uint64_t *, hipStream_t);

}  // namespace tsdf
