// What the handles beside a volume share besides their arrays (device_buffer.hpp) and their stream order (handle_order.hpp)
// ("scratch arrays"):
//   CounterBlock       a few counter words on the device and the pinned host copy where they land: VoxelSet (voxel_set.hpp:
//                      tsdf_explorer, tsdf_objects, tsdf_frame_diff), tsdf_columns, tsdf_render and tsdf_reach
//   block_counts_*     how a workgroup closes its counters: LDS totals, then one global atomic per counter that is not zero
//   wave_reduce_roots  the per-root reduction of a wave, for the rows of a clustered set
//   handle_create      the frame of a tsdf_*_create
// The single pinned words of tsdf_esdf, tsdf_snapshot and tsdf_mesh are not counter blocks: their device side lives inside another
// array (the aux struct, the scan's parts), so they stay where they are.  Like device_buffer.hpp this includes only the HIP runtime and
// the public header, and nothing here owns memory.
#pragma once

#include <cstring>
#include <new>

#include <hip/hip_runtime.h>

#include "tsdf_amd.h"

namespace tsdf {

void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what);

// N words of type T on the device and their pinned mirror: T is unsigned long long for the word arrays, a struct of words (N = 1) where
// they have names (reach.hip).  Plain data: all zero is "not created".  A range is `n` elements from `first`, a pointer into the device
// block; a download lands at the same place in the mirror.  The failure texts are the caller's.
template <class T, size_t N = 1>
struct CounterBlock {
    T *dev;
    T *host;   // pinned

    // both allocations and the mirror zeroed; a failure leaves an empty block
    hipError_t create() {
        dev = host = nullptr;
        hipError_t e = hipMalloc((void **)&dev, N * sizeof(T));
        if (e != hipSuccess) dev = nullptr;
        else if ((e = hipHostMalloc((void **)&host, N * sizeof(T), hipHostMallocDefault)) != hipSuccess) host = nullptr;
        if (e == hipSuccess) std::memset(host, 0, N * sizeof(T));
        else release();
        return e;
    }

    // fine on a block that was never created, half created or released before
    void release() {
        (void)hipFree(dev);
        (void)hipHostFree(host);
        dev = host = nullptr;
    }

    template <class M>
    hipError_t reset(M *first, size_t n, hipStream_t stream) const {
        return hipMemsetAsync(first, 0, n * sizeof(M), stream);
    }
    hipError_t reset(hipStream_t stream) const { return reset(dev, N, stream); }

    template <class M>
    hipError_t download(M *first, size_t n, hipStream_t stream) const {
        char *to = reinterpret_cast<char *>(host) + (reinterpret_cast<const char *>(first) - reinterpret_cast<const char *>(dev));
        return hipMemcpyAsync(to, first, n * sizeof(M), hipMemcpyDeviceToHost, stream);
    }
    hipError_t download(hipStream_t stream) const { return download(dev, N, stream); }

    static constexpr uint64_t device_bytes() { return N * sizeof(T); }
};

// ---- the workgroup closing of the counters ----------------------------------------------------------------------------------------
// totals: K words of LDS.  Every lane of the workgroup calls clear and flush (they hold the barriers); how a wave forms its sum is the
// kernel's: ballot and popcount over flags, shuffles over per-lane counts, registers added up over its chunks.
template <uint32_t K>
__device__ inline void block_counts_clear(uint32_t (&totals)[K]) {
    if (threadIdx.x < K) totals[threadIdx.x] = 0;
    __syncthreads();
}

// the wave's sum for one counter, given by every lane and added by the wave's leader where it is not zero
__device__ inline void block_counts_wave(uint32_t *totals, uint32_t slot, uint32_t sum) {
    if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(totals + slot, sum);
}

// ... all K sums of a wave that keeps them in registers
template <uint32_t K>
__device__ inline void block_counts_wave(uint32_t (&totals)[K], const uint32_t (&sums)[K]) {
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (uint32_t c = 0; c < K; c++)
            if (sums[c]) atomicAdd(&totals[c], sums[c]);
    }
}

// emit(k, total) by lane k for every total that is not zero
template <uint32_t K, class Emit>
__device__ inline void block_counts_flush(const uint32_t (&totals)[K], Emit emit) {
    __syncthreads();
    if (threadIdx.x < K && totals[threadIdx.x]) emit(threadIdx.x, totals[threadIdx.x]);
}

// ... one integer atomic per counter into words[first .. first + K)
template <uint32_t K>
__device__ inline void block_counts_flush(const uint32_t (&totals)[K], unsigned long long *__restrict__ words, uint32_t first) {
    block_counts_flush(totals, [=](uint32_t k, uint32_t total) { atomicAdd(words + first + k, (unsigned long long)total); });
}

// K per-lane counts of a workgroup of 256 into words[first .. first + K): wave sums by shuffles, the four waves through LDS, one integer
// atomic per counter and workgroup.  Every lane of the workgroup calls it.  (All the voxels of a grid fit 32 bits: so does every sum.)
template <int K>
__device__ inline void block_counts_add(const uint32_t (&counts)[K], unsigned long long *__restrict__ words, uint32_t first) {
    __shared__ uint32_t totals[K];
    block_counts_clear(totals);
#pragma unroll
    for (int c = 0; c < K; c++) {
        uint32_t v = counts[c];
        for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor(v, o);
        block_counts_wave(totals, c, v);
    }
    block_counts_flush(totals, words, first);
}

// ---- the per-root reduction of a wave ------------------------------------------------------------------------------------------------
// Every lane of the wave calls it.  A valid lane brings its root's label, kRanged values that are reduced to a minimum, a maximum and a
// sum, and kSummed values that are summed only.  The wave takes its distinct roots in turn: the leading lane's label, the ballot of
// the lanes that share it, the reduction among them by shuffles (the others hold the neutral values), emit(lead, count, lo, hi, sum,
// more) by the leading lane, and those lanes retired.  Bounded: at most 64 trips, every trip retires its leading lane.  (The caller sees
// to it that a wave's sums fit 32 bits.)
template <int kRanged, int kSummed, class Emit>
__device__ inline void wave_reduce_roots(bool valid, uint32_t label, const uint32_t (&v)[kRanged], const uint32_t *summed, Emit emit) {
    uint64_t remaining = __ballot(valid);
    for (int trip = 0; trip < 64 && remaining; trip++) {
        const int first = __ffsll((unsigned long long)remaining) - 1;
        const uint32_t lead = __shfl(label, first);
        const bool mine = valid && label == lead;
        const uint64_t same = __ballot(mine);
        uint32_t lo[kRanged], hi[kRanged], sum[kRanged], more[kSummed ? kSummed : 1];
        for (int k = 0; k < kRanged; k++) {
            lo[k] = mine ? v[k] : 0xffffffffu;
            hi[k] = mine ? v[k] : 0u;
            sum[k] = mine ? v[k] : 0u;
        }
        for (int k = 0; k < kSummed; k++) more[k] = mine ? summed[k] : 0u;
        for (int o = 32; o > 0; o >>= 1) {
            for (int k = 0; k < kRanged; k++) {
                lo[k] = min(lo[k], (uint32_t)__shfl_xor(lo[k], o));
                hi[k] = max(hi[k], (uint32_t)__shfl_xor(hi[k], o));
                sum[k] += (uint32_t)__shfl_xor(sum[k], o);
            }
            for (int k = 0; k < kSummed; k++) more[k] += (uint32_t)__shfl_xor(more[k], o);
        }
        if ((int)(threadIdx.x & 63u) == first) emit(lead, (uint32_t)__popcll(same), lo, hi, sum, more);
        remaining &= ~same;
    }
}

// ---- the frame of a tsdf_*_create ----------------------------------------------------------------------------------------------------
// A value-initialised handle (a handle that is memset besides does so first thing in its init), init(handle), and on failure its
// free function (fine on a half-created handle) and TSDF_ERR_NOMEM or TSDF_ERR_DEVICE under `alloc_failed`.
template <class Handle, class Init, class Free>
int handle_create(Handle **out, const char *who, const char *alloc_failed, Init init, Free free_handle) {
    if (!out) {
        set_error("%s: null argument", who);
        return TSDF_ERR_INVALID;
    }
    *out = nullptr;
    Handle *s = new (std::nothrow) Handle();
    if (!s) {
        set_error("out of host memory");
        return TSDF_ERR_NOMEM;
    }
    const hipError_t e = init(s);
    if (e != hipSuccess) {
        free_handle(s);
        return hip_fail(e, alloc_failed);
    }
    *out = s;
    return TSDF_OK;
}

}  // namespace tsdf
