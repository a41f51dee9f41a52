// Mesh smoothing: lambda|mu (Taubin) passes over an indexed mesh, an option to pin its open border, and area-weighted vertex normals
// from the faces, on the device (include/tsdf_amd.h, "mesh smoothing").  A pass moves every vertex towards (away from)
// the mean of the other two corners of the live triples that name it, computed from the previous pass's positions.
//   smooth_count_kernel         one lane per triple: validates it (the first kernel that reads I), and a live one -- three different
//                               corners, none loose -- adds 1 to the row length of each corner (integer atomics)
//   smooth_row_sums_kernel      the row lengths of 64 vertices summed; mesh_scan_*_kernel (mesh_scan.hip) turn the sums into bases
//   smooth_row_starts_kernel    per vertex where its row begins: its chunk's base plus the lengths below it in the chunk
//   smooth_fill_kernel          one lane per triple: the other two corners into each corner's row at an atomic cursor.  The order inside a
//                               row is that of arrival, which no result depends on: every sum over a row is an integer sum
//   smooth_edges_kernel         TSDF_SMOOTH_PIN_BOUNDARY: the three edges of every live triple counted in the open-addressed table
//   smooth_pin_kernel           (key (min << 32) | max; table_claim, mesh_device.hpp); a slot counted once flags both its ends
//   smooth_pass_kernel          the hot path, 2 x iterations launches: one lane per vertex walks its row and gathers 12 bytes per neighbour
//                               from the previous buffer; no atomics.  A row longer than a wave is walked by the whole wave
//   smooth_face_normals_kernel  one lane per live triple: the cross product in double, quantised, nine 64-bit integer atomic adds
//   smooth_emit_normals_kernel  one lane per vertex: the sums normalised
// No lane waits for another anywhere: the table's walk ends on "was empty" or "was my key" (the argument is at table_claim), everything
// else is atomic adds.  Every result is a unique value -- integer sums, double arithmetic on them in a fixed order -- so two runs give the
// same bytes whatever order the waves run in.
#include <cmath>

#include "common.hpp"
#include "mesh_device.hpp"
#include "mesh_handle.hpp"

namespace tsdf {

constexpr uint32_t kWaveRow = 64;               // a row with more pairs than this is walked by its whole wave
constexpr uint32_t kSmoothMaxIterations = 1024;

// rule 1, in float on the positions given (NaN fails the comparison)
__device__ inline bool smooth_loose(const float *__restrict__ vertices, uint32_t v) {
    return !coordinate_in_range(vertices[3 * (size_t)v]) || !coordinate_in_range(vertices[3 * (size_t)v + 1]) ||
           !coordinate_in_range(vertices[3 * (size_t)v + 2]);
}

// The corners of triple t when it is live.  An index that is not below n_vertices makes the triple dead (load_triple; *bad says so).
__device__ inline bool smooth_live(uint32_t n_vertices, const uint32_t *__restrict__ indices, const float *__restrict__ vertices, uint64_t t, uint32_t c[3],
                                   bool *bad) {
    *bad = !load_triple(n_vertices, indices, t, c);
    if (*bad || c[0] == c[1] || c[0] == c[2] || c[1] == c[2]) return false;
    return !smooth_loose(vertices, c[0]) && !smooth_loose(vertices, c[1]) && !smooth_loose(vertices, c[2]);
}

__global__ __launch_bounds__(256) void smooth_count_kernel(uint32_t n_vertices, uint32_t n_triples, const uint32_t *__restrict__ indices,
                                                           const float *__restrict__ vertices, uint32_t *counts, uint64_t *__restrict__ error) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_triples) return;
    uint32_t c[3];
    bool bad;
    if (!smooth_live(n_vertices, indices, vertices, t, c, &bad)) {
        if (bad) raise_error(error, kErrorIndex);
        return;
    }
    if (!counts) return;   // (a call without passes only validates)
    for (int k = 0; k < 3; k++) atomicAdd(counts + c[k], 1u);
}

// (the pairs of all rows are at most n_indices <= 2^32 - 1: every sum fits 32 bits)
__global__ __launch_bounds__(256) void smooth_row_sums_kernel(uint32_t n_vertices, const uint32_t *__restrict__ counts, uint32_t v_chunks,
                                                              uint32_t *__restrict__ v_base) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= v_chunks) return;
    const uint64_t at = (uint64_t)chunk * 64 + lane;
    const uint32_t sum = wave_inclusive_sum(at < n_vertices ? counts[at] : 0u, lane);
    if (lane == 63) v_base[chunk] = sum;
}

// counts -> the fill's cursors, in place: a row's cursor starts where the row begins and ends where it ends
__global__ __launch_bounds__(256) void smooth_row_starts_kernel(uint32_t n_vertices, uint32_t v_chunks, const uint32_t *__restrict__ v_base,
                                                                uint32_t *__restrict__ row_begin, uint32_t *__restrict__ cursor) {
    const uint32_t lane = threadIdx.x & 63u, chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= v_chunks) return;
    const uint64_t at = (uint64_t)chunk * 64 + lane;
    const uint32_t count = at < n_vertices ? cursor[at] : 0u;
    const uint32_t begin = v_base[chunk] + wave_inclusive_sum(count, lane) - count;
    if (at < n_vertices) row_begin[at] = cursor[at] = begin;
}

__global__ __launch_bounds__(256) void smooth_fill_kernel(uint32_t n_vertices, uint32_t n_triples, const uint32_t *__restrict__ indices,
                                                          const float *__restrict__ vertices, uint32_t *cursor, uint2 *__restrict__ rows) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_triples) return;
    uint32_t c[3];
    bool bad;
    if (!smooth_live(n_vertices, indices, vertices, t, c, &bad)) return;
    for (int k = 0; k < 3; k++) rows[atomicAdd(cursor + c[k], 1u)] = make_uint2(c[(k + 1) % 3], c[(k + 2) % 3]);
}

// (three edges per live triple: at most n_indices keys in a table of at least twice as many slots)
__global__ __launch_bounds__(256) void smooth_edges_kernel(uint32_t n_vertices, uint32_t n_triples, const uint32_t *__restrict__ indices,
                                                           const float *__restrict__ vertices, uint32_t bits, unsigned long long *keys, uint32_t *counts,
                                                           uint64_t *__restrict__ error) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_triples) return;
    uint32_t c[3];
    bool bad;
    if (!smooth_live(n_vertices, indices, vertices, t, c, &bad)) return;
    for (int k = 0; k < 3; k++) {
        const uint32_t u = c[k], w = c[(k + 1) % 3];
        const unsigned long long key = (unsigned long long)(u < w ? u : w) << 32 | (u < w ? w : u);
        uint64_t slot;
        if (!table_claim(keys, bits, key, &slot)) {
            raise_error(error, kErrorTableFull);
            return;
        }
        atomicAdd(counts + slot, 1u);
    }
}

// (lanes that flag the same vertex store the same byte)
__global__ __launch_bounds__(256) void smooth_pin_kernel(uint64_t slots, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ counts,
                                                         uint8_t *__restrict__ pinned) {
    const uint64_t slot = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (slot >= slots) return;
    const unsigned long long key = keys[slot];
    if (key == kEmptyKey || counts[slot] != 1u) return;
    pinned[key >> 32] = 1;
    pinned[key & 0xffffffffull] = 1;
}

// q of rule 2 for the two neighbours of one pair (|P| < 2^21: the products are exact and below 2^31)
__device__ inline void smooth_gather(const float *__restrict__ from, const uint2 pair, long long sum[3]) {
    const float *a = from + 3 * (size_t)pair.x, *b = from + 3 * (size_t)pair.y;
    for (int k = 0; k < 3; k++) sum[k] += quantise_coordinate(a[k]) + quantise_coordinate(b[k]);
}

// One pass with factor f, rules 2 and 3.  One lane per vertex; a row of more than kWaveRow pairs (a fan's hub) is left out of the lane's
// own loop and walked by the 64 lanes of its wave together, so no lane loops for longer than kWaveRow pairs on its own.
__global__ __launch_bounds__(256) void smooth_pass_kernel(uint32_t n_vertices, const uint32_t *__restrict__ row_begin, const uint32_t *__restrict__ row_end,
                                                          const uint2 *__restrict__ rows, const uint8_t *__restrict__ pinned, const float *__restrict__ from,
                                                          float *__restrict__ to, float f) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool mine = v < n_vertices;
    uint32_t begin = 0, end = 0;
    float p[3] = {0.0f, 0.0f, 0.0f};
    if (mine) {
        begin = row_begin[v];
        end = row_end[v];
        for (int k = 0; k < 3; k++) p[k] = from[3 * v + k];
    }
    const uint32_t pairs = end - begin;
    const bool moves = pairs != 0 && !(pinned && pinned[v]);   // (a loose vertex is in no live triple: its row is empty)
    const bool wide = moves && pairs > kWaveRow;
    long long sum[3] = {0, 0, 0};
    if (moves && !wide)
        for (uint32_t i = begin; i < end; i++) smooth_gather(from, rows[i], sum);
    for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1) {
        const int owner = __ffsll((unsigned long long)todo) - 1;
        const uint32_t first = __shfl(begin, owner), last = __shfl(end, owner);
        long long part[3] = {0, 0, 0};
        for (uint64_t i = (uint64_t)first + lane; i < last; i += 64) smooth_gather(from, rows[i], part);
        for (int k = 0; k < 3; k++) {
            for (int o = 32; o > 0; o >>= 1) part[k] += __shfl_xor(part[k], o);
            if ((int)lane == owner) sum[k] = part[k];
        }
    }
    if (!mine) return;
    float out[3] = {p[0], p[1], p[2]};
    if (moves) {
        const double degree = (double)(2ull * pairs);
        bool good = true;
        for (int k = 0; k < 3; k++) {
            const double d = ((double)sum[k] / degree) / 1024.0;
            out[k] = (float)((double)p[k] + (double)f * (d - (double)p[k]));
            good = good && coordinate_in_range(out[k]);   // rule 3 (NaN and inf fail it)
        }
        if (!good)
            for (int k = 0; k < 3; k++) out[k] = p[k];
    }
    for (int k = 0; k < 3; k++) to[3 * v + k] = out[k];
}

// Rule 6.  Raises the error word as well: tsdf_vertex_normals_device and tsdf_mesh_compute_normals read I with this kernel first.
__global__ __launch_bounds__(256) void smooth_face_normals_kernel(uint32_t n_vertices, uint32_t n_triples, const uint32_t *__restrict__ indices,
                                                                  const float *__restrict__ vertices, int64_t *sums, uint64_t *__restrict__ error) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_triples) return;
    uint32_t c[3];
    bool bad;
    if (!smooth_live(n_vertices, indices, vertices, t, c, &bad)) {
        if (bad) raise_error(error, kErrorIndex);
        return;
    }
    const float *A = vertices + 3 * (size_t)c[0], *B = vertices + 3 * (size_t)c[2], *C = vertices + 3 * (size_t)c[1];   // extract_surface's wiring
    double e1[3], e2[3];
    for (int k = 0; k < 3; k++) {
        e1[k] = (double)B[k] - (double)A[k];
        e2[k] = (double)C[k] - (double)A[k];
    }
    const double cross[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    for (int k = 0; k < 3; k++) {
        const long long q = llrint(cross[k] * 65536.0);   // |cross| < 2^45: below 2^61
        if (q)
            for (int corner = 0; corner < 3; corner++) atomicAdd((unsigned long long *)(sums + 3 * (size_t)c[corner] + k), (unsigned long long)q);
    }
}

__global__ __launch_bounds__(256) void smooth_emit_normals_kernel(uint32_t n_vertices, const int64_t *__restrict__ sums, float *__restrict__ normals) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    store_unit_or_nan(normals + 3 * v, (double)sums[3 * v], (double)sums[3 * v + 1], (double)sums[3 * v + 2]);
}

}  // namespace tsdf

using namespace tsdf;

namespace {

// Rule 6 enqueued: sums (3 n_vertices words) zeroed, filled and normalised into normals.
int normals_on(uint32_t nv, uint32_t n_triples, const float *vertices, const uint32_t *indices, int64_t *sums, uint64_t *error, float *normals,
               hipStream_t stream) {
    TSDF_HIP(hipMemsetAsync(sums, 0, (size_t)nv * 3 * sizeof(int64_t), stream), "mesh normals sums");
    if (n_triples)
        hipLaunchKernelGGL(smooth_face_normals_kernel, grid_for(n_triples, 256), dim3(256), 0, stream, nv, n_triples, indices, vertices, sums, error);
    hipLaunchKernelGGL(smooth_emit_normals_kernel, grid_for(nv, 256), dim3(256), 0, stream, nv, sums, normals);
    TSDF_HIP(hipGetLastError(), "mesh normals kernels failed");
    return TSDF_OK;
}

// Everything between the argument checks and the counts in dst->info.  n_vertices > 0; dst->info is already that of an empty mesh.
int smooth_on(uint32_t nv, uint32_t n_triples, const float *vertices, const uint32_t *indices, const float *normals, const uint8_t *rgb, uint32_t iterations,
              float lambda, float mu, uint32_t flags, tsdf_mesh *dst, hipStream_t stream, const char *who) {
    const float factor[2] = {lambda, mu};
    const uint64_t passes = n_triples ? (uint64_t)iterations * ((lambda != 0.0f) + (mu != 0.0f)) : 0;   // (without a triple nothing moves)
    const bool pins = passes != 0 && (flags & TSDF_SMOOTH_PIN_BOUNDARY), face_normals = (flags & TSDF_SMOOTH_NORMALS) != 0;
    const uint32_t v_chunks = (nv + 63) / 64, n_parts = mesh_scan_parts(v_chunks);
    const size_t n_indices = (size_t)n_triples * 3;
    const uint32_t bits = mesh_table_bits(n_indices);   // three edges per triple
    const size_t slots = (size_t)1 << bits;
    hipError_t e = device_reserve(dst->vertices, dst->vertices_cap, (size_t)nv * 3);
    if (e == hipSuccess) e = device_reserve(dst->indices, dst->indices_cap, n_indices ? n_indices : 1);
    if (e == hipSuccess && (normals || face_normals)) e = device_reserve(dst->normals, dst->normals_cap, (size_t)nv * 3);
    if (e == hipSuccess && rgb) e = device_reserve(dst->rgb, dst->rgb_cap, (size_t)nv * 3);
    if (e != hipSuccess) return hip_fail(e, "mesh array alloc failed");
    e = device_reserve(dst->parts, dst->parts_cap, 2 * ((size_t)n_parts + 1) + 1);   // the sums, the two totals, the error word
    if (e == hipSuccess && passes) e = device_reserve(dst->keep_bases, dst->keep_bases_cap, (size_t)v_chunks);
    if (e == hipSuccess && passes) e = device_reserve(dst->row_begin, dst->row_begin_cap, (size_t)nv);
    if (e == hipSuccess && passes) e = device_reserve(dst->row_end, dst->row_end_cap, (size_t)nv);
    if (e == hipSuccess && passes) e = device_reserve(dst->rows, dst->rows_cap, n_indices);
    if (e == hipSuccess && passes > 1) e = device_reserve(dst->smooth_positions, dst->smooth_positions_cap, (size_t)nv * 3);
    if (e == hipSuccess && pins) e = device_reserve(dst->pinned, dst->pinned_cap, (size_t)nv);
    if (e == hipSuccess && pins) e = device_reserve(dst->cell_keys, dst->cell_keys_cap, slots);
    if (e == hipSuccess && pins) e = device_reserve(dst->cell_reps, dst->cell_reps_cap, slots);
    if (e == hipSuccess && face_normals) e = device_reserve(dst->normal_sums, dst->normal_sums_cap, (size_t)nv * 3);
    if (e != hipSuccess) return hip_fail(e, "mesh smooth scratch alloc failed");
    uint64_t *error = dst->parts + 2 * ((size_t)n_parts + 1);
    TSDF_HIP(hipMemsetAsync(error, 0, sizeof(uint64_t), stream), "mesh smooth error word");
    // what the call carries over as the same bytes
    if (n_indices) TSDF_HIP(hipMemcpyAsync(dst->indices, indices, n_indices * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream), "mesh smooth indices");
    if (normals && !face_normals)
        TSDF_HIP(hipMemcpyAsync(dst->normals, normals, (size_t)nv * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream), "mesh smooth normals");
    if (rgb) TSDF_HIP(hipMemcpyAsync(dst->rgb, rgb, (size_t)nv * 3, hipMemcpyDeviceToDevice, stream), "mesh smooth colours");

    if (n_triples) {
        // the rows; a call without passes only validates the indices
        uint32_t *cursor = passes ? dst->row_end : nullptr;
        if (passes) TSDF_HIP(hipMemsetAsync(cursor, 0, (size_t)nv * sizeof(uint32_t), stream), "mesh smooth rows");
        hipLaunchKernelGGL(smooth_count_kernel, grid_for(n_triples, 256), dim3(256), 0, stream, nv, n_triples, indices, vertices, cursor, error);
        if (passes) {
            uint32_t *v_base = dst->keep_bases;
            hipLaunchKernelGGL(smooth_row_sums_kernel, dim3((v_chunks + 3) / 4), dim3(256), 0, stream, nv, cursor, v_chunks, v_base);
            mesh_scan(ArrayCounts{v_base, v_chunks, nullptr, 0u}, n_parts, dst->parts, stream);
            hipLaunchKernelGGL(smooth_row_starts_kernel, dim3((v_chunks + 3) / 4), dim3(256), 0, stream, nv, v_chunks, v_base, dst->row_begin, cursor);
            hipLaunchKernelGGL(smooth_fill_kernel, grid_for(n_triples, 256), dim3(256), 0, stream, nv, n_triples, indices, vertices, cursor, dst->rows);
        }
        if (pins) {
            TSDF_HIP(hipMemsetAsync(dst->cell_keys, 0xff, slots * sizeof(uint64_t), stream), "mesh smooth table");
            TSDF_HIP(hipMemsetAsync(dst->cell_reps, 0, slots * sizeof(uint32_t), stream), "mesh smooth table");
            TSDF_HIP(hipMemsetAsync(dst->pinned, 0, (size_t)nv, stream), "mesh smooth pins");
            hipLaunchKernelGGL(smooth_edges_kernel, grid_for(n_triples, 256), dim3(256), 0, stream, nv, n_triples, indices, vertices, bits,
                               (unsigned long long *)dst->cell_keys, dst->cell_reps, error);
            hipLaunchKernelGGL(smooth_pin_kernel, grid_for(slots, 256), dim3(256), 0, stream, (uint64_t)slots, (const unsigned long long *)dst->cell_keys,
                               dst->cell_reps, dst->pinned);
        }
        TSDF_HIP(hipGetLastError(), "mesh smooth row kernels failed");
        uint64_t host = 0;
        const int rc = error_word_checked(who, nv, error, &host, 1, 0, stream);   // the one synchronisation: no pass runs on a mesh that is refused
        if (rc != TSDF_OK) return rc;
        TSDF_REQUIRE(host == 0, "%s: the edge table overflowed", who);
    }

    // the passes alternate between two buffers so that the last one writes dst->vertices; the first one reads the source
    if (passes == 0) {
        TSDF_HIP(hipMemcpyAsync(dst->vertices, vertices, (size_t)nv * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream), "mesh smooth vertices");
    } else {
        const float *from = vertices;
        uint64_t left = passes;
        for (uint32_t i = 0; i < iterations; i++)
            for (int k = 0; k < 2; k++) {
                if (factor[k] == 0.0f) continue;   // (-0.0f as well)
                left--;
                float *to = left % 2 == 0 ? dst->vertices : dst->smooth_positions;
                hipLaunchKernelGGL(smooth_pass_kernel, grid_for(nv, 256), dim3(256), 0, stream, nv, dst->row_begin, dst->row_end, dst->rows,
                                   pins ? dst->pinned : (const uint8_t *)nullptr, from, to, factor[k]);
                from = to;
            }
        TSDF_HIP(hipGetLastError(), "mesh smooth pass kernels failed");
    }
    if (face_normals) {
        const int rc = normals_on(nv, n_triples, dst->vertices, indices, dst->normal_sums, error, dst->normals, stream);
        if (rc != TSDF_OK) return rc;
    }
    dst->info.n_vertices = nv;
    dst->info.n_indices = n_indices;
    return TSDF_OK;
}

// the checks both entry points share, and the run as a call into dst
int smooth_checked(uint64_t n_vertices, uint64_t n_indices, const float *vertices, const uint32_t *indices, const float *normals, const uint8_t *rgb,
                   uint32_t iterations, float lambda, float mu, uint32_t flags, tsdf_mesh *dst, hipStream_t stream, const char *who) {
    const int rc = arrays_checked(who, n_vertices, n_indices, vertices, indices);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(std::isfinite(lambda) && std::isfinite(mu), "%s: lambda (%g) and mu (%g) must be finite", who, (double)lambda, (double)mu);
    TSDF_REQUIRE(iterations <= kSmoothMaxIterations, "%s: %u iterations are more than the %u one call takes", who, iterations, kSmoothMaxIterations);
    TSDF_REQUIRE((flags & ~(uint32_t)(TSDF_SMOOTH_PIN_BOUNDARY | TSDF_SMOOTH_NORMALS)) == 0, "%s: unknown flags %#x", who, flags);
    const uint32_t info_flags = (normals || (flags & TSDF_SMOOTH_NORMALS) ? TSDF_MESH_NORMALS : 0u) | (rgb ? TSDF_MESH_COLOURS : 0u);
    return mesh_into(who, n_vertices, n_indices, info_flags, dst, stream, [&] {
        return smooth_on((uint32_t)n_vertices, (uint32_t)(n_indices / 3), vertices, indices, normals, rgb, iterations, lambda, mu, flags, dst, stream, who);
    });
}

// the error word of a normals call, read back: the one synchronisation
int normals_verdict(const uint64_t *error, uint64_t n_vertices, hipStream_t stream, const char *who) {
    uint64_t host = 0;
    return error_word_checked(who, n_vertices, error, &host, 1, 0, stream);
}

}  // namespace

extern "C" {

int tsdf_smooth_mesh_device(uint64_t n_vertices, uint64_t n_indices, const float *device_vertices, const uint32_t *device_indices,
                            const float *device_normals, const uint8_t *device_rgb, uint32_t iterations, float lambda, float mu, uint32_t flags,
                            tsdf_mesh *dst, void *hip_stream) {
    TSDF_REQUIRE(dst, "tsdf_smooth_mesh_device: null dst");
    return smooth_checked(n_vertices, n_indices, device_vertices, device_indices, device_normals, device_rgb, iterations, lambda, mu, flags, dst,
                          (hipStream_t)hip_stream, "tsdf_smooth_mesh_device");
}

int tsdf_mesh_smooth(tsdf_mesh *src, uint32_t iterations, float lambda, float mu, uint32_t flags, tsdf_mesh *dst, void *hip_stream) {
    const char *who = "tsdf_mesh_smooth";
    hipStream_t stream = (hipStream_t)hip_stream;
    return mesh_from_handle(who, "smooth", src, dst, flags & TSDF_SMOOTH_NORMALS ? TSDF_MESH_NORMALS : 0u, stream,
                            [&](uint64_t nv, uint64_t ni, const float *vertices, const uint32_t *indices, const float *normals, const uint8_t *rgb) {
                                return smooth_checked(nv, ni, vertices, indices, normals, rgb, iterations, lambda, mu, flags, dst, stream, who);
                            });
}

int tsdf_vertex_normals_device(uint64_t n_vertices, uint64_t n_indices, const float *device_vertices, const uint32_t *device_indices,
                               float *device_normals_out, void *hip_stream) {
    const char *who = "tsdf_vertex_normals_device";
    int rc = arrays_checked(who, n_vertices, n_indices, device_vertices, device_indices);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(device_normals_out || n_vertices == 0, "%s: null device_normals_out with n_vertices = %llu", who, (unsigned long long)n_vertices);
    if (n_vertices == 0) return n_indices ? index_refused(who, 0) : TSDF_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    int64_t *sums = nullptr;   // three sums per vertex and the error word, for the duration of the call
    TSDF_HIP(hipMalloc((void **)&sums, ((size_t)n_vertices * 3 + 1) * sizeof(int64_t)), "mesh normals scratch alloc failed");
    uint64_t *error = (uint64_t *)(sums + (size_t)n_vertices * 3);
    rc = hipMemsetAsync(error, 0, sizeof(uint64_t), stream) == hipSuccess ? TSDF_OK : hip_fail(hipGetLastError(), "mesh normals error word");
    if (rc == TSDF_OK) rc = normals_on((uint32_t)n_vertices, (uint32_t)(n_indices / 3), device_vertices, device_indices, sums, error, device_normals_out, stream);
    const int rc2 = normals_verdict(error, n_vertices, stream, who);   // (synchronises whatever was enqueued before the scratch goes)
    (void)hipFree(sums);
    return rc != TSDF_OK ? rc : rc2;
}

int tsdf_mesh_compute_normals(tsdf_mesh *m, void *hip_stream) {
    const char *who = "tsdf_mesh_compute_normals";
    TSDF_REQUIRE(m, "%s: null mesh", who);
    hipStream_t stream = (hipStream_t)hip_stream;
    int rc = mesh_join(m, stream);
    if (rc != TSDF_OK) return rc;
    const size_t nv = (size_t)m->info.n_vertices;
    if (nv == 0) {
        m->info.flags |= TSDF_MESH_NORMALS;
        return TSDF_OK;
    }
    hipError_t e = device_reserve(m->normal_sums, m->normal_sums_cap, nv * 3);
    if (e == hipSuccess) e = device_reserve(m->parts, m->parts_cap, (size_t)1);   // the error word
    if (e != hipSuccess) return hip_fail(e, "mesh normals scratch alloc failed");
    if (m->normals_cap < nv * 3) {   // (with the array gone the mesh has no normals, should anything below fail)
        m->info.flags &= ~(uint32_t)TSDF_MESH_NORMALS;
        e = device_reserve(m->normals, m->normals_cap, nv * 3);
        if (e != hipSuccess) return hip_fail(e, "mesh array alloc failed");
    }
    TSDF_HIP(hipMemsetAsync(m->parts, 0, sizeof(uint64_t), stream), "mesh normals error word");
    rc = normals_on((uint32_t)nv, (uint32_t)(m->info.n_indices / 3), m->vertices, m->indices, m->normal_sums, m->parts, m->normals, stream);
    if (rc == TSDF_OK) rc = normals_verdict(m->parts, nv, stream, who);
    const int rc2 = mesh_leave(m, stream);
    if (rc != TSDF_OK) return rc;
    m->info.flags |= TSDF_MESH_NORMALS;
    return rc2;
}

}  // extern "C"
