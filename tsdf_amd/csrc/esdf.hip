// The Euclidean distance field for gfx950 (include/tsdf_amd.h, "distance field"): for every voxel of a whole volume the distance to
// the nearest site -- an observed voxel with an observed 6-neighbour of the other sign -- signed and capped.  No reference counterpart.
//
// The value is a unique set of bits: q(v) = min over sites s of A.z*(float)(dz*dz) + (A.y*(float)(dy*dy) + A.x*(float)(dx*dx)), every
// fp32 operation rounded on its own.  fp32 addition is monotone, so the minimum commutes with it and three passes give exactly q:
//   esdf_sites_kernel    work = 0 at a site, +inf elsewhere; counts the sites and flags the planes that hold one
//   esdf_pass_x_kernel   work -> out:  min_j A.x*(float)(j*j) over the sites of the row, the row staged in LDS by the wave that owns it
//   esdf_pass_y_kernel   out -> work:  min_j (A.y*(float)(j*j) + in[y +- j]), lanes along x, every load a coalesced row of the plane
//   esdf_pass_z_kernel   work -> out:  the same along z, then sqrtf, the cap, the sign and the rule for unobserved voxels
// Every scan runs outwards, j = 1, 2, ..., and stops as soon as A*(float)(j*j) >= best: the term is monotone in j and the other addend
// is >= 0, so no later candidate can be smaller (exact).  It also stops at j = ceil(max_distance / voxel_size) + 1: a candidate beyond
// costs at least (max_distance + voxel_size)^2 (1 - 2^-23) > max_distance^2 -- j <= 4096, so the margin 2 voxel_size / max_distance
// is >= 2^-11 -- and the cap replaces whatever is left there, so a value below the cap is never changed.  A row without a site (a
// ballot over the staged row) and a plane without one (the flag the sites kernel left) are skipped whole.
// One writer per word, no float atomics: the array is the same on every run.  Nothing of the volume is written.
#include "common.hpp"
#include "field_sample.hpp"
#include "handle_counters.hpp"
#include "handle_order.hpp"
#include "voxel_grid.hpp"

namespace tsdf {

constexpr uint32_t kEsdfMaxAxis = 4096;   // (float)(j*j) is exact for j <= 4096
constexpr int kEsdfRows = 4;              // rows (waves) of a workgroup: blocks are 64 x 4 lanes, x fastest

// what the passes share: the count of sites, then one word per plane (1 = the plane holds a site); zeroed before every computation
struct EsdfAux {
    unsigned long long n_sites;
    uint32_t plane[kEsdfMaxAxis];
};

__global__ __launch_bounds__(256) void esdf_sites_kernel(const float *__restrict__ dist, const WeightView wv, const uint32_t X,
                                                         const uint32_t Y, const uint32_t Z, float *__restrict__ work,
                                                         EsdfAux *__restrict__ aux) {
    const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * kEsdfRows + threadIdx.y, z = blockIdx.z;
    bool site = false;
    if (x < X && y < Y) {
        const size_t xy = (size_t)X * Y, ip = (size_t)X * y + x;
        if (voxel_observed(wv, xy, ip, z)) {
            const bool neg = voxel_occupied(dist, xy * z + ip);
            // an observed neighbour inside the grid of the other sign
            auto other = [&](size_t ip2, uint32_t z2) { return voxel_observed(wv, xy, ip2, z2) && voxel_occupied(dist, xy * z2 + ip2) != neg; };
            site = (x > 0 && other(ip - 1, z)) || (x + 1 < X && other(ip + 1, z)) || (y > 0 && other(ip - X, z)) ||
                   (y + 1 < Y && other(ip + X, z)) || (z > 0 && other(ip, z - 1)) || (z + 1 < Z && other(ip, z + 1));
        }
        work[xy * z + ip] = site ? 0.0f : INFINITY;
    }
    const unsigned long long sites = __ballot(site);   // (a wave is one row of the block)
    if (sites != 0ull && threadIdx.x == 0) {
        aux->plane[z] = 1u;
        atomicAdd(&aux->n_sites, (unsigned long long)__popcll(sites));
    }
}

// One wave per row (y, z); blockDim.x / 64 rows a workgroup, `pitch` (X rounded up to 64) floats of LDS each.
__global__ __launch_bounds__(256) void esdf_pass_x_kernel(const float *__restrict__ in, float *__restrict__ out, const uint32_t X,
                                                          const uint32_t pitch, const uint64_t n_rows, const float A, const uint32_t jmax) {
    extern __shared__ float esdf_rows[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    float *row = esdf_rows + (size_t)wave * pitch;
    const uint64_t r = (uint64_t)blockIdx.x * waves + wave;
    const bool live = r < n_rows;
    bool any = false;
    for (uint32_t x = lane; x < pitch; x += 64u) {
        const float v = (live && x < X) ? in[r * X + x] : INFINITY;
        row[x] = v;
        any |= v < INFINITY;
    }
    __syncthreads();
    if (!live) return;
    float *dst = out + r * X;
    if (__ballot(any) == 0ull) {   // a row without a site
        for (uint32_t x = lane; x < X; x += 64u) dst[x] = INFINITY;
        return;
    }
    for (uint32_t x = lane; x < X; x += 64u) {
        float best = row[x];
        const uint32_t reach = max(x, X - 1u - x), jend = min(reach, jmax);
        for (uint32_t j = 1; j <= jend; j++) {
            const float t = A * (float)(j * j);
            if (t >= best) break;
            if ((j <= x && row[x - j] == 0.0f) || (x + j < X && row[x + j] == 0.0f)) {
                best = t;
                break;
            }
        }
        dst[x] = best;
    }
}

__global__ __launch_bounds__(256) void esdf_pass_y_kernel(const float *__restrict__ in, float *__restrict__ out, const uint32_t X,
                                                          const uint32_t Y, const float A, const uint32_t jmax,
                                                          const EsdfAux *__restrict__ aux) {
    const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * kEsdfRows + threadIdx.y, z = blockIdx.z;
    if (x >= X || y >= Y) return;
    const size_t col = (size_t)X * Y * z + x;
    if (aux->plane[z] == 0u) {   // a plane without a site
        out[col + (size_t)X * y] = INFINITY;
        return;
    }
    float best = in[col + (size_t)X * y];
    const uint32_t reach = max(y, Y - 1u - y), jend = min(reach, jmax);
    for (uint32_t j = 1; j <= jend; j++) {
        const float t = A * (float)(j * j);
        if (t >= best) break;
        if (j <= y) best = fminf(best, t + in[col + (size_t)X * (y - j)]);
        if (y + j < Y) best = fminf(best, t + in[col + (size_t)X * (y + j)]);
    }
    out[col + (size_t)X * y] = best;
}

__global__ __launch_bounds__(256) void esdf_pass_z_kernel(const float *__restrict__ in, float *__restrict__ out, const uint32_t X,
                                                          const uint32_t Y, const uint32_t Z, const float A, const uint32_t jmax,
                                                          const EsdfAux *__restrict__ aux, const float *__restrict__ dist,
                                                          const WeightView wv, const float max_distance, const int fill_unknown) {
    const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * kEsdfRows + threadIdx.y, z = blockIdx.z;
    if (x >= X || y >= Y) return;
    const size_t xy = (size_t)X * Y, ip = (size_t)X * y + x;
    float best = aux->plane[z] != 0u ? in[xy * z + ip] : INFINITY;
    if (aux->n_sites != 0ull) {
        const uint32_t reach = max(z, Z - 1u - z), jend = min(reach, jmax);
        for (uint32_t j = 1; j <= jend; j++) {
            const float t = A * (float)(j * j);
            if (t >= best) break;
            // (the flags are wave-uniform: a plane without a site is all +inf and is not loaded)
            if (j <= z && aux->plane[z - j] != 0u) best = fminf(best, t + in[xy * (z - j) + ip]);
            if (z + j < Z && aux->plane[z + j] != 0u) best = fminf(best, t + in[xy * (z + j) + ip]);
        }
    }
    float e = sqrtf(best);
    if (!(e < max_distance)) e = max_distance;
    float r;
    if (voxel_observed(wv, xy, ip, z))
        r = voxel_occupied(dist, xy * z + ip) ? -e : e;
    else
        r = fill_unknown ? e : NAN;
    out[xy * z + ip] = r;
}

}  // namespace tsdf

using namespace tsdf;

struct tsdf_esdf : HandleOrder {
    int computed;           // a computation has been enqueued into this handle
    float *out;             // the distance array
    float *work;            // the other side of the ping-pong
    size_t out_cap, work_cap;   // in floats
    EsdfAux *aux;
    unsigned long long *n_sites_host;   // pinned: where the count lands
    Geom g;                 // the volume's geometry when computed (sampling needs no volume)
    int fast_div;
    tsdf_esdf_info info;
};

namespace {

void esdf_free(tsdf_esdf *s) {
    s->destroy();
    device_free_all(s->out, s->work, s->aux);
    (void)hipHostFree(s->n_sites_host);
    delete s;
}

// the host waits for the computation in flight; its count of sites has then landed
int esdf_wait(const tsdf_esdf *cs) {
    if (!cs->pending) return TSDF_OK;
    const int rc = cs->wait("esdf wait");
    if (rc == TSDF_OK) const_cast<tsdf_esdf *>(cs)->info.n_sites = *cs->n_sites_host;
    return rc;
}

// the last scan index that can matter under the cap: ceil(max_distance / voxel_size) + 1, the whole axis where that is longer
uint32_t esdf_window(float max_distance, float voxel_size) {
    const double q = (double)max_distance / (double)voxel_size;
    if (!(q < (double)kEsdfMaxAxis)) return kEsdfMaxAxis;
    return (uint32_t)ceil(q) + 1u;
}

FieldView esdf_view(const tsdf_esdf *s) {
    return {s->out, {nullptr, nullptr, 0}, s->g, make_tri_const(s->g)};
}

int esdf_sample_check(const tsdf_esdf *s, uint64_t n, const float *points, const float *distance, const float *gradient, int flags) {
    TSDF_REQUIRE(s, "tsdf_esdf_sample: null handle");
    TSDF_REQUIRE(s->computed, "tsdf_esdf_sample: the handle has never been computed (tsdf_volume_compute_esdf)");
    TSDF_REQUIRE(distance || gradient, "tsdf_esdf_sample: no output asked for (both are NULL)");
    TSDF_REQUIRE(n == 0 || points, "tsdf_esdf_sample: null points");
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_esdf_create(tsdf_esdf **out) {
    return handle_create(out, "tsdf_esdf_create", "esdf alloc failed", [](tsdf_esdf *s) {
        std::memset(s, 0, sizeof(*s));
        hipError_t e = s->create();
        if (e == hipSuccess) e = hipMalloc((void **)&s->aux, sizeof(EsdfAux));
        if (e == hipSuccess) e = hipHostMalloc((void **)&s->n_sites_host, sizeof(unsigned long long), hipHostMallocDefault);
        if (e == hipSuccess) *s->n_sites_host = 0;
        return e;
    }, esdf_free);
}

void tsdf_esdf_destroy(tsdf_esdf *s) {
    if (s) esdf_free(s);
}

int tsdf_volume_compute_esdf(const tsdf_volume *cv, float max_distance, uint32_t flags, tsdf_esdf *s) {
    TSDF_REQUIRE(cv && s, "tsdf_volume_compute_esdf: null argument");
    tsdf_volume *v = const_cast<tsdf_volume *>(cv);
    const Geom &g = v->g;
    // (no 32-bit voxel ids here: the kernels index with size_t, and the axes are bounded below)
    int rc = whole_volume_checked("tsdf_volume_compute_esdf", v, s->device, "the nearest site may lie in another slab", kAcceptsWideIds);
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(max_distance > 0.0f, "tsdf_volume_compute_esdf: max_distance must be > 0 (INFINITY: no cap), got %g", (double)max_distance);
    TSDF_REQUIRE((flags & ~(uint32_t)TSDF_ESDF_FILL_UNKNOWN) == 0, "tsdf_volume_compute_esdf: unknown flags %#x", flags);
    TSDF_REQUIRE(g.X <= kEsdfMaxAxis && g.Y <= kEsdfMaxAxis && g.Z <= kEsdfMaxAxis,
                 "tsdf_volume_compute_esdf: an axis of %u x %u x %u is longer than %u voxels", g.X, g.Y, g.Z, kEsdfMaxAxis);
    rc = s->join(v->stream, "esdf stream order");   // what a previous computation into this handle left in flight
    if (rc != TSDF_OK) return rc;
    const size_t n = (size_t)g.X * g.Y * g.Z;
    hipError_t e = device_reserve(s->out, s->out_cap, n);
    if (e == hipSuccess) e = device_reserve(s->work, s->work_cap, n);
    if (e != hipSuccess) {
        s->computed = 0;
        return hip_fail(e, "esdf array alloc failed");
    }
    s->g = g;
    s->fast_div = v->fast_div;
    geometry_into(s->info, g);
    s->info.flags = flags;
    s->info.max_distance = max_distance;
    s->info.n_sites = 0;
    s->computed = 1;
    if (n == 0) return TSDF_OK;

    const float ax = g.vs.x * g.vs.x, ay = g.vs.y * g.vs.y, az = g.vs.z * g.vs.z;
    const uint32_t jx = esdf_window(max_distance, g.vs.x), jy = esdf_window(max_distance, g.vs.y), jz = esdf_window(max_distance, g.vs.z);
    const WeightView wv = {v->weight, v->wpacked, v->wmode};
    const dim3 grid((g.X + 63) / 64, (g.Y + kEsdfRows - 1) / kEsdfRows, g.Z), block(64, kEsdfRows);
    TSDF_HIP(hipMemsetAsync(s->aux, 0, sizeof(EsdfAux), v->stream), "esdf flags reset");
    hipLaunchKernelGGL(esdf_sites_kernel, grid, block, 0, v->stream, v->dist, wv, g.X, g.Y, g.Z, s->work, s->aux);
    // rows of up to 1024 voxels: four to a workgroup (16 KiB of LDS at most); longer ones: one wave, one row (16 KiB at most)
    const uint32_t pitch = (g.X + 63u) & ~63u, waves = pitch <= 1024u ? (uint32_t)kEsdfRows : 1u;
    const uint64_t n_rows = (uint64_t)g.Y * g.Z;
    hipLaunchKernelGGL(esdf_pass_x_kernel, dim3((unsigned)((n_rows + waves - 1) / waves)), dim3(64 * waves), waves * pitch * sizeof(float),
                       v->stream, s->work, s->out, g.X, pitch, n_rows, ax, jx);
    hipLaunchKernelGGL(esdf_pass_y_kernel, grid, block, 0, v->stream, s->out, s->work, g.X, g.Y, ay, jy, s->aux);
    hipLaunchKernelGGL(esdf_pass_z_kernel, grid, block, 0, v->stream, s->work, s->out, g.X, g.Y, g.Z, az, jz, s->aux, v->dist, wv,
                       max_distance, (flags & TSDF_ESDF_FILL_UNKNOWN) ? 1 : 0);
    TSDF_HIP(hipGetLastError(), "esdf kernels failed");
    TSDF_HIP(hipMemcpyAsync(s->n_sites_host, &s->aux->n_sites, sizeof(unsigned long long), hipMemcpyDeviceToHost, v->stream), "esdf count download");
    return s->leave(v->stream, "esdf event");
}

int tsdf_esdf_get_info(const tsdf_esdf *s, tsdf_esdf_info *info) {
    TSDF_REQUIRE(s && info, "tsdf_esdf_get_info: null argument");
    const int rc = esdf_wait(s);
    if (rc != TSDF_OK) return rc;
    *info = s->info;
    return TSDF_OK;
}

int tsdf_esdf_buffer(const tsdf_esdf *s, const float **device_distance) {
    TSDF_REQUIRE(s && device_distance, "tsdf_esdf_buffer: null argument");
    const int rc = esdf_wait(s);
    if (rc != TSDF_OK) return rc;
    *device_distance = s->computed ? s->out : nullptr;
    return TSDF_OK;
}

int tsdf_esdf_download(const tsdf_esdf *s, float *host_distance) {
    TSDF_REQUIRE(s && host_distance, "tsdf_esdf_download: null argument");
    TSDF_REQUIRE(s->computed, "tsdf_esdf_download: the handle has never been computed (tsdf_volume_compute_esdf)");
    const int rc = esdf_wait(s);
    if (rc != TSDF_OK) return rc;
    const size_t n = (size_t)s->g.X * s->g.Y * s->g.Z;
    if (n) TSDF_HIP(hipMemcpy(host_distance, s->out, n * sizeof(float), hipMemcpyDeviceToHost), "esdf download");
    return TSDF_OK;
}

int tsdf_esdf_sample_device(const tsdf_esdf *s, uint64_t n, const float *device_points, float *device_distance, float *device_gradient,
                            int flags, void *hip_stream) {
    const int rc0 = esdf_sample_check(s, n, device_points, device_distance, device_gradient, flags);
    if (rc0 != TSDF_OK) return rc0;
    if (n == 0) return TSDF_OK;
    // the caller's stream behind the computation
    const int rc = s->join((hipStream_t)hip_stream, "esdf stream order");
    if (rc != TSDF_OK) return rc;
    return sample_field_view(esdf_view(s), s->fast_div != 0, n, device_points, device_distance, device_gradient, nullptr, flags,
                             (hipStream_t)hip_stream);
}

int tsdf_esdf_sample(const tsdf_esdf *s, uint64_t n, const float *host_points, float *host_distance, float *host_gradient, int flags) {
    const int rc0 = esdf_sample_check(s, n, host_points, host_distance, host_gradient, flags);
    if (rc0 != TSDF_OK) return rc0;
    if (n == 0) return TSDF_OK;
    TSDF_REQUIRE(n <= ((uint64_t)1 << 40), "tsdf_esdf_sample: too many points");
    const int rcw = esdf_wait(s);
    if (rcw != TSDF_OK) return rcw;
    // one allocation: points (3n), then distance (n) and gradient (3n) as far as asked for; on the null stream, blocking
    const size_t fn = (size_t)n;
    const size_t o_d = 3 * fn, o_g = o_d + (host_distance ? fn : 0), total = o_g + (host_gradient ? 3 * fn : 0);
    HostStage st;
    int rc = st.begin(nullptr, total * sizeof(float), "tsdf_esdf_sample: couldn't allocate %zu bytes for the points and results");
    if (rc != TSDF_OK) return rc;
    float *const buf = static_cast<float *>(st.buf);
    float *d = host_distance ? buf + o_d : nullptr, *g = host_gradient ? buf + o_g : nullptr;
    st.up(buf, host_points, 3 * fn * sizeof(float));
    if (st.ok()) rc = sample_field_view(esdf_view(s), s->fast_div != 0, n, buf, d, g, nullptr, flags, nullptr);
    if (rc == TSDF_OK) {
        if (d) st.down(host_distance, d, fn * sizeof(float));
        if (g) st.down(host_gradient, g, 3 * fn * sizeof(float));
    }
    return st.finish(rc, "Distance field sample failed");
}

int tsdf_esdf_scratch_bytes(const tsdf_esdf *s, uint64_t *bytes) {
    TSDF_REQUIRE(s && bytes, "tsdf_esdf_scratch_bytes: null argument");
    *bytes = (uint64_t)s->work_cap * sizeof(float) + sizeof(EsdfAux) + sizeof(unsigned long long);
    return TSDF_OK;
}

}  // extern "C"
