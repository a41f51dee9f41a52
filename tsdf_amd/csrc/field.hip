// Field queries for gfx950: the trilinear distance, its central-difference gradient and the weight of the fused field at world
// points (include/tsdf_amd.h, "field queries").  No reference counterpart: the reference's volume can be fused into, rendered and
// meshed, but a caller who wants the distance at a point has to download the grid.
//
// One kernel, one thread per point, a template on the outputs asked for:
//   - q = p - offset per axis (the ray cast's space_min: ray-cast and mesh vertices are in this frame);
//   - every sample S(.) is the ray cast's own trilinear() (through field_sample.hpp, where the rules of reading the field at a point
//     are): the same voxel_for_point, lower-corner rule on the unclamped point, tap clamping at the far faces and eight-term sum, so a
//     query agrees bit for bit with what the cast saw;
//   - the gradient is six more full samples at q -+ voxel_size along each axis.  Each sample derives its own cell -- the cells of the
//     seven samples are not assumed to be neighbours: at a cell face rounding decides -- so the 56 taps are 56 loads of which 32
//     are distinct voxels; the repeats hit in the vector L1 / L2 (LABNOTES.md, "field queries").  An instance asked for the distance
//     or the weight only has none of that code in it;
//   - the weight is read from whatever storage the volume has now (weights.hip: 8- or 16-bit counts z-packed four or two planes a
//     dword, or fp32) and never converts it.
// Nothing of the volume is written: no occupancy flag, no dirty mark, no counter.
#include "common.hpp"
#include "field_sample.hpp"

namespace tsdf {

template <bool DIST, bool GRAD, bool WEIGHT, bool FASTDIV>
__global__ __launch_bounds__(256) void field_sample_kernel(const FieldView f, const uint64_t n_points, const float *__restrict__ points,
                                                           float *__restrict__ out_distance, float *__restrict__ out_gradient,
                                                           float *__restrict__ out_weight, const int unit) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_points) return;
    const float qx = points[3 * i + 0] - f.g.offset.x;
    const float qy = points[3 * i + 1] - f.g.offset.y;
    const float qz = points[3 * i + 2] - f.g.offset.z;
    const bool valid = field_valid(f, qx, qy, qz);

    if (DIST) out_distance[i] = valid ? field_distance<FASTDIV>(f, qx, qy, qz) : NAN;

    if (WEIGHT) out_weight[i] = valid ? field_weight<FASTDIV>(f, qx, qy, qz) : 0.0f;

    if (GRAD) {
        const FieldStencil s = field_stencil(f, qx, qy, qz);
        float gx = NAN, gy = NAN, gz = NAN;
        if (field_stencil_valid(f, s)) {
            field_gradient<FASTDIV>(f, s, gx, gy, gz);
            if (unit) {
                const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
                if (len > 0.0f) {   // (false for NaN)
                    gx = gx / len;
                    gy = gy / len;
                    gz = gz / len;
                } else {
                    gx = gy = gz = NAN;
                }
            }
        }
        out_gradient[3 * i + 0] = gx;
        out_gradient[3 * i + 1] = gy;
        out_gradient[3 * i + 2] = gz;
    }
}

template <bool DIST, bool GRAD, bool WEIGHT>
static void launch_field_instance(const FieldView &f, bool fast_div, uint64_t n, const float *points, float *d, float *grad, float *w,
                                  int unit, hipStream_t stream) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (fast_div)
        hipLaunchKernelGGL((field_sample_kernel<DIST, GRAD, WEIGHT, true>), grid, block, 0, stream, f, n, points, d, grad, w, unit);
    else
        hipLaunchKernelGGL((field_sample_kernel<DIST, GRAD, WEIGHT, false>), grid, block, 0, stream, f, n, points, d, grad, w, unit);
}

static int field_check(const tsdf_volume *v, const char *what) {
    TSDF_REQUIRE(v, "%s: null volume", what);
    return field_refuse_slab(v, what);
}

// the launch on a view (field_sample.hpp: also the distance field's samples, esdf.hip); at least one output is asked for, n > 0
int sample_field_view(const FieldView &v, bool fast_div, uint64_t n, const float *points, float *d, float *grad, float *w, int flags,
                      hipStream_t stream) {
    TSDF_REQUIRE((n + 255) / 256 <= 0x7FFFFFFFull, "tsdf_volume_sample_field: too many points");
    const int unit = (flags & TSDF_FIELD_UNIT_GRADIENT) ? 1 : 0;
    switch ((d ? 1 : 0) | (grad ? 2 : 0) | (w ? 4 : 0)) {
        case 1: launch_field_instance<true, false, false>(v, fast_div, n, points, d, grad, w, unit, stream); break;
        case 2: launch_field_instance<false, true, false>(v, fast_div, n, points, d, grad, w, unit, stream); break;
        case 3: launch_field_instance<true, true, false>(v, fast_div, n, points, d, grad, w, unit, stream); break;
        case 4: launch_field_instance<false, false, true>(v, fast_div, n, points, d, grad, w, unit, stream); break;
        case 5: launch_field_instance<true, false, true>(v, fast_div, n, points, d, grad, w, unit, stream); break;
        case 6: launch_field_instance<false, true, true>(v, fast_div, n, points, d, grad, w, unit, stream); break;
        default: launch_field_instance<true, true, true>(v, fast_div, n, points, d, grad, w, unit, stream); break;
    }
    TSDF_HIP(hipGetLastError(), "Field sample kernel failed");
    return TSDF_OK;
}

// the launch; v has passed field_check, at least one output is asked for, n > 0
static int sample_field(const tsdf_volume *v, uint64_t n, const float *points, float *d, float *grad, float *w, int flags,
                        hipStream_t stream) {
    return sample_field_view(make_field_view(v), v->fast_div != 0, n, points, d, grad, w, flags, stream);
}

}  // namespace tsdf

using namespace tsdf;

extern "C" {

int tsdf_volume_sample_field_device(const tsdf_volume *v, uint64_t n, const float *device_points, float *device_distance,
                                    float *device_gradient, float *device_weight, int flags, void *hip_stream) {
    const int rc = field_check(v, "tsdf_volume_sample_field");
    if (rc != TSDF_OK) return rc;
    TSDF_REQUIRE(device_distance || device_gradient || device_weight, "tsdf_volume_sample_field: no output asked for (all three are NULL)");
    TSDF_REQUIRE(n == 0 || device_points, "tsdf_volume_sample_field: null points");
    if (n == 0) return TSDF_OK;
    return sample_field(v, n, device_points, device_distance, device_gradient, device_weight, flags, (hipStream_t)hip_stream);
}

int tsdf_volume_sample_field(const tsdf_volume *v, uint64_t n, const float *host_points, float *host_distance, float *host_gradient,
                             float *host_weight, int flags) {
    const int rc0 = field_check(v, "tsdf_volume_sample_field");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(host_distance || host_gradient || host_weight, "tsdf_volume_sample_field: no output asked for (all three are NULL)");
    TSDF_REQUIRE(n == 0 || host_points, "tsdf_volume_sample_field: null points");
    if (n == 0) return TSDF_OK;
    TSDF_REQUIRE(n <= ((uint64_t)1 << 40), "tsdf_volume_sample_field: too many points");
    // one allocation: points (3n), then distance (n), gradient (3n), weight (n) as far as asked for
    const size_t fn = (size_t)n;
    const size_t o_d = 3 * fn, o_g = o_d + (host_distance ? fn : 0), o_w = o_g + (host_gradient ? 3 * fn : 0), total = o_w + (host_weight ? fn : 0);
    HostStage st;
    int rc = st.begin(v->stream, total * sizeof(float), "tsdf_volume_sample_field: couldn't allocate %zu bytes for the points and results");
    if (rc != TSDF_OK) return rc;
    float *const buf = static_cast<float *>(st.buf);
    float *d = host_distance ? buf + o_d : nullptr, *g = host_gradient ? buf + o_g : nullptr, *w = host_weight ? buf + o_w : nullptr;
    st.up(buf, host_points, 3 * fn * sizeof(float));
    if (st.ok()) rc = sample_field(v, n, buf, d, g, w, flags, v->stream);
    if (rc == TSDF_OK) {
        if (d) st.down(host_distance, d, fn * sizeof(float));
        if (g) st.down(host_gradient, g, 3 * fn * sizeof(float));
        if (w) st.down(host_weight, w, fn * sizeof(float));
    }
    return st.finish(rc, "Field sample failed");
}

int tsdf_raycast_gradient_normals_device(const tsdf_volume *v, uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                                         float *device_vertices, float *device_normals) {
    const int rc0 = field_check(v, "tsdf_raycast_gradient_normals");
    if (rc0 != TSDF_OK) return rc0;
    TSDF_REQUIRE(device_vertices && device_normals, "tsdf_raycast_gradient_normals: null buffer");
    const int rc = tsdf_raycast_device(v, width, height, pose, kinv, device_vertices, nullptr);
    if (rc != TSDF_OK) return rc;
    // a miss is a NaN vertex: not valid, the NaN triple
    return sample_field(v, (uint64_t)width * height, device_vertices, nullptr, device_normals, nullptr, TSDF_FIELD_UNIT_GRADIENT, v->stream);
}

}  // extern "C"
