// Stand-alone host program for a sanitizer build (make sanitize-scene-flow): every argument check and refusal of
// tsdf_volume_apply_scene_flow[_device] (tsdf_amd/csrc/scene_flow.hip), which all return before any device work, on hand-made handles.
// It is linked with scene_flow.hip alone: the four library functions that file calls after its checks are stubs that must not be
// reached.  No GPU is needed or used.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "mesh_handle.hpp"

static char g_message[512];
static int g_reached = 0;

namespace tsdf {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_message, sizeof(g_message), fmt, ap);
    va_end(ap);
}
int hip_fail(hipError_t, const char *) { g_reached++; return TSDF_ERR_DEVICE; }
int deform_points_on(const tsdf_volume *, int, float *, hipStream_t) { g_reached++; return TSDF_ERR_DEVICE; }
}  // namespace tsdf
extern "C" int tsdf_volume_deformation(tsdf_volume *, tsdf_deformation_node **) { g_reached++; return TSDF_ERR_DEVICE; }

static int failures = 0;
static void expect(int rc, int want, const char *needle, const char *what) {
    if (rc != want || (needle && !strstr(g_message, needle))) {
        std::printf("FAIL %s: rc %d (want %d), message \"%s\"\n", what, rc, want, g_message);
        failures++;
    }
    g_message[0] = 0;
}

int main() {
    tsdf_volume *v = (tsdf_volume *)calloc(1, sizeof(tsdf_volume));
    tsdf_mesh *m = (tsdf_mesh *)calloc(1, sizeof(tsdf_mesh));
    v->g.X = 24; v->g.Y = 20; v->g.Z = 17;
    v->z_begin = 0; v->z_end = 17;
    v->g.z_store_end = 17;
    m->grid[0] = 24; m->grid[1] = 20; m->grid[2] = 17;
    const uint32_t W = 40, H = 30;
    std::vector<uint16_t> depth(W * H, 400);
    std::vector<float> flow(W * H * 3, 1.0f);
    float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, inv_pose[16], k[9] = {35, 0, 0, 0, 35, 0, 20, 15, 1}, kinv[9];
    memcpy(inv_pose, pose, sizeof(pose));
    memcpy(kinv, k, sizeof(k));
    tsdf_scene_flow_info info;
    auto call = [&](tsdf_volume *vv, tsdf_mesh *mm, const uint16_t *d, const float *f, uint32_t w, uint32_t h, const float *p, const float *ip,
                    const float *kk, const float *ki, float threshold, uint32_t flags, bool device) {
        return device ? tsdf_volume_apply_scene_flow_device(vv, mm, d, f, w, h, p, ip, kk, ki, threshold, flags, &info, nullptr)
                      : tsdf_volume_apply_scene_flow(vv, mm, d, f, w, h, p, ip, kk, ki, threshold, flags, &info);
    };
    for (int device = 0; device < 2; device++) {
        const bool dv = device != 0;
        // an empty whole-grid mesh: a successful no-op with an all-zero info, nothing reached
        memset(&info, 0xff, sizeof(info));
        expect(call(v, m, depth.data(), flow.data(), W, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_OK, nullptr, "empty mesh");
        if (info.n_vertices || info.n_correspondences || info.n_nodes_moved) { std::printf("FAIL empty mesh: info not zero\n"); failures++; }
        expect(call(nullptr, m, depth.data(), flow.data(), W, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "null", "null volume");
        expect(call(v, nullptr, depth.data(), flow.data(), W, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "null", "null mesh");
        expect(call(v, m, nullptr, flow.data(), W, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "null", "null depth");
        expect(call(v, m, depth.data(), nullptr, W, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "null", "null flow");
        expect(call(v, m, depth.data(), flow.data(), W, H, nullptr, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "null", "null pose");
        expect(call(v, m, depth.data(), flow.data(), W, H, pose, nullptr, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "null", "null inv_pose");
        expect(call(v, m, depth.data(), flow.data(), W, H, pose, inv_pose, nullptr, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "null", "null k");
        expect(call(v, m, depth.data(), flow.data(), W, H, pose, inv_pose, k, nullptr, 10.0f, 0, dv), TSDF_ERR_INVALID, "null", "null kinv");
        expect(call(v, m, depth.data(), flow.data(), W, H, pose, inv_pose, k, kinv, 10.0f, 2u, dv), TSDF_ERR_INVALID, "flags", "unknown flags");
        expect(call(v, m, depth.data(), flow.data(), 0, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "image", "no pixels");
        expect(call(v, m, depth.data(), flow.data(), 65536u, 65536u, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "image", "too many pixels");
        const float thresholds[4] = {0.0f, -1.0f, NAN, -INFINITY};
        for (float t : thresholds) expect(call(v, m, depth.data(), flow.data(), W, H, pose, inv_pose, k, kinv, t, 0, dv), TSDF_ERR_INVALID, "threshold", "threshold");
        for (int which = 0; which < 4; which++)
            for (int at = 0; at < (which < 2 ? 16 : 9); at++) {
                float p[16], ip[16], kk[9], ki[9];
                memcpy(p, pose, sizeof(p)); memcpy(ip, inv_pose, sizeof(ip)); memcpy(kk, k, sizeof(kk)); memcpy(ki, kinv, sizeof(ki));
                (which == 0 ? p : which == 1 ? ip : which == 2 ? kk : ki)[at] = (at & 1) ? INFINITY : NAN;
                expect(call(v, m, depth.data(), flow.data(), W, H, p, ip, kk, ki, 10.0f, 0, dv), TSDF_ERR_INVALID, "non-finite", "matrix");
            }
        v->slab = 1;
        expect(call(v, m, depth.data(), flow.data(), W, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "slab", "slab");
        v->slab = 0;
        v->z_end = 9;
        expect(call(v, m, depth.data(), flow.data(), W, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "slab", "owned planes");
        v->z_end = 17;
        m->device = 1;
        expect(call(v, m, depth.data(), flow.data(), W, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "device", "devices");
        m->device = 0;
        m->grid[2] = 16;
        expect(call(v, m, depth.data(), flow.data(), W, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "whole grid", "other dimensions");
        m->grid[0] = m->grid[1] = m->grid[2] = 0;
        expect(call(v, m, depth.data(), flow.data(), W, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "whole grid", "not a whole-grid mesh");
        m->grid[0] = 24; m->grid[1] = 20; m->grid[2] = 17;
        // vertices, but a handle whose records are too few for the grid: refused before the nodes are touched
        m->info.n_vertices = 5;
        if (dv) expect(call(v, m, depth.data(), flow.data(), W, H, pose, inv_pose, k, kinv, 10.0f, 0, dv), TSDF_ERR_INVALID, "records", "records");
        m->info.n_vertices = 0;
    }
    if (g_reached) { std::printf("FAIL: %d calls went past the checks\n", g_reached); failures++; }
    free(v);
    free(m);
    std::printf(failures ? "scene flow refusals: %d FAILED\n" : "scene flow refusals ok\n", failures);
    return failures ? 1 : 0;
}
