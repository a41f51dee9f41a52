// process_frames (reference: src/SceneFusion/SceneFusion_krnl.cu:235-401) in three steps: extract the indexed mesh, apply the scene
// flow with the reference's threshold, done.  All device work is behind the C ABI (tsdf_amd/csrc/mesh.hip, scene_flow.hip).
#include "SceneFusion_krnl.hpp"

#include "host_common.hpp"
#include "tsdf_amd.h"

const int8_t *tsdf_host_mc_triangle_table();   // MarkAndSweepMC.cpp

namespace {
const float kThreshold = 10.0f;   // "based on voxel size of 50" (:14-15)
}

void process_frames(TSDFVolume *volume, const Camera *const camera, const uint16_t width, const uint16_t height,
                    const uint16_t *const h_depth_data, const float3 *const h_scene_flow) {
    tsdf_mesh *mesh = nullptr;
    tsdf_host::check(tsdf_mesh_create(&mesh), "Couldn't extract the surface");
    int rc = tsdf_volume_extract_mesh(volume->handle(), tsdf_host_mc_triangle_table(), nullptr, 0u, mesh);
    if (rc != TSDF_OK) {
        tsdf_mesh_destroy(mesh);
        tsdf_host::check(rc, "Couldn't extract the surface");
    }
    try {
        volume->apply_scene_flow(mesh, h_depth_data, h_scene_flow, width, height, *camera, kThreshold);
    } catch (...) {
        tsdf_mesh_destroy(mesh);
        throw;
    }
    tsdf_mesh_destroy(mesh);
}
