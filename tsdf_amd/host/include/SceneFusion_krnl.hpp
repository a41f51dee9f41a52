// One frame of scene fusion: same entry point as the reference's process_frames (src/include/SceneFusion_krnl.hpp:8-13), over the C ABI
// (include/tsdf_amd.h, "scene flow").  Nodes are updated deterministically: the reference's sum with one thread running at a time.
#ifndef TSDF_AMD_HOST_SCENE_FUSION_KRNL_INCLUDED
#define TSDF_AMD_HOST_SCENE_FUSION_KRNL_INCLUDED

#include <cstdint>

#include "Camera.hpp"
#include "TSDFVolume.hpp"

// Extracts the indexed mesh of the whole grid, finds the mesh vertices the depth frame sees (the reference's threshold, 10) and pushes
// the scene flow at their pixels (width * height float3, row major) into the deformation nodes of the voxels that bracket them.
void process_frames(TSDFVolume *volume, const Camera *const camera, const uint16_t width, const uint16_t height,
                    const uint16_t *const h_depth_data, const float3 *const h_scene_flow);

#endif
