// Mesh rendering (include/tsdf_amd.h, "mesh rendering"; not in the reference, which renders its volume only): an indexed mesh
// rasterised from a pinhole camera into depth, vertex, normal, colour and triangle-id maps on the device, through a handle that keeps
// its scratch between renders.
#ifndef TSDF_AMD_MESH_RENDERER_HPP
#define TSDF_AMD_MESH_RENDERER_HPP

#include <cstdint>
#include <vector>

#include "vector_types.h"

struct tsdf_mesh;    // indexed-mesh handle (include/tsdf_amd.h)
struct tsdf_render;  // renderer handle (include/tsdf_amd.h)

class MeshRenderer {
public:
    // which maps a render fills
    enum Target : uint32_t { TRIANGLE = 1, Z = 2, DEPTH = 4, VERTICES = 8, NORMALS = 16, RGB = 32, ALL_BUT_RGB = 31, ALL = 63 };

    // The requested maps in pixel order y * width + x (the others stay empty) and the counts of tsdf_render_info.  A miss is
    // 0xFFFFFFFF / NaN / 0 / a NaN triple / a NaN triple / (0, 0, 0).
    struct Maps {
        uint32_t width, height;
        std::vector<uint32_t> triangle;
        std::vector<float> z;
        std::vector<uint16_t> depth;
        std::vector<float3> vertices, normals;
        std::vector<uchar3> rgb;
        uint64_t n_triangles, n_live, n_dropped, n_large, n_pixels_hit;
    };

    MeshRenderer();    // throws std::invalid_argument / exits like every device failure when the handle cannot be made
    ~MeshRenderer();
    MeshRenderer(const MeshRenderer &) = delete;
    MeshRenderer &operator=(const MeshRenderer &) = delete;

    // A mesh handle seen through inv_pose[16] and k[9] (column-major, what Camera::inverse_pose().data() and Camera::k().data() give):
    // triangles with every corner in [z_near, z_far] are drawn; flags: TSDF_RENDER_CULL_BACK.  Blocking.  Throws std::invalid_argument
    // on the refusals (a non-standard k, z_near <= 0, an RGB target for a mesh without colours, an index that is not below the vertex count, ...).
    Maps render(tsdf_mesh *mesh, uint32_t width, uint32_t height, const float inv_pose[16], const float k[9], float z_near, float z_far,
                uint32_t flags = 0, uint32_t targets = DEPTH);
    // The same of host arrays: triangles wired as the class surface hands them out, (I[3t], I[3t+2], I[3t+1]); normals and colours per
    // vertex, or null.
    Maps render(const std::vector<float3> &vertices, const std::vector<int3> &triangles, const std::vector<float3> *normals,
                const std::vector<uchar3> *colours, uint32_t width, uint32_t height, const float inv_pose[16], const float k[9], float z_near,
                float z_far, uint32_t flags = 0, uint32_t targets = DEPTH);

    uint64_t scratch_bytes() const;
    tsdf_render *handle() const { return m_handle; }

private:
    tsdf_render *m_handle;
};

#endif
