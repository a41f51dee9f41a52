// MeshRenderer over the C ABI (include/tsdf_amd.h, "mesh rendering").
#include "MeshRenderer.hpp"

#include <cstring>

#include "host_common.hpp"

static_assert(sizeof(uchar3) == 3 && sizeof(float3) == 12 && sizeof(int3) == 12, "packed vector types");

namespace {

// the requested maps sized for the image, and the host pointers of those that were asked for
tsdf_render_targets sized(MeshRenderer::Maps &m, uint32_t width, uint32_t height, uint32_t targets) {
    const size_t n = (size_t)width * height;
    m = MeshRenderer::Maps();
    m.width = width;
    m.height = height;
    if (targets & MeshRenderer::TRIANGLE) m.triangle.resize(n);
    if (targets & MeshRenderer::Z) m.z.resize(n);
    if (targets & MeshRenderer::DEPTH) m.depth.resize(n);
    if (targets & MeshRenderer::VERTICES) m.vertices.resize(n);
    if (targets & MeshRenderer::NORMALS) m.normals.resize(n);
    if (targets & MeshRenderer::RGB) m.rgb.resize(n);
    // (an image without pixels is refused by the call; the pointer only says "asked for")
    static char none;
    tsdf_render_targets t;
    t.triangle = (targets & MeshRenderer::TRIANGLE) ? (n ? m.triangle.data() : (uint32_t *)&none) : nullptr;
    t.z = (targets & MeshRenderer::Z) ? (n ? m.z.data() : (float *)&none) : nullptr;
    t.depth = (targets & MeshRenderer::DEPTH) ? (n ? m.depth.data() : (uint16_t *)&none) : nullptr;
    t.vertices = (targets & MeshRenderer::VERTICES) ? (n ? (float *)m.vertices.data() : (float *)&none) : nullptr;
    t.normals = (targets & MeshRenderer::NORMALS) ? (n ? (float *)m.normals.data() : (float *)&none) : nullptr;
    t.rgb = (targets & MeshRenderer::RGB) ? (n ? (uint8_t *)m.rgb.data() : (uint8_t *)&none) : nullptr;
    return t;
}

void counted(MeshRenderer::Maps &m, const tsdf_render_info &info) {
    m.n_triangles = info.n_triangles;
    m.n_live = info.n_live;
    m.n_dropped = info.n_dropped;
    m.n_large = info.n_large;
    m.n_pixels_hit = info.n_pixels_hit;
}

// device copies that go when the call ends, however it ends
struct DeviceArrays {
    std::vector<void *> held;
    ~DeviceArrays() {
        for (void *p : held) tsdf_device_free(p);
    }
    int make(size_t bytes, const void *host, void **out) {
        *out = nullptr;
        int rc = tsdf_device_alloc(bytes ? bytes : 4, out);
        if (rc != TSDF_OK) return rc;
        held.push_back(*out);
        return host && bytes ? tsdf_device_upload(*out, host, bytes) : TSDF_OK;
    }
};

}  // namespace

MeshRenderer::MeshRenderer() : m_handle(nullptr) { tsdf_host::check(tsdf_render_create(&m_handle), "Couldn't create the mesh renderer"); }

MeshRenderer::~MeshRenderer() { tsdf_render_destroy(m_handle); }

uint64_t MeshRenderer::scratch_bytes() const {
    uint64_t bytes = 0;
    tsdf_host::check(tsdf_render_scratch_bytes(m_handle, &bytes), "Couldn't read the mesh renderer's scratch size");
    return bytes;
}

MeshRenderer::Maps MeshRenderer::render(tsdf_mesh *mesh, uint32_t width, uint32_t height, const float inv_pose[16], const float k[9], float z_near,
                                        float z_far, uint32_t flags, uint32_t targets) {
    if (targets & ~(uint32_t)ALL) throw std::invalid_argument("MeshRenderer::render: unknown targets");
    Maps m;
    const tsdf_render_targets t = sized(m, width, height, targets);
    tsdf_render_info info;
    tsdf_host::check(tsdf_mesh_render(m_handle, mesh, width, height, inv_pose, k, z_near, z_far, flags, &t, &info), "Couldn't render the mesh");
    counted(m, info);
    return m;
}

MeshRenderer::Maps MeshRenderer::render(const std::vector<float3> &vertices, const std::vector<int3> &triangles, const std::vector<float3> *normals,
                                        const std::vector<uchar3> *colours, uint32_t width, uint32_t height, const float inv_pose[16], const float k[9],
                                        float z_near, float z_far, uint32_t flags, uint32_t targets) {
    if (targets & ~(uint32_t)ALL) throw std::invalid_argument("MeshRenderer::render: unknown targets");
    if ((normals && normals->size() != vertices.size()) || (colours && colours->size() != vertices.size()))
        throw std::invalid_argument("MeshRenderer::render: normals or colours differ from the vertices in length");
    std::vector<uint32_t> indices;
    indices.reserve(triangles.size() * 3);
    for (const int3 &t : triangles) {   // back to the index buffer's order
        indices.push_back((uint32_t)t.x);
        indices.push_back((uint32_t)t.z);
        indices.push_back((uint32_t)t.y);
    }
    Maps m;
    const tsdf_render_targets host = sized(m, width, height, targets);
    const size_t n = (size_t)width * height;
    const size_t bytes[6] = {4 * n, 4 * n, 2 * n, 12 * n, 12 * n, 3 * n};
    void *const host_maps[6] = {host.triangle, host.z, host.depth, host.vertices, host.normals, host.rgb};
    DeviceArrays d;
    void *dv, *di, *dn = nullptr, *dc = nullptr, *maps[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc = d.make(vertices.size() * sizeof(float3), vertices.data(), &dv);
    if (rc == TSDF_OK) rc = d.make(indices.size() * sizeof(uint32_t), indices.data(), &di);
    if (rc == TSDF_OK && normals) rc = d.make(normals->size() * sizeof(float3), normals->data(), &dn);
    if (rc == TSDF_OK && colours) rc = d.make(colours->size() * sizeof(uchar3), colours->data(), &dc);
    for (int i = 0; i < 6 && rc == TSDF_OK; i++)
        if (host_maps[i]) rc = d.make(bytes[i], nullptr, &maps[i]);
    tsdf_render_info info;
    if (rc == TSDF_OK) {
        const tsdf_render_targets t = {(uint32_t *)maps[0], (float *)maps[1], (uint16_t *)maps[2], (float *)maps[3], (float *)maps[4], (uint8_t *)maps[5]};
        rc = tsdf_render_mesh_device(m_handle, vertices.size(), indices.size(), (const float *)dv, (const uint32_t *)di, (const float *)dn,
                                     (const uint8_t *)dc, width, height, inv_pose, k, z_near, z_far, flags, &t, &info, nullptr);
    }
    for (int i = 0; i < 6 && rc == TSDF_OK; i++)
        if (maps[i] && bytes[i]) rc = tsdf_device_download(host_maps[i], maps[i], bytes[i]);
    tsdf_host::check(rc, "Couldn't render the mesh");
    counted(m, info);
    return m;
}
