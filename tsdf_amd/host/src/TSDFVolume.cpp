// TSDFVolume class surface over the C ABI.  Behaviour follows the host side of the reference's
// src/TSDF/TSDFVolume.cu (cited per method); the device work itself is in tsdf_amd/csrc.
#include "TSDFVolume.hpp"

#include <cassert>
#include <algorithm>
#include <cmath>
#include <fstream>
#include <stdexcept>

#include "GPURaycaster.hpp"
#include "host_common.hpp"
#include "SparseFile.hpp"

using tsdf_host::check;

namespace {
const char *kBadSize = "Attempt to construct TSDFVolume with zero or negative size";
}

// reference: src/TSDF/TSDFVolume.cu:396-423
TSDFVolume::~TSDFVolume() {
    if (tsdf_host::verbose()) std::cout << "Destroying TSDFVolume" << std::endl;
    deallocate();
}

void TSDFVolume::deallocate() {
    if (m_handle) {
        tsdf_volume_destroy(m_handle);
        m_handle = nullptr;
    }
}

// reference: src/TSDF/TSDFVolume.cu:430-437.  set_size takes uint16_t, so 32-bit sizes narrow.
TSDFVolume::TSDFVolume(const UInt3 &size, const Float3 &physical_size) : m_handle{nullptr}, m_offset{0.0f, 0.0f, 0.0f} {
    if (size.x > 0 && size.y > 0 && size.z > 0 && physical_size.x > 0 && physical_size.y > 0 && physical_size.z > 0) {
        set_size(size.x, size.y, size.z, physical_size.x, physical_size.y, physical_size.z);
    } else {
        throw std::invalid_argument(kBadSize);
    }
}

// reference: src/TSDF/TSDFVolume.cu:449-457
TSDFVolume::TSDFVolume(uint16_t volume_x, uint16_t volume_y, uint16_t volume_z, float psize_x, float psize_y,
                       float psize_z)
    : m_handle{nullptr}, m_offset{0.0f, 0.0f, 0.0f} {
    if (volume_x > 0 && volume_y > 0 && volume_z > 0 && psize_x > 0 && psize_y > 0 && psize_z > 0) {
        set_size(volume_x, volume_y, volume_z, psize_x, psize_y, psize_z);
    } else {
        throw std::invalid_argument("Attempt to construct CPUTSDFVolume with zero or negative size");
    }
}

void TSDFVolume::refresh_from_handle() {
    tsdf_volume_info i;
    check(tsdf_volume_get_info(m_handle, &i), "Couldn't query TSDF");
    m_size = dim3{i.size[0], i.size[1], i.size[2]};
    m_physical_size = float3{i.physical_size[0], i.physical_size[1], i.physical_size[2]};
    m_voxel_size = float3{i.voxel_size[0], i.voxel_size[1], i.voxel_size[2]};
    m_offset = float3{i.offset[0], i.offset[1], i.offset[2]};
    m_truncation_distance = i.truncation_distance;
    m_max_weight = i.max_weight;
    m_global_translation = float3{i.global_translation[0], i.global_translation[1], i.global_translation[2]};
    m_global_rotation = float3{i.global_rotation[0], i.global_rotation[1], i.global_rotation[2]};
}

// reference: src/TSDF/TSDFVolume.cu:679-722 (offset is maintained across a resize)
void TSDFVolume::set_size(uint16_t volume_x, uint16_t volume_y, uint16_t volume_z, float psize_x, float psize_y,
                          float psize_z) {
    if ((volume_x != 0 && volume_y != 0 && volume_z != 0) && (psize_x != 0 && psize_y != 0 && psize_z != 0)) {
        float3 keep = m_offset;
        deallocate();
        check(tsdf_volume_create(volume_x, volume_y, volume_z, psize_x, psize_y, psize_z, &m_handle),
              "Couldn't allocate space for TSDF");
        if (keep.x != 0.0f || keep.y != 0.0f || keep.z != 0.0f) {
            // the reference clears with m_offset already in place, so the grid carries it
            check(tsdf_volume_set_offset(m_handle, keep.x, keep.y, keep.z), "Couldn't set offset");
            check(tsdf_volume_clear(m_handle), "Couldn't clear TSDF");
            check(tsdf_volume_synchronize(m_handle), "Couldn't clear TSDF");
        }
        refresh_from_handle();
    } else {
        throw std::invalid_argument("Attempt to set TSDF size or physical size to zero");
    }
}

// reference: src/include/TSDFVolume.hpp:139-143
void TSDFVolume::offset(float ox, float oy, float oz) {
    m_offset = float3{ox, oy, oz};
    check(tsdf_volume_set_offset(m_handle, ox, oy, oz), "Couldn't set offset");
}

// reference: src/TSDF/TSDFVolume.cu:812-845
void TSDFVolume::clear() {
    check(tsdf_volume_clear(m_handle), "Couldn't clear TSDF");
    check(tsdf_volume_synchronize(m_handle), "Couldn't clear TSDF");
}

// ---- data access (reference: src/include/TSDFVolume.hpp:175-203, src/TSDF/TSDFVolume.cu:731-757)
TSDFVolume::DeformationNode *TSDFVolume::deformation() const {
    tsdf_deformation_node *p = nullptr;
    check(tsdf_volume_deformation(m_handle, &p), "Couldn't allocate space for deformation nodes for TSDF");
    return reinterpret_cast<DeformationNode *>(p);
}

void TSDFVolume::set_deformation(DeformationNode *deformation) {
    static_assert(sizeof(DeformationNode) == sizeof(tsdf_deformation_node), "DeformationNode must be 24 bytes");
    check(tsdf_volume_set_deformation(m_handle, reinterpret_cast<const tsdf_deformation_node *>(deformation)),
          "Couldn't set deformation");
}

const float *TSDFVolume::distance_data() const {
    float *p = nullptr;
    check(tsdf_volume_distances(m_handle, &p), "Couldn't get distance data");
    return p;
}

void TSDFVolume::set_distance_data(const float *distance_data) {
    check(tsdf_volume_set_distance_data(m_handle, distance_data), "Couldn't set distance data");
}

const float *TSDFVolume::weight_data() const {
    float *p = nullptr;
    check(tsdf_volume_weights(m_handle, &p), "Couldn't get weight data");
    return p;
}

void TSDFVolume::set_weight_data(const float *weight_data) {
    check(tsdf_volume_set_weight_data(m_handle, weight_data), "Couldn't set weight data");
}

// reference: src/TSDF/TSDFVolume.cu:861-902
void TSDFVolume::integrate(const uint16_t *depth_map, uint32_t width, uint32_t height, const Camera &camera) {
    assert(depth_map);
    if (tsdf_host::verbose()) std::cout << "Integrating depth map size " << width << "x" << height << std::endl;
    // Eigen is column-major: .data() is already the Mat44 / Mat33 image the C ABI expects (:867-877)
    const Eigen::Matrix3f k = camera.k(), kinv = camera.kinv();
    check(tsdf_integrate(m_handle, depth_map, width, height, camera.pose().data(), camera.inverse_pose().data(),
                         k.data(), kinv.data()),
          "Integrate kernel failed");
    if (tsdf_host::verbose()) std::cout << "Integration finished" << std::endl;
}

// ---- weight cap (what the reference's m_max_weight was for)
void TSDFVolume::deintegrate(const uint16_t *depth_map, uint32_t width, uint32_t height, const Camera &camera) {
    assert(depth_map);
    const Eigen::Matrix3f k = camera.k(), kinv = camera.kinv();
    check(tsdf_deintegrate(m_handle, depth_map, width, height, camera.pose().data(), camera.inverse_pose().data(), k.data(), kinv.data()),
          "De-integrate kernel failed");
}

void TSDFVolume::sample_field(const std::vector<float3> &points, std::vector<float> *distances, std::vector<float3> *gradients,
                              std::vector<float> *weights, bool unit_gradient) const {
    static_assert(sizeof(float3) == 3 * sizeof(float), "float3 must be 3 packed floats");
    if (!distances && !gradients && !weights) throw std::invalid_argument("sample_field: no output asked for");
    const size_t n = points.size();
    // (one element more than needed: data() of an empty vector may be null, which the C ABI reads as "not asked for")
    if (distances) distances->assign(n + 1, 0.0f);
    if (gradients) gradients->assign(n + 1, float3{0.0f, 0.0f, 0.0f});
    if (weights) weights->assign(n + 1, 0.0f);
    check(tsdf_volume_sample_field(m_handle, n, reinterpret_cast<const float *>(points.data()), distances ? distances->data() : nullptr,
                                   gradients ? reinterpret_cast<float *>(gradients->data()) : nullptr,
                                   weights ? weights->data() : nullptr, unit_gradient ? TSDF_FIELD_UNIT_GRADIENT : 0),
          "Couldn't sample the field");
    if (distances) distances->resize(n);
    if (gradients) gradients->resize(n);
    if (weights) weights->resize(n);
}

void TSDFVolume::compute_esdf(float max_distance, bool fill_unknown, tsdf_esdf *esdf) const {
    check(tsdf_volume_compute_esdf(m_handle, max_distance, fill_unknown ? TSDF_ESDF_FILL_UNKNOWN : 0u, esdf), "Couldn't compute the distance field");
}

std::vector<float> TSDFVolume::compute_esdf(float max_distance, bool fill_unknown) const {
    tsdf_esdf *esdf = nullptr;
    check(tsdf_esdf_create(&esdf), "Couldn't compute the distance field");
    int rc = tsdf_volume_compute_esdf(m_handle, max_distance, fill_unknown ? TSDF_ESDF_FILL_UNKNOWN : 0u, esdf);
    tsdf_esdf_info info;
    if (rc == TSDF_OK) rc = tsdf_esdf_get_info(esdf, &info);
    std::vector<float> distances;
    if (rc == TSDF_OK) {
        // (one element more than needed: data() of an empty vector may be null)
        distances.assign((size_t)info.size[0] * info.size[1] * info.size[2] + 1, 0.0f);
        rc = tsdf_esdf_download(esdf, distances.data());
        distances.pop_back();
    }
    tsdf_esdf_destroy(esdf);
    check(rc, "Couldn't compute the distance field");
    return distances;
}

TSDFVolume::Explorer::Explorer() : m_handle{nullptr} { check(tsdf_explorer_create(&m_handle), "Couldn't create the explorer handle"); }

TSDFVolume::Explorer::~Explorer() { tsdf_explorer_destroy(m_handle); }

namespace {

tsdf_explorer_info explorer_info(const tsdf_explorer *e) {
    tsdf_explorer_info info;
    check(tsdf_explorer_get_info(e, &info), "Couldn't query the explorer");
    return info;
}

}  // namespace

uint64_t TSDFVolume::Explorer::n_unknown() const { return explorer_info(m_handle).n_unknown; }
uint64_t TSDFVolume::Explorer::n_free() const { return explorer_info(m_handle).n_free; }
uint64_t TSDFVolume::Explorer::n_occupied() const { return explorer_info(m_handle).n_occupied; }
uint64_t TSDFVolume::Explorer::n_frontiers() const { return explorer_info(m_handle).n_frontiers; }

std::vector<uint32_t> TSDFVolume::Explorer::voxels() const {
    // (one element more than needed: data() of an empty vector may be null)
    std::vector<uint32_t> ids((size_t)explorer_info(m_handle).n_frontiers + 1, 0u);
    check(tsdf_explorer_frontier_download(m_handle, ids.data()), "Couldn't download the frontiers");
    ids.pop_back();
    return ids;
}

uint64_t TSDFVolume::Explorer::cluster(uint32_t connectivity, uint32_t min_size) {
    check(tsdf_explorer_cluster_frontiers(m_handle, connectivity, min_size, nullptr), "Couldn't cluster the frontiers");
    return explorer_info(m_handle).n_clusters;
}

std::vector<uint32_t> TSDFVolume::Explorer::labels() const {
    std::vector<uint32_t> labels((size_t)explorer_info(m_handle).n_frontiers + 1, 0u);
    check(tsdf_explorer_cluster_download(m_handle, labels.data(), nullptr), "Couldn't download the frontier labels");
    labels.pop_back();
    return labels;
}

std::vector<tsdf_frontier_cluster> TSDFVolume::Explorer::clusters() const {
    std::vector<tsdf_frontier_cluster> rows((size_t)explorer_info(m_handle).n_listed_clusters + 1, tsdf_frontier_cluster());
    check(tsdf_explorer_cluster_download(m_handle, nullptr, rows.data()), "Couldn't download the frontier clusters");
    rows.pop_back();
    return rows;
}

void TSDFVolume::find_frontiers(Explorer &into) const { check(tsdf_volume_find_frontiers(m_handle, 0u, into.handle()), "Couldn't find the frontiers"); }

uint64_t TSDFVolume::view_gain(Explorer &explorer, const std::vector<float3> &origins, const std::vector<float3> &directions,
                               const std::vector<float> *t_max, bool keep, std::vector<uint32_t> *unknown, std::vector<uint32_t> *free_voxels,
                               std::vector<uint8_t> *stop) const {
    static_assert(sizeof(float3) == 3 * sizeof(float), "float3 must be 3 packed floats");
    const size_t n = origins.size();
    if (directions.size() != n) throw std::invalid_argument("view_gain: origins and directions differ in length");
    if (t_max && t_max->size() != n) throw std::invalid_argument("view_gain: t_max and the rays differ in length");
    // (one element more than needed: data() of an empty vector may be null, which the C ABI reads as "not asked for")
    if (unknown) unknown->assign(n + 1, 0u);
    if (free_voxels) free_voxels->assign(n + 1, 0u);
    if (stop) stop->assign(n + 1, (uint8_t)0);
    uint64_t gain = 0;
    check(tsdf_volume_view_gain(m_handle, explorer.handle(), n, reinterpret_cast<const float *>(origins.data()),
                                reinterpret_cast<const float *>(directions.data()), (t_max && n) ? t_max->data() : nullptr,
                                keep ? TSDF_GAIN_KEEP_MASK : 0u, unknown ? unknown->data() : nullptr, free_voxels ? free_voxels->data() : nullptr,
                                stop ? stop->data() : nullptr, &gain),
          "Couldn't compute the view gain");
    if (unknown) unknown->resize(n);
    if (free_voxels) free_voxels->resize(n);
    if (stop) stop->resize(n);
    return gain;
}

TSDFVolume::Reach::Reach() : m_handle{nullptr} { check(tsdf_reach_create(&m_handle), "Couldn't create the reach handle"); }

TSDFVolume::Reach::~Reach() { tsdf_reach_destroy(m_handle); }

tsdf_reach_info TSDFVolume::Reach::info() const {
    tsdf_reach_info info;
    check(tsdf_reach_get_info(m_handle, &info), "Couldn't query the reach handle");
    return info;
}

std::vector<uint32_t> TSDFVolume::Reach::costs() const {
    const tsdf_reach_info i = info();
    // (one element more than needed: data() of an empty vector may be null)
    std::vector<uint32_t> out((size_t)i.size[0] * i.size[1] * i.size[2] + 1, 0u);
    check(tsdf_reach_download(m_handle, out.data()), "Couldn't download the costs");
    out.pop_back();
    return out;
}

std::vector<uint32_t> TSDFVolume::Reach::lookup(const std::vector<float3> &points) const {
    static_assert(sizeof(float3) == 3 * sizeof(float), "float3 must be 3 packed floats");
    const size_t n = points.size();
    std::vector<uint32_t> out(n + 1, 0u);
    check(tsdf_reach_lookup(m_handle, n, reinterpret_cast<const float *>(points.data()), out.data()), "Couldn't look the costs up");
    out.resize(n);
    return out;
}

std::vector<std::vector<uint32_t>> TSDFVolume::Reach::paths(const std::vector<float3> &goals, uint32_t max_len, std::vector<uint32_t> *lengths) const {
    const size_t n = goals.size();
    std::vector<uint32_t> len(n + 1, 0u), rows;
    uint32_t row = max_len ? max_len : 1u;
    for (;;) {   // at most twice: rows of one first when every path is wanted whole, then rows as long as the longest
        rows.assign(n * row + 1, TSDF_REACH_UNREACHED);
        check(tsdf_reach_paths(m_handle, n, reinterpret_cast<const float *>(goals.data()), row, len.data(), rows.data()), "Couldn't walk the paths");
        uint32_t longest = 0;
        for (size_t i = 0; i < n; i++) longest = std::max(longest, len[i]);
        if (max_len || longest <= row) break;
        row = longest;
    }
    std::vector<std::vector<uint32_t>> out(n);
    for (size_t i = 0; i < n; i++) out[i].assign(rows.begin() + i * row, rows.begin() + i * row + std::min(len[i], row));
    if (lengths) lengths->assign(len.begin(), len.begin() + n);
    return out;
}

std::vector<tsdf_reach_cluster> TSDFVolume::Reach::rank(const Explorer &explorer) {
    tsdf_explorer_info ei;
    check(tsdf_explorer_get_info(explorer.handle(), &ei), "Couldn't query the explorer");
    std::vector<tsdf_reach_cluster> rows((size_t)ei.n_listed_clusters + 1, tsdf_reach_cluster());
    check(tsdf_reach_rank_frontiers(m_handle, explorer.handle(), rows.data()), "Couldn't rank the frontier clusters");
    rows.pop_back();
    return rows;
}

void TSDFVolume::reach(const std::vector<float3> &seeds, uint32_t connectivity, const tsdf_esdf *esdf, float clearance, uint32_t max_cost,
                       uint32_t flags, Reach &into) const {
    check(tsdf_volume_compute_reach(m_handle, seeds.size(), reinterpret_cast<const float *>(seeds.data()), connectivity, esdf, clearance, max_cost,
                                    flags, into.handle()),
          "Couldn't compute the reach");
}

TSDFVolume::ColumnMap::ColumnMap() : m_handle{nullptr} { check(tsdf_columns_create(&m_handle), "Couldn't create the columns handle"); }

TSDFVolume::ColumnMap::~ColumnMap() { tsdf_columns_destroy(m_handle); }

tsdf_columns_info TSDFVolume::ColumnMap::info() const {
    tsdf_columns_info info;
    check(tsdf_columns_get_info(m_handle, &info), "Couldn't query the columns handle");
    return info;
}

std::vector<tsdf_column> TSDFVolume::ColumnMap::columns() const {
    const tsdf_columns_info i = info();
    // (one element more than needed: data() of an empty vector may be null)
    std::vector<tsdf_column> rows((size_t)i.map_size[0] * i.map_size[1] + 1, tsdf_column());
    check(tsdf_columns_download(m_handle, rows.data()), "Couldn't download the columns");
    rows.pop_back();
    return rows;
}

std::vector<uint8_t> TSDFVolume::ColumnMap::classify(uint32_t max_step, uint32_t min_headroom) {
    const tsdf_columns_info i = info();
    std::vector<uint8_t> cells((size_t)i.map_size[0] * i.map_size[1] + 1, (uint8_t)0);
    check(tsdf_columns_classify(m_handle, max_step, min_headroom, 0u, cells.data()), "Couldn't classify the columns");
    cells.pop_back();
    return cells;
}

float TSDFVolume::ColumnMap::height_world(const tsdf_column &row) const {
    const tsdf_columns_info i = info();
    const float along = (i.flags & TSDF_COLUMNS_REVERSED) ? (float)i.hi - row.height : (float)i.lo + row.height;
    const float scaled = along * i.voxel_size[i.axis];
    return i.offset[i.axis] + scaled;
}

void TSDFVolume::column_map(ColumnMap &into, uint32_t axis, uint32_t lo, uint32_t hi, bool reversed, const tsdf_esdf *esdf) const {
    check(tsdf_volume_project_columns(m_handle, axis, lo, hi, esdf, reversed ? TSDF_COLUMNS_REVERSED : 0u, into.handle()),
          "Couldn't project the columns");
}

TSDFVolume::Objects::Objects() : m_handle{nullptr} { check(tsdf_objects_create(&m_handle), "Couldn't create the objects handle"); }

TSDFVolume::Objects::~Objects() { tsdf_objects_destroy(m_handle); }

namespace {

tsdf_objects_info objects_info(const tsdf_objects *o) {
    tsdf_objects_info info;
    check(tsdf_objects_get_info(o, &info), "Couldn't query the objects");
    return info;
}

}  // namespace

uint64_t TSDFVolume::Objects::n_labelled() const { return objects_info(m_handle).n_labelled; }
uint64_t TSDFVolume::Objects::n_objects() const { return objects_info(m_handle).n_objects; }

std::vector<uint32_t> TSDFVolume::Objects::voxels() const {
    // (one element more than needed: data() of an empty vector may be null, which the C ABI reads as "not asked for")
    std::vector<uint32_t> ids((size_t)objects_info(m_handle).n_labelled + 1, 0u);
    check(tsdf_objects_download(m_handle, ids.data(), nullptr, nullptr), "Couldn't download the labelled voxels");
    ids.pop_back();
    return ids;
}

std::vector<uint32_t> TSDFVolume::Objects::labels() const {
    std::vector<uint32_t> labels((size_t)objects_info(m_handle).n_labelled + 1, 0u);
    check(tsdf_objects_download(m_handle, nullptr, labels.data(), nullptr), "Couldn't download the object labels");
    labels.pop_back();
    return labels;
}

std::vector<tsdf_class_object> TSDFVolume::Objects::objects() const {
    std::vector<tsdf_class_object> rows((size_t)objects_info(m_handle).n_listed_objects + 1, tsdf_class_object());
    check(tsdf_objects_download(m_handle, nullptr, nullptr, rows.data()), "Couldn't download the objects");
    rows.pop_back();
    return rows;
}

std::vector<uint32_t> TSDFVolume::Objects::lookup(const std::vector<float3> &points) const {
    static_assert(sizeof(float3) == 3 * sizeof(float), "float3 must be 3 packed floats");
    const size_t n = points.size();
    std::vector<uint32_t> rows(n + 1, TSDF_OBJECT_NONE);
    check(tsdf_objects_lookup(m_handle, n, n ? reinterpret_cast<const float *>(points.data()) : nullptr, rows.data()), "Couldn't look the points up");
    rows.pop_back();
    return rows;
}

void TSDFVolume::find_objects(Objects &into, uint32_t min_votes, const std::vector<uint8_t> *select, uint32_t connectivity, uint32_t min_size) const {
    // (an empty selection admits nothing: one zero byte, so that the pointer is not null)
    static const uint8_t none = 0;
    const uint8_t *bytes = !select ? nullptr : select->empty() ? &none : select->data();
    const size_t n_select = !select ? 0 : select->empty() ? 1 : select->size();
    if (n_select > 65535) throw std::invalid_argument("find_objects: more than 65535 selection bytes");
    check(tsdf_volume_find_objects(m_handle, min_votes, bytes, (uint32_t)n_select, connectivity, min_size, 0u, into.handle()), "Couldn't find the objects");
}

void TSDFVolume::cast_rays(const std::vector<float3> &origins, const std::vector<float3> &directions, std::vector<float3> &points,
                           std::vector<float> *t, std::vector<float3> *normals, const std::vector<float> *t_max) const {
    static_assert(sizeof(float3) == 3 * sizeof(float), "float3 must be 3 packed floats");
    const size_t n = origins.size();
    if (directions.size() != n) throw std::invalid_argument("cast_rays: origins and directions differ in length");
    if (t_max && t_max->size() != n) throw std::invalid_argument("cast_rays: t_max and the rays differ in length");
    // (one element more than needed: data() of an empty vector may be null, which the C ABI reads as "not asked for")
    points.assign(n + 1, float3{0.0f, 0.0f, 0.0f});
    if (t) t->assign(n + 1, 0.0f);
    if (normals) normals->assign(n + 1, float3{0.0f, 0.0f, 0.0f});
    check(tsdf_volume_cast_rays(m_handle, n, reinterpret_cast<const float *>(origins.data()), reinterpret_cast<const float *>(directions.data()),
                                (t_max && n) ? t_max->data() : nullptr, reinterpret_cast<float *>(points.data()), t ? t->data() : nullptr,
                                normals ? reinterpret_cast<float *>(normals->data()) : nullptr),
          "Couldn't cast the rays");
    points.resize(n);
    if (t) t->resize(n);
    if (normals) normals->resize(n);
}

void TSDFVolume::cast_rays(const std::vector<float3> &origins, const std::vector<float3> &directions, std::vector<float3> &points,
                           std::vector<uchar3> &colours, std::vector<float> *t, std::vector<float3> *normals,
                           const std::vector<float> *t_max) const {
    static_assert(sizeof(uchar3) == 3, "uchar3 must be 3 packed bytes");
    const size_t n = origins.size();
    if (directions.size() != n) throw std::invalid_argument("cast_rays: origins and directions differ in length");
    if (t_max && t_max->size() != n) throw std::invalid_argument("cast_rays: t_max and the rays differ in length");
    // (one element more than needed: data() of an empty vector may be null, which the C ABI refuses or reads as "not asked for")
    points.assign(n + 1, float3{0.0f, 0.0f, 0.0f});
    colours.assign(n + 1, uchar3{0, 0, 0});
    if (t) t->assign(n + 1, 0.0f);
    if (normals) normals->assign(n + 1, float3{0.0f, 0.0f, 0.0f});
    check(tsdf_volume_cast_rays_colour(m_handle, n, reinterpret_cast<const float *>(origins.data()),
                                       reinterpret_cast<const float *>(directions.data()), (t_max && n) ? t_max->data() : nullptr,
                                       reinterpret_cast<float *>(points.data()), t ? t->data() : nullptr,
                                       normals ? reinterpret_cast<float *>(normals->data()) : nullptr,
                                       reinterpret_cast<uint8_t *>(colours.data())),
          "Couldn't cast the rays");
    points.resize(n);
    colours.resize(n);
    if (t) t->resize(n);
    if (normals) normals->resize(n);
}

Eigen::Matrix4d TSDFVolume::align_points(const std::vector<float3> &points, const Eigen::Matrix4d &T0, uint32_t iterations, float gate,
                                         float *residual, float *inliers) const {
    static_assert(sizeof(float3) == 3 * sizeof(float), "float3 must be 3 packed floats");
    if (points.size() > 0xFFFFFFFFull) throw std::invalid_argument("align_points: too many points");
    tsdf_volume_info info;
    check(tsdf_volume_get_info(m_handle, &info), "Couldn't read the volume's geometry");
    // one object owns the aligner and the device copy of the points, whatever is thrown
    struct Scratch {
        tsdf_aligner *aligner = nullptr;
        void *points = nullptr;
        ~Scratch() {
            if (aligner) tsdf_aligner_destroy(aligner);
            if (points) tsdf_device_free(points);
        }
    } s;
    check(tsdf_aligner_create(&s.aligner), "Couldn't create the aligner");
    void *stream = nullptr;
    check(tsdf_volume_stream(m_handle, &stream), "Couldn't read the volume's stream");
    check(tsdf_aligner_set_stream(s.aligner, stream), "Couldn't set the aligner's stream");
    const size_t bytes = points.size() * sizeof(float3);
    if (bytes) {
        check(tsdf_device_alloc(bytes, &s.points), "Couldn't allocate the points");
        check(tsdf_device_upload(s.points, points.data(), bytes), "Couldn't upload the points");
    }
    Eigen::Matrix4d T = T0;
    const tsdf_align_stage stage = {static_cast<const float *>(s.points), (uint32_t)points.size(), iterations};
    check(tsdf_aligner_run(s.aligner, m_handle, 1, &stage, gate <= 0.0f ? info.truncation_distance : gate, T.data(), residual, inliers),
          "Align kernels failed");
    return T;
}

Eigen::Matrix4d TSDFVolume::align_points(const std::vector<float3> &points, const std::vector<float> &intensity, const Eigen::Matrix4d &T0,
                                         float colour_gate, float colour_weight, uint32_t iterations, float gate, float *residual,
                                         float *inliers) const {
    if (points.size() > 0xFFFFFFFFull) throw std::invalid_argument("align_points: too many points");
    if (intensity.size() != points.size()) throw std::invalid_argument("align_points: points and intensities differ in length");
    tsdf_volume_info info;
    check(tsdf_volume_get_info(m_handle, &info), "Couldn't read the volume's geometry");
    struct Scratch {
        tsdf_aligner *aligner = nullptr;
        void *points = nullptr, *intensity = nullptr;
        ~Scratch() {
            if (aligner) tsdf_aligner_destroy(aligner);
            if (points) tsdf_device_free(points);
            if (intensity) tsdf_device_free(intensity);
        }
    } s;
    check(tsdf_aligner_create(&s.aligner), "Couldn't create the aligner");
    void *stream = nullptr;
    check(tsdf_volume_stream(m_handle, &stream), "Couldn't read the volume's stream");
    check(tsdf_aligner_set_stream(s.aligner, stream), "Couldn't set the aligner's stream");
    if (!points.empty()) {
        check(tsdf_device_alloc(points.size() * sizeof(float3), &s.points), "Couldn't allocate the points");
        check(tsdf_device_upload(s.points, points.data(), points.size() * sizeof(float3)), "Couldn't upload the points");
        check(tsdf_device_alloc(intensity.size() * sizeof(float), &s.intensity), "Couldn't allocate the intensities");
        check(tsdf_device_upload(s.intensity, intensity.data(), intensity.size() * sizeof(float)), "Couldn't upload the intensities");
    }
    Eigen::Matrix4d T = T0;
    const tsdf_align_colour_stage stage = {static_cast<const float *>(s.points), static_cast<const float *>(s.intensity),
                                           (uint32_t)points.size(), iterations};
    check(tsdf_aligner_run_colour(s.aligner, m_handle, 1, &stage, gate <= 0.0f ? info.truncation_distance : gate, colour_gate, colour_weight,
                                  T.data(), residual, inliers),
          "Align kernels failed");
    return T;
}

std::vector<float> TSDFVolume::sample_intensity(const std::vector<float3> &points, std::vector<float3> *gradient) const {
    static_assert(sizeof(float3) == 3 * sizeof(float), "float3 must be 3 packed floats");
    const size_t n = points.size();
    // (one element more than needed: data() of an empty vector may be null, which the C ABI reads as "not asked for")
    std::vector<float> intensity(n + 1, 0.0f);
    if (gradient) gradient->assign(n + 1, float3{0.0f, 0.0f, 0.0f});
    check(tsdf_volume_sample_intensity(m_handle, n, reinterpret_cast<const float *>(points.data()), intensity.data(),
                                       gradient ? reinterpret_cast<float *>(gradient->data()) : nullptr),
          "Couldn't sample the intensity");
    intensity.resize(n);
    if (gradient) gradient->resize(n);
    return intensity;
}

uint64_t TSDFVolume::fuse(const TSDFVolume &src, const Eigen::Matrix4f &dst_to_src) {
    uint64_t fused = 0;
    check(tsdf_volume_fuse(m_handle, src.m_handle, dst_to_src.data(), &fused), "Fuse kernel failed");
    return fused;
}

uint64_t TSDFVolume::integrate_rays(const std::vector<float3> &origins, const std::vector<float3> &points, bool band_only, float min_range,
                                    float max_range) {
    static_assert(sizeof(float3) == 3 * sizeof(float), "float3 must be 3 packed floats");
    uint64_t updated = 0;
    check(tsdf_integrate_rays(m_handle, points.size(), reinterpret_cast<const float *>(origins.data()), origins.size(),
                              reinterpret_cast<const float *>(points.data()), min_range, max_range, band_only ? TSDF_RAYS_BAND_ONLY : 0, &updated),
          "Ray integration failed");
    return updated;
}

uint64_t TSDFVolume::integrate_rays(const std::vector<float3> &origins, const std::vector<float3> &points, const std::vector<uchar3> &rgb,
                                    bool band_only, float min_range, float max_range) {
    static_assert(sizeof(uchar3) == 3, "uchar3 must be 3 packed bytes");
    if (rgb.size() != points.size()) throw std::invalid_argument("integrate_rays: points and rgb differ in length");
    uint64_t updated = 0;
    check(tsdf_integrate_rays_colour(m_handle, points.size(), reinterpret_cast<const float *>(origins.data()), origins.size(),
                                     reinterpret_cast<const float *>(points.data()), reinterpret_cast<const uint8_t *>(rgb.data()), min_range,
                                     max_range, band_only ? TSDF_RAYS_BAND_ONLY : 0, &updated),
          "Ray integration failed");
    return updated;
}

uint64_t TSDFVolume::ray_scratch_bytes() const {
    uint64_t bytes = 0;
    check(tsdf_volume_ray_scratch_bytes(m_handle, &bytes), "Couldn't query the ray scratch");
    return bytes;
}

void TSDFVolume::release_ray_scratch() { check(tsdf_volume_release_ray_scratch(m_handle), "Couldn't release the ray scratch"); }

void TSDFVolume::weight_cap(uint32_t cap) { check(tsdf_volume_set_weight_cap(m_handle, cap), "Couldn't set the weight cap"); }

uint32_t TSDFVolume::weight_cap() const {
    uint32_t cap = 0;
    check(tsdf_volume_weight_cap(m_handle, &cap), "Couldn't query the weight cap");
    return cap;
}

// ---- colour fusion (no reference counterpart)
void TSDFVolume::enable_colour(bool enabled) {
    check(tsdf_volume_enable_colour(m_handle, enabled ? 1 : 0), "Couldn't enable colour");
    check(tsdf_volume_synchronize(m_handle), "Couldn't enable colour");
}

bool TSDFVolume::colour_enabled() const {
    int enabled = 0;
    check(tsdf_volume_colour_enabled(m_handle, &enabled), "Couldn't query colour");
    return enabled != 0;
}

const uint32_t *TSDFVolume::colour_data() const {
    uint32_t *p = nullptr;
    check(tsdf_volume_colours(m_handle, &p), "Couldn't get colour data");
    return p;
}

void TSDFVolume::integrate(const uint16_t *depth_map, const uint8_t *rgb, uint32_t width, uint32_t height, const Camera &camera) {
    assert(depth_map && rgb);
    const Eigen::Matrix3f k = camera.k(), kinv = camera.kinv();
    check(tsdf_integrate_colour(m_handle, depth_map, rgb, width, height, camera.pose().data(), camera.inverse_pose().data(), k.data(),
                                kinv.data()),
          "Integrate kernel failed");
}

// ---- class fusion (no reference counterpart)
void TSDFVolume::enable_classes(bool enabled) {
    check(tsdf_volume_enable_classes(m_handle, enabled ? 1 : 0), "Couldn't enable classes");
    check(tsdf_volume_synchronize(m_handle), "Couldn't enable classes");
}

bool TSDFVolume::classes_enabled() const {
    int enabled = 0;
    check(tsdf_volume_classes_enabled(m_handle, &enabled), "Couldn't query classes");
    return enabled != 0;
}

void TSDFVolume::integrate_classes(const uint16_t *depth_map, const uint16_t *classes, uint32_t width, uint32_t height, const Camera &camera,
                                   const uint8_t *confidence, const uint8_t *rgb) {
    const Eigen::Matrix3f k = camera.k(), kinv = camera.kinv();
    check(tsdf_integrate_classes(m_handle, depth_map, rgb, classes, confidence, width, height, camera.pose().data(),
                                 camera.inverse_pose().data(), k.data(), kinv.data()),
          "Class integrate failed");
}

void TSDFVolume::sample_classes(const std::vector<float3> &points, std::vector<uint16_t> &classes, std::vector<uint16_t> *votes) const {
    const size_t n = points.size(), in_bytes = n * 3 * sizeof(float), out_bytes = n * sizeof(uint16_t);
    classes.assign(n, (uint16_t)TSDF_CLASS_VOID);
    if (votes) votes->assign(n, 0);
    void *d_buf = nullptr, *stream = nullptr;
    check(tsdf_volume_stream(m_handle, &stream), "Class sample failed");
    // (n == 0 still goes through the entry point: it refuses a volume without classes)
    check(tsdf_device_alloc(in_bytes + 2 * out_bytes + 4, &d_buf), "Class sample alloc failed");
    float *d_points = static_cast<float *>(d_buf);
    uint16_t *d_classes = reinterpret_cast<uint16_t *>(d_points + 3 * n), *d_votes = d_classes + n;
    int rc = n ? tsdf_device_upload(d_points, points.data(), in_bytes) : TSDF_OK;
    if (rc == TSDF_OK) rc = tsdf_volume_sample_classes_device(m_handle, n, d_points, d_classes, d_votes, stream);
    const int rs = tsdf_stream_synchronize(stream);   // (before the buffer goes, whatever happened)
    if (rc == TSDF_OK) rc = rs;
    if (rc == TSDF_OK && n) rc = tsdf_device_download(classes.data(), d_classes, out_bytes);
    if (rc == TSDF_OK && n && votes) rc = tsdf_device_download(votes->data(), d_votes, out_bytes);
    (void)tsdf_device_free(d_buf);
    check(rc, "Class sample failed");
}

std::vector<uint64_t> TSDFVolume::class_counts(uint32_t n_classes, uint32_t min_votes) const {
    std::vector<uint64_t> counts(n_classes ? n_classes : 1);
    check(tsdf_volume_class_counts(m_handle, n_classes, min_votes, counts.data()), "Class counts failed");
    return counts;
}

void TSDFVolume::integrate_weighted(const uint16_t *depth_map, const float *weights, uint32_t width, uint32_t height, const Camera &camera,
                                    const uint8_t *rgb) {
    assert(depth_map);
    const Eigen::Matrix3f k = camera.k(), kinv = camera.kinv();
    check(tsdf_integrate_weighted(m_handle, depth_map, weights, rgb, width, height, camera.pose().data(), camera.inverse_pose().data(), k.data(),
                                  kinv.data()),
          "Weighted integrate failed");
}

std::vector<float> TSDFVolume::depth_weights(const uint16_t *depth_map, uint32_t width, uint32_t height, const Camera &camera, uint32_t flags,
                                             float z_ref) {
    std::vector<float> weights((size_t)width * height);
    const Eigen::Matrix3f kinv = camera.kinv();
    check(tsdf_depth_weights(width, height, depth_map, kinv.data(), flags, z_ref, weights.data()), "Depth weights failed");
    return weights;
}

// reference: src/TSDF/TSDFVolume.cu:1054-1058
void TSDFVolume::raycast(uint16_t width, uint16_t height, const Camera &camera,
                         Eigen::Matrix<float, 3, Eigen::Dynamic> &vertices,
                         Eigen::Matrix<float, 3, Eigen::Dynamic> &normals) const {
    GPURaycaster raycaster(width, height);
    raycaster.raycast(*this, camera, vertices, normals);
}

// reference: src/TSDF/TSDFVolume.cu:265-291 (upload, deformation_kernel, download), in place like there
void TSDFVolume::deform_mesh(const int num_points, float3 *points) const {
    check(tsdf_volume_deform_points(m_handle, num_points, reinterpret_cast<float *>(points)), "Deformation kernel failed");
}

// ---- scene flow (include/tsdf_amd.h, "scene flow")
uint64_t TSDFVolume::apply_scene_flow(tsdf_mesh *mesh, const uint16_t *depth_map, const float3 *scene_flow, uint32_t width, uint32_t height,
                                      const Camera &camera, float threshold, bool deformed, uint64_t *correspondences) {
    static_assert(sizeof(float3) == 12, "packed vector types");
    const Eigen::Matrix3f k = camera.k(), kinv = camera.kinv();
    tsdf_scene_flow_info info;
    check(tsdf_volume_apply_scene_flow(m_handle, mesh, depth_map, reinterpret_cast<const float *>(scene_flow), width, height, camera.pose().data(),
                                       camera.inverse_pose().data(), k.data(), kinv.data(), threshold, deformed ? TSDF_SCENE_FLOW_DEFORMED : 0u, &info),
          "Scene flow kernels failed");
    if (correspondences) *correspondences = info.n_correspondences;
    return info.n_nodes_moved;
}

// ---- file format (reference: src/TSDF/TSDFVolume.cu:911-1027 writer, :463-664 reader):
// 68-byte header {dim3 size, float3 physical, float3 offset, float trunc, float max_weight,
// float3 global_translation, float3 global_rotation} then float dist[N], float weight[N],
// uchar3 colour[N], DeformationNode[N]; little-endian, no padding.  The colour block holds each voxel's r, g, b when colour is
// enabled, zeros otherwise (the reference writes its never-written array).
bool TSDFVolume::save_to_file(const std::string &file_name) const {
    const size_t n = (size_t)m_size.x * m_size.y * m_size.z;
    std::vector<float> dist(n), weight(n);
    if (tsdf_volume_get_distance_data(m_handle, dist.data()) != TSDF_OK) {
        std::cout << "Failed to copy voxel data from device memory [" << tsdf_last_error() << "] " << std::endl;
        return false;
    }
    if (tsdf_volume_get_weight_data(m_handle, weight.data()) != TSDF_OK) {
        std::cout << "Failed to copy weight data from device memory [" << tsdf_last_error() << "] " << std::endl;
        return false;
    }
    std::ofstream ofs{file_name, std::ios::out | std::ios::binary};
    if (!ofs.good()) return false;
    ofs.write((const char *)&m_size, sizeof(m_size));
    ofs.write((const char *)&m_physical_size, sizeof(m_physical_size));
    ofs.write((const char *)&m_offset, sizeof(m_offset));
    ofs.write((const char *)&m_truncation_distance, sizeof(m_truncation_distance));
    ofs.write((const char *)&m_max_weight, sizeof(m_max_weight));
    ofs.write((const char *)&m_global_translation, sizeof(m_global_translation));
    ofs.write((const char *)&m_global_rotation, sizeof(m_global_rotation));
    ofs.write((const char *)dist.data(), n * sizeof(float));
    ofs.write((const char *)weight.data(), n * sizeof(float));
    // colours: r, g, b of the colour dwords when colour is enabled; otherwise all zero, streamed plane by plane
    if (colour_enabled()) {
        std::vector<uint32_t> colour(n);
        if (tsdf_volume_get_colour_data(m_handle, colour.data()) != TSDF_OK) {
            std::cout << "Failed to copy colour data from device memory [" << tsdf_last_error() << "] " << std::endl;
            return false;
        }
        std::vector<unsigned char> rgb(n * 3);
        for (size_t i = 0; i < n; i++) {
            rgb[3 * i + 0] = (unsigned char)colour[i];
            rgb[3 * i + 1] = (unsigned char)(colour[i] >> 8);
            rgb[3 * i + 2] = (unsigned char)(colour[i] >> 16);
        }
        ofs.write((const char *)rgb.data(), rgb.size());
    } else {
        std::vector<unsigned char> zeros((size_t)m_size.x * m_size.y * 3, 0);
        for (unsigned z = 0; z < m_size.z; z++) ofs.write((const char *)zeros.data(), zeros.size());
    }
    // deformation nodes, as the reference writes m_deformation_nodes (src/TSDF/TSDFVolume.cu:1003-1018): the device array when
    // a caller has touched it (deformation() / set_deformation()), else the regular grid clear() would have written --
    // tsdf_volume_get_deformation_planes hands out either, plane by plane
    {
        std::vector<DeformationNode> plane((size_t)m_size.x * m_size.y);
        for (unsigned z = 0; z < m_size.z; z++) {
            if (tsdf_volume_get_deformation_planes(m_handle, z, 1, reinterpret_cast<tsdf_deformation_node *>(plane.data())) != TSDF_OK) {
                std::cout << "Failed to copy deformation data from device memory [" << tsdf_last_error() << "] " << std::endl;
                return false;
            }
            ofs.write((const char *)plane.data(), plane.size() * sizeof(DeformationNode));
        }
    }
    ofs.close();
    return ofs.good();
}

TSDFVolume::TSDFVolume(const std::string &file_name) : m_handle{nullptr}, m_offset{0.0f, 0.0f, 0.0f} {
    std::ifstream ifs{file_name, std::ios::in | std::ios::binary};
    std::string why;
    dim3 size;
    float3 phys, offset, gt, gr;
    float trunc = 0, max_weight = 0;
    if (!ifs.read((char *)&size, sizeof(size))) {
        why = "Couldn't load file data";
    } else if (!ifs.read((char *)&phys, sizeof(phys))) {
        why = "Couldn't load physical size";
    } else if (!(ifs.read((char *)&offset, sizeof(offset)) && ifs.read((char *)&trunc, sizeof(trunc)) &&
                 ifs.read((char *)&max_weight, sizeof(max_weight)) && ifs.read((char *)&gt, sizeof(gt)) &&
                 ifs.read((char *)&gr, sizeof(gr)))) {
        why = "Couldn't load header data";
    }
    if (why.empty()) {
        if (tsdf_host::verbose())
            std::cout << "Loading TSDF with size " << size.x << "x" << size.y << "x" << size.z << std::endl;
        if (tsdf_volume_create(size.x, size.y, size.z, phys.x, phys.y, phys.z, &m_handle) != TSDF_OK)
            why = std::string("Failed to allocate device memory for distance data: ") + tsdf_last_error();
    }
    if (why.empty()) {
        const float o[3] = {offset.x, offset.y, offset.z}, t[3] = {gt.x, gt.y, gt.z}, r[3] = {gr.x, gr.y, gr.z};
        tsdf_volume_set_header(m_handle, o, trunc, max_weight, t, r);
        const size_t n = (size_t)size.x * size.y * size.z;
        std::vector<float> buf(n);
        if (!ifs.read((char *)buf.data(), n * sizeof(float))) why = "Failed to read distance data";
        else if (tsdf_volume_set_distance_data(m_handle, buf.data()) != TSDF_OK) why = "Failed to copy distance data to device";
        if (why.empty()) {
            if (!ifs.read((char *)buf.data(), n * sizeof(float))) why = "Failed to read weight data";
            else if (tsdf_volume_set_weight_data(m_handle, buf.data()) != TSDF_OK) why = "Failed to copy weight data to device";
        }
        if (why.empty()) {
            // colours: a block with a nonzero byte enables colour fusion (files of volumes without colour load as before).  The
            // observation count is not in the file: n = min(max((int)weight, 1), 255) for a voxel whose colour is not (0, 0, 0),
            // n = 0 otherwise -- so a voxel observed as pure black reads back as unobserved.
            std::vector<unsigned char> rgb(n * 3);
            if (!ifs.read((char *)rgb.data(), rgb.size())) why = "Failed to read colour data";
            bool any = false;
            for (size_t i = 0; i < rgb.size() && why.empty() && !any; i++) any = rgb[i] != 0;
            if (any) {
                std::vector<uint32_t> colour(n);
                for (size_t i = 0; i < n; i++) {
                    const uint32_t c = rgb[3 * i] | ((uint32_t)rgb[3 * i + 1] << 8) | ((uint32_t)rgb[3 * i + 2] << 16);
                    const int w = (int)buf[i];   // (buf holds the weights just read)
                    colour[i] = c ? c | ((uint32_t)std::min(std::max(w, 1), 255) << 24) : 0u;
                }
                if (tsdf_volume_enable_colour(m_handle, 1) != TSDF_OK || tsdf_volume_set_colour_data(m_handle, colour.data()) != TSDF_OK)
                    why = std::string("Failed to copy colour data to device: ") + tsdf_last_error();
            }
        }
        if (why.empty()) {
            // deformation nodes: keep the grid implicit when the file holds the regular grid
            std::vector<DeformationNode> nodes(n);
            if (!ifs.read((char *)nodes.data(), n * sizeof(DeformationNode))) {
                why = "Failed to read deformation data";
            } else {
                // The reference keeps the block verbatim.  When it is the regular grid clear() wrote for some constant offset oc
                // (node = ((v + 0.5) * vs) + oc, src/TSDF/TSDFVolume.cu:783-785; oc = the offset current at that clear(), Q1)
                // the nodes stay implicit and the volume is told oc.  oc is read off node 0 and its fp32 neighbours are tried
                // too: 0.5*vs + oc was rounded, so node0 - 0.5*vs need not give oc back, while any oc that reproduces every node
                // bit for bit is as good as the original (the kernels only ever form these sums).
                const float3 vs = float3{phys.x / (float)size.x, phys.y / (float)size.y, phys.z / (float)size.z};
                const size_t stride[3] = {1, (size_t)size.x, (size_t)size.x * size.y};
                const unsigned count[3] = {size.x, size.y, size.z};
                const float vsa[3] = {vs.x, vs.y, vs.z};
                float oc[3] = {0.0f, 0.0f, 0.0f};
                bool regular = true;
                auto component = [](const DeformationNode &nd, int axis) {
                    return axis == 0 ? nd.translation.x : axis == 1 ? nd.translation.y : nd.translation.z;
                };
                for (int axis = 0; axis < 3 && regular; axis++) {
                    const float first = component(nodes[0], axis);
                    const float centre = first - (0.5f * vsa[axis]);
                    bool found = false;
                    for (int k = 0; k < 9 && !found; k++) {          // 0, +1, -1, +2, -2, ... ulps: the nearest fit wins
                        float guess = centre;
                        for (int step = 0; step < (k + 1) / 2; step++) guess = std::nextafter(guess, (k & 1) ? INFINITY : -INFINITY);
                        bool ok = true;
                        for (unsigned i = 0; i < count[axis] && ok; i++)
                            ok = component(nodes[i * stride[axis]], axis) == (((int)i + 0.5f) * vsa[axis]) + guess;
                        if (ok) {
                            oc[axis] = guess;
                            found = true;
                        }
                    }
                    regular = found;
                }
                // the three axis sequences fit: now every node (translations that do not vary across the grid, rotations zero)
                size_t i = 0;
                for (unsigned z = 0; z < size.z && regular; z++)
                    for (unsigned y = 0; y < size.y && regular; y++)
                        for (unsigned x = 0; x < size.x; x++, i++) {
                            const DeformationNode &nd = nodes[i];
                            if (nd.translation.x != (((int)x + 0.5f) * vs.x) + oc[0] ||
                                nd.translation.y != (((int)y + 0.5f) * vs.y) + oc[1] ||
                                nd.translation.z != (((int)z + 0.5f) * vs.z) + oc[2] ||
                                nd.rotation.x != 0.0f || nd.rotation.y != 0.0f || nd.rotation.z != 0.0f) {
                                regular = false;
                                break;
                            }
                        }
                if (regular && tsdf_volume_set_offset_at_clear(m_handle, oc) != TSDF_OK) why = "Failed to restore the node offset";
                if (!regular &&
                    tsdf_volume_set_deformation(m_handle, reinterpret_cast<const tsdf_deformation_node *>(nodes.data())) != TSDF_OK)
                    why = "Failed to copy deformation data to device";
            }
        }
    }
    if (!why.empty()) {
        deallocate();
        throw std::invalid_argument("Failed to load TSDF " + file_name + " " + why);
    }
    refresh_from_handle();
}

// reference: src/TSDF/TSDFVolume.cu:1035-1047 -- a stub there too
bool TSDFVolume::load_from_file(const std::string &file_name) {
    (void)file_name;
    std::cout << "Not yet implemented: load_from_file" << std::endl;
    return false;
}

// ---- sparse snapshots (include/tsdf_amd.h, "sparse snapshot")
TSDFVolume::Snapshot::Snapshot() : m_handle{nullptr} { check(tsdf_snapshot_create(&m_handle), "Couldn't create the snapshot handle"); }

TSDFVolume::Snapshot::~Snapshot() { tsdf_snapshot_destroy(m_handle); }

namespace {
tsdf_snapshot_info snapshot_info(const tsdf_snapshot *s) {
    tsdf_snapshot_info info;
    check(tsdf_snapshot_get_info(s, &info), "Couldn't query the snapshot");
    return info;
}
}  // namespace

uint64_t TSDFVolume::Snapshot::n_bricks() const { return snapshot_info(m_handle).n_bricks; }
uint64_t TSDFVolume::Snapshot::bytes() const { return snapshot_info(m_handle).bytes; }
uint32_t TSDFVolume::Snapshot::weight_bits() const { return snapshot_info(m_handle).weight_bits; }
bool TSDFVolume::Snapshot::has_colour() const { return (snapshot_info(m_handle).flags & TSDF_SNAPSHOT_COLOUR) != 0; }

void TSDFVolume::Snapshot::download(std::vector<uint32_t> &bricks, std::vector<float> &distances, std::vector<unsigned char> &weights,
                                    std::vector<uint32_t> &colours) const {
    const tsdf_snapshot_info info = snapshot_info(m_handle);
    const size_t n = (size_t)info.n_bricks, pad = n ? 0 : 1;   // (an empty vector's pointer may be null)
    const bool colour = (info.flags & TSDF_SNAPSHOT_COLOUR) != 0;
    bricks.resize(n + pad);
    distances.resize(n * 512 + pad);
    weights.resize(n * 512 * (info.weight_bits / 8) + pad);
    colours.resize(colour ? n * 512 + pad : 0);
    check(tsdf_snapshot_download(m_handle, bricks.data(), distances.data(), weights.data(), colour ? colours.data() : nullptr),
          "Couldn't download the snapshot");
    bricks.resize(n);
    distances.resize(n * 512);
    weights.resize(n * 512 * (info.weight_bits / 8));
    if (colour) colours.resize(n * 512);
}

void TSDFVolume::snapshot(Snapshot &into) const { check(tsdf_volume_snapshot(m_handle, 0u, into.handle()), "Couldn't take the snapshot"); }

void TSDFVolume::restore(const Snapshot &from) { check(tsdf_volume_restore(m_handle, from.handle()), "Couldn't restore the snapshot"); }

// ---- rolling volume (include/tsdf_amd.h, "rolling volume")
void TSDFVolume::Snapshot::select(const int32_t lo[3], const int32_t hi[3], uint32_t flags, Snapshot &into) const {
    check(tsdf_snapshot_select(m_handle, lo, hi, flags, into.handle()), "Couldn't select from the snapshot");
}

void TSDFVolume::restore(const Snapshot &from, const int32_t shift[3], uint32_t flags) {
    check(tsdf_volume_restore_shifted(m_handle, from.handle(), shift, flags), "Couldn't restore the shifted snapshot");
}

void TSDFVolume::shift(const int32_t box_shift[3], Snapshot &work, Snapshot *leaving) {
    check(tsdf_volume_shift(m_handle, box_shift, work.handle(), leaving ? leaving->handle() : nullptr), "Couldn't shift the volume");
    refresh_from_handle();   // (the offset has moved)
}

bool TSDFVolume::save_sparse(const std::string &file_name) const { return save_sparse(m_handle, file_name); }

bool TSDFVolume::save_sparse(const tsdf_volume *handle, const std::string &file_name) {
    tsdf_volume_info vi;
    if (!handle || tsdf_volume_get_info(handle, &vi) != TSDF_OK) return false;
    if (vi.deformation_materialised) {
        std::cout << "save_sparse: the volume has a materialised deformation-node array, which a .tsdfs file does not carry" << std::endl;
        return false;
    }
    std::vector<uint32_t> ids, colours;
    std::vector<float> dist;
    std::vector<unsigned char> weights;
    tsdf_snapshot_info si;
    try {
        Snapshot snap;
        check(tsdf_volume_snapshot(handle, 0u, snap.handle()), "Couldn't take the snapshot");
        si = snapshot_info(snap.handle());
        snap.download(ids, dist, weights, colours);
    } catch (const std::invalid_argument &e) {
        std::cout << "save_sparse: " << e.what() << std::endl;
        return false;
    }
    tsdf_host::SparseFileInfo fi;
    std::memset(&fi, 0, sizeof(fi));
    for (int a = 0; a < 3; a++) {
        fi.size[a] = vi.size[a];
        fi.physical_size[a] = vi.physical_size[a];
        fi.offset[a] = vi.offset[a];
        fi.global_translation[a] = vi.global_translation[a];
        fi.global_rotation[a] = vi.global_rotation[a];
    }
    fi.truncation_distance = vi.truncation_distance;
    fi.max_weight = vi.max_weight;
    fi.brick = TSDF_SNAPSHOT_BRICK;
    fi.flags = si.flags;
    fi.weight_bits = si.weight_bits;
    fi.weight_bound = si.weight_bound;
    fi.fill_distance = si.fill_distance;
    fi.n_bricks = si.n_bricks;
    unsigned char head[tsdf_host::kSparseHeaderBytes];
    tsdf_host::pack_sparse_header(fi, head);
    std::ofstream ofs{file_name, std::ios::out | std::ios::binary};
    if (!ofs.good()) {
        std::cout << "save_sparse: couldn't open " << file_name << std::endl;
        return false;
    }
    ofs.write((const char *)head, sizeof(head));
    ofs.write((const char *)ids.data(), ids.size() * sizeof(uint32_t));
    ofs.write((const char *)dist.data(), dist.size() * sizeof(float));
    ofs.write((const char *)weights.data(), weights.size());
    ofs.write((const char *)colours.data(), colours.size() * sizeof(uint32_t));
    ofs.close();
    return ofs.good();
}

bool TSDFVolume::load_sparse(const std::string &file_name) {
    tsdf_host::SparseFileInfo fi;
    std::vector<uint32_t> ids, colours;
    std::vector<float> dist;
    std::vector<unsigned char> weights;
    const std::string why = tsdf_host::read_sparse_file(file_name, fi, &ids, &dist, &weights, &colours);
    if (!why.empty()) {
        std::cout << "load_sparse: " << file_name << ": " << why << std::endl;
        return false;
    }
    if (fi.size[0] != m_size.x || fi.size[1] != m_size.y || fi.size[2] != m_size.z) {
        std::cout << "load_sparse: " << file_name << " holds a " << fi.size[0] << "x" << fi.size[1] << "x" << fi.size[2] << " grid, the volume is "
                  << m_size.x << "x" << m_size.y << "x" << m_size.z << std::endl;
        return false;
    }
    tsdf_volume_info vi;
    if (tsdf_volume_get_info(m_handle, &vi) != TSDF_OK) return false;
    if (vi.deformation_materialised || vi.z_store_begin != 0 || vi.z_store_end != vi.size[2]) {
        std::cout << "load_sparse: not supported on a Z-slab or a volume with a materialised deformation-node array" << std::endl;
        return false;
    }
    tsdf_snapshot_info si;
    std::memset(&si, 0, sizeof(si));
    for (int a = 0; a < 3; a++) {
        si.size[a] = fi.size[a];
        si.voxel_size[a] = fi.physical_size[a] / (float)fi.size[a];
        si.offset[a] = fi.offset[a];
    }
    si.flags = fi.flags;
    si.weight_bits = fi.weight_bits;
    si.fill_distance = fi.fill_distance;
    si.n_bricks = fi.n_bricks;
    try {
        Snapshot snap;
        check(tsdf_snapshot_upload(snap.handle(), &si, ids.data(), dist.data(), weights.data(), colours.empty() ? nullptr : colours.data()),
              "Couldn't upload the snapshot");
        check(tsdf_volume_set_header(m_handle, fi.offset, fi.truncation_distance, fi.max_weight, fi.global_translation, fi.global_rotation),
              "Couldn't set the header");
        restore(snap);
        check(tsdf_volume_synchronize(m_handle), "Couldn't restore the snapshot");
    } catch (const std::invalid_argument &e) {
        std::cout << "load_sparse: " << e.what() << std::endl;
        return false;
    }
    refresh_from_handle();
    return true;
}
