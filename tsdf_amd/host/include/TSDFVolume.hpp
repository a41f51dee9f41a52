// Dense TSDF voxel grid resident in GPU memory (MI355X): same public surface as the reference's
// TSDFVolume (src/include/TSDFVolume.hpp:21-304) so callers such as src/Tools/kinfu.cpp compile
// unchanged.  All device work goes through the C ABI of include/tsdf_amd.h.
#ifndef TSDF_AMD_HOST_TSDF_VOLUME_INCLUDED
#define TSDF_AMD_HOST_TSDF_VOLUME_INCLUDED

#include "Camera.hpp"

#include <Eigen/Core>
#include "vector_types.h"

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

struct tsdf_volume;  // C-ABI handle (include/tsdf_amd.h)
struct tsdf_esdf;    // distance-field handle (include/tsdf_amd.h)
struct tsdf_mesh;    // indexed-mesh handle (include/tsdf_amd.h)
struct tsdf_snapshot;  // sparse-snapshot handle (include/tsdf_amd.h)
struct tsdf_explorer;  // exploration handle (include/tsdf_amd.h)
struct tsdf_frontier_cluster;  // a row of its cluster table (include/tsdf_amd.h)
struct tsdf_reach;          // reachability handle (include/tsdf_amd.h)
struct tsdf_reach_info;     // what it reports of its last computation (include/tsdf_amd.h)
struct tsdf_reach_cluster;  // a row of its ranking of frontier clusters (include/tsdf_amd.h)
struct tsdf_columns;        // column map handle (include/tsdf_amd.h)
struct tsdf_columns_info;   // what it reports of its last projection and classification (include/tsdf_amd.h)
struct tsdf_column;         // a row of the map (include/tsdf_amd.h)
struct tsdf_objects;       // class-objects handle (include/tsdf_amd.h)
struct tsdf_class_object;  // a row of its table (include/tsdf_amd.h)

class TSDFVolume {
public:
    // 24-byte deformation node: where the voxel centre sits, and a rotation (unused by the path)
    struct DeformationNode {
        float3 translation;
        float3 rotation;
    };

    // float triple, implicitly convertible from/to float3
    struct Float3 {
        float x, y, z;
        inline Float3(const float3 &v) : x(v.x), y(v.y), z(v.z) {}
        inline Float3(float fx = 0.0f, float fy = 0.0f, float fz = 0.0f) : x(fx), y(fy), z(fz) {}
        inline operator float3() const { return float3{x, y, z}; }
        inline Float3 operator-(const Float3 &o) const { return float3{x - o.x, y - o.y, z - o.z}; }
        inline Float3 operator+(const Float3 &o) const { return float3{x + o.x, y + o.y, z + o.z}; }
        inline Float3 operator/(const float s) const { return float3{x / s, y / s, z / s}; }
        inline Float3 operator*(const Float3 &o) const { return float3{x * o.x, y * o.y, z * o.z}; }
        inline float norm() const { return std::sqrt(x * x + y * y + z * z); }
    };

    struct Int3 {
        int16_t x, y, z;
    };

    // unsigned triple, implicitly convertible from/to dim3
    struct UInt3 {
        unsigned int x, y, z;
        inline UInt3(const dim3 &d) : x{d.x}, y{d.y}, z{d.z} {}
        inline UInt3(uint32_t vx, uint32_t vy, uint32_t vz) : x{vx}, y{vy}, z{vz} {}
        inline operator dim3() const { return dim3{x, y, z}; }
    };

    ~TSDFVolume();

    // size in voxels, physical size in mm; throws std::invalid_argument on zero / negative sizes
    TSDFVolume(const UInt3 &size = UInt3{64, 64, 64}, const Float3 &physical_size = Float3{3000.0f, 3000.0f, 3000.0f});
    TSDFVolume(uint16_t volume_x, uint16_t volume_y, uint16_t volume_z, float psize_x, float psize_y, float psize_z);
    // load a volume written by save_to_file; throws std::invalid_argument on failure
    TSDFVolume(const std::string &file_name);

    // drop the contents, re-allocate and clear; the offset is kept
    void set_size(uint16_t volume_x, uint16_t volume_y, uint16_t volume_z, float psize_x, float psize_y, float psize_z);

    inline UInt3 size() const { return (UInt3)m_size; }
    inline Float3 voxel_size() const { return (Float3)m_voxel_size; }
    inline Float3 physical_size() const { return (Float3)m_physical_size; }
    inline float truncation_distance() const { return m_truncation_distance; }

    // world position of the corner of voxel (0,0,0); setting it does not move the deformation grid
    void offset(float ox, float oy, float oz);
    inline Float3 offset() const { return (Float3)m_offset; }

    // weights <- 0, distances <- truncation distance, deformation grid <- regular voxel centres
    void clear();

    inline size_t index(int x, int y, int z) const { return x + (y * m_size.x) + (z * m_size.x * m_size.y); }

    // Per-voxel arrays: DEVICE pointers (x fastest), blocking whole-array uploads from host memory
    DeformationNode *deformation() const;
    void set_deformation(DeformationNode *deformation);
    const float *distance_data() const;
    void set_distance_data(const float *distance_data);
    const float *weight_data() const;
    void set_weight_data(const float *weight_data);

    inline float3 global_rotation() const { return m_global_rotation; }
    inline float3 global_translation() const { return m_global_translation; }

    // apply the deformation field to mesh points in place (host memory)
    void deform_mesh(const int num_points, float3 *points) const;

    // fuse one depth frame (uint16 mm, 0 = invalid) seen from `camera`
    void integrate(const uint16_t *depth_map, uint32_t width, uint32_t height, const Camera &camera);

    // Colour fusion (include/tsdf_amd.h, "colour fusion"; not in the reference's class): one {r, g, b, n} dword per voxel while
    // enabled.  enable_colour(true) allocates it zeroed (throws std::invalid_argument on a Z-slab), false frees it.
    void enable_colour(bool enabled);
    bool colour_enabled() const;
    // DEVICE pointer to the colour dwords (x fastest); throws std::invalid_argument while colour is off
    const uint32_t *colour_data() const;
    // integrate() plus the colour of `rgb` (8-bit interleaved RGB, width * height * 3, registered to the depth map); needs colour on
    void integrate(const uint16_t *depth_map, const uint8_t *rgb, uint32_t width, uint32_t height, const Camera &camera);

    // Class fusion (include/tsdf_amd.h, "class fusion"; not in the reference's class): one {class, votes} dword per voxel while enabled.
    // enable_classes(true) allocates it zeroed (throws std::invalid_argument on a Z-slab), false frees it.
    void enable_classes(bool enabled);
    bool classes_enabled() const;
    // integrate() plus the vote of `classes` (width * height class ids registered to the depth map, TSDF_CLASS_VOID = none) with the
    // strength `confidence` (width * height bytes; nullptr: 1 everywhere); `rgb` (or nullptr) as in the coloured integrate().  Throws
    // std::invalid_argument while classes are off, on null classes and on rgb without colour.
    void integrate_classes(const uint16_t *depth_map, const uint16_t *classes, uint32_t width, uint32_t height, const Camera &camera,
                           const uint8_t *confidence = nullptr, const uint8_t *rgb = nullptr);
    // classes[i] / votes[i] (votes may be null): the class of the voxel points[i] (world, mm) lies in and its votes; (TSDF_CLASS_VOID, 0)
    // for NaN, off-grid and unclassified voxels
    void sample_classes(const std::vector<float3> &points, std::vector<uint16_t> &classes, std::vector<uint16_t> *votes = nullptr) const;
    // counts[k], k < n_classes (1..65535): the voxels whose class is k with at least max(min_votes, 1) votes
    std::vector<uint64_t> class_counts(uint32_t n_classes, uint32_t min_votes = 1) const;

    // De-integration (include/tsdf_amd.h, "de-integration"; not in the reference's class): takes the frame of an earlier integrate() --
    // the same depth map at the same camera -- back out.  Throws std::invalid_argument on a volume with a weight cap.
    void deintegrate(const uint16_t *depth_map, uint32_t width, uint32_t height, const Camera &camera);

    // Weighted integration (include/tsdf_amd.h, "weighted integration"; what the reference's current_weight was for): integrate() with
    // one fp32 weight per pixel (width * height); a pixel whose weight is not finite and > 0 counts as a pixel without depth.  `rgb` (or
    // nullptr) as in the coloured integrate().  The volume goes to fp32 weights.  Throws std::invalid_argument on null weights.
    void integrate_weighted(const uint16_t *depth_map, const float *weights, uint32_t width, uint32_t height, const Camera &camera,
                            const uint8_t *rgb = nullptr);
    // The standard weight models of a depth frame (tsdf_depth_weights): `flags` a combination of TSDF_WEIGHTS_INVERSE_SQUARE and
    // TSDF_WEIGHTS_COSINE, z_ref in depth units; the result has width * height entries, 0 where the depth is 0.  Throws
    // std::invalid_argument on unknown flags and on a z_ref that is not finite and > 0 with the inverse-square flag.
    static std::vector<float> depth_weights(const uint16_t *depth_map, uint32_t width, uint32_t height, const Camera &camera, uint32_t flags,
                                            float z_ref = 0.0f);

    // Weight cap (include/tsdf_amd.h, "weight cap"; what the reference's m_max_weight was for): integrate stores min(weight + 1, cap),
    // the blend's divisor stays weight + 1.  0 = off (the default), 1 .. 65535; throws std::invalid_argument above that.
    void weight_cap(uint32_t cap);
    uint32_t weight_cap() const;

    // Field queries (include/tsdf_amd.h, "field queries"; not in the reference's class): the trilinear distance the ray cast samples, its
    // central-difference gradient (unit_gradient: normalised; it points out of the surface) and the weight of the voxel each world
    // point (mm, in the frame of ray-cast and mesh vertices: the current offset) lies in.  Any of the three outputs may be null; each
    // one given is resized to points.size().  Outside the grid: NaN, the NaN triple, 0.  Throws std::invalid_argument on a Z-slab and
    // when all three are null.
    void sample_field(const std::vector<float3> &points, std::vector<float> *distances, std::vector<float3> *gradients,
                      std::vector<float> *weights, bool unit_gradient = false) const;

    // Ray queries (include/tsdf_amd.h, "ray queries"; not in the reference's class): where each ray (origin and direction in world mm,
    // the frame of ray-cast and mesh vertices; the direction is used as given) first meets the surface, marched as the image cast
    // marches a pixel's ray.  points[i] is the hit point, (*t)[i] its ray parameter in units of the direction, (*normals)[i] the unit
    // gradient of the field there; NaN on a miss.  With t_max a hit counts only if t <= (*t_max)[i].  Throws std::invalid_argument on
    // a Z-slab and when origins, directions and t_max differ in length.
    void cast_rays(const std::vector<float3> &origins, const std::vector<float3> &directions, std::vector<float3> &points,
                   std::vector<float> *t = nullptr, std::vector<float3> *normals = nullptr, const std::vector<float> *t_max = nullptr) const;
    // the same with colours[i] = the {r, g, b} of the voxel hit i lies in, (0, 0, 0) on a miss; also throws std::invalid_argument
    // while colour is off
    void cast_rays(const std::vector<float3> &origins, const std::vector<float3> &directions, std::vector<float3> &points,
                   std::vector<uchar3> &colours, std::vector<float> *t = nullptr, std::vector<float3> *normals = nullptr,
                   const std::vector<float> *t_max = nullptr) const;

    // Volume fusion (include/tsdf_amd.h, "volume fusion"; not in the reference's class): resamples the field of `src` onto this volume's
    // grid through the rigid transform dst_to_src (this volume's world frame -> src's) and blends it in, weights added; returns the
    // number of voxels updated.  Grids, voxel sizes, offsets and truncation distances may differ; src is not changed.  Throws
    // std::invalid_argument on the refusals (src == this, a Z-slab or materialised deformation nodes on either side, a non-finite
    // matrix entry).
    uint64_t fuse(const TSDFVolume &src, const Eigen::Matrix4f &dst_to_src);

    // Ray integration (include/tsdf_amd.h, "ray integration"; not in the reference's class): fuses a LiDAR scan or a point cloud --
    // ray i runs from its origin (origins holds one sensor position for all, or one per point) to points[i], world mm in the frame of
    // ray-cast and mesh vertices.  Every voxel the rays cross takes the mean of their observations as one observation (weight + 1);
    // band_only: only within the truncation distance of each point.  Rays shorter than min_range or longer than max_range are left
    // out.  Returns the number of voxels updated.  Throws std::invalid_argument on the refusals (origins neither one nor one per
    // point, more than 2^23 points, a Z-slab, materialised deformation nodes).
    uint64_t integrate_rays(const std::vector<float3> &origins, const std::vector<float3> &points, bool band_only = false,
                            float min_range = 0.0f, float max_range = INFINITY);
    // the same with rgb[i] the colour of points[i]: the voxels within the truncation distance of a point also take the mean colour of
    // their rays as one colour observation (rules 9 - 12).  Also throws std::invalid_argument while colour is off and when rgb and
    // points differ in length.
    uint64_t integrate_rays(const std::vector<float3> &origins, const std::vector<float3> &points, const std::vector<uchar3> &rgb,
                            bool band_only = false, float min_range = 0.0f, float max_range = INFINITY);
    // frees the scratch integrate_rays keeps between calls (8 bytes per voxel, 16 more once colours were fused)
    void release_ray_scratch();
    // the bytes of that scratch held right now
    uint64_t ray_scratch_bytes() const;

    // Field alignment (include/tsdf_amd.h, "field alignment"; not in the reference's class): the rigid pose that puts `points` on this
    // volume's surface -- `iterations` Gauss-Newton steps on the squared field distance from T0 (points' frame -> the frame of ray-cast
    // and mesh vertices), points further than `gate` (<= 0: the truncation distance) from the surface left out.  residual / inliers
    // (may be null): the sum of squared distances and the inlier count of the last step; 0 inliers means the chain ended blind.
    // Throws std::invalid_argument on the refusals (a Z-slab, a non-finite entry in T0's top three rows).
    Eigen::Matrix4d align_points(const std::vector<float3> &points, const Eigen::Matrix4d &T0, uint32_t iterations = 10, float gate = 0.0f,
                                 float *residual = nullptr, float *inliers = nullptr) const;
    // Colour alignment (include/tsdf_amd.h, "colour alignment"): align_points with a photometric row per point beside the geometric one --
    // intensity[i] is the observed intensity Y = (77 r + 150 g + 29 b) / 256 of points[i] (NaN: none), compared with the intensity of
    // the fused colours where the point lands; differences of colour_gate and more are left out, colour_weight (volume units squared per
    // intensity squared; scene-dependent) scales the colour term's sums.  residual / inliers (may be null): two floats each, the
    // geometric and the colour term's.  Also throws std::invalid_argument while colour is off, when intensity and points differ in
    // length, when colour_gate is not > 0 and when colour_weight is negative or not finite.
    Eigen::Matrix4d align_points(const std::vector<float3> &points, const std::vector<float> &intensity, const Eigen::Matrix4d &T0,
                                 float colour_gate, float colour_weight, uint32_t iterations = 10, float gate = 0.0f,
                                 float *residual = nullptr, float *inliers = nullptr) const;
    // The intensity of the fused colours at world points (the frame of ray-cast and mesh vertices) and, when `gradient` is given, the
    // exact derivative of that trilinear interpolant; NaN outside the grid and where one of the eight voxels has no colour.  Throws
    // std::invalid_argument while colour is off.
    std::vector<float> sample_intensity(const std::vector<float3> &points, std::vector<float3> *gradient = nullptr) const;

    // Distance field (include/tsdf_amd.h, "distance field"; not in the reference's class): per voxel the Euclidean distance (mm) to the
    // nearest site -- an observed voxel with an observed 6-neighbour of the other sign -- negative behind the surface, capped at
    // max_distance (INFINITY: no cap), NaN where unobserved (fill_unknown: the positive distance); index order x + y X + z X Y.
    // Throws std::invalid_argument on the refusals (a Z-slab, materialised deformation nodes, max_distance not > 0, an axis > 4096).
    std::vector<float> compute_esdf(float max_distance, bool fill_unknown = false) const;
    // the same into a caller's handle (tsdf_esdf_create), where it stays on the device: tsdf_esdf_buffer, tsdf_esdf_sample_device
    void compute_esdf(float max_distance, bool fill_unknown, tsdf_esdf *esdf) const;

    // Exploration (include/tsdf_amd.h, "exploration"; not in the reference's class): the free voxels with an unobserved face neighbour
    // (frontiers), their clusters, and the mask of unobserved voxels that view-gain rays have passed, in a handle that keeps its device
    // arrays between calls.
    class Explorer {
    public:
        Explorer();    // throws std::invalid_argument / exits like every device failure when the handle cannot be made
        ~Explorer();
        Explorer(const Explorer &) = delete;
        Explorer &operator=(const Explorer &) = delete;
        inline tsdf_explorer *handle() const { return m_handle; }
        // the whole-grid counts of the last find_frontiers
        uint64_t n_unknown() const;
        uint64_t n_free() const;
        uint64_t n_occupied() const;
        uint64_t n_frontiers() const;
        // the ids (z * Y + y) * X + x of the frontier voxels, ascending; a blocking download
        std::vector<uint32_t> voxels() const;
        // Label the connected sets of frontier voxels, connectivity 6 or 26; the table lists those of at least min_size voxels.
        // Returns the number of clusters (of any size).  Throws std::invalid_argument on another connectivity or before find_frontiers.
        uint64_t cluster(uint32_t connectivity = 26, uint32_t min_size = 1);
        // per listed voxel the smallest list index of its cluster / the table's rows in ascending label (tsdf_frontier_cluster,
        // include/tsdf_amd.h); blocking downloads
        std::vector<uint32_t> labels() const;
        std::vector<tsdf_frontier_cluster> clusters() const;

    private:
        tsdf_explorer *m_handle;
    };
    // The frontiers of this volume into `into` (nothing of the volume is written).  Throws std::invalid_argument on the refusals (a
    // Z-slab, materialised deformation nodes).
    void find_frontiers(Explorer &into) const;
    // View gain: every ray (world mm, the direction used as given, t_max in units of it or null for no limit) is walked voxel by voxel
    // until it leaves the grid or passes t_max (stop 1) or meets an occupied voxel (stop 2; 0: the ray was skipped); unknown / free count
    // the voxels it passed in either state.  Returns the number of distinct unobserved voxels marked in `explorer` after the call; `keep`
    // adds to the marks of earlier calls.  The three outputs may be null.  Throws std::invalid_argument on the refusals (arrays of
    // different lengths, an explorer that holds another volume's geometry).
    uint64_t view_gain(Explorer &explorer, const std::vector<float3> &origins, const std::vector<float3> &directions,
                       const std::vector<float> *t_max = nullptr, bool keep = false, std::vector<uint32_t> *unknown = nullptr,
                       std::vector<uint32_t> *free_voxels = nullptr, std::vector<uint8_t> *stop = nullptr) const;

    // Reachability (include/tsdf_amd.h, "reachability"; not in the reference's class): the travel cost from seed points through free
    // voxels to every voxel, the voxel paths back to the seeds and the nearest voxel of every frontier cluster, in a handle that keeps
    // its device arrays between calls and needs no volume once computed.
    class Reach {
    public:
        Reach();    // throws std::invalid_argument / exits like every device failure when the handle cannot be made
        ~Reach();
        Reach(const Reach &) = delete;
        Reach &operator=(const Reach &) = delete;
        inline tsdf_reach *handle() const { return m_handle; }
        // tsdf_reach_info of the last computation (rounds is a diagnostic, not a unique value)
        tsdf_reach_info info() const;
        // the cost per voxel id (z * Y + y) * X + x, TSDF_REACH_UNREACHED where there is none; a blocking download
        std::vector<uint32_t> costs() const;
        // the cost of the voxel each world point lies in, TSDF_REACH_UNREACHED off the grid
        std::vector<uint32_t> lookup(const std::vector<float3> &points) const;
        // The voxel path of each goal back to a seed, goal first, at most max_len ids a path (0: every path whole); `lengths` (may be
        // null) takes the lengths of the whole paths.  A goal off the grid or not reached has an empty path.
        std::vector<std::vector<uint32_t>> paths(const std::vector<float3> &goals, uint32_t max_len = 0, std::vector<uint32_t> *lengths = nullptr) const;
        // one row per row of explorer.clusters(): the smallest (cost, voxel id) among the cluster's voxels.  Throws std::invalid_argument
        // for an explorer that is not clustered or holds another geometry.
        std::vector<tsdf_reach_cluster> rank(const Explorer &explorer);

    private:
        tsdf_reach *m_handle;
    };
    // The cost field of this volume from `seeds` (world mm) into `into` (nothing of the volume is written): connectivity 6 or 26, esdf
    // (may be null) and clearance as TRAVERSABLE takes them, max_cost 0 for no cap, flags TSDF_REACH_THROUGH_UNKNOWN or 0.  Returns when
    // the field is final.  Throws std::invalid_argument on the refusals.
    void reach(const std::vector<float3> &seeds, uint32_t connectivity, const tsdf_esdf *esdf, float clearance, uint32_t max_cost,
               uint32_t flags, Reach &into) const;

    // Column maps (include/tsdf_amd.h, "column maps"; not in the reference's class): every column of voxels along one axis reduced to one
    // row of a 2-D map over the two other axes, and a 2.5-D traversability class per cell, in a handle that keeps its device arrays
    // between calls and needs no volume once projected.
    class ColumnMap {
    public:
        ColumnMap();    // throws std::invalid_argument / exits like every device failure when the handle cannot be made
        ~ColumnMap();
        ColumnMap(const ColumnMap &) = delete;
        ColumnMap &operator=(const ColumnMap &) = delete;
        inline tsdf_columns *handle() const { return m_handle; }
        // tsdf_columns_info of the last projection and classification; waits for the handle's pending work
        tsdf_columns_info info() const;
        // the rows in cell order, cell (u, v) at v * map_size[0] + u (tsdf_column, include/tsdf_amd.h); a blocking download
        std::vector<tsdf_column> columns() const;
        // one class per cell (TSDF_CELL_NO_GROUND / _TRAVERSABLE / _BLOCKED) in cell order.  Throws std::invalid_argument before any
        // projection.
        std::vector<uint8_t> classify(uint32_t max_step, uint32_t min_headroom);
        // rule 4's world coordinate of a row's height on the map's axis, in fp32 (NaN where the cell has no ground)
        float height_world(const tsdf_column &row) const;

    private:
        tsdf_columns *m_handle;
    };
    // The map of this volume's columns along `axis` over the band [lo, hi) (hi 0: the axis' end) into `into` (nothing of the volume is
    // written); reversed: "up" is towards smaller indices; esdf (may be null): the handle whose values min_distance is the minimum of.
    // Does not wait.  Throws std::invalid_argument on the refusals (an axis above 2, an empty band or one that leaves the axis, a
    // Z-slab, materialised deformation nodes, an ESDF never computed or of another geometry).
    void column_map(ColumnMap &into, uint32_t axis = 2, uint32_t lo = 0, uint32_t hi = 0, bool reversed = false, const tsdf_esdf *esdf = nullptr) const;

    // Class objects (include/tsdf_amd.h, "class objects"; not in the reference's class): the connected pieces of each fused class and
    // their table, in a handle that keeps its device arrays between calls.
    class Objects {
    public:
        Objects();    // throws std::invalid_argument / exits like every device failure when the handle cannot be made
        ~Objects();
        Objects(const Objects &) = delete;
        Objects &operator=(const Objects &) = delete;
        inline tsdf_objects *handle() const { return m_handle; }
        // the labelled voxels and the objects (of any size) of the last find_objects
        uint64_t n_labelled() const;
        uint64_t n_objects() const;
        // the ids (z * Y + y) * X + x of the labelled voxels, ascending / per listed voxel the smallest list index of its object / the
        // table's rows in ascending label (tsdf_class_object, include/tsdf_amd.h); blocking downloads
        std::vector<uint32_t> voxels() const;
        std::vector<uint32_t> labels() const;
        std::vector<tsdf_class_object> objects() const;
        // per point (world mm, the frame of sample_classes) the row in objects() of the object whose voxel it lies in, or
        // TSDF_OBJECT_NONE; blocking.  Throws std::invalid_argument before any find_objects.
        std::vector<uint32_t> lookup(const std::vector<float3> &points) const;

    private:
        tsdf_objects *m_handle;
    };
    // The objects of this volume into `into` (nothing of the volume is written): voxels with at least max(min_votes, 1) votes and, when
    // `select` is given, select[class] != 0 (classes beyond its end are left out); neighbours at `connectivity` (6 or 26) of the same
    // class are joined; the table lists the objects of at least min_size voxels.  Throws std::invalid_argument on the refusals
    // (classes not enabled, another connectivity, more than 65535 selection bytes).
    void find_objects(Objects &into, uint32_t min_votes = 1, const std::vector<uint8_t> *select = nullptr, uint32_t connectivity = 26,
                      uint32_t min_size = 1) const;

    // Scene flow (include/tsdf_amd.h, "scene flow"; the device part of the reference's process_frames, SceneFusion_krnl.hpp): the
    // vertices of `mesh` -- a handle holding tsdf_volume_extract_mesh of this volume's whole grid -- that the depth frame sees take the
    // scene flow (width * height float3, row major, world units) at their pixel, and it is added, weighted, to the translations of the
    // deformation nodes of the voxels that bracket them.  threshold: how far (mm, along z) the depth's point may lie from the vertex;
    // deformed: the vertices are pushed through the current deformation before they are projected (the later frames of a sequence).
    // Returns the number of nodes written; correspondences (may be null) receives the number of vertices that found a pixel.  Throws
    // std::invalid_argument on the refusals (a mesh that is not the whole grid's, a threshold not > 0, a non-finite matrix entry).
    uint64_t apply_scene_flow(tsdf_mesh *mesh, const uint16_t *depth_map, const float3 *scene_flow, uint32_t width, uint32_t height,
                              const Camera &camera, float threshold = 10.0f, bool deformed = false, uint64_t *correspondences = nullptr);

    bool save_to_file(const std::string &file_name) const;
    bool load_from_file(const std::string &file_name);

    // Sparse snapshots (include/tsdf_amd.h, "sparse snapshot"; not in the reference's class): the bricks of 8^3 voxels that hold anything
    // but what clear() leaves, as compact device arrays in a handle that keeps them and its scratch between calls.
    class Snapshot {
    public:
        Snapshot();    // throws std::invalid_argument / exits like every device failure when the handle cannot be made
        ~Snapshot();
        Snapshot(const Snapshot &) = delete;
        Snapshot &operator=(const Snapshot &) = delete;
        inline tsdf_snapshot *handle() const { return m_handle; }
        uint64_t n_bricks() const;
        uint64_t bytes() const;          // of the four device arrays
        uint32_t weight_bits() const;    // 8, 16 or 32: the element type of the weights
        bool has_colour() const;
        // blocking download: n_bricks ids, 512 n_bricks distances, weights (weight_bits / 8 bytes each) and, with colour, colour words
        void download(std::vector<uint32_t> &bricks, std::vector<float> &distances, std::vector<unsigned char> &weights,
                      std::vector<uint32_t> &colours) const;
        // `into` becomes the snapshot of the bricks with coordinates inside the box [lo, hi), or with TSDF_SELECT_OUTSIDE outside it
        // (tsdf_snapshot_select); throws std::invalid_argument when into is this snapshot or this one was never filled
        void select(const int32_t lo[3], const int32_t hi[3], uint32_t flags, Snapshot &into) const;

    private:
        tsdf_snapshot *m_handle;
    };
    // Take the live bricks into `into` (nothing of the volume is written) / put the state of `from` back, bit for bit; the header
    // fields, the offset, the weight cap and the stream are not touched.  Both throw std::invalid_argument on the refusals (a Z-slab,
    // materialised deformation nodes, a snapshot of a grid of another size, a handle that was never filled).
    void snapshot(Snapshot &into) const;
    void restore(const Snapshot &from);
    // Rolling volume (include/tsdf_amd.h, "rolling volume"): brick b takes brick b - shift of `from`, whose grid may be of another size;
    // flags: 0 or TSDF_RESTORE_KEEP_OTHERS (tsdf_volume_restore_shifted) ...
    void restore(const Snapshot &from, const int32_t shift[3], uint32_t flags);
    // ... and the box moved by box_shift bricks in the world, the content staying where it is: through `work`, the bricks that fall out
    // into `leaving` if given (tsdf_volume_shift).  Both throw std::invalid_argument on the refusals (those above; for shift also
    // leaving == &work, a grid that is no multiple of 8 on every axis, classes enabled).
    void shift(const int32_t box_shift[3], Snapshot &work, Snapshot *leaving);
    // The volume's live bricks and header as a .tsdfs file; false with a message when the volume cannot be saved so
    // (materialised deformation nodes are not stored) or the file cannot be written.
    bool save_sparse(const std::string &file_name) const;
    // the same for a volume held as a C-ABI handle (tools/kinfu_stream.cpp)
    static bool save_sparse(const tsdf_volume *handle, const std::string &file_name);
    // The state and header of a .tsdfs file of this volume's grid size; false with a message when the file does not validate (the
    // checks touch no device) or is of another size.  The volume is unchanged then.
    bool load_sparse(const std::string &file_name);

    // ray cast the zero crossing from `camera`: 3 x (width*height) vertices and normals
    void raycast(uint16_t width, uint16_t height, const Camera &camera,
                 Eigen::Matrix<float, 3, Eigen::Dynamic> &vertices,
                 Eigen::Matrix<float, 3, Eigen::Dynamic> &normals) const;

    // C-ABI handle, for the other classes of this library
    inline tsdf_volume *handle() const { return m_handle; }

private:
    void deallocate();
    void refresh_from_handle();

    tsdf_volume *m_handle;

    // host mirror of the handle's geometry (kept so the accessors above stay inline)
    dim3 m_size;
    float3 m_physical_size;
    float3 m_offset;
    float3 m_voxel_size;
    float m_truncation_distance;
    float m_max_weight;
    float3 m_global_translation;
    float3 m_global_rotation;
};
#endif /* TSDF_AMD_HOST_TSDF_VOLUME_INCLUDED */
