/*
 * tsdf_amd.h -- C ABI of the MI355X (gfx950) TSDF hot path: volume lifecycle, depth-map
 * integration, TSDF ray casting + normals, bilateral depth filter.
 *
 * This is the drop-in boundary.  Everything above it (the C++ classes in
 * tsdf_amd/host/include that keep the reference's TSDFVolume / GPURaycaster /
 * BilateralFilter surface, and the Python mirror used by tests and bench.py) reaches the
 * GPU only through these entry points; they take plain pointers and sizes, no C++ or
 * torch types.  Each group names the reference interface it replaces (paths relative to
 * the Scoobadood/TSDF tree).
 *
 * Conventions
 *   - Every function returns TSDF_OK or an error code; tsdf_last_error() gives the text of
 *     the last failure on the calling thread.  No exceptions cross the boundary.  (The C++
 *     surface maps TSDF_ERR_INVALID to std::invalid_argument and TSDF_ERR_DEVICE to the
 *     reference's "print and exit(-1)", src/Utilities/cuda_utilities.cu:5-11.)
 *   - Matrices are column-major float arrays, byte-for-byte what the reference memcpy's
 *     out of Eigen into Mat44/Mat33 (src/TSDF/TSDFVolume.cu:867-877,
 *     src/include/cuda_utilities.hpp:12-23): 4x4 = m[col*4+row], 3x3 = m[col*3+row].
 *   - Units are millimetres; depth is uint16 mm with 0 = invalid; pixel order y*width+x;
 *     voxel order x + y*X + z*X*Y (src/include/TSDFVolume.hpp:165-167).
 *   - "_device" variants take device pointers, enqueue on the volume's stream
 *     (tsdf_volume_set_stream) and return without synchronising.  The others take host
 *     pointers and are blocking, like the reference's methods.
 *   - Not thread-safe per object, like the reference.
 */
#ifndef TSDF_AMD_H
#define TSDF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_OK 0
#define TSDF_ERR_INVALID 1 /* bad argument                                   */
#define TSDF_ERR_DEVICE 2  /* a HIP call or kernel failed                    */
#define TSDF_ERR_NOMEM 3   /* allocation failed                              */

typedef struct tsdf_volume tsdf_volume;       /* opaque: one TSDFVolume (or one Z-slab of it) */
typedef struct tsdf_bilateral tsdf_bilateral; /* opaque: one BilateralFilter                  */
typedef struct tsdf_icp tsdf_icp;             /* opaque: one ICPOdometry                      */

/* Mirror of the reference's private state, src/include/TSDFVolume.hpp:269-303. */
typedef struct tsdf_volume_info {
    uint32_t size[3];            /* m_size: voxels of the GLOBAL grid                          */
    uint32_t z_begin, z_end;     /* planes this object owns (0..Z for a whole volume)           */
    uint32_t z_store_begin, z_store_end; /* planes resident in HBM (owned + one halo plane)     */
    float physical_size[3];      /* m_physical_size (mm)                                        */
    float voxel_size[3];         /* m_voxel_size = physical / size                              */
    float offset[3];             /* m_offset                                                    */
    float offset_at_clear[3];    /* m_offset when clear() last initialised the deformation grid */
    float truncation_distance;   /* m_truncation_distance = 1.1f * |voxel_size|                 */
    float max_weight;            /* m_max_weight = 15 (unused by integrate, as in the reference)*/
    float global_translation[3]; /* m_global_translation                                       */
    float global_rotation[3];    /* m_global_rotation                                          */
    int32_t deformation_materialised; /* 0 while the 24-B/voxel node array is still implicit    */
    int32_t fast_division_verified;   /* 1 = reciprocal division proven bit-equal to IEEE for this voxel size */
} tsdf_volume_info;

/* Layout of one deformation node, src/include/TSDFVolume.hpp:23-26 (2 x float3 = 24 bytes). */
typedef struct tsdf_deformation_node {
    float translation[3];
    float rotation[3];
} tsdf_deformation_node;

/* ---- errors / device ------------------------------------------------------------------ */
const char *tsdf_last_error(void);
int tsdf_device_count(int *count);
int tsdf_set_device(int device);
int tsdf_get_device(int *device);
/* Name of the GPU architecture the library was compiled for ("gfx950"). */
const char *tsdf_build_arch(void);

/* Device memory for callers that keep frames and maps resident in HBM (the _device entry points, tsdf_pipeline_*) without
 * including the HIP headers: hipMalloc / hipFree / blocking hipMemcpy. */
int tsdf_device_alloc(size_t bytes, void **device_ptr);
int tsdf_device_free(void *device_ptr);
int tsdf_device_upload(void *device_dst, const void *host_src, size_t bytes);
int tsdf_device_download(void *host_dst, const void *device_src, size_t bytes);
/* hipStreamSynchronize for the same callers (e.g. a tsdf_exchange_fn that stages the records through the host). */
int tsdf_stream_synchronize(void *hip_stream);

/* ---- volume lifecycle ------------------------------------------------------------------ */
/* Replaces TSDFVolume::TSDFVolume / set_size (src/TSDF/TSDFVolume.cu:430-457, 679-722):
 * validates sizes (TSDF_ERR_INVALID if any is zero/negative), computes voxel size and
 * truncation distance, allocates distances + weights in HBM and clears them.  Dimensions
 * above 65535 are rejected (the reference narrows them to uint16_t). */
int tsdf_volume_create(uint32_t size_x, uint32_t size_y, uint32_t size_z, float physical_x,
                       float physical_y, float physical_z, tsdf_volume **out);
/* One Z-slab [z_begin, z_end) of a size_x*size_y*size_z grid, for one-process-per-GPU
 * sharding (no reference equivalent).  Stores one halo plane above the slab. */
int tsdf_volume_create_slab(uint32_t size_x, uint32_t size_y, uint32_t size_z, float physical_x,
                            float physical_y, float physical_z, uint32_t z_begin, uint32_t z_end,
                            tsdf_volume **out);
/* Replaces TSDFVolume::~TSDFVolume / deallocate (src/TSDF/TSDFVolume.cu:396-423). */
int tsdf_volume_destroy(tsdf_volume *volume);
/* HIP stream (hipStream_t) used by this volume's kernels and copies; NULL = default stream. */
int tsdf_volume_set_stream(tsdf_volume *volume, void *hip_stream);
int tsdf_volume_stream(const tsdf_volume *volume, void **hip_stream);   /* the stream the volume's kernels are enqueued on now */
int tsdf_volume_synchronize(const tsdf_volume *volume);
/* Replaces TSDFVolume::clear (src/TSDF/TSDFVolume.cu:812-845): weights <- 0,
 * distances <- truncation distance, deformation grid <- voxel centres + current offset. */
int tsdf_volume_clear(tsdf_volume *volume);
/* Replaces size()/voxel_size()/physical_size()/truncation_distance()/offset()/
 * global_rotation()/global_translation() (src/include/TSDFVolume.hpp:120-153, 216-225). */
int tsdf_volume_get_info(const tsdf_volume *volume, tsdf_volume_info *info);
/* Replaces TSDFVolume::offset(ox,oy,oz) (src/include/TSDFVolume.hpp:139-143); like the
 * reference it does not re-initialise the deformation grid. */
int tsdf_volume_set_offset(tsdf_volume *volume, float ox, float oy, float oz);

/* Restores the header fields a saved volume carries (file constructor,
 * src/TSDF/TSDFVolume.cu:463-505): offset, truncation distance, max weight, global
 * translation / rotation.  The voxel size stays physical/size, as the reference recomputes it. */
int tsdf_volume_set_header(tsdf_volume *volume, const float offset[3], float truncation_distance,
                           float max_weight, const float global_translation[3],
                           const float global_rotation[3]);

/* ---- volume data access ---------------------------------------------------------------- */
/* Replace distance_data()/weight_data()/deformation() (src/include/TSDFVolume.hpp:175-203):
 * DEVICE pointers to the resident planes.  tsdf_volume_deformation materialises the node
 * array on first use (until then integrate computes voxel centres analytically with the
 * same float expression as initialise_deformation, src/TSDF/TSDFVolume.cu:783-785). */
int tsdf_volume_distances(const tsdf_volume *volume, float **device_ptr);
/* Call after writing distances through the raw device pointer (the reference only ever reads through it):
 * the ray caster's brick-occupancy summary is rebuilt before the next ray cast.  Writes through the raw pointers must be
 * ORDERED ON THE VOLUME'S STREAM (tsdf_volume_set_stream / tsdf_pipeline_streams), after the tsdf_volume_distances /
 * tsdf_volume_weights / tsdf_volume_mark_dirty call that precedes them: those calls make that stream wait for a tightening of
 * the occupancy flags that tsdf_pipeline_step may have left running on its second stream (it reads the distances). */
int tsdf_volume_mark_dirty(tsdf_volume *volume);
/* weight_data(): a device pointer to one fp32 weight per resident voxel, the reference's layout.  Until this is called a volume may
 * hold its weights more compactly (integrate only ever adds 1 to a weight, src/TSDF/TSDFVolume.cu:375-377: 8- or 16-bit counts,
 * tsdf_volume_weight_storage); the call converts them and the volume keeps fp32 weights from then on, clear() included, because the
 * caller may hold the pointer.  set_weight_data / get_weight_data speak fp32 whatever the storage and do not pin it. */
int tsdf_volume_weights(const tsdf_volume *volume, float **device_ptr);
/* How the weights are stored now: 8 or 16 (bits per voxel, counts) or 32 (fp32); *pinned (may be NULL) = 1 once tsdf_volume_weights
 * has handed the fp32 pointer out.  Integration computes the same bits in every storage ((float)count is exact). */
int tsdf_volume_weight_storage(const tsdf_volume *volume, int *bits_per_weight, int *pinned);
/* Widen the storage now -- 8 -> 16 -> 32 bits per weight, values unchanged -- instead of when a count is about to overflow in the middle
 * of a stream (the conversion allocates and synchronises: a caller that knows a session will revisit one region for hundreds of
 * frames pays it up front).  Narrowing is refused; clear() returns an unpinned volume to the starting mode. */
int tsdf_volume_set_weight_storage(tsdf_volume *volume, int bits_per_weight);
/* Self-test of the kernel arithmetic behind packed weights: integrate divides by (count + 1) with a short exact sequence instead of
 * the division instruction sequence (integrate_packed.hip: div_by_count, with the proof); this compares the two bit for bit for every
 * mantissa of the dividend (both signs, three exponents) and every divisor in [b_begin, b_end), 1 <= b_begin < b_end <= 2^17 + 1, and
 * returns the number of differences (0).  About a second for all 65536 divisors the 16-bit counts can reach. */
int tsdf_selftest_count_division(uint32_t b_begin, uint32_t b_end, unsigned long long *mismatches);
/* Self-tests of the bilateral filter's accumulation chain (bilateral_chain.hpp: the staged 15 x 15 kernel runs a half column of taps as
 * fp32 fmas where a test proves that this rounds like the reference's float/double expression, and in double elsewhere).  Both run on
 * the host, with the very expressions the kernel compiles, and need no GPU.
 * _taps: for n taps (weight w in {0} or [2^-120, 1], v4 = 4 * intensity < 2^18, running sum s in {0} or [2^-120, 2^40]) the new sum by
 * the fp32 tap, by the reference's tap, and whether the test certifies the tap (as a run of one) to be equal.
 * _image: the whole staged kernel on a host image (8 or 16 bits per pixel; sigmas that select it: radius 7, smallest weight >= 2^-120):
 * the filtered image (may be NULL) and, over interior waves (16 x 4 pixels, every tap inside the image),
 * counts = {half columns of waves, those where some lane failed the test (the wave falls back to double), half columns of lanes,
 * those that failed}. */
int tsdf_selftest_bilateral_chain_taps(size_t n, const float *w, const uint32_t *v4, const float *s, float *s_f32, float *s_f64,
                                       uint8_t *certified);
int tsdf_selftest_bilateral_chain_image(float sigma_colour, float sigma_space, const void *image, int bits_per_pixel, int width, int height,
                                        void *filtered, unsigned long long counts[4]);
/* Self-test of the pixel boxes of the cell-parallel ray cast (cell_boxes.hpp: which pixels a mixed cell can be seen by -- a bound, whose
 * arithmetic is chosen for speed and has to err on the wide side).  Runs on the host, with the very expressions the kernel compiles, and
 * needs no GPU.  r = rows 1-3 of world -> camera (3 x 4), k = rows 1-2 of the intrinsics (2 x 3), grid = voxels per axis; z_clip and
 * z_near as the cast chooses them (no sample of the view is nearer than z_clip; in front of z_near > 0 a cell takes the fast bound).
 * For each of n cells (the lower voxel's coordinates, 3 per cell, each + 1 below the grid's size): boxes = {u0, v0, width, height}
 * (zeros when no pixel sees the cell) and seen = 1 when some pixel does, + 2 when the cell took the corners' bound (at or behind z_near;
 * corners_only != 0 asks for it everywhere). */
int tsdf_selftest_cell_boxes(const float *r, const float *k, const float *voxel_size, const float *offset, const uint32_t *grid,
                             uint32_t width, uint32_t height, float z_clip, float z_near, size_t n, const uint32_t *cells, int corners_only,
                             int32_t *boxes, uint8_t *seen);
/* Self-test of the rule by which the cell-parallel ray cast gives every sample to ONE dual cell (cell_owner.hpp: cell_owns, two exact
 * comparisons per axis).  Runs on the host, with the very expression the kernel compiles, and needs no GPU.  grid = voxels per axis
 * (2 .. 65535), voxel_size per axis.  For each of n points (grid millimetres, 3 per point) and cells (the lower voxel's coordinates, 3 per
 * cell, each + 1 below the grid's size): owns = bit a set when the cell owns the point along axis a, + 8 when it owns it on all three;
 * lower = per axis the lower tap the reference's trilinearly_interpolate chooses for the point (restated: voxel_for_point,
 * centre_of_voxel_at, the clamps; -1 where it leaves through its off-grid return), its quotient formed by IEEE division, or with
 * fast_division != 0 by the three-instruction sequence of the kernels (without the check a volume makes before it uses that). */
int tsdf_selftest_cell_owner(const uint32_t *grid, const float *voxel_size, int fast_division, size_t n, const float *points,
                             const uint32_t *cells, uint8_t *owns, int32_t *lower);
/* Self-test of the Gauss-Newton back end that ICP and the field aligners share (gn_solve.hpp: icp_finish_step -- the second stage of the
 * 29-entry reduction, the unpivoted and the pivoted 6 x 6 LDL^T, the SE3 exponential, T <- exp(x) * T).  One launch of the very kernel
 * ICP and the plain aligner finish a step with, on sums the caller makes up: partial = n_blocks x 32 floats (a workgroup's 29 sums in
 * [0, 29): the upper triangle of (A | b) row by row, the residual, the inlier count), 1 <= n_blocks <= 256; the device buffer always has
 * 256 blocks and those at and past n_blocks hold a large finite value that the kernel has to leave out.  T_in: 4 x 4 column-major;
 * update != 0: solve and T <- exp(x) * T.  state_out[64]: [0, 16) the pose, [16] residual, [17] inliers, [18, 54) A (float values),
 * [54, 60) b. */
int tsdf_selftest_gn_finish(const float *partial, int n_blocks, const double T_in[16], int update, double state_out[64]);
int tsdf_volume_deformation(tsdf_volume *volume, tsdf_deformation_node **device_ptr);
/* Replace set_distance_data/set_weight_data/set_deformation (src/TSDF/TSDFVolume.cu:731-757):
 * blocking H2D of every resident voxel. */
int tsdf_volume_set_distance_data(tsdf_volume *volume, const float *host);
int tsdf_volume_set_weight_data(tsdf_volume *volume, const float *host);
int tsdf_volume_set_deformation(tsdf_volume *volume, const tsdf_deformation_node *host);
/* TSDFVolume::deform_mesh (src/TSDF/TSDFVolume.cu:265-291, kernel :226-263): num_points xyz triples are replaced by the
 * trilinear blend of the surrounding deformation nodes' translations, rotated by global_rotation and shifted by
 * global_translation.  Points outside the volume are left unchanged (the reference reads uninitialised memory there). */
int tsdf_volume_deform_points(const tsdf_volume *volume, int num_points, float *host_points);
int tsdf_volume_deform_points_device(const tsdf_volume *volume, int num_points, float *device_points);
/* Blocking D2H of every resident voxel (what save_to_file does, src/TSDF/TSDFVolume.cu:911-1027). */
int tsdf_volume_get_distance_data(const tsdf_volume *volume, float *host);
int tsdf_volume_get_weight_data(const tsdf_volume *volume, float *host);
/* The deformation nodes of resident planes [plane_begin, plane_begin + plane_count) (plane 0 = the first resident one), X*Y
 * nodes each, as save_to_file writes m_deformation_nodes (src/TSDF/TSDFVolume.cu:1003-1018): the device array when it has been
 * materialised (deformation() / set_deformation()), otherwise the regular grid initialise_deformation would have written
 * (src/TSDF/TSDFVolume.cu:783-785: voxel centre + the offset at the last clear(), rotation 0) -- without materialising it. */
int tsdf_volume_get_deformation_planes(const tsdf_volume *volume, uint32_t plane_begin, uint32_t plane_count,
                                       tsdf_deformation_node *host);
/* File constructor (src/TSDF/TSDFVolume.cu:463-664): a saved volume's node block is loaded verbatim.  When that block is the
 * regular grid of some constant offset (what clear() wrote, Q1) the nodes can stay implicit; this tells the volume which offset
 * they carry.  Refused once the node array is materialised. */
int tsdf_volume_set_offset_at_clear(tsdf_volume *volume, const float offset_at_clear[3]);

/* ---- integrate -------------------------------------------------------------------------- */
/* Replaces TSDFVolume::integrate + integrate_kernel (src/TSDF/TSDFVolume.cu:861-902, 308-392).
 * pose / inv_pose: 4x4, k / kinv: 3x3 (camera.pose(), inverse_pose(), k(), kinv()).
 * Host variant: blocking, depth in host memory.  Device variant: depth in HBM, asynchronous. */
int tsdf_integrate(tsdf_volume *volume, const uint16_t *host_depth, uint32_t width, uint32_t height,
                   const float pose[16], const float inv_pose[16], const float k[9], const float kinv[9]);
int tsdf_integrate_device(tsdf_volume *volume, const uint16_t *device_depth, uint32_t width,
                          uint32_t height, const float pose[16], const float inv_pose[16],
                          const float k[9], const float kinv[9]);
/* tsdf_integrate_device for a depth image whose tile maxima the caller already holds in HBM (written by
 * tsdf_bilateral_filter_u16_device_tiles for this very image, earlier on the same stream): same result, one launch fewer.
 * device_tile_max[ty * ceil(width / TSDF_DEPTH_TILE) + tx] must be >= every pixel of tile (tx, ty) and 0 only if all of
 * them are 0; a wrong array makes the culling drop bricks the frame updates. */
int tsdf_integrate_device_tiles(tsdf_volume *volume, const uint16_t *device_depth, uint32_t width,
                                uint32_t height, const float pose[16], const float inv_pose[16],
                                const float k[9], const float kinv[9], const uint16_t *device_tile_max);
/* The first half of tsdf_integrate_device_tiles ahead of time: the brick culling of a frame (it reads the tile maxima and the
 * pose, not the volume) on `hip_stream` -- e.g. a lower-priority stream, while the previous frame's ray cast runs on the
 * volume's stream.  The next tsdf_integrate_device_tiles with the same image, matrices and tile maxima launches only the
 * integrate kernel; any other integrate call ignores the preparation.  The caller orders the streams: the prepare call after
 * the volume's previous integrate has finished, the integrate call after the prepare call's work (events).  Same result.
 * The preparation is recognised by the ARGUMENTS (pointers, sizes, matrices), not by the buffers' content: between the prepare
 * call and the integrate call the image and its tile maxima must not be rewritten -- a caller that does rewrite them calls
 * tsdf_integrate_discard_prepared first (clear, a new offset or header, set_deformation discard it themselves). */
int tsdf_integrate_prepare_device_tiles(tsdf_volume *volume, const uint16_t *device_depth, uint32_t width,
                                        uint32_t height, const float pose[16], const float inv_pose[16],
                                        const float k[9], const float kinv[9], const uint16_t *device_tile_max,
                                        void *hip_stream);
int tsdf_integrate_discard_prepared(tsdf_volume *volume);
/* Optional kernel timing for roofline reports: when enabled, every launch of integrate_kernel (which = 0) and of
 * process_ray_kernel (which = 1) and process_ray_tail_kernel (which = 2) is bracketed by HIP events on the volume's stream; tsdf_volume_kernel_time
 * synchronises the stream and returns the number of bracketed launches and their average duration since timing was
 * (re-)enabled.  enabled = n > 1 brackets every n-th launch only: an event record costs a few microseconds of stream
 * time, which a sub-millisecond step notices (measured: 9 % with every launch bracketed).  Off by default. */
int tsdf_volume_set_timing(tsdf_volume *volume, int enabled);
int tsdf_volume_kernel_time(tsdf_volume *volume, int which, uint32_t *launches, float *average_ms);

/* Diagnostics: when enabled, integrate also counts the voxels whose weight changed (U in the
 * roofline model) and the distances it stored -- fewer: a distance whose bits the blend leaves as
 * they are is not written back.  Costs two atomics per wave; leave off when timing. */
int tsdf_volume_set_counting(tsdf_volume *volume, int enabled);
int tsdf_volume_last_updated_voxels(const tsdf_volume *volume, uint64_t *count);
int tsdf_volume_last_distance_stores(const tsdf_volume *volume, uint64_t *count);

/* ---- weight cap (what the reference's m_max_weight was for: src/include/TSDFVolume.hpp, src/TSDF/TSDFVolume.cu:375-381) ------------ */
/* Opt-in per volume, off by default.  With cap == 0 nothing changes anywhere: the plain kernels, no allocation, no launch -- a volume
 * averages every frame it has ever seen, as the reference's does.  With a cap c in 1 .. 65535, every voxel that the plain integrate
 * updates (same frustum, depth and sdf >= -trunc tests, same voxels) gets
 *       new_distance  = (prior_distance * prior_weight + tsdf * 1.0f) / (prior_weight + 1.0f)        (unchanged, :375-381)
 *       stored_weight = (prior_weight + 1.0f > (float)c) ? (float)c : prior_weight + 1.0f
 * The divisor is always prior_weight + 1; only the weight that is STORED is clamped.  (The reference's commented-out line, :378, clamps
 * the divisor itself: a saturated voxel would then compute D + tsdf / c every frame and run away, which is presumably why it is
 * commented out.)  So:
 *   - the distance of a saturated voxel is an exponential average with factor c / (c + 1): a surface that moves shows after a few
 *     times c frames instead of never;
 *   - a weight found above the cap (uploaded, or integrated before the cap was set) is used as it is for that blend and comes out
 *     as c; a NaN weight stays NaN (the comparison form above); voxels the frame does not update keep their weight;
 *   - the cap is a run-time setting of the volume object: tsdf_volume_clear keeps it, it is not written to .tsdf files, and
 *     tsdf_volume_info.max_weight stays the inert header field it is.  tsdf_volume_set_weight_cap(v, (uint32_t)info.max_weight) gives
 *     what the reference's field was for.  cap > 65535 is TSDF_ERR_INVALID with a message;
 *   - the cap may be changed between any two integrates; 0 returns to the plain kernels from the next integrate on.  A slab volume
 *     carries its own cap: the caller gives all slabs of one grid the same one;
 *   - storage (tsdf_volume_weight_storage): with 1 <= c <= 255 a volume with 8-bit counts keeps them for ever -- no look at the
 *     counts, no host round trip inside integrate, no widening; with c >= 256 it may go to 16 bits by the usual rule and never
 *     to fp32 for reasons of overflow.  Setting a cap never narrows: a volume at 16 or 32 bits stays there until clear().
 *     tsdf_volume_set_weight_data with counts above the cap is accepted and stored as without one;
 *   - colour is untouched: tsdf_integrate_colour with a cap gives the capped distances and weights and exactly the colour words
 *     it gives without one (the colour count n has its own saturation);
 *   - tsdf_volume_last_updated_voxels counts the voxels the frame updated, capped or not (the same number as without a cap);
 *     tsdf_volume_last_distance_stores counts the distance stores made.
 * Every integrate entry point honours it: tsdf_integrate*, tsdf_integrate_colour*, tsdf_pipeline_step*, tsdf_tracker_integrate*. */
int tsdf_volume_set_weight_cap(tsdf_volume *volume, uint32_t cap);   /* 0 = off (default: the reference's behaviour), 1..65535 */
int tsdf_volume_weight_cap(const tsdf_volume *volume, uint32_t *cap);

/* ---- de-integration (no reference counterpart: the reference's volume can only accumulate) ------------------------------------------ */
/* Takes a fused frame back out.  tsdf_deintegrate* takes the arguments of tsdf_integrate* and visits every voxel that tsdf_integrate
 * visits for the same depth image and camera -- the same frustum, depth and sdf >= -trunc tests, the same tsdf value, the same handling
 * of deformation nodes; that set depends on the image and the camera only, never on the volume's contents.  A volume on which it is
 * never called launches and allocates nothing new.  With w = prior_weight and D = prior_distance, in fp32, every operation rounded on
 * its own, in this order:
 *       if (!(w >= 1.0f))          the voxel is left alone            (never fused, already removed, a NaN weight)
 *       else  nw = w - 1.0f
 *             if (nw > 0.0f)  new_distance = ((D * w) - (tsdf * 1.0f)) / nw ;  weight = nw
 *             else            new_distance = truncation_distance ;             weight = 0     (what tsdf_volume_clear leaves)
 * So:
 *   - sequence property: after any sequence of integrates on a cleared, uncapped volume, de-integrating all of the same frames, in any
 *     order, leaves every distance at truncation_distance and every weight at 0, bit for bit;
 *   - one removal gives the other frames' average up to rounding.  With u = 2^-24 and T = truncation_distance: an integrate changes
 *     the voxel's sum D * w by the frame's tsdf within (3 w - 1) u T (the product at most (w - 1) T, the sum at most w T, the quotient
 *     at most T, each rounded once), a removal by -tsdf within 3 w u T.  Removing the frame integrated last therefore returns the
 *     distance the voxel had before it within (5 w / (w - 1) + 1) u T <= 11 u T < 6 * 2^-23 * T for every prior weight w >= 2: the
 *     bound does not grow with w.  Removing an earlier frame differs from the fp32 average of the remaining frames by the rounding
 *     of both running means as well, 3 u T per operation in the worst case -- any two orders of averaging differ by that;
 *   - weight cap: a volume with tsdf_volume_weight_cap != 0 is refused, TSDF_ERR_INVALID with a message: a saturated count is not a
 *     frame count;
 *   - colour words are never touched: the integer colour blend (rounded, saturating at 255) is not invertible.  There is no coloured
 *     variant;
 *   - storage: packed 8- and 16-bit counts go down in their own field (w >= 1: no borrow); the storage neither widens nor narrows,
 *     the bound behind tsdf_volume_weight_storage stays an upper bound.  Volumes the packed kernel does not serve (explicit
 *     deformation nodes, cameras not of the standard shape) take the fp32 layout as they do for tsdf_integrate;
 *   - tsdf_volume_last_updated_voxels counts the voxels whose weight went down, tsdf_volume_last_distance_stores the distance stores
 *     made (a distance whose bits stay is not written back);
 *   - occupancy stays a conservative superset: a removal that pulls a distance down flags its bricks as an integrate does; a ray
 *     cast after a removal gives exactly the picture it gives after a forced rebuild of the flags;
 *   - Z-slab volumes take out their own planes; the caller de-integrates on every slab of a grid.
 * Host variant: blocking, depth in host memory.  Device variant: depth in HBM, asynchronous on the volume's stream.  The frame must be
 * given exactly as it was integrated (the filtered image where the filtered image was fused) and at the same camera. */
int tsdf_deintegrate(tsdf_volume *volume, const uint16_t *host_depth, uint32_t width, uint32_t height,
                     const float pose[16], const float inv_pose[16], const float k[9], const float kinv[9]);
int tsdf_deintegrate_device(tsdf_volume *volume, const uint16_t *device_depth, uint32_t width, uint32_t height,
                            const float pose[16], const float inv_pose[16], const float k[9], const float kinv[9]);

/* ---- weighted integration (what the reference's current_weight was for: src/TSDF/TSDFVolume.cu:375-381 sets it to 1.0f) ------------- */
/* tsdf_integrate_weighted* takes the arguments of tsdf_integrate_colour* plus one fp32 weight per pixel (width * height floats, row
 * major like the depth image; rgb may be NULL).  A volume on which it is never called launches and allocates nothing new.
 *   - valid pixels: a pixel takes part iff its depth is > 0 and its weight p is finite and > 0.  Every other pixel -- p = 0, -0,
 *     negative, NaN, +-inf -- is treated exactly as if its depth were 0: for culling, the distance update, the colour update and the
 *     counters.  (The call works on a masked copy of the depth image in scratch owned by the volume.)  The caller's arrays are only read;
 *   - blend: on every voxel tsdf_integrate would update for that masked image, with p the weight of the voxel's pixel, w = prior_weight
 *     and D = prior_distance, in fp32, every operation rounded on its own, no contraction, in this order:
 *           nw = w + p
 *           new_distance = ((D * w) + (tsdf * p)) / nw
 *           stored weight = nw                                        without a weight cap
 *                         = nw > (float)cap ? (float)cap : nw         with one (tsdf_volume_set_weight_cap: the cap's comparison form;
 *                                                                     the divisor is never clamped, a NaN weight stays NaN)
 *   - unit property: with every p == 1.0f, distances, weights, colour words, occupancy marks and counters are bit for bit what
 *     tsdf_integrate* / tsdf_integrate_colour* leave on a volume with fp32 weights;
 *   - storage: the call moves the volume to fp32 weights first (tsdf_volume_weight_storage reports 32); counts already fused keep their
 *     values as floats.  It never narrows; tsdf_volume_clear returns an unpinned volume to its starting mode, as after any widening;
 *   - volumes with explicit deformation nodes, cameras not of the standard shape and Z-slab volumes are served (a slab updates its own
 *     planes; the caller integrates on every slab of a grid);
 *   - a distance whose bits stay is not stored, a weight whose bits stay neither; occupancy stays a conservative superset: a ray cast
 *     after weighted frames gives exactly the picture it gives after a forced rebuild of the flags;
 *   - colour: rgb != NULL on a colour volume gives exactly the colour words tsdf_integrate_colour gives for the masked image; the
 *     colour counts are not weighted.  On a volume without colour (or with explicit nodes) rgb != NULL is refused, as
 *     tsdf_integrate_colour is;
 *   - tsdf_volume_last_updated_voxels / tsdf_volume_last_distance_stores count as for tsdf_integrate of the masked image;
 *   - there is no weighted removal: fl(fl(w + p) - p) is not w.  tsdf_deintegrate* keeps its formula on whatever weights it finds;
 *   - refused (TSDF_ERR_INVALID, with a message): a NULL weight array, and whatever tsdf_integrate refuses;
 *   - tsdf_pipeline_step* does not take weights (its prepared culling recognises a frame by its pointer); tsdf_tracker_set_weighting does.
 * Host variant: blocking, arrays in host memory.  Device variant: arrays in HBM, asynchronous on the volume's stream; the arrays must
 * stay valid until the call's work on that stream is done. */
int tsdf_integrate_weighted(tsdf_volume *volume, const uint16_t *host_depth, const float *host_pixel_weight, const uint8_t *host_rgb /* or NULL */,
                            uint32_t width, uint32_t height, const float pose[16], const float inv_pose[16], const float k[9],
                            const float kinv[9]);
int tsdf_integrate_weighted_device(tsdf_volume *volume, const uint16_t *device_depth, const float *device_pixel_weight,
                                   const uint8_t *device_rgb /* or NULL */, uint32_t width, uint32_t height, const float pose[16],
                                   const float inv_pose[16], const float k[9], const float kinv[9]);
/* The standard weight models of a depth frame, for callers without a confidence plane: one fp32 weight per pixel, 0 where the depth
 * is 0, else the product of the factors `flags` selects (flags == 0: 1).  fp32, every operation rounded on its own (division and sqrtf
 * correctly rounded), in exactly this order, d = (float)depth:
 *       w = 1
 *   TSDF_WEIGHTS_INVERSE_SQUARE (the sensor's noise grows with z^2):
 *       r = z_ref / d ;  f = r * r ;  f = f > 1 ? 1 : f ;  w = w * f
 *     z_ref is in depth units (readings at or nearer than z_ref count fully); not finite or not > 0 is refused with this flag.
 *   TSDF_WEIGHTS_COSINE (the cosine of the incidence angle, from central differences of the back-projected image):
 *       P(x, y) = (ip * (d(x, y) / ip.z)) with ip = ((kinv.m11 * x + kinv.m12 * y) + kinv.m13, ... rows 2 and 3 alike), each component
 *                 ip.c * scale -- the point tsdf_depth_to_points_device forms
 *       a = P(x + 1, y) - P(x - 1, y) ;  b = P(x, y + 1) - P(x, y - 1)
 *       n = (a.y * b.z - a.z * b.y,  a.z * b.x - a.x * b.z,  a.x * b.y - a.y * b.x)
 *       np = (n.x * P.x + n.y * P.y) + n.z * P.z ;  nn = (n.x * n.x + n.y * n.y) + n.z * n.z ;  pp = (P.x * P.x + P.y * P.y) + P.z * P.z
 *       c = fabsf(np) / (sqrtf(nn) * sqrtf(pp)) ;  c = c > 1 ? 1 : c ;  c = c > 0 ? c : 0 ;  w = w * c
 *     A pixel with a neighbour off the image or of depth 0 has c = 0 (silhouettes and flying pixels are not fused), and so has one
 *     whose c is not > 0 (NaN included).
 * With both flags the inverse-square factor is multiplied in first.  Unknown flag bits, NULL arrays and images wider or higher than
 * 65535 are refused.  The depth image is only read.  Device variant: asynchronous on hip_stream; host variant: blocking. */
#define TSDF_WEIGHTS_INVERSE_SQUARE 1u
#define TSDF_WEIGHTS_COSINE 2u
int tsdf_depth_weights_device(uint32_t width, uint32_t height, const uint16_t *device_depth, const float kinv[9], uint32_t flags, float z_ref,
                              float *device_weight, void *hip_stream);
int tsdf_depth_weights(uint32_t width, uint32_t height, const uint16_t *host_depth, const float kinv[9], uint32_t flags, float z_ref,
                       float *host_weight);

/* ---- colour fusion (no reference counterpart: the reference allocates a uchar3 colour per voxel, src/include/TSDFVolume.hpp:290-293,
 * that none of its kernels writes) --------------------------------------------------------------------------------------------- */
/* Opt-in per volume.  A volume that never enables colour behaves exactly as without this group: no allocation, no launch.
 *   Storage: one dword per voxel {r, g, b, n} -- r in bits 0-7, g 8-15, b 16-23, n = colour observations (saturating at 255) in
 *     bits 24-31 -- x fastest like the distances; allocated and zeroed by tsdf_volume_enable_colour(v, 1) (4 bytes a voxel: 512 MiB
 *     at 512^3), freed by (v, 0), zeroed by tsdf_volume_clear.
 *   Integrate: tsdf_integrate_colour updates distances, weights, occupancy and counters with exactly the bits of tsdf_integrate for
 *     the same depth and camera, and updates the colour of every voxel that update touched (in the frustum, depth > 0,
 *     sdf >= -trunc: src/TSDF/TSDFVolume.cu:337-366) whose sdf is also <= +trunc, from the pixel (u, v) whose depth it used.  rgb
 *     is 8-bit interleaved RGB, width x height x 3, REGISTERED to the depth image (same camera, same size: TUM's depth frames are
 *     registered to its RGB frames).  Per channel, with c the pixel's value, in uint32 arithmetic:
 *         new = (old * n + c + ((n + 1) >> 1)) / (n + 1);     n' = min(n + 1, 255)
 *     (with n capped, later observations blend at 1/256).  Voxels with sdf > trunc (free space) keep their colour.  Where the
 *     volume's weights are packed counts and the camera standard, the packed integrate kernel makes the colour update itself
 *     (integrate_packed_colour_kernel); otherwise a colour pass follows the integrate kernel on the same stream and brick list.  The
 *     words are the same either way.
 *   Per frame: tsdf_pipeline_step_colour and tsdf_tracker_integrate_colour (below) are tsdf_pipeline_step and
 *     tsdf_tracker_integrate with a colour integrate of the filtered frame; tsdf_pipeline_step and tsdf_tracker_integrate leave the
 *     colours of a colour-enabled volume alone.
 *   Sampling: a world point p (mm) takes voxel i = (int)floorf(((p - offset) - offset_at_clear) / voxel_size) per axis, in fp32 in
 *     that order -- the cell whose centre as integrate forms it is nearest -- and reads that voxel's {r, g, b}; (0, 0, 0) for a NaN
 *     coordinate, an index outside the grid, or a voxel with n == 0.
 *   Refused (TSDF_ERR_INVALID, with a message): enabling colour on a Z-slab volume (tsdf_volume_create_slab); colour integrate on a
 *     volume whose deformation nodes are explicit (tsdf_volume_deformation / tsdf_volume_set_deformation); colour integrate,
 *     sampling or data access on a volume without colour enabled.
 *   Ray sets: tsdf_integrate_rays_colour* ("ray integration", rules 9 - 12) fuses a colour per point, tsdf_volume_cast_rays_colour*
 *     ("ray queries") reads the colour at the hits of arbitrary rays.
 *   Out of scope: slab (multi-GPU) colour, in a volume or a sharded pipeline; colour sampled inside the cast kernels; trilinear colour
 *     interpolation; colour with explicit deformation nodes; RGB cameras with intrinsics or extrinsics of their own. */
int tsdf_volume_enable_colour(tsdf_volume *volume, int enabled);   /* 1: allocate zeroed (kept if already enabled), 0: free */
int tsdf_volume_colour_enabled(const tsdf_volume *volume, int *enabled);
int tsdf_volume_colours(const tsdf_volume *volume, uint32_t **device_ptr);   /* the device array, one dword per resident voxel */
/* Blocking copies of every resident voxel's dword. */
int tsdf_volume_get_colour_data(const tsdf_volume *volume, uint32_t *host);
int tsdf_volume_set_colour_data(tsdf_volume *volume, const uint32_t *host);
/* tsdf_integrate / tsdf_integrate_device with the colour update of the same frame (same stream, same brick list). */
int tsdf_integrate_colour(tsdf_volume *volume, const uint16_t *host_depth, const uint8_t *host_rgb, uint32_t width, uint32_t height,
                          const float pose[16], const float inv_pose[16], const float k[9], const float kinv[9]);
int tsdf_integrate_colour_device(tsdf_volume *volume, const uint16_t *device_depth, const uint8_t *device_rgb, uint32_t width,
                                 uint32_t height, const float pose[16], const float inv_pose[16], const float k[9],
                                 const float kinv[9]);
/* n points (3 floats each, device) -> 3 bytes each (device), one thread per point, on hip_stream (NULL = the default stream). */
int tsdf_volume_sample_colours_device(const tsdf_volume *volume, uint64_t n, const float *device_points, uint8_t *device_rgb,
                                      void *hip_stream);
/* tsdf_raycast / tsdf_raycast_device, then the sampling of every vertex (misses are NaN: 0, 0, 0); 3 * width * height bytes. */
int tsdf_raycast_colour(const tsdf_volume *volume, uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                        float *host_vertices, float *host_normals, uint8_t *host_rgb);
int tsdf_raycast_colour_device(const tsdf_volume *volume, uint32_t width, uint32_t height, const float pose[16],
                               const float kinv[9], float *device_vertices, float *device_normals, uint8_t *device_rgb);

/* ---- class fusion (no reference counterpart; what Voxblox++, Kimera and SemanticFusion keep beside their distances) ------------------ */
/* Fuses the per-pixel class ids of a segmentation network and reads the fused class back where colour is read.  Opt-in per volume: a
 * volume that never enables classes behaves exactly as without this group: no allocation, no launch.
 *   Storage: one dword per voxel {class, votes} -- class in bits 0-15, votes in bits 16-31 -- x fastest like the distances; allocated
 *     and zeroed by tsdf_volume_enable_classes(v, 1) (kept if already enabled; 4 bytes a voxel: 512 MiB at 512^3), freed by (v, 0) and
 *     by destroy, zeroed by tsdf_volume_clear.  A word with votes == 0 is always 0x00000000: there is one "unclassified" word.  Valid
 *     class ids are 0..65534; TSDF_CLASS_VOID marks a pixel without a class, and a sample without one.
 *   Integrate: tsdf_integrate_classes* takes the arguments of tsdf_integrate_colour* plus classes (uint16, width * height, row-major,
 *     registered to the depth image) and confidence (uint8, width * height, or NULL: every pixel has strength 1).  rgb may be NULL.
 *     Distances, weights, weight storage, weight cap, occupancy and counters end up with exactly the bits tsdf_integrate leaves.  With
 *     rgb != NULL on a colour volume the colour words are exactly those of tsdf_integrate_colour.  The class update visits exactly the
 *     voxels the colour update visits -- in the frustum, depth > 0, -trunc <= sdf <= +trunc, sdf and pixel being the bits integrate
 *     computed -- free space keeps its word.  For such a voxel with pixel p, k = classes[p] and s = confidence ? confidence[p] : 1:
 *     if k == TSDF_CLASS_VOID or s == 0 the word is untouched; otherwise, with the old word (c, n), in uint32:
 *         n == 0          -> (k, s)
 *         c == k          -> (k, min(n + s, 65535))
 *         c != k, n >  s  -> (c, n - s)
 *         c != k, n == s  -> 0x00000000
 *         c != k, n <  s  -> (k, s - n)
 *     the weighted Boyer-Moore majority vote.  One writer per word and no atomics: a call's result is a unique set of bits.  The
 *     update is a pass of its own (band_pass_kernel with the policy ClassVote) behind the integrate kernel -- and behind the colour update, when rgb is
 *     given -- on the volume's stream over the frame's brick list, for standard and general cameras and all three weight storages.
 *   Sampling: tsdf_volume_sample_classes_device reads the voxel tsdf_volume_sample_colours_device reads -- the same frame
 *     (offset_at_clear subtracted), the same index expression -- and gives (TSDF_CLASS_VOID, 0) for a NaN coordinate, an off-grid
 *     index or a word with votes == 0.  device_votes may be NULL.  n == 0 is TSDF_OK and launches nothing.
 *   Ray cast: tsdf_raycast_classes* is tsdf_raycast*, then the sampling of every vertex; misses give VOID.  The cast's kernel choice
 *     and state are those of tsdf_raycast*.
 *   Counts: counts[k], k < n_classes, = the resident voxels whose word has class == k and votes >= max(min_votes, 1): the volume a
 *     class occupies in the band, in voxels.  counts is overwritten, not accumulated; n_classes in 1..65535, classes >= n_classes are
 *     not counted.  Integer atomics only, so the counts are unique (class_counts_kernel: a histogram per workgroup in LDS up to 4096
 *     classes, global atomics beyond).
 *   Refused (TSDF_ERR_INVALID, with a message naming the function, nothing written): enabling classes on a Z-slab volume
 *     (tsdf_volume_create_slab); class integrate on a volume whose deformation nodes are explicit; any call of this group, enabling
 *     aside, on a volume without classes enabled; NULL depth or classes; an empty image; rgb != NULL on a volume without colour;
 *     n_classes out of range; NULL outputs.
 *   Left alone: tsdf_integrate*, tsdf_integrate_colour*, tsdf_integrate_weighted*, tsdf_deintegrate* (a vote is not invertible),
 *     tsdf_integrate_rays*, tsdf_volume_fuse, snapshots and restore, the .tsdf and .tsdfs files, tsdf_pipeline_step* and
 *     tsdf_tracker_* neither read nor write class words.
 *   Out of scope: classes in the pipeline step, the tracker and kinfu_stream; classes from ray sets; classes through fuse, snapshots
 *     and files; a per-vertex class array inside the mesh handle and a filter by class; the class at tsdf_volume_cast_rays* hits.  (The connected pieces of each
 *     class, and which of them a point lies in: group "class objects".) */
#define TSDF_CLASS_VOID 0xFFFFu
int tsdf_volume_enable_classes(tsdf_volume *volume, int enabled);   /* 1: allocate zeroed (kept if already enabled), 0: free */
int tsdf_volume_classes_enabled(const tsdf_volume *volume, int *enabled);
int tsdf_volume_classes(const tsdf_volume *volume, uint32_t **device_ptr);   /* the device array, one dword per resident voxel */
/* Blocking copies of the whole array (resident voxels x 4 bytes). */
int tsdf_volume_get_class_data(const tsdf_volume *volume, uint32_t *host);
int tsdf_volume_set_class_data(tsdf_volume *volume, const uint32_t *host);
/* tsdf_integrate / tsdf_integrate_device (tsdf_integrate_colour* with rgb) with the class vote of the same frame. */
int tsdf_integrate_classes(tsdf_volume *volume, const uint16_t *host_depth, const uint8_t *host_rgb /* or NULL */,
                           const uint16_t *host_classes, const uint8_t *host_confidence /* or NULL */, uint32_t width, uint32_t height,
                           const float pose[16], const float inv_pose[16], const float k[9], const float kinv[9]);
int tsdf_integrate_classes_device(tsdf_volume *volume, const uint16_t *device_depth, const uint8_t *device_rgb /* or NULL */,
                                  const uint16_t *device_classes, const uint8_t *device_confidence /* or NULL */, uint32_t width,
                                  uint32_t height, const float pose[16], const float inv_pose[16], const float k[9],
                                  const float kinv[9]);
/* n points (3 floats each, device) -> a class and a vote count each (device), one thread per point, on hip_stream. */
int tsdf_volume_sample_classes_device(const tsdf_volume *volume, uint64_t n, const float *device_points, uint16_t *device_classes,
                                      uint16_t *device_votes /* or NULL */, void *hip_stream);
/* tsdf_raycast / tsdf_raycast_device, then the sampling of every vertex; width * height classes and (or NULL) votes. */
int tsdf_raycast_classes(const tsdf_volume *volume, uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                         float *host_vertices, float *host_normals, uint16_t *host_classes, uint16_t *host_votes /* or NULL */);
int tsdf_raycast_classes_device(const tsdf_volume *volume, uint32_t width, uint32_t height, const float pose[16],
                                const float kinv[9], float *device_vertices, float *device_normals, uint16_t *device_classes,
                                uint16_t *device_votes /* or NULL */);
/* Voxels per class: n_classes 64-bit counts (host: blocking, on the volume's stream; device: on hip_stream). */
int tsdf_volume_class_counts(const tsdf_volume *volume, uint32_t n_classes, uint32_t min_votes, uint64_t *host_counts);
int tsdf_volume_class_counts_device(const tsdf_volume *volume, uint32_t n_classes, uint32_t min_votes, uint64_t *device_counts,
                                    void *hip_stream);

/* ---- field queries (no reference counterpart: the reference's volume can be fused into, rendered and meshed, not asked) ---------- */
/* The trilinear distance, its gradient and the weight of the fused field at world points.  Opt-in by being called: a volume on which
 * these are never called does exactly what it did.
 *   Frame: for a world point p (mm), q = p - offset per axis in fp32, offset being the volume's CURRENT offset -- the space_min of the
 *     ray cast and the frame tsdf_volume_marching_cubes emits vertices in, because the points one asks about are ray-cast and mesh
 *     vertices.  This is deliberately NOT the frame of tsdf_volume_sample_colours_device, which also subtracts offset_at_clear.
 *   S(q): the ray cast's trilinear sample (src/RayCaster/GPURaycaster.cu:53-124 as tsdf_raycast evaluates it), bit for bit: the same
 *     voxel_for_point, the same lower-corner rule on the unclamped point, the same tap clamping at the far faces, the same eight-term
 *     sum in the same order, every fp32 operation rounded on its own.
 *   valid(q): every component is finite, >= 0 and < size[i] * voxel_size[i] (the fp32 product); -0.0 is valid.
 *   distance: S(q) if valid(q), else NaN.
 *   weight: the weight of the voxel (int)floorf(q[i] / voxel_size[i]) (IEEE division) as a float if valid(q), else 0.0f -- the same
 *     value in all three storages (8-bit counts, 16-bit counts, fp32); uploaded non-integer or NaN fp32 weights come back as stored.
 *     (A valid point within rounding of the upper bound can divide to size[i] itself: there is no such voxel, the weight is 0.0f and
 *     the distance, as in the ray cast, NaN.)  The query never widens, pins or converts the storage: tsdf_volume_weight_storage
 *     reports the same before and after.
 *   gradient: with h = voxel_size, for each axis a, q+ = q with q[a] + h[a] and q- = q with q[a] - h[a] (one fp32 add each) and
 *         grad[a] = (S(q+) - S(q-)) / (h[a] + h[a])
 *     each S a full sample as above.  If q or any of the six shifted points is not valid, the whole gradient is (NaN, NaN, NaN): within
 *     one voxel of a face the distance is a number and the gradient is not.  The TSDF is positive in front of a surface, so the
 *     gradient points out of it.
 *   TSDF_FIELD_UNIT_GRADIENT: len = sqrtf((gx * gx + gy * gy) + gz * gz), the output is grad / len per component; if len is not > 0
 *     (zero, or NaN) the output is the NaN triple.  (Correctly rounded sqrtf and division.)
 *   Explicit deformation nodes are ignored, as the ray cast ignores them.
 *   Refused (TSDF_ERR_INVALID, with a message): a Z-slab volume (tsdf_volume_create_slab: the taps cross slab boundaries); all three
 *     outputs NULL; NULL points with n > 0.  n == 0 is TSDF_OK and launches nothing.
 *   Stream order: the query reads the distance array and the weight storage on the stream it is given (NULL = the default stream);
 *     the caller orders that stream behind the integrates it wants to see (and in front of whatever replaces the weight storage:
 *     an integrate that widens it, tsdf_volume_weights, clear).  It writes nothing that belongs to the volume: no occupancy flag, no
 *     dirty mark, no counter.
 *   Out of scope: slab volumes, queries in the deformed space, colour interpolation, use inside the tracker. */
#define TSDF_FIELD_UNIT_GRADIENT 1
/* n points (3 floats each, device) -> distance (n floats), gradient (3 n floats), weight (n floats): any of the three may be NULL and
 * then costs nothing (a distance-only or weight-only query reads none of the gradient's taps). */
int tsdf_volume_sample_field_device(const tsdf_volume *volume, uint64_t n, const float *device_points, float *device_distance,
                                    float *device_gradient, float *device_weight, int flags, void *hip_stream);
/* The same on host arrays, on the volume's stream; blocking. */
int tsdf_volume_sample_field(const tsdf_volume *volume, uint64_t n, const float *host_points, float *host_distance,
                             float *host_gradient, float *host_weight, int flags);
/* tsdf_raycast_device, then the unit gradient at every vertex in place of compute_normals (whose cross products are NaN along every
 * silhouette and beside every miss); a miss is the NaN triple.  The vertices are those of tsdf_raycast_device.  Asynchronous on the
 * volume's stream. */
int tsdf_raycast_gradient_normals_device(const tsdf_volume *volume, uint32_t width, uint32_t height, const float pose[16],
                                         const float kinv[9], float *device_vertices, float *device_normals);

/* ---- ray queries (no reference counterpart: the reference casts the rays of a pinhole image only) ---------------------------------- */
/* Where does THIS ray hit the surface?  n rays of the caller's own -- a spinning LiDAR or fisheye model, a visibility test between two
 * points, a collision probe, a few rays around a tracked feature -- each marched as the image cast marches a pixel's ray.  Opt-in by
 * being called: a volume on which these are never called does exactly what it did.
 *   Frame: origins and directions are 3 n floats in world millimetres, the frame of ray-cast and mesh vertices (the volume's CURRENT
 *     offset is the box's space_min, offset + physical size its space_max), like the points of "field queries".
 *   The march of ray i: process_ray (src/RayCaster/GPURaycaster.cu:265-377) as tsdf_raycast evaluates it, with origin = origins[i] and
 *     dir = directions[i] used AS GIVEN -- the reference normalises neither (Q6), so the step along the ray is 0.05 * trunc * |dir|:
 *     the same ray/box test giving near_t and max_t, the same start point ((near_t * dir) + origin) - space_min, the same sample
 *     parameters T[k] (T[0] = 0, T[k+1] = T[k] + step in fp32), the same trilinear sample S ("field queries"), the same stop at the first
 *     sample <= 0, the same refinement of its parameter with previous_tsdf == trunc (Q7) giving th, the same `t >= max_t` and
 *     4402-sample limits, every fp32 operation rounded on its own.  A ray given a pixel's origin and direction returns that pixel's
 *     vertex of tsdf_raycast bit for bit.
 *   points[i]: the reference's hit point ((th * dir) + start) + space_min, or (NaN, NaN, NaN) on a miss.
 *   t[i]: near_t + th (one fp32 add), the ray parameter of the hit measured from the origin in units of dir -- millimetres for a
 *     unit direction; NaN on a miss.
 *   normals[i]: exactly what tsdf_volume_sample_field_device(..., TSDF_FIELD_UNIT_GRADIENT) returns at points[i] (the NaN triple
 *     within a voxel of a face); the NaN triple on a miss.
 *   t_max (n floats, or NULL = no limit): the march's FIRST hit counts only if t[i] <= t_max[i]; otherwise the ray is a miss (a
 *     surface behind the limit is not looked for past an earlier one).  A NaN t_max[i] is therefore a miss, +inf no limit.
 *   Decreed misses, decided before any march: a non-finite component of the origin or the direction; a direction of all zeros (-0.0
 *     included).
 *   Explicit deformation nodes are ignored, as the image cast ignores them.
 *   Refused (TSDF_ERR_INVALID, with a message): a NULL volume; a Z-slab volume (tsdf_volume_create_slab); all three outputs NULL; NULL
 *     origins or directions with n > 0; more rays than a launch holds (n > (2^31 - 1) * 256).  n == 0 is TSDF_OK and launches nothing.
 *   Side effects: distances, weights, colours and counters are never written.  The brick occupancy the march skips by is refreshed as
 *     the image cast refreshes it, so a query after an integrate, tsdf_volume_set_distance_data, tsdf_volume_mark_dirty or clear sees
 *     the current field.  Nothing of the image cast's scheduling state changes: an image cast after a ray query takes the same kernels
 *     (tsdf_volume_last_raycast_kind) and gives the same bits as without the query.  One thing the query does in the image cast's
 *     place: the first ray cast of either kind after a bulk change of the distances (tsdf_volume_set_distance_data,
 *     tsdf_volume_mark_dirty, clear, a loaded file) rebuilds the flags, counts the flagged bricks the image cast chooses its kernels
 *     by, and waits for the volume's stream once -- so that one query blocks, also through the device entry point, and until the next
 *     cell-parallel cast tsdf_volume_last_cell_list reports that count, not the list of a cast.
 *   Output order is input order; the rays are not sorted.
 *   Colour at the hits (tsdf_volume_cast_rays_colour*): tsdf_volume_cast_rays* with the same arguments -- points, t and normals come out
 *     bit for bit -- and then, one thread per ray on the same stream, rgb[3i..3i+2]: with q = points[i] - offset (the CURRENT offset),
 *     if valid(q) in the sense of "field queries", the voxel (int)floorf(q[k] / voxel_size[k]) -- the one whose weight a field query
 *     reports -- gives its {r, g, b} if its n > 0; (0, 0, 0) on a miss, when q is not valid, when an index reaches size[k], or when
 *     n == 0.  This is the ray frame, the one rule 9 of "ray integration" writes in: nothing is done with offset_at_clear.  It equals
 *     tsdf_volume_sample_colours_device (which subtracts offset_at_clear) wherever offset_at_clear is zero.  Refused as well: a volume
 *     without colour enabled, NULL rgb, NULL points (the sample needs them).
 *   Out of scope: slab or multi-GPU volumes, rays in the deformed space, trilinear colour. */
/* Device pointers; any of the three outputs may be NULL, not all.  Asynchronous on the volume's stream, like tsdf_raycast_device
 * (and like it synchronising once after a bulk change of the distances: see "Side effects"). */
int tsdf_volume_cast_rays_device(const tsdf_volume *volume, uint64_t n, const float *device_origins, const float *device_directions,
                                 const float *device_t_max /* n floats, or NULL = no limit */,
                                 float *device_points, float *device_t, float *device_normals);
/* The same on host arrays, on the volume's stream; blocking. */
int tsdf_volume_cast_rays(const tsdf_volume *volume, uint64_t n, const float *host_origins, const float *host_directions,
                          const float *host_t_max, float *host_points, float *host_t, float *host_normals);
/* The two calls above with the colour at every hit (3 n bytes); points and rgb must be given.  See "Colour at the hits". */
int tsdf_volume_cast_rays_colour_device(const tsdf_volume *volume, uint64_t n, const float *device_origins,
                                        const float *device_directions, const float *device_t_max /* or NULL */, float *device_points,
                                        float *device_t, float *device_normals, uint8_t *device_rgb);
int tsdf_volume_cast_rays_colour(const tsdf_volume *volume, uint64_t n, const float *host_origins, const float *host_directions,
                                 const float *host_t_max, float *host_points, float *host_t, float *host_normals, uint8_t *host_rgb);

/* ---- volume fusion (no reference counterpart: the reference's volume is filled from depth frames only) ------------------------------ */
/* Resamples the field of `src` onto the grid of `dst` through a rigid transform and blends it in: merging a second session's volume or
 * a sub-map, re-posing a volume after a loop closure, moving a volume to a finer or coarser grid, re-centring the grid.  Opt-in by
 * being called.  Grids, voxel sizes, offsets and truncation distances of the two volumes may all differ.
 *   dst_to_src is column-major like a pose; only its top three rows are used.  fused_voxels may be NULL.
 *   Every kernel goes on dst's stream after that stream has waited for src's.  With fused_voxels non-NULL the call synchronises and
 *   stores the number of voxels it updated; otherwise it is asynchronous like tsdf_integrate_device.
 * Everything below is separately rounded fp32 in exactly this order.  For every voxel (x, y, z) of dst:
 *   1. centre: c.x = ((x + 0.5f) * voxel_size_dst.x) + offset_dst.x, likewise y and z -- dst's CURRENT offset, the frame of ray-cast and
 *      mesh vertices, the one the field queries use;
 *   2. transform: p.x = ((m[0] * c.x + m[4] * c.y) + m[8] * c.z) + m[12], likewise rows 1 and 2;
 *   3. source point: q = p - offset_src; the voxel is skipped unless valid(q) in the sense of the field queries;
 *   4. sample: s = S(q) of src, the ray cast's trilinear sample, bit for bit (see "field queries");
 *   5. eight taps: the ones that sample reads -- the same lower-corner rule on the unclamped point, the same clamping of the +1 taps at
 *      the far faces, so taps may coincide.  The voxel is skipped unless all eight tap weights are > 0: a tap that was never observed
 *      holds the cleared distance and would otherwise bleed into the blend;
 *   6. source weight: ws, the weight of the source voxel q lies in -- the one a field query reports, always one of the eight taps;
 *   7. a NaN s skips the voxel; otherwise s = fminf(fmaxf(s, -trunc_dst), trunc_dst);
 *   8. blend: d' = ((d * w) + (s * ws)) / (w + ws), w' = w + ws (IEEE division);
 *   9. weight cap: with tsdf_volume_set_weight_cap on dst the stored weight is min(w + ws, cap), the divisor stays w + ws.
 * Skipped voxels keep their distance and weight bit for bit.  src is never written and its weight storage is not converted.
 *   Weight storage of dst: counts stay counts.  Before the launch dst is widened (8 -> 16 bits -> fp32) whenever its weight bound plus
 *   the largest source weight could pass what its storage holds (the source's bound: its integration count in packed storage, a max
 *   reduction over fp32 weights); a cap that fits the field needs no room.  If src holds fp32 weights that are not all non-negative
 *   integers <= 65535, dst takes fp32 storage.  All nine combinations of {8, 16, 32}-bit storage on the two sides give the same bits.
 *   The ray caster's summary of dst is handed over as tsdf_volume_mark_dirty does: the next cast rebuilds it from the distances.
 *   Colour is out of scope: dst's colour array is left untouched.
 * Refused (TSDF_ERR_INVALID, with a message, nothing written): null arguments; dst == src; volumes on different devices; a Z-slab on
 * either side; a materialised deformation-node array on either side (voxel centres must be the implicit grid); a non-finite entry in
 * the top three rows of the matrix. */
int tsdf_volume_fuse(tsdf_volume *dst, const tsdf_volume *src, const float dst_to_src[16], uint64_t *fused_voxels);
/* Diagnostics of the last tsdf_volume_fuse into dst: how many of its 64 x 4 x 32-voxel bricks the cull kept, and how many there are
 * (both 0 before the first fuse).  Synchronises dst's stream. */
int tsdf_volume_last_fuse_bricks(const tsdf_volume *dst, uint32_t *listed_bricks, uint32_t *total_bricks);

/* ---- ray integration (no reference counterpart: the reference's volume is filled from pinhole depth frames only) -------------------- */
/* Fuses n rays of the caller's own -- a spinning LiDAR's scan, a fisheye depth sensor, a stereo point cloud, a merged scan, the point
 * set tsdf_aligner_* has just posed -- into the volume: ray i runs from its origin (the sensor's position) to points[i] (the surface
 * it measured).  Opt-in by being called: a volume on which these are never called does exactly what it did.
 *   points: n xyz triples, fp32, world millimetres in the frame of ray-cast and mesh vertices (the volume's CURRENT offset), like the
 *     points of "field queries" and the rays of "ray queries".  origins: one triple (n_origins == 1: one sensor position for the whole
 *     scan) or n triples (n_origins == n).
 *   updated_voxels may be NULL.  Non-NULL: the call synchronises and stores the number of voxels it changed, as tsdf_volume_fuse does
 *     with fused_voxels; otherwise the device variant is asynchronous on the volume's stream, like tsdf_integrate_device.
 *   ONE CALL IS ONE OBSERVATION PER VOXEL: a voxel that any number of the call's rays cross takes the mean of their observations and
 *     its weight goes up by 1, exactly as a voxel seen by one depth frame.  Weights stay frame counts: the 8 / 16 / 32-bit storage,
 *     its widening before a count could overflow and the weight cap all behave as for tsdf_integrate.
 * The rules.  Every operation is separately rounded fp32 in the order written, unless marked as double; o is the ray's origin, p its
 * point, N_k the grid's size, offset the current offset, trunc the truncation distance.
 *   1. Ray: d = p - o per component; r = sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z); u = d / r (three divisions).  The ray is a decreed skip,
 *      before any walk, if a component of o or p is not finite, if r is zero or not finite, if r < min_range, if r > max_range (+inf:
 *      no limit), or if either range is NaN.
 *   2. Stretch: te = r + trunc; ts = 0, or fmaxf(r - trunc, 0) with TSDF_RAYS_BAND_ONLY.  The default is what the depth integrate does,
 *      which updates every voxel with sdf >= -trunc, the free space in front of the surface included.
 *   3. Grid coordinates: a_k = (o_k - offset_k) / voxel_size_k, s_k = u_k / voxel_size_k.
 *   4. Clip of [t0, t1] = [ts, te] to the box [0, N_k]: an axis with s_k == 0 skips the ray unless 0 <= a_k < N_k; otherwise
 *      ta = (0 - a_k) / s_k, tb = ((float)N_k - a_k) / s_k, t0 = fmaxf(t0, fminf(ta, tb)), t1 = fminf(t1, fmaxf(ta, tb)).  The ray is
 *      skipped unless t0 < t1.
 *   5. Walk (Amanatides-Woo, without drift): the start cell is i_k = clamp((int)floorf(a_k + t0 * s_k), 0, N_k - 1).  Repeat: visit i;
 *      for each axis with s_k != 0, tn_k = ((float)(i_k + (s_k > 0 ? 1 : 0)) - a_k) / s_k -- recomputed from the integer cell every
 *      time, never accumulated; take the axis with the smallest tn_k (on a tie x before y, y before z); stop if that tn_k > t1; step
 *      that axis by sign(s_k); stop when the cell leaves the grid.  No ray visits more than X + Y + Z cells.
 *   6. Observation of a visited voxel (x, y, z): its centre c.x = ((x + 0.5f) * voxel_size.x) + offset.x, likewise y and z (the
 *      expression of "volume fusion"); e = c - o; sdf = r - ((e.x*u.x + e.y*u.y) + e.z*u.z).  No observation if sdf < -trunc.
 *      tsdf = sdf > 0 ? fminf(sdf, trunc) : sdf;  q = (int)rintf((tsdf / trunc) * 32768.0f), an integer in [-32768, 32768].
 *   7. Accumulation: per voxel, over the call's rays, the count n_v of observations and the exact integer sum S_v of their q.  Integer
 *      sums have no order: the result does not depend on the order of the rays, nor on which lanes run them.
 *   8. Apply, for every voxel with n_v >= 1: m = (float)(((double)S_v / (double)n_v) * ((double)trunc * (1.0 / 32768.0))) (double);
 *      d' = ((d * w) + m) / (w + 1) with IEEE division; w' = w + 1, stored as min(w + 1, cap) under tsdf_volume_set_weight_cap (the
 *      divisor stays w + 1).  Every other voxel keeps its distance and weight bit for bit.
 * Coloured (tsdf_integrate_rays_colour*): the plain call plus a colour update.  Distances, weights, the weight storage, the weight cap,
 * updated_voxels and the occupancy hand-over come out with exactly the bits tsdf_integrate_rays* produces for the same arguments.
 *   9. Colour observation: rgb[3i..3i+2] is the colour of points[i].  A visited voxel takes a colour observation from ray i iff rule 6
 *      gave it an observation and its UNCLAMPED sdf also satisfies sdf <= trunc: the depth path's band -trunc <= sdf <= +trunc
 *      ("colour fusion").  Free space in front of the surface is carved but keeps its colour.  The test is on sdf, not on q:
 *      q == 32768 is also reached by rounding from below trunc.
 *  10. Accumulation: per voxel, over the call's rays, the count c_v of colour observations and the exact integer sums R_v, G_v, B_v of
 *      their channels.  Integer sums have no order.
 *  11. One call is one colour observation: for every voxel with c_v >= 1, per channel in unsigned 64-bit arithmetic,
 *      m = (2 * SUM_v + c_v) / (2 * c_v) -- the mean rounded half up, so m <= 255.
 *  12. Blend: with old = {r, g, b, n} of that voxel's colour word, the depth path's blend in uint32 per channel:
 *      new = (old * n + m + ((n + 1) >> 1)) / (n + 1), n' = min(n + 1, 255).  Every other colour word keeps its bits.
 *   Which word: the colour word has the index of the distance the same call updates -- the cell (x, y, z) of rule 5 -- and nothing is
 *     done with offset_at_clear.  (tsdf_volume_sample_colours_device subtracts offset_at_clear and this does not: the two agree
 *     wherever offset_at_clear is zero; tsdf_volume_cast_rays_colour* reads in this frame.)
 *   Refused as well (TSDF_ERR_INVALID, with a message, nothing written): a volume without colour enabled; NULL rgb with n > 0.
 *   Scratch: the first coloured call adds 16 bytes per voxel (2 GiB at 512^3 on top of the plain 1 GiB), allocated zeroed, all zero
 *     again whenever a call ends, freed by tsdf_volume_release_ray_scratch or with the volume.  tsdf_integrate_rays* never allocates
 *     or touches it.  tsdf_volume_ray_scratch_bytes reports what is held (0 when none).
 * Left alone by tsdf_integrate_rays*: colour.  By both: a prepared integrate (tsdf_integrate_prepare_device_tiles) is neither used nor
 *   discarded; explicit deformation nodes are refused, not ignored.  The ray caster's summary is handed over as tsdf_volume_mark_dirty
 *   does: the next cast rebuilds it from the distances.  The call does not count towards the periodic tightening of that summary.
 * Scratch: 8 bytes per voxel (1 GiB at 512^3) plus one byte per 64 x 4 x 32-voxel brick, allocated zeroed by the first call, all zero
 *   again whenever a call ends, kept until tsdf_volume_destroy or tsdf_volume_release_ray_scratch.
 * Refused (TSDF_ERR_INVALID, with a message, nothing written): a NULL volume; unknown flag bits; n_origins neither 1 nor n; n > 2^23
 *   (S_v then fits 40 bits beside a 24-bit count in one 64-bit word); NULL points or origins with n > 0; a Z-slab
 *   (tsdf_volume_create_slab); a materialised deformation-node array (voxel centres must be the implicit grid, as for
 *   tsdf_volume_fuse).  n == 0 is TSDF_OK and changes nothing.
 * Out of scope: taking a ray set back out, coloured or not (tsdf_deintegrate* has no ray counterpart: the mean of a call's observations
 *   is not kept), colour through tsdf_volume_fuse, trilinear colour, a brick-sparse scratch, slab or multi-GPU volumes, rays in the
 *   deformed space. */
#define TSDF_RAYS_BAND_ONLY 1   /* update only within trunc of the end point: no free-space carving */
int tsdf_integrate_rays_device(tsdf_volume *volume, uint64_t n, const float *device_origins, uint64_t n_origins,
                               const float *device_points, float min_range, float max_range, int flags, uint64_t *updated_voxels);
/* The same on host arrays, on the volume's stream; blocking. */
int tsdf_integrate_rays(tsdf_volume *volume, uint64_t n, const float *host_origins, uint64_t n_origins, const float *host_points,
                        float min_range, float max_range, int flags, uint64_t *updated_voxels);
/* The two calls above with the colour of every point (3 n bytes): rules 9 - 12. */
int tsdf_integrate_rays_colour_device(tsdf_volume *volume, uint64_t n, const float *device_origins, uint64_t n_origins,
                                      const float *device_points, const uint8_t *device_rgb /* 3 n bytes */, float min_range,
                                      float max_range, int flags, uint64_t *updated_voxels);
int tsdf_integrate_rays_colour(tsdf_volume *volume, uint64_t n, const float *host_origins, uint64_t n_origins, const float *host_points,
                               const uint8_t *host_rgb, float min_range, float max_range, int flags, uint64_t *updated_voxels);
/* Frees the scratch of the four calls above (synchronises the volume's stream); the next call allocates it again. */
int tsdf_volume_release_ray_scratch(tsdf_volume *volume);
/* The bytes of ray-integration scratch the volume holds right now; 0 when none is held. */
int tsdf_volume_ray_scratch_bytes(const tsdf_volume *volume, uint64_t *bytes);

/* ---- field alignment (no reference counterpart: nothing in the reference produces a transform from the field itself) --------------- */
/* The rigid pose that puts a point set on the zero level of the fused field: Gauss-Newton on sum S(T x)^2, which is point-to-plane ICP
 * with the association replaced by a trilinear sample (the field is the model: distance 0 on the surface, the gradient its normal).
 * No ray cast, no model maps, no projective association.  Opt-in by being called: a process that never calls these does what it did.
 *   Pose: T is a column-major double[16] mapping the points' frame to the frame of the field queries -- the volume's CURRENT offset,
 *     in volume units.  Only its top three rows are read; the bottom row comes back as (0, 0, 0, 1).
 *   Pivot: the pose is kept about the centre of the volume's box, so that the rotation columns of the system are not inflated by the
 *     distance to the world origin: h[a] = 0.5f * max[a] with max[a] the fp32 product size[a] * voxel_size[a], and
 *     T_c = Tr(-(offset + h)) * T, formed in double on the host, which also converts back on the way out.
 *   Per point x, every fp32 operation rounded on its own: R, t are T_c narrowed to fp32;
 *         u[r] = ((R[r,0] * x0 + R[r,1] * x1) + R[r,2] * x2) + t[r]          (ICP's expression)
 *         q = u + h per axis;  d = S(q), the sample of "field queries";
 *         g = the raw central-difference gradient of "field queries" at q (six more samples at q -+ voxel_size e_a, each difference
 *             divided by voxel_size[a] + voxel_size[a]).
 *     The point is an inlier iff valid(q) and valid of all six shifted points ("field queries": NaN and infinite points fall out
 *     here); the weight of the voxel q lies in is > 0 and so is the weight of the voxel each shifted point lies in (the field query's
 *     weight, any storage: an unobserved neighbourhood holds the cleared distance, not a surface); d and all of g are finite;
 *     fabsf(d) < gate; (gx * gx + gy * gy) + gz * gz > 0.
 *     Row: (gx, gy, gz, u1 * gz - u2 * gy, u2 * gx - u0 * gz, u0 * gy - u1 * gx, -d).  An inlier adds the row's 28 upper-triangular
 *     products (for o < 7, for i >= o: sum[s++] += row[o] * row[i]) and 1.0f to entry 28; entry 27 is the sum of d^2.
 *   Order of the sums (part of the contract, as for ICP): B = min(256, ceil(n / 256)) workgroups of 256 threads; thread (b, t) takes
 *     points i = 256 b + t, then i += 256 B, sequentially in fp32; then the wave64 shuffle-down tree (offsets 32 ... 1); then the four
 *     waves as ((w0 + w1) + w2) + w3; the per-workgroup sums are then added as tsdf_icp_* adds them (8 groups of 32 workgroups in
 *     double, narrowed to fp32), and the solve (6 x 6 LDL^T in double, zero pivots give zero components), the SE3 exponential and
 *     T_c <- exp(x) * T_c are those of tsdf_icp_get_incremental_transformation.
 *   Nothing of the volume is written; the calls read the distances and the weight storage on the aligner's stream, which the caller
 *     orders behind the integrates it wants seen.
 *   Refused (TSDF_ERR_INVALID, with a message, nothing written): null arguments; a Z-slab volume; a non-finite entry in T's top three
 *     rows; gate not > 0; more than 8 stages; step == 0; volume and aligner on different devices.
 *   Out of scope: robust weights, slab volumes, the deformed space.  (A colour term: "colour alignment", below.) */
typedef struct tsdf_aligner tsdf_aligner;   /* opaque: partial sums, the double-buffered state, a pinned in/out block and a stream */
int tsdf_aligner_create(tsdf_aligner **out);   /* on the current device */
void tsdf_aligner_destroy(tsdf_aligner *aligner);
int tsdf_aligner_set_stream(tsdf_aligner *aligner, void *hip_stream);
int tsdf_aligner_stream(const tsdf_aligner *aligner, void **hip_stream);
/* One step's sums at T without an update (the counterpart of tsdf_icp_estimate_step): the 6 x 6 normal matrix A, b, {sum of d^2,
 * inliers}.  n points of 3 floats on the device.  device_rows (may be NULL): 7 n floats, the row of every point, the NaN row for an
 * outlier.  n == 0 gives zeros and launches nothing.  Blocking. */
int tsdf_aligner_step(tsdf_aligner *aligner, const tsdf_volume *volume, uint32_t n, const float *device_points, const double T[16],
                      float gate, float A[36], float b[6], float residual_inliers[2], float *device_rows);
typedef struct tsdf_align_stage {
    const float *device_points;   /* n points of 3 floats */
    uint32_t n;
    uint32_t iterations;
} tsdf_align_stage;
/* Up to 8 stages queued back to back as one chain on the aligner's stream: each launch finishes the step before it, one finishing
 * launch and one synchronise come at the end; the pose travels through pinned memory.  A stage with n == 0 or iterations == 0 is
 * skipped.  A step with 0 inliers leaves the pose as it is; residual / inliers (either may be NULL) are the sum of d^2 and the inlier
 * count of the last step, so inliers == 0 says the chain ended blind: the caller judges.  A chain that never moved the pose returns T
 * as given, bit for bit. */
int tsdf_aligner_run(tsdf_aligner *aligner, const tsdf_volume *volume, uint32_t n_stages, const tsdf_align_stage *stages, float gate,
                     double T[16] /* in: start, out */, float *residual, float *inliers);
/* Pixel (x * step, y * step) of a uint16 depth image (millimetres) -> the camera-frame point (kinv * (px, py, 1)) * (depth / z of
 * that product), kinv column-major 3 x 3, each row summed as (k1 * px + k2 * py) + k3; the NaN triple for depth 0 or depth >
 * depth_cutoff (millimetres; INFINITY: none).  ceil(width / step) x ceil(height / step) interleaved points, row-major.  Asynchronous
 * on hip_stream. */
int tsdf_depth_to_points_device(uint32_t width, uint32_t height, const uint16_t *device_depth, const float kinv[9], uint32_t step,
                                float depth_cutoff, float *device_points, void *hip_stream);

/* ---- colour alignment (no reference counterpart) ------------------------------------------------------------------------------------ */
/* Field alignment with a photometric row per point beside the geometric one, sampled from the fused colour field ("colour fusion")
 * exactly where the distance is sampled.  Where the geometry does not constrain the pose -- a flat wall, a floor, a corridor: the
 * distance gradient has no in-plane component, the normal matrix is singular there and the solve zeroes those directions -- the
 * texture can.  Opt-in by being called: tsdf_aligner_step, tsdf_aligner_run, tsdf_tracker_align_field and their kernels are as they
 * were.  Every fp32 operation below is rounded on its own.
 *   Intensity of a colour: Y(r, g, b) = (float)(77 r + 150 g + 29 b) * 0x1p-8f -- exact in fp32 (an integer <= 65280 times a power of
 *     two).  A voxel's intensity is Y of its colour word {r, g, b, n}; it is defined only when n > 0.
 *   Intensity of the field at q (the frame of "field queries"): with the trilinear cell of the distance sample S(q) -- the same lower
 *     voxel l, the same u, v, w and the same clamped tap offsets that the ray cast's trilinear sample forms -- and I_ijk the intensity
 *     of the voxel at l + (i, j, k) (a tap past the far face is clamped onto its lower neighbour),
 *         I(q) = I000 (1-u)(1-v)(1-w) + I001 (1-u)(1-v) w + I010 (1-u) v (1-w) + I011 (1-u) v w
 *              + I100 u (1-v)(1-w) + I101 u (1-v) w + I110 u v (1-w) + I111 u v w,
 *     the distance sample's eight-term expression term for term: each term multiplied left to right, the terms added left to right.
 *     The gradient is the exact derivative of that interpolant inside the cell, not a central difference:
 *         gx = ((I100-I000)(1-v)(1-w) + (I101-I001)(1-v) w + (I110-I010) v (1-w) + (I111-I011) v w) / voxel_size.x
 *         gy = ((I010-I000)(1-u)(1-w) + (I011-I001)(1-u) w + (I110-I100) u (1-w) + (I111-I101) u w) / voxel_size.y
 *         gz = ((I001-I000)(1-u)(1-v) + (I011-I010)(1-u) v + (I101-I100) u (1-v) + (I111-I110) u v) / voxel_size.z
 *     each term multiplied left to right, the four added left to right, the division the sampler's own for that axis (it equals the
 *     IEEE quotient).  The tap differences are exact in fp32.  A tap clamped onto its lower neighbour gives a zero difference: that is
 *     the definition, not an error.  Valid iff valid(q) ("field queries"), the volume has colour enabled and all eight taps have
 *     n > 0; otherwise the intensity is NaN and the gradient the NaN triple (so too where valid(q) divides to size[i] itself and
 *     the distance is NaN).  Eight colour dwords a point.
 *   Photometric row of a point x with observed intensity y: u and q are those of the geometric row ("field alignment");
 *         c = I(q), e = c - y, gc = the gradient above,
 *         row_c = (gcx, gcy, gcz, u1 * gcz - u2 * gcy, u2 * gcx - u0 * gcz, u0 * gcy - u1 * gcx, -e).
 *     The point is a colour inlier iff it is a geometric inlier (the colour term acts at the surface only, within `gate`), I(q) is
 *     valid, y is finite (a NaN y marks a point without colour) and fabsf(e) < colour_gate.  A zero colour gradient is allowed: it
 *     adds e^2 and the count only.
 *   Sums: a second block of 29 -- the 28 products of row_c in the geometric block's order (the sum of e^2 at entry 27) and the colour
 *     inlier count at entry 28 -- accumulated beside the geometric block in exactly its order (per-thread strided fp32, the wave64
 *     shuffle tree, ((w0 + w1) + w2) + w3, 8 groups of 32 workgroups in double, narrowed to fp32).  The system handed to the solve is,
 *     per entry of A and b, (float)((double)S_g + (double)colour_weight * (double)S_c); colour_weight == 0 therefore reproduces
 *     tsdf_aligner_run's pose bit for bit.  The solve, the SE3 exponential and the update are those of "field alignment".
 *     Residuals and inlier counts are reported per term and never combined.  colour_weight is in (volume units)^2 per intensity^2
 *     (mm^2 per intensity^2 with the usual millimetres) and scene-dependent: it trades a distance residual against a brightness one.
 *   Nothing of the volume is written; distances, weights and colour words are read on the aligner's stream.
 *   Refused (TSDF_ERR_INVALID, with a message, nothing written): everything tsdf_aligner_* refuses; a volume without colour enabled;
 *     NULL intensities; colour_gate not > 0; colour_weight negative or not finite; both outputs of a sample NULL.
 *   Out of scope: robust weights, colour in ICP's projective path, slab volumes, the deformed space, trilinear colour for rendering. */
/* I(q) (n floats) and its gradient (3 n floats) at n world points (q = p - offset as in "field queries"); either output may be NULL,
 * not both.  n == 0 is TSDF_OK and launches nothing.  Asynchronous on hip_stream (NULL = the default stream). */
int tsdf_volume_sample_intensity_device(const tsdf_volume *volume, uint64_t n, const float *device_points, float *device_intensity,
                                        float *device_gradient, void *hip_stream);
/* The same on host arrays, on the volume's stream; blocking. */
int tsdf_volume_sample_intensity(const tsdf_volume *volume, uint64_t n, const float *host_points, float *host_intensity,
                                 float *host_gradient);
/* Pixel (x * step, y * step) of an RGB frame (3 bytes a pixel) -> Y: ceil(width / step) x ceil(height / step) floats, row-major -- the
 * order and count of tsdf_depth_to_points_device's points, so the two arrays pair up.  Asynchronous on hip_stream. */
int tsdf_rgb_to_intensity_device(uint32_t width, uint32_t height, const uint8_t *device_rgb, uint32_t step, float *device_intensity,
                                 void *hip_stream);
/* tsdf_aligner_step with the colour term: A and b are the combined system, residual_inliers = {sum of d^2, inliers, sum of e^2, colour
 * inliers}.  device_intensity: n floats, the observed intensity of every point (NaN: none).  device_rows (may be NULL): 14 n floats,
 * the geometric then the photometric row of every point; an outlier of a term gets the NaN row for that term.  Blocking. */
int tsdf_aligner_step_colour(tsdf_aligner *aligner, const tsdf_volume *volume, uint32_t n, const float *device_points,
                             const float *device_intensity, const double T[16], float gate, float colour_gate, float colour_weight,
                             float A[36], float b[6], float residual_inliers[4], float *device_rows);
typedef struct tsdf_align_colour_stage {
    const float *device_points;      /* n points of 3 floats */
    const float *device_intensity;   /* n floats */
    uint32_t n;
    uint32_t iterations;
} tsdf_align_colour_stage;
/* tsdf_aligner_run with the colour term: the chaining, the skipping of empty stages, the rule that a chain that never moved the pose
 * returns T as given bit for bit, and the pinned in/out block are its.  residual / inliers (either may be NULL): {geometric, colour}
 * of the last step. */
int tsdf_aligner_run_colour(tsdf_aligner *aligner, const tsdf_volume *volume, uint32_t n_stages, const tsdf_align_colour_stage *stages,
                            float gate, float colour_gate, float colour_weight, double T[16] /* in: start, out */, float residual[2],
                            float inliers[2]);

/* ---- raycast ---------------------------------------------------------------------------- */
/* Replaces GPURaycaster::raycast = get_vertices/process_ray + compute_normals
 * (src/RayCaster/GPURaycaster.cu:519-547, 432-486, 265-377, 393-427, 496-510).
 * pose: camera pose (origin = translation column, rot = upper-left 3x3), kinv: 3x3.
 * vertices / normals: 3*width*height floats each (packed float3, pixel order y*width+x);
 * a miss is (NaN,NaN,NaN).  normals may be NULL (get_vertices only, as render_to_depth_image
 * needs, src/RayCaster/GPURaycaster.cu:555-606). */
int tsdf_raycast(const tsdf_volume *volume, uint32_t width, uint32_t height, const float pose[16],
                 const float kinv[9], float *host_vertices, float *host_normals);
int tsdf_raycast_device(const tsdf_volume *volume, uint32_t width, uint32_t height,
                        const float pose[16], const float kinv[9], float *device_vertices,
                        float *device_normals);
/* compute_normals alone (src/RayCaster/GPURaycaster.cu:393-427) on device buffers. */
int tsdf_normals_device(uint32_t width, uint32_t height, const float *device_vertices,
                        float *device_normals, void *hip_stream);
/* The per-pixel part of GPURaycaster::render_to_depth_image (src/RayCaster/GPURaycaster.cu:575-579) on device
 * buffers: depth = (uint16_t)roundf(Camera::world_to_camera(vertex).z) with the vertex map of a ray cast; pixels the
 * cast missed (NaN) and depths outside 1..65535 give 0 (the reference's conversion of NaN is undefined). */
int tsdf_vertices_to_depth_device(uint32_t width, uint32_t height, const float *device_vertices,
                                  const float inv_pose[16], uint16_t *device_depth, void *hip_stream);
/* GPURaycaster::render_to_depth_image (src/RayCaster/GPURaycaster.cu:554-589) in one call on device buffers: the ray cast with the
 * depth formed from every hit as above, without a vertex map in between (device_vertices may be NULL; when given it is filled
 * as tsdf_raycast_device fills it).  Asynchronous on the volume's stream. */
int tsdf_raycast_depth_device(const tsdf_volume *volume, uint32_t width, uint32_t height, const float pose[16],
                              const float inv_pose[16], const float kinv[9], uint16_t *device_depth, float *device_vertices);
/* Which kernels the volume's last ray cast took: 1 = the cell-parallel cast (one wave per flagged brick, no ray is marched), 0 = the
 * march kernels.  Scheduling only -- both produce the same bits -- reported by bench.py beside the kernels' times. */
int tsdf_volume_last_raycast_kind(const tsdf_volume *volume, int *cell_parallel);
/* Diagnostics: how many tasks (flagged bricks in view, large ones counted by their parts) the volume's last cell-parallel cast listed.
 * Waits for the volume's stream.  0 before the first such cast. */
int tsdf_volume_last_cell_list(const tsdf_volume *volume, uint32_t *listed);
/* Diagnostics for the roofline model: S = trilinear samples evaluated, T = distinct voxels
 * touched by any tap, of one raycast with these arguments (runs an instrumented kernel). */
int tsdf_raycast_stats(const tsdf_volume *volume, uint32_t width, uint32_t height, const float pose[16],
                       const float kinv[9], uint64_t *samples, uint64_t *touched_voxels, uint64_t *hits);

/* Diagnostics: trilinear samples the production kernel actually evaluates (the rest of the reference's S
 * samples are passed by exact empty-space skipping), and the state of the brick occupancy it skips on. */
int tsdf_raycast_evaluated_samples(const tsdf_volume *volume, uint32_t width, uint32_t height,
                                   const float pose[16], const float kinv[9], uint64_t *evaluated,
                                   float *host_per_ray /* optional 3*W*H: samples, loop trips, count */);
int tsdf_volume_occupancy(const tsdf_volume *volume, uint64_t *occupied_bricks, uint64_t *total_bricks);
/* Diagnostics / tests: the per-brick bytes themselves (ceil(X/4) * ceil(Y/4) * ceil(Z/4) each, x fastest; any pointer
 * may be NULL).  force_rebuild != 0 recomputes the flags from the distance array first. */
int tsdf_volume_get_occupancy_data(const tsdf_volume *volume, int force_rebuild, uint8_t *host_fine, uint8_t *host_cell,
                                   uint8_t *host_reach);

/* Replaces the device part of extract_surface (src/MarchingCubes/MarkAndSweepMC.cu:506-555): marching cubes over the
 * volume's distance array on the GPU.  Cubes in the reference's order (x fastest, then y, then z), its corner / edge
 * numbering (:9-36, :80-97), sign rule (:110-124) and interpolate() arithmetic (:47-63); three consecutive vertices per
 * triangle (the caller wires them (i, i+2, i+1), :549).  table = 256 x 32 edge numbers, three per triangle, -1
 * terminated (the host library generates it: tsdf_host_mc_table).  *n_vertices receives the vertex count; when
 * host_vertices is not NULL and capacity (in vertices) suffices, it receives 3 floats per vertex.  A Z-slab marches the cube layers
 * rooted in its own planes: the slabs' arrays concatenated in slab order are the whole volume's. */
int tsdf_volume_marching_cubes(const tsdf_volume *volume, const int8_t *table, uint64_t *n_vertices, float *host_vertices,
                               uint64_t capacity);

/* ---- indexed mesh (no reference counterpart: the reference's extract_surface emits a triangle soup) ------------------------------- */
/* Marching cubes whose output is an indexed mesh that stays on the device: shared vertices, an index buffer, optionally a normal and a
 * colour per shared vertex, of the whole grid or of a box of it.  Opt-in by being called: tsdf_volume_marching_cubes and everything
 * else do exactly what they did.
 *   Contract: let S be the soup tsdf_volume_marching_cubes emits (cubes x fastest, then y, then z), restricted to the marched cubes.
 *     The mesh is (V, I):
 *     V: one vertex per lattice edge that a marched cube uses.  A lattice edge is (x, y, z, a): the voxel at its lower end and its
 *       axis (0, 1, 2 = x, y, z); it is used when its two ends differ in d < 0 (NaN and both zeros are not < 0) and at least one of the
 *       up to four cubes round it is marched.  Sorted by the key ((z * Y + y) * X + x) * 3 + a, X, Y the WHOLE grid's sizes.  The
 *       position is the 12 bytes the soup has for that edge: every cube round an edge computes the same bytes, because all twelve cube
 *       edges run in the positive direction of an axis, corner positions depend on the absolute voxel coordinate only and interpolate()
 *       orders its end points by sign.
 *     I: one uint32 per soup vertex, in soup order, with V[I[k]] == S[k] bit for bit.  Triangle t is (I[3t], I[3t+2], I[3t+1]), the
 *       wiring extract_surface uses.
 *     Welding is by lattice edge, NOT by position: where a voxel is exactly 0 the crossings of several edges fall on the same point;
 *       they stay distinct vertices, and the triangles between them stay as degenerate as the reference makes them.
 *   Box: {x0, y0, z0, x1, y1, z1} marches the cubes rooted at voxels in [x0, x1) x [y0, y1) x [z0, z1); the ends are clipped to
 *     X - 1, Y - 1, Z - 1 (tsdf_mesh_info.box has the box as clipped); NULL is the whole grid.  A begin that is not below its end on
 *     some axis, before clipping, is refused; a box that clips to nothing gives an empty mesh, as does a grid with an axis shorter than
 *     2.  The keys are the whole grid's, so an edge has the same bytes in every box that holds it, and boxes that tile the grid give,
 *     cube for cube, the whole soup.
 *   TSDF_MESH_NORMALS: one normal per vertex of V: the bytes tsdf_volume_sample_field_device(..., TSDF_FIELD_UNIT_GRADIENT) gives there
 *     (NaN triples included).  TSDF_MESH_COLOURS: the 3 bytes tsdf_volume_sample_colours_device gives there; refused on a volume
 *     without colour.  Both are those entry points, called on V on the volume's stream.
 *   The handle owns the device arrays and its scratch and keeps them between extractions; they only grow, so a per-frame re-mesh into
 *     a warm handle allocates nothing.  Scratch: 32 bytes per 64 voxels of the marched range (three 64-bit masks of used edges and two
 *     bases; a vertex's index is a base plus popcounts, no per-edge index array exists), 16 bytes per 65536 voxels, the table:
 *     tsdf_mesh_scratch_bytes <= 1 byte per voxel of the whole grid + 64 KiB, whatever the box.
 *   Stream order: tsdf_volume_extract_mesh enqueues on the volume's stream, synchronises it once (to size the arrays from the counts)
 *     and returns with the kernels that fill the arrays enqueued.  tsdf_mesh_buffers and tsdf_mesh_download wait for them; a later
 *     extraction into the same handle is ordered behind them.  A handle is used by one thread at a time, on the device it was made on.
 *   The result is the same arrays on every run: no atomics, nothing depends on the order in which waves finish.  The volume is not
 *     written: no distance, weight, occupancy flag, dirty mark or ray-cast state.
 *   Refused (TSDF_ERR_INVALID, with a message): NULL volume, table or mesh; a Z-slab volume (tsdf_volume_create_slab:
 *     tsdf_volume_marching_cubes serves those); a table tsdf_volume_marching_cubes refuses; unknown flags; more than 2^32 - 1 vertices
 *     or indices (extract in boxes); tsdf_mesh_download into an array the mesh was extracted without.
 *   Out of scope: slab volumes, skipping empty rows by the occupancy flags (their "low voxel" is not the sign test).  Welding by
 *     position and simplification are the group "mesh simplification" below. */
typedef struct tsdf_mesh tsdf_mesh;
#define TSDF_MESH_NORMALS 1u
#define TSDF_MESH_COLOURS 2u
typedef struct tsdf_mesh_info {
    uint64_t n_vertices, n_indices;
    uint32_t flags;
    uint32_t box[6];   /* as clipped */
} tsdf_mesh_info;
int tsdf_mesh_create(tsdf_mesh **out);   /* on the current device */
void tsdf_mesh_destroy(tsdf_mesh *mesh);
int tsdf_volume_extract_mesh(const tsdf_volume *volume, const int8_t *table, const uint32_t box[6], uint32_t flags, tsdf_mesh *mesh);
int tsdf_mesh_get_info(const tsdf_mesh *mesh, tsdf_mesh_info *info);
/* The device arrays of the last extraction: 3 floats per vertex, one uint32 per index, 3 floats / 3 bytes per vertex.  Any out pointer
 * may be NULL; an array the mesh lacks (or any array of an empty mesh) gives NULL.  Valid until the next extraction into the handle. */
int tsdf_mesh_buffers(const tsdf_mesh *mesh, const float **device_vertices, const uint32_t **device_indices,
                      const float **device_normals, const uint8_t **device_rgb);
/* Blocking copies to host arrays sized from tsdf_mesh_get_info; any may be NULL. */
int tsdf_mesh_download(const tsdf_mesh *mesh, float *host_vertices, uint32_t *host_indices, float *host_normals, uint8_t *host_rgb);
/* Device bytes the handle holds besides the four output arrays.  After an extraction alone that is the bound above; the first
 * components call (group "mesh components") adds 8 bytes per vertex (labels and sizes) and 32 bytes, a filter INTO the handle 12 bytes
 * per 64 vertices and per 64 triples of its source, a simplification INTO the handle what the group "mesh simplification" states, a
 * smoothing INTO the handle (or tsdf_mesh_compute_normals ON it) what the group "mesh smoothing" states, a scene-flow call WITH the
 * handle what the group "scene flow" states. */
int tsdf_mesh_scratch_bytes(const tsdf_mesh *mesh, uint64_t *bytes);

/* ---- mesh components (no reference counterpart: the reference's soup has no connectivity to ask about) ----------------------------- */
/* The connected pieces of an indexed mesh, labelled on the device, and a filter that drops the small ones (the floaters every fused
 * scan of real depth data carries) without the mesh leaving the device.  Opt-in by being called: no other entry point, launch or
 * result changes.
 *   Graph: n_vertices vertices and n_indices indices, n_indices a multiple of 3.  Index triple t joins the three vertices I[3t],
 *     I[3t+1], I[3t+2]; the wiring order does not matter.  Degenerate triples (a, a, b) and (a, a, a) and repeated triples all count as
 *     triangles and join whatever distinct vertices they name.  A vertex that no triple names is a component of its own.
 *   Outputs (unique values, whatever computes them):
 *     L[v]: the smallest vertex index in v's component (uint32).
 *     T[v]: the number of index triples whose first index lies in v's component -- so all three do -- the same for every vertex of the
 *       component (uint32).
 *     tsdf_components_info: n_components; n_triangles = n_indices / 3; largest_triangles and largest_label: the component with the most
 *       triangles, ties going to the smallest label.  For n_vertices == 0: n_components = 0, largest_label = 0xFFFFFFFF,
 *       largest_triangles = 0.  The largest component is found from T: a tsdf_label_components_device call without
 *       device_component_triangles reports largest_triangles = 0 and largest_label = 0xFFFFFFFF.
 *     Nothing depends on the order in which waves run: two runs give the same bytes.
 *   How: a lock-free union-find over L itself, hooks towards the smaller index (DESIGN.md 20 argues the invariants): parent[v] <= v
 *     always, a word changes only to a smaller member of the same component, so every chain strictly decreases, the final root is the
 *     component's minimum and no lane ever waits for another.  Triangle counts are integer atomics.
 *   tsdf_label_components_device: any index buffer on the device.  Blocking: it synchronises hip_stream once, to read the info and
 *     the error word.  device_labels (n_vertices words) is its parent array, device_component_triangles (n_vertices words, may be NULL)
 *     its counter array: the counts land at the roots and are broadcast in place.  Beyond those it holds 32 bytes of device scratch
 *     for the duration of the call.  An index >= n_vertices is found on the device by the first kernel that reads I, before any lane
 *     uses it as an address: the call returns TSDF_ERR_INVALID, the two arrays hold unspecified values inside [0, n_vertices) and
 *     nothing outside that range has been touched.
 *   tsdf_mesh_label_components: the handle's last extraction (or filter into it).  Labels and sizes are kept in the handle, allocated by
 *     the first components call (never by tsdf_volume_extract_mesh), until the next extraction or filter into it;
 *     tsdf_mesh_component_buffers gives the device arrays (NULL for an empty mesh), tsdf_mesh_component_download copies them (either
 *     pointer may be NULL).  Both refuse a handle that has not been labelled since.
 *   tsdf_mesh_filter_components: labels src first if it has not been labelled since its last extraction.  A component is kept iff
 *     T >= min_triangles and, with TSDF_MESH_KEEP_LARGEST, it is the largest one.  dst receives the kept vertices in their order (the
 *     sort by key survives), the kept triples in their order with indices remapped, normals and colours where src has them as the same
 *     bytes, info.flags and info.box as src's.  So V'[I'[k]] is the soup's vertex for every kept soup vertex bit for bit, and
 *     min_triangles == 0 without the flag gives dst equal to src array for array.  An empty src gives an empty dst.  dst keeps its
 *     arrays and only grows them, as an extraction does.  At most two synchronisations: one for the labelling (when it is needed), one
 *     for the two counts.  No atomics in the filter: keep flags by ballot over 64 vertices / triples, popcount bases, a chunk scan; a
 *     new index is a base plus the popcount below the lane.  src and the volume are never written, apart from src's own label arrays.
 *   Stream order: the mesh calls enqueue on hip_stream (NULL: the default stream) behind the handle's pending extraction, and later
 *     tsdf_mesh_buffers / tsdf_mesh_download / extractions are ordered behind them in turn.
 *   Refused (TSDF_ERR_INVALID, with a message): NULL device_labels, NULL device_indices with n_indices > 0, a NULL handle;
 *     n_indices % 3 != 0; n_vertices or n_indices above 2^32 - 1; an index >= n_vertices; dst == src; unknown flags; handles made on
 *     different devices.
 *   Out of scope: slab volumes, components of the volume's voxels (those of its frontier voxels: group "exploration"), hole filling, labelling inside tsdf_volume_extract_mesh, labels
 *     that stay stable across re-meshes.  Welding by position and simplification are the group "mesh simplification" below. */
typedef struct tsdf_components_info {
    uint64_t n_components, n_triangles, largest_triangles;
    uint32_t largest_label;
} tsdf_components_info;
#define TSDF_MESH_KEEP_LARGEST 1u
int tsdf_label_components_device(uint64_t n_vertices, uint64_t n_indices, const uint32_t *device_indices, uint32_t *device_labels,
                                 uint32_t *device_component_triangles, tsdf_components_info *info, void *hip_stream);
int tsdf_mesh_label_components(tsdf_mesh *mesh, tsdf_components_info *info, void *hip_stream);
int tsdf_mesh_component_buffers(const tsdf_mesh *mesh, const uint32_t **device_labels, const uint32_t **device_component_triangles);
int tsdf_mesh_component_download(const tsdf_mesh *mesh, uint32_t *host_labels, uint32_t *host_component_triangles);
int tsdf_mesh_filter_components(tsdf_mesh *src, uint64_t min_triangles, uint32_t flags, tsdf_mesh *dst, void *hip_stream);

/* ---- mesh simplification (no reference counterpart: the reference's soup goes to a file as it is) ---------------------------------- */
/* A level of detail of an indexed mesh, made on the device: vertex clustering on a grid of cubic cells (Rossignac-Borrel).  The vertices
 * of one cell become one vertex, the mean of its members; triples that no longer have three corners are dropped.  Opt-in by being
 * called: no other entry point, launch or result changes.
 *   The result (unique values, whatever computes them), with h = cell_size, fp32, finite and > 0:
 *   1. Cell.  f_a = floorf(V_a / h) per axis a: one fp32 divide, correctly rounded, then floor.  A vertex is LOOSE if any coordinate is
 *     not finite, or any |f_a| is not < 2^20, or any |V_a| is not < 2^21 (tested in float, before anything becomes an integer); a
 *     loose vertex is a cluster of its own.  Every other vertex has the 63-bit key ((f_z + 2^20) << 42) | ((f_y + 2^20) << 21) |
 *     (f_x + 2^20); vertices with equal keys form a cluster.  (Extracted meshes carry loose vertices: the NaN crossings next to a NaN
 *     voxel.)
 *   2. Order.  A cluster's representative is its member with the smallest source index; output vertex j is the cluster whose
 *     representative is the j-th smallest.  So the order of an extracted mesh (sorted by lattice-edge key) survives as far as it can.
 *     A cluster is an output vertex whether or not a kept triple names it: tsdf_mesh_filter_components(dst, 1, 0, ...) removes the
 *     unreferenced ones.
 *   3. Position.  A cluster of one member (a loose vertex included) keeps that member's 12 bytes: -0.0, NaN and denormals survive.
 *     Otherwise, per axis, q = llrintf(V_a * 1024.0f) (the product is exact, the rounding to nearest-even), S the int64 sum of q over
 *     the n members, and the output is (float)(((double)S / (double)n) / 1024.0).  Integers are summed, so no arrival order can change
 *     the sum; a member moves by at most 2^-11 of the unit (mm), fp32's own spacing at 4 m.
 *   4. Normals (when given).  A cluster of one keeps the bytes.  Otherwise d_a = the sum of llrintf(N_a * 1048576.0f) over the members
 *     whose normal is finite in all three components, as doubles; L = sqrt(d_x * d_x + d_y * d_y + d_z * d_z) in double arithmetic, no
 *     contraction, added left to right; the output is (float)(d_a / L), and a NaN triple when L == 0 (no finite member, or the normals
 *     cancel).  Normals are expected to be of unit size or thereabouts: a component at or above 2^20 may overflow a sum.
 *   5. Colours (when given).  Per channel (2 S + n) / (2 n) in integers, S the sum of the members' bytes: the mean rounded half up, as
 *     the colour blend rounds.  A cluster of one is its own byte.
 *   6. Triples.  Each index is replaced by its cluster's output index; a triple with two equal new indices is dropped (one that was
 *     degenerate in the source included); the rest stay in their order, wiring and winding untouched.  Two triples on the same three
 *     clusters are both kept.
 *   7. The position weld.  With a cell so small that no two distinct positions share one, the result is the source minus its exactly
 *     coincident vertices (which an extracted mesh has where a voxel is exactly 0: "welding is by lattice edge") and the triples that
 *     die with them.
 *   8. dst->info: n_vertices = the clusters, n_indices = 3 x the kept triples, flags = TSDF_MESH_NORMALS / TSDF_MESH_COLOURS according to
 *     the arrays given; dst is not labelled.  An empty source gives an empty dst; vertices with n_indices == 0 are legal.
 *   tsdf_simplify_mesh_device: any arrays on the device (3 floats per vertex, one uint32 per index, 3 floats / 3 bytes per vertex or
 *     NULL); dst->info.box is all zero.  tsdf_mesh_simplify: src's arrays, normals and colours where src has them, info.box = src's.
 *   How: no sort.  One lane per vertex puts its key into an open-addressed table of the smallest power of two >= 2 n_vertices slots
 *     with one 64-bit compare-and-swap per probe, linear probing; a probe ends on "was empty" or "was my key", anything else moves on.
 *     No lane waits for another: at load <= 1/2 an empty slot lies on every walk.  The slot's representative word takes
 *     an atomicMin of the vertex index.  Keep bits by ballot over 64, popcount bases and the chunk scan are the components filter's;
 *     the sums are integer atomics into dense per-cluster rows; one lane per cluster divides.  No float is ever added atomically.
 *   At most one synchronisation of hip_stream (NULL: the default stream), to size dst's arrays from the two counts and read the error
 *     word; the call returns with the kernels that fill the arrays enqueued, and stream order is that of the components filter.  src
 *     and the volume are never written.  dst keeps its arrays and scratch and only grows them: a warm re-simplify allocates nothing.
 *   Scratch of a simplification into dst, counted by tsdf_mesh_scratch_bytes(dst), with P the smallest power of two >= 2 n_vertices
 *     (so P < 4 n_vertices) and n_clusters the output's vertices:
 *       12 P + 4 n_vertices + 80 n_clusters + 12 (ceil(n_vertices / 64) + ceil(n_triples / 64)) + 16 (ceil(chunks / 1024) + 1) + 8
 *     bytes, chunks the larger of the two ceilings (8 bytes of key and 4 of representative per slot, 4 per vertex, up to 10 words per
 *     cluster, the filter's masks and bases, the scan's parts), on top of what the handle held before.
 *   Refused (TSDF_ERR_INVALID, with a message, before any device work where the host can tell): NULL dst or src; NULL vertices with
 *     n_vertices > 0, NULL indices with n_indices > 0; n_indices % 3 != 0; counts above 2^32 - 1; more than 2^30 vertices (the table's
 *     slots are numbered in 32 bits: simplify in boxes); cell_size not finite or not > 0; flags other than 0 (there are none yet);
 *     dst == src; handles made on different devices; an index >= n_vertices -- found on the device by the first kernel that reads I,
 *     before any lane uses it as an address: the call returns the error and dst is left empty.
 *   Out of scope: removing duplicate triangles, quadric error placement, edge collapse, preserving boundaries or manifoldness,
 *     simplifying inside tsdf_volume_extract_mesh, slab volumes (they have no indexed mesh).  Smoothing is the group "mesh smoothing"
 *     below. */
int tsdf_simplify_mesh_device(uint64_t n_vertices, uint64_t n_indices, const float *device_vertices, const uint32_t *device_indices,
                              const float *device_normals, const uint8_t *device_rgb, float cell_size, uint32_t flags, tsdf_mesh *dst,
                              void *hip_stream);
int tsdf_mesh_simplify(tsdf_mesh *src, float cell_size, uint32_t flags, tsdf_mesh *dst, void *hip_stream);

/* ---- mesh smoothing (no reference counterpart: the reference's soup goes to a file as it is) --------------------------------------- */
/* lambda|mu (Taubin) smoothing of an indexed mesh on the device, an option to pin its open border, and area-weighted vertex normals
 * from the faces: what takes the voxel-scale stair-stepping and the sensor noise out of an extracted surface (or of a clustered level
 * of detail of one) without the mesh leaving the device.  Opt-in by being called: no other entry point, launch or result changes.
 *   The result (unique values, whatever computes them), for n_vertices positions, n_indices indices (a multiple of 3), iterations, the
 *   fp32 factors lambda and mu, and flags:
 *   1. Loose vertices and live triples.  A vertex is LOOSE if any coordinate is not finite or any |V_a| is not < 2^21 (the
 *     simplification's test, in float, on the source positions, once).  An index triple is LIVE iff its three indices are pairwise
 *     different and none of its corners is loose; only live triples count, everywhere below, and a repeated live triple counts as often
 *     as it appears.  deg(v) = 2 x the live triples that name v.
 *   2. One pass with factor f.  Every vertex is computed from the previous pass's positions (Jacobi, never in place); a pass whose
 *     factor is exactly 0.0f or -0.0f is not run.  A vertex with deg(v) == 0, a loose vertex or a pinned vertex (4) keeps its 12
 *     bytes.  Otherwise, per axis: q(u) = llrintf(P_a(u) * 1024.0f) (the product is exact, the rounding to nearest-even); S the int64 sum
 *     of q(u1) + q(u2) over the live triples that name v, u1 and u2 the triple's other two corners; d = ((double)S / (double)deg) /
 *     1024.0; out = (float)((double)p + (double)f * (d - (double)p)), double arithmetic, no contraction, in exactly that order.
 *     Integers are summed, so no arrival order can change a sum: permuting the triples does not change a byte.  This is the umbrella
 *     operator weighted by edge multiplicity: an interior edge counts twice, a border edge once.
 *   3. Guard.  If any of the three out values is not finite or not < 2^21 in magnitude, the vertex keeps its previous position for
 *     this pass, all three coordinates.  So a position that is not loose stays below 2^21, q below 2^31, and no sum can overflow.
 *   4. TSDF_SMOOTH_PIN_BOUNDARY.  m{u, v} is the number of live triples that name both u and v; a vertex is PINNED iff it is an end of
 *     an edge with m == 1 (edges with m >= 3 do not pin).  Pins come from the source connectivity, once, and hold for all passes.  A
 *     mesh extracted in a box keeps the bytes of its open border, so neighbouring boxes still agree on the edges they share.
 *   5. The call runs `iterations` times: a pass with lambda, then a pass with mu.  iterations == 0, or both factors zero, gives dst
 *     equal to the source array for array.  dst receives the smoothed positions, the indices as the same bytes, colours where given as
 *     the same bytes, normals as the source's bytes where given -- with TSDF_SMOOTH_NORMALS they are (6) on the smoothed positions,
 *     whether or not the source had any, and dst->info.flags says so.  info.box is the source's (all zero for
 *     tsdf_smooth_mesh_device); dst is not labelled.
 *   6. Vertex normals from faces, area-weighted.  For a live triple A = V[I[3t]], B = V[I[3t+2]], C = V[I[3t+1]] (the wiring
 *     extract_surface uses); in double, without contraction, e1 = B - A, e2 = C - A, c = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z,
 *     e1.x e2.y - e1.y e2.x); k_a = llrint(c_a * 65536.0).  For each vertex d_a is the int64 sum of k_a over the live triples that
 *     name it, as a double; L = sqrt(d_x d_x + d_y d_y + d_z d_z), added left to right; the output is (float)(d_a / L), and a NaN
 *     triple when L == 0 (loose vertices, vertices no live triple names, faces that cancel).  On an extracted mesh the normal points
 *     out of the surface, like the field queries' unit gradient.  The 2^-16 quantisation is the price of order independence: it moves
 *     a component by a few 1e-7 at 10 mm voxels and a few 1e-4 at 0.5 mm voxels.  |c_a| is at most twice the product of two edge
 *     lengths, and a sum may wrap once the |c_a| round a vertex add up to 2^47: faces with edges below 2^16 units (65 m in mm) stay
 *     below 2^33 each, which leaves room for 2^14 of them round one vertex.
 *   tsdf_smooth_mesh_device: any arrays on the device (3 floats per vertex, one uint32 per index, 3 floats / 3 bytes per vertex or
 *     NULL).  tsdf_mesh_smooth: src's arrays, normals and colours where src has them.  tsdf_vertex_normals_device: (6) of any arrays
 *     into device_normals_out (3 floats per vertex); blocking, it holds 24 bytes per vertex + 8 of device scratch for the duration of
 *     the call; when it refuses an index the n_vertices triples hold unspecified values and nothing outside them has been touched.tsdf_mesh_compute_normals: (6) of the handle's own arrays; it replaces or creates the handle's normal array and sets
 *     TSDF_MESH_NORMALS (labels stay: the connectivity is untouched); blocking.
 *   How: neighbour rows are built once per call -- integer atomic counts, the chunk scan of the components filter, a fill with an
 *     atomic cursor that writes the other two corners of every live triple into each corner's row (the order inside a row is that of
 *     arrival, harmless because every sum is an integer sum).  Each pass is a gather without atomics, one lane per vertex, between two
 *     position buffers; a row of more than 64 pairs (a fan's hub) is walked by its whole wave.  Pins: the simplification's
 *     open-addressed table with the key (min << 32) | max and a count per slot, load <= 1/2, so no lane waits for another;
 *     slots counted once flag both ends.  Normals: nine 64-bit integer atomic adds per live triple.  No float is ever added atomically.
 *   Kernels are enqueued on hip_stream (NULL: the default stream) behind a pending extraction; at most one synchronisation, for the
 *     error word, after the rows are built; the call returns with the passes enqueued, and stream order is that of the components
 *     filter.  src and the volume are never written.  dst keeps its arrays and scratch and only grows them: a warm repeat allocates
 *     nothing.
 *   Scratch of a smoothing into dst, counted by tsdf_mesh_scratch_bytes(dst), with passes = iterations x the factors that are not
 *     zero (0 for a mesh without triples):
 *       16 (ceil(ceil(n_vertices / 64) / 1024) + 1) + 8                         the scan's parts and the error word, always
 *       + 8 n_vertices + 8 n_indices + 4 ceil(n_vertices / 64)                  passes > 0: row bounds, one pair per index, chunk bases
 *       + 12 n_vertices                                                         passes > 1: the second position buffer
 *       + n_vertices + 12 E                                                     passes > 0 with TSDF_SMOOTH_PIN_BOUNDARY: the pin flags and
 *                                                                               the edge table, E the smallest power of two >= 2 n_indices
 *       + 24 n_vertices                                                         TSDF_SMOOTH_NORMALS (and tsdf_mesh_compute_normals ON a handle)
 *     bytes, on top of what the handle held before (the edge table is the simplification's cell table: a handle that has both holds
 *     the larger).
 *   Refused (TSDF_ERR_INVALID, with a message, before any device work where the host can tell): NULL dst, src or mesh; NULL arrays
 *     with non-zero counts; n_indices % 3 != 0; counts above 2^32 - 1; lambda or mu not finite; iterations above 1024; unknown flags;
 *     dst == src; handles made on different devices; an index >= n_vertices -- found on the device by the first kernel that reads I,
 *     before any lane uses it as an address: the call returns the error and dst is left empty.  An empty source gives an empty dst;
 *     vertices with n_indices == 0 are legal.
 *   Out of scope: cotangent or other geometric weights, feature-preserving or bilateral mesh filters, smoothing the distance field,
 *     smoothing inside tsdf_volume_extract_mesh, in-place smoothing (dst == src), slab volumes, hole filling, removing duplicate
 *     triangles. */
#define TSDF_SMOOTH_PIN_BOUNDARY 1u
#define TSDF_SMOOTH_NORMALS 2u
int tsdf_smooth_mesh_device(uint64_t n_vertices, uint64_t n_indices, const float *device_vertices, const uint32_t *device_indices,
                            const float *device_normals, const uint8_t *device_rgb, uint32_t iterations, float lambda, float mu,
                            uint32_t flags, tsdf_mesh *dst, void *hip_stream);
int tsdf_mesh_smooth(tsdf_mesh *src, uint32_t iterations, float lambda, float mu, uint32_t flags, tsdf_mesh *dst, void *hip_stream);
int tsdf_vertex_normals_device(uint64_t n_vertices, uint64_t n_indices, const float *device_vertices, const uint32_t *device_indices,
                               float *device_normals_out, void *hip_stream);
int tsdf_mesh_compute_normals(tsdf_mesh *mesh, void *hip_stream);

/* ---- mesh rendering (no reference counterpart: the reference renders its volume, never a mesh) ------------------------------------- */
/* An indexed mesh rasterised from a pinhole camera into depth, vertex, normal, colour and triangle-id maps, on the device: the view of
 * a mesh that no longer matches a resident volume (simplified, smoothed, filtered, deformed, loaded, or paged out).  Opt-in by being
 * called: no other entry point, launch or result changes.  A volume is not an argument.
 *   The result (unique bytes, whatever computes them), for V (n_vertices float triples), I (n_indices uint32, a multiple of 3),
 *   optionally a normal (float triple) and a colour (3 bytes) per vertex, width, height, inv_pose[16] and k[9] (column-major), z_near,
 *   z_far and flags.  Triangle t has the corners (I[3t], I[3t+2], I[3t+1]), the wiring extract_surface uses; corner 0, 1, 2 below are
 *   those, in that order.  Every fp32 operation is rounded on its own (no contraction), in exactly the order written.
 *   1. Camera point, per shared vertex: c = world_to_camera(V[e], inv_pose) (cuda_coordinate_transforms.cu:108-121): each row
 *     ((m_i1 x + m_i2 y) + m_i3 z) + m_i4, then x, y, z each divided by w.  r = 1.0f / c.z.
 *   2. Screen point: sx = fx * (c.x / c.z) + cx, sy = fy * (c.y / c.z) + cy with fx = k[0], fy = k[4], cx = k[6], cy = k[7].  Pixel
 *     (i, j) has its centre at the screen point (i, j) (world_to_pixel's roundf).  X = (int32)rintf(sx * 256.0f), Y likewise.  A vertex
 *     is USABLE iff c is finite, z_near <= c.z <= z_far and |sx|, |sy| <= 2^20 (so |X|, |Y| <= 2^28).
 *   3. A triangle is LIVE iff its three indices are < n_vertices, its three corners are usable and
 *     A2 = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0), formed in 64 bits, is not 0.  With TSDF_RENDER_CULL_BACK also A2 < 0: that is the
 *     FRONT-FACING sign -- x to the right, y down, the camera looking along +z -- and the one extract_surface's wiring of a fused surface
 *     has when seen from outside through a rigid pose.  There is no near-plane clipping: a triangle with a corner that is not usable is
 *     dropped and counted (n_dropped).
 *   4. Coverage of pixel (i, j), at P = (256 i, 256 j): with s = sign(A2), for k = 0, 1, 2 and (A, B) = (P1, P2), (P2, P0), (P0, P1),
 *     E_k(P) = a_k P.x + b_k P.y + c_k, a_k = -s (B.y - A.y), b_k = s (B.x - A.x), c_k = s ((B.y - A.y) A.x - (B.x - A.x) A.y), all in
 *     64 bits; E_0 + E_1 + E_2 == |A2|.  The pixel is covered iff for every k: E_k > 0, or E_k == 0 and edge k is TOP-LEFT: a_k > 0, or
 *     a_k == 0 and b_k > 0.  Only pixels of the image inside the corners' bounding box are asked, so |P| <= 2^28 and every product stays
 *     below 2^58.  Two triangles that share an edge with opposite directions cover each centre on it exactly once.
 *   5. Depth: b1 = (float)E_1 / (float)|A2|, b2 = (float)E_2 / (float)|A2| (int64 to fp32, round to nearest even);
 *     rr = r0 + (b1 * (r1 - r0) + b2 * (r2 - r0)); z = 1.0f / rr.  A covered pixel yields a fragment iff z is finite and
 *     z_near <= z <= z_far.
 *   6. Visibility: a fragment's key is ((uint64)bits(z) << 32) | t; the pixel's winner is the smallest key over all its fragments
 *     (z > 0: the bits order like the values), so equal depths go to the smaller triangle index.  No fragment: a miss.
 *   7. Targets, each an optional device pointer of tsdf_render_targets, in pixel order y * width + x, of the winner:
 *     triangle (uint32) t, 0xFFFFFFFF on a miss.  z (fp32) the key's z, NaN on a miss.  depth (uint16) tsdf_vertices_to_depth_device's
 *     conversion of z: (uint16)roundf(z), 0 on a miss or outside 1..65535.
 *     With q1 = (b1 * r1) * z, q2 = (b2 * r2) * z and mix(a0, a1, a2) = a0 + (q1 * (a1 - a0) + q2 * (a2 - a0)) (perspective-correct):
 *     vertices (float triple) mix per component of the corners' world positions, a NaN triple on a miss: the layout of
 *     tsdf_raycast_device's vertex map, so it feeds tsdf_normals_device, ICP, the reach and object lookups.
 *     normals (float triple), with vertex normals: n = mix per component of the corners' normals, then n / L per component with
 *     L = sqrtf((n.x n.x + n.y n.y) + n.z n.z); a NaN triple if a component of n is not finite or L == 0.  Without vertex normals: the
 *     same normalisation of the face normal u x w = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x), u = V1 - V0, w = V2 - V0
 *     in fp32: it points out of a fused surface, as the field queries' unit gradient does.  NaN triple on a miss.
 *     rgb (3 bytes): per channel f = mix of the corners' bytes as floats, + 0.5f, then 0 unless f > 0, 255 where f > 255, truncated;
 *     (0, 0, 0) on a miss.
 *   8. tsdf_render_info: n_triangles = n_indices / 3; n_live (3); n_dropped: triangles with valid indices and a corner that is not
 *     usable; n_large: live triangles whose clipped pixel box held more than TSDF_RENDER_LARGE_BOX pixels (tsdf_render_set_large_box; they take
 *     render_large_kernel; scheduling only); n_pixels_hit.  Integer atomics, one per counter and workgroup, read through a pinned
 *     mirror.  A render synchronises only when `info` is not NULL; tsdf_render_get_info waits for the last render and gives the same.
 *   An index >= n_vertices is found on the device before it is used as an address (its triangle is dead) and reported as
 *     TSDF_ERR_INVALID by the next call that waits: the render itself when info is given, tsdf_render_get_info, tsdf_mesh_render.  The
 *     targets then hold the render of the other triangles.  With n_vertices == 0 any index is refused on the host.  An empty mesh is a
 *     successful render of all misses.
 *   tsdf_render_mesh_device: any arrays on the device, device targets, enqueued on hip_stream (NULL: the default stream).
 *     tsdf_mesh_render_device: a mesh handle's arrays (normals and colours where it has them), ordered behind its pending work; the
 *     mesh is not written.  tsdf_mesh_render: the same into host arrays, blocking.
 *   The handle begins with the stream order every handle has; it owns its scratch, which only grows: 8 bytes per pixel (the keys), 16
 *     bytes per shared vertex ({X, Y, r, usable}), 4 bytes per triangle + 4 (the large list), 40 bytes of counters
 *     (tsdf_render_scratch_bytes).  A warm repeat allocates nothing.  A handle is used by one thread at a time, on its device.
 *   How: render_project_kernel, a lane per shared vertex; the keys set to all ones by a memset; render_raster_kernel, a lane per
 *     triangle walking its box; render_large_kernel, a wave per listed triangle in 8 x 8 tiles; render_resolve_kernel, a lane per
 *     pixel.  Visibility is one 64-bit atomicMin without return per fragment, behind a plain load and a skip when the fragment's key
 *     is not smaller (words only fall).  No float atomics, no compare-and-swap loop, no lane waits for another.
 *   Refused (TSDF_ERR_INVALID, with a message, before any device work): NULL handle, mesh, targets, arrays with non-zero counts or
 *     matrices; n_indices % 3 != 0; counts above 2^32 - 1; an image of no pixels or of 2^32 - 1 or more; a matrix entry that is not
 *     finite; a k whose other entries differ from (0, 0, 0, 0, 1); z_near or z_far not finite, z_near <= 0, z_near > z_far; unknown
 *     flags; an rgb target for a mesh without colours; handles made on different devices.
 *   Out of scope: near-plane clipping, several meshes in one key buffer, anti-aliasing, general cameras, textures, use inside the
 *     tracker or the pipeline, visibility for the scene-flow correspondence. */
typedef struct tsdf_render tsdf_render;
#define TSDF_RENDER_CULL_BACK 1u
#define TSDF_RENDER_LARGE_BOX 256u
typedef struct tsdf_render_targets {
    uint32_t *triangle;
    float *z;
    uint16_t *depth;
    float *vertices;
    float *normals;
    uint8_t *rgb;
} tsdf_render_targets;
typedef struct tsdf_render_info {
    uint64_t n_triangles, n_live, n_dropped, n_large, n_pixels_hit;
} tsdf_render_info;
int tsdf_render_create(tsdf_render **out);   /* on the current device */
void tsdf_render_destroy(tsdf_render *render);
int tsdf_render_scratch_bytes(const tsdf_render *render, uint64_t *bytes);
int tsdf_render_get_info(const tsdf_render *render, tsdf_render_info *info);
/* Scheduling only: from how many pixels of its clipped box on a live triangle goes to render_large_kernel (TSDF_RENDER_LARGE_BOX when the
 * handle is made; 0xFFFFFFFF: every triangle stays on the lane path).  No target changes by a byte; n_large counts by this value. */
int tsdf_render_set_large_box(tsdf_render *render, uint32_t pixels);
int tsdf_render_mesh_device(tsdf_render *render, uint64_t n_vertices, uint64_t n_indices, const float *device_vertices,
                            const uint32_t *device_indices, const float *device_normals, const uint8_t *device_rgb, uint32_t width,
                            uint32_t height, const float inv_pose[16], const float k[9], float z_near, float z_far, uint32_t flags,
                            const tsdf_render_targets *device_targets, tsdf_render_info *info, void *hip_stream);
int tsdf_mesh_render_device(tsdf_render *render, tsdf_mesh *mesh, uint32_t width, uint32_t height, const float inv_pose[16],
                            const float k[9], float z_near, float z_far, uint32_t flags, const tsdf_render_targets *device_targets,
                            tsdf_render_info *info, void *hip_stream);
int tsdf_mesh_render(tsdf_render *render, tsdf_mesh *mesh, uint32_t width, uint32_t height, const float inv_pose[16], const float k[9],
                     float z_near, float z_far, uint32_t flags, const tsdf_render_targets *host_targets, tsdf_render_info *info);

/* ---- scene flow (replaces the device part of process_frames, src/SceneFusion/SceneFusion_krnl.cu:235-401) ------------------------- */
/* One frame of the reference's non-rigid step: the mesh vertices a depth frame sees take the scene flow at their pixel, and the flow
 * is pushed into the deformation nodes of the two voxels that bracket each vertex -- the reference's update made deterministic.  Opt-in
 * by being called: a volume on which these are never called allocates and launches nothing new.
 *   Inputs: a whole volume; a mesh handle holding an indexed extraction of that volume's WHOLE grid (tsdf_volume_extract_mesh with a
 *     NULL box: V, I and the handle's per-64-voxel edge records are used); a depth image (uint16, width * height, 0 = invalid); a
 *     scene-flow image (width * height float triples, row major, world units); pose, inv_pose, k, kinv as tsdf_integrate takes them;
 *     threshold > 0 (the reference hard-codes 10).
 *   The result (a unique set of bits, whatever computes it; all arithmetic fp32, every operation rounded on its own):
 *   1. Correspondence (find_mesh_vertex_correspondences, :74-114).  For shared vertex e with position p: pix = world_to_pixel(p,
 *     inv_pose, k) in the reference's operation order (src/Utilities/cuda_coordinate_transforms.cu:10-30; roundf, saturating
 *     conversion, NaN -> 0).  e corresponds iff pix is inside the image, the depth there is > 0 and
 *     fabsf(pixel_to_world(pix, pose, kinv, depth).z - p.z) < threshold (:40-67, its division by w included) -- and, ours, the flow
 *     triple at pix is finite in all three components.  Its pixel index is pix.y * width + pix.x.
 *     TSDF_SCENE_FLOW_DEFORMED: p is V[e] pushed through the volume's current deformation first (the arithmetic of
 *     tsdf_volume_deform_points_device, global rotation and translation included, on a scratch copy: the handle's vertices do not
 *     change) -- what the second and later frames of a sequence need.  Without it p is the canonical vertex, as in the reference.
 *   2. Multiplicity.  m(e) = the number of k with I[k] == e: the soup vertices on edge e (the reference counts soup vertices,
 *     src/MarchingCubes/MarkAndSweepMC.cu:297-298).  count[v] = the sum of m(e) over the up to six used edges that end in voxel v.
 *   3. Update.  For every voxel v with count[v] > 0, its incident edges taken in the order -x, +x, -y, +y, -z, +z: acc = 0; for
 *     every used incident edge that corresponds, per component, acc = acc + (float)m(e) * flow[pix(e)]; then
 *     translation = translation + (1.0f / (float)count[v]) * acc.  rotation is untouched; a node none of whose edges corresponds
 *     keeps its bytes.  This is the reference's sum with one thread running at a time, up to the order of the additions.
 *   Side effects: the node array is materialised as tsdf_volume_deformation does it, a brick list prepared ahead is discarded as
 *     tsdf_volume_set_deformation does it.  Distances, weights and colours are never written.
 *   info (may be NULL): the mesh's vertices, the vertices that correspond, the nodes written (those with a corresponding edge).
 *   How: one lane per vertex finds its pixel; integer atomic adds over I count m; one wave per 64-voxel record GATHERS each voxel's
 *     six edges from mask bits (an edge's vertex index is a base plus popcounts, as in the extraction), so every node has one writer
 *     and no float is added atomically; a wave with no used edge near its 64 voxels leaves after reading the masks.  The same bytes on
 *     every run.
 *   Scratch lives in the mesh handle, only grows and is counted by tsdf_mesh_scratch_bytes: 8 bytes per vertex (pixel index and
 *     multiplicity), 12 more per vertex once TSDF_SCENE_FLOW_DEFORMED was asked for, 16 bytes of counters; the host variant also
 *     keeps its uploads of the two images (14 bytes per pixel).
 *   Stream order: tsdf_volume_apply_scene_flow uploads and enqueues on the volume's stream.  tsdf_volume_apply_scene_flow_device
 *     enqueues on hip_stream (NULL: the default stream) behind the handle's pending extraction; ordering hip_stream against other
 *     work on the volume's stream is the caller's.  Either synchronises its stream once, to read the info; with info == NULL the
 *     device variant returns with its kernels enqueued.  (The first call on a volume whose nodes are still implicit also waits for
 *     their materialisation, as tsdf_volume_deformation does.)  A later extraction into the handle is ordered behind the kernels.
 *   Refused (TSDF_ERR_INVALID, with a message, before any device work): NULL arguments other than info; a Z-slab volume; a mesh that
 *     is not a whole-grid extraction of a volume of these dimensions (a box, a filter's or a simplification's output, a handle never
 *     extracted into); a non-finite matrix entry; a threshold that is not > 0 (NaN included); unknown flags; an image of no pixels or
 *     of 2^32 - 1 or more; handles made on different devices; TSDF_SCENE_FLOW_DEFORMED with more than 2^31 - 1 vertices.  An empty mesh
 *     is a successful no-op: nothing is allocated, launched or materialised, the info is all zero.
 *   Out of scope: the SceneFusion class, RGBDDevice and MockKinect, the scene-flow file loaders and TinyXml, rotations of nodes, ray
 *     casts in the deformed space, use inside the tracker or kinfu_stream. */
#define TSDF_SCENE_FLOW_DEFORMED 1u
typedef struct tsdf_scene_flow_info {
    uint64_t n_vertices, n_correspondences, n_nodes_moved;
} tsdf_scene_flow_info;
int tsdf_volume_apply_scene_flow(tsdf_volume *volume, tsdf_mesh *mesh, const uint16_t *host_depth, const float *host_flow, uint32_t width,
                                 uint32_t height, const float pose[16], const float inv_pose[16], const float k[9], const float kinv[9],
                                 float threshold, uint32_t flags, tsdf_scene_flow_info *info);
int tsdf_volume_apply_scene_flow_device(tsdf_volume *volume, tsdf_mesh *mesh, const uint16_t *device_depth, const float *device_flow,
                                        uint32_t width, uint32_t height, const float pose[16], const float inv_pose[16], const float k[9],
                                        const float kinv[9], float threshold, uint32_t flags, tsdf_scene_flow_info *info, void *hip_stream);

/* ---- distance field (no reference counterpart: the reference's volume knows the truncated, projective distance only) ------------- */
/* The Euclidean signed distance field (ESDF) of a whole volume: per voxel, how far the nearest surface is -- what a planner, a
 * collision checker or a gripper asks -- computed on the device from the distances and weights where they lie.  Opt-in by being
 * called: a volume on which these are never called does exactly what it did.
 *   The value (a unique set of bits, whatever computes it): X x Y x Z voxels, voxel sizes vs[a] (the fp32 values of tsdf_volume_info),
 *     distances d, weights w as every accessor reports them (the same in 8-bit, 16-bit and fp32 storage).
 *     observed(v): w(v) > 0 (a NaN weight is not observed).  neg(v): d(v) < 0, the mesh's sign test (NaN and both zeros are not negative).
 *     site(v): observed(v), and some 6-neighbour u inside the grid has observed(u) and neg(u) != neg(v): the ends of the lattice edges
 *       the surface crosses between two OBSERVED voxels.  An observed / unobserved boundary is not a surface.
 *     A[a] = vs[a] * vs[a] (one fp32 multiply).  For a voxel v and a site s with integer index differences dx, dy, dz the fp32 cost,
 *       every operation rounded on its own, is
 *           c(v, s) = A[2]*(float)(dz*dz) + (A[1]*(float)(dy*dy) + A[0]*(float)(dx*dx))
 *       (the integer squares are exact in fp32: an axis longer than 4096 is refused).
 *     q(v) = min over all sites of c(v, s), +inf when there are none.  e(v) = sqrtf(q(v)), correctly rounded; if !(e < max_distance),
 *       e = max_distance.  max_distance only caps: it never changes a value below it.
 *     Output: one fp32 per voxel in the volume's index order x + y X + z X Y: -e for an observed voxel with neg, +e for an observed
 *       voxel without, NaN for an unobserved voxel (+e with TSDF_ESDF_FILL_UNKNOWN).  A site gets -+0.0 by the same rule.
 *     The minimum is separable -- fp32 addition is monotone, so the minimum commutes with it -- and three passes along x, y and z give
 *       exactly q.
 *   Accuracy of the definition: sites are voxel centres next to the surface, not the surface, so against the true distance t to the
 *     surface -max(vs) <= e - t <= |vs| (the voxel diagonal); -0.996 and +0.40 voxels measured on a sphere.  Within a voxel of the
 *     surface the TSDF itself (tsdf_volume_sample_field) is the better answer.
 *   max_distance: mm, > 0; INFINITY means no cap, and a volume without sites then gives +inf (or NaN).
 *   The handle owns the output array and its scratch and keeps both between calls; both only grow, so a warm recompute allocates
 *     nothing.  It snapshots the geometry (sizes, voxel sizes, offset), so sampling needs no volume and survives the volume's
 *     destruction.  A handle is used by one thread at a time, on the device it was made on.  Scratch besides the 4 bytes a voxel of
 *     output: at most 4 bytes a voxel + 64 KiB (tsdf_esdf_scratch_bytes).
 *   Stream order: tsdf_volume_compute_esdf enqueues on the volume's stream and returns; tsdf_esdf_get_info, tsdf_esdf_buffer,
 *     tsdf_esdf_download and tsdf_esdf_sample wait for it, tsdf_esdf_sample_device orders its stream behind it.  n_sites is counted
 *     with an integer atomic; the distance array has one writer per word and is the same on every run.
 *   The volume is not written: no distance, weight, weight storage mode, occupancy flag, dirty mark or ray-cast state.
 *   Refused (TSDF_ERR_INVALID, with a message): NULL arguments; a Z-slab volume; a materialised deformation-node array; max_distance
 *     that is not > 0 (NaN included); unknown flags; an axis longer than 4096; sampling or downloading a handle that has never been
 *     computed.  tsdf_esdf_destroy(NULL) is ignored.
 *   tsdf_esdf_sample[_device]: the trilinear distance and the central-difference gradient of the ESDF at world points, in the frame of
 *     the field queries (p - offset, the snapshot's offset), by the field queries' own kernel on the ESDF array: bit for bit what
 *     tsdf_volume_sample_field_device returns on a volume of the same geometry whose distance array holds the ESDF -- the same valid(q),
 *     NaN outside, TSDF_FIELD_UNIT_GRADIENT, NULL-output and n == 0 rules.  NaN taps (unknown voxels) propagate; that is intended.
 *   Out of scope: incremental updates, a box of the grid, Z-slabs, sub-voxel site positions, keeping TSDF values inside the band. */
typedef struct tsdf_esdf tsdf_esdf;
#define TSDF_ESDF_FILL_UNKNOWN 1u
typedef struct tsdf_esdf_info {
    uint32_t size[3];
    uint32_t flags;
    float voxel_size[3];
    float offset[3];        /* the volume's current offset when computed */
    float max_distance;
    uint64_t n_sites;
} tsdf_esdf_info;
int tsdf_esdf_create(tsdf_esdf **out);   /* on the current device */
void tsdf_esdf_destroy(tsdf_esdf *esdf);
int tsdf_volume_compute_esdf(const tsdf_volume *volume, float max_distance, uint32_t flags, tsdf_esdf *esdf);
int tsdf_esdf_get_info(const tsdf_esdf *esdf, tsdf_esdf_info *info);
/* The device array of the last computation (NULL before the first); valid until the next computation into the handle. */
int tsdf_esdf_buffer(const tsdf_esdf *esdf, const float **device_distance);
/* Blocking copy to size[0] * size[1] * size[2] floats. */
int tsdf_esdf_download(const tsdf_esdf *esdf, float *host_distance);
/* n points (3 floats each) -> distance (n floats), gradient (3 n floats); either may be NULL, not both. */
int tsdf_esdf_sample_device(const tsdf_esdf *esdf, uint64_t n, const float *device_points, float *device_distance,
                            float *device_gradient, int flags, void *hip_stream);
/* The same on host arrays; blocking. */
int tsdf_esdf_sample(const tsdf_esdf *esdf, uint64_t n, const float *host_points, float *host_distance,
                     float *host_gradient, int flags);
/* Device bytes the handle holds besides the output array. */
int tsdf_esdf_scratch_bytes(const tsdf_esdf *esdf, uint64_t *bytes);

/* ---- exploration (no reference counterpart: the reference's volume is asked about its surface only) -------------------------------- */
/* What has not been seen yet, and from where could it be seen?  The free voxels that border unseen space (frontiers), their connected
 * clusters, and the number of unseen voxels a set of rays would pass through (view gain) -- what a robot's next-best-view planner, a
 * "scan here next" hint or a coverage report asks.  Opt-in by being called: no other entry point, launch or result changes; distances,
 * weights, colours, classes, occupancy flags and counters are never written.  Results are integers and sets only (unique values,
 * whatever computes them); two runs give the same bytes.
 *   1. Voxel states.  X x Y x Z voxels, voxel (x, y, z) has id (z * Y + y) * X + x (uint32: more than 2^32 - 1 voxels are refused);
 *      distances d and weights w as every accessor reports them (the same in 8-bit, 16-bit and fp32 storage).
 *        UNKNOWN(v):  not w(v) > 0 (a NaN weight is unknown).
 *        OCCUPIED(v): w(v) > 0 and d(v) < 0 -- the mesh's and the distance field's sign test: NaN and both zeros are not negative.
 *        FREE(v):     otherwise.
 *        FRONTIER(v): FREE(v) and at least one of the six face neighbours INSIDE the grid is UNKNOWN.  The grid border is not unknown
 *                     space: a neighbour outside the grid counts for nothing.
 *   2. tsdf_volume_find_frontiers fills the handle with the list of the ids of all frontier voxels in ascending order, and with the
 *      whole-grid counts n_unknown, n_free, n_occupied (they sum to X * Y * Z) and n_frontiers (the length of the list).  It also
 *      keeps, per 64 consecutive voxel ids, the 64-bit mask of the frontier voxels among them (bit l: id 64 c + l) and the list index of
 *      the chunk's first frontier (the base): a listed voxel's list index is base[id / 64] + popcount(mask[id / 64] & ((1 << id % 64) - 1)),
 *      and a voxel is listed iff its mask bit is set.  It runs on the volume's stream and waits for it once, to size the list.
 *   3. tsdf_explorer_cluster_frontiers labels the listed voxels.  Two listed voxels are adjacent when their coordinates differ by at
 *      most 1 on every axis and, at connectivity 6, on exactly one axis (face neighbours); at 26 on one, two or three axes (face, edge
 *      and corner neighbours).  A cluster is a connected set of that graph.
 *        L[i] (uint32, one per listed voxel): the smallest LIST INDEX in the cluster of list entry i.
 *        Per cluster: label = that smallest index, size = its number of voxels, lo[k] / hi[k] = the smallest / largest coordinate on
 *          axis k (the inclusive box; k = 0, 1, 2 for x, y, z), sum[k] = the integer sum of the coordinates on axis k -- the centroid
 *          in voxel units is sum[k] / size, exact for whoever divides; its world position is offset[k] + (sum[k] / size + 0.5) * voxel_size[k].
 *        The table holds one tsdf_frontier_cluster row per cluster with size >= min_size, in ascending label.  info.n_clusters counts
 *          all clusters, info.n_listed_clusters the rows; info.connectivity is the connectivity last used (0: not clustered).
 *      It runs on hip_stream behind the handle's pending work and waits for it once, to size the table.  How: the lock-free union-find
 *      of "mesh components" over the list indices (hooks towards the smaller index), a lane per listed voxel uniting
 *      with its 3 or 13 forward neighbours found through mask and base; sizes, sums and boxes by integer atomics.
 *   4. View gain: n rays of the caller's own, in the ray frame of "ray queries": origins and directions are 3 n floats in world
 *      millimetres, the volume's CURRENT offset is the grid's lower corner, the direction is used AS GIVEN and t is in units of it.
 *      Every fp32 operation below is rounded on its own.  With o, d the origin and direction of ray i, offset and vs the volume's
 *      offset and voxel size, N = (X, Y, Z):
 *        a. The ray is SKIPPED (stop = 0, both counts 0) if a component of o or d is not finite; if d is all zeros (-0.0 included);
 *           if t_max[i] is NaN or <= 0 (t_max NULL: +inf for every ray); or if any a_k or s_k of b. is not finite.
 *        b. a_k = (o_k - offset_k) / vs_k, s_k = d_k / vs_k: the ray in voxel units, position a + t s.
 *        c. Clip: t0 = 0, t1 = t_max[i].  Per axis k = x, y, z in turn: if s_k == 0, the ray is skipped unless 0 <= a_k < (float)N_k;
 *           otherwise ta = (0 - a_k) / s_k, tb = ((float)N_k - a_k) / s_k, t0 = fmaxf(t0, fminf(ta, tb)), t1 = fminf(t1, fmaxf(ta, tb)).
 *           Then the ray is skipped unless t0 < t1.
 *        d. Start voxel: i_k = clamp((int)floorf(a_k + t0 * s_k), 0, N_k - 1) (the conversion saturates, NaN gives 0).  Per axis
 *           step_k = +1 if s_k > 0 else -1, ahead_k = 1 if s_k > 0 else 0.
 *        e. Walk, at most X + Y + Z voxels.  Visit the current voxel (f.).  Then the next boundary per axis with s_k != 0 is
 *           tn_k = ((float)(i_k + ahead_k) - a_k) / s_k; the smallest wins, x before y before z on ties (y replaces x, and z the
 *           winner so far, only if strictly smaller).  The walk ends if no axis has s_k != 0, if the winner's tn > t1, or if
 *           i_k + step_k of the winning axis leaves [0, N_k); otherwise i_k += step_k and the next voxel is visited.
 *        f. A visited voxel that is UNKNOWN: unknown[i] += 1, and the voxel's bit is set in a mask of one bit per voxel id that the
 *           handle keeps.  OCCUPIED: the walk stops, stop[i] = 2, the voxel is counted nowhere.  FREE: free[i] += 1.  A walk that
 *           ends in any other way (e., or the visit limit) has stop[i] = 1.
 *        g. *host_gain = the number of set bits of the mask after the call: a voxel seen by many rays counts once.  The mask is
 *           zeroed before the rays are walked unless TSDF_GAIN_KEEP_MASK is given; with it successive calls accumulate (the union), so
 *           a greedy planner asks what a view adds to the views already chosen.  (A handle's first call, and the first after a
 *           tsdf_volume_find_frontiers of another grid size, start from an empty mask either way.)
 *      Any of unknown, free, stop and host_gain may be NULL, not all four.  The call enqueues on the volume's stream; with host_gain it
 *      waits for it once, like tsdf_volume_fuse with fused_voxels.  n == 0 is TSDF_OK: no ray is walked (the mask is still zeroed or
 *      kept, and counted when host_gain is given).
 *   The handle (tsdf_explorer_create, on the current device) owns the list, the masks and bases, the labels, the table and the gain
 *     mask, keeps them between calls and only grows them: a warm second call allocates nothing.  It remembers the geometry (sizes,
 *     voxel sizes, offset) of the last tsdf_volume_find_frontiers, or of its first view gain, so nothing downstream needs the volume.
 *     Scratch: 12 bytes per 64 voxels for masks and bases (3/16 byte a voxel) and 1 bit a voxel for the gain mask; clustering adds
 *     56 bytes per listed voxel and 12 per 64 of them (tsdf_explorer_scratch_bytes: everything but the list, the labels and the table).
 *     A handle is used by one thread at a time.  tsdf_explorer_destroy(NULL) is ignored.
 *   tsdf_explorer_frontier_buffers: the device arrays (any pointer may be NULL; the list is NULL when it is empty);
 *     tsdf_explorer_frontier_download copies the list (n_frontiers words).  tsdf_explorer_cluster_buffers gives the labels (n_frontiers
 *     words) and the table (n_listed_clusters rows), NULL where empty; tsdf_explorer_cluster_download copies them (either pointer may be
 *     NULL).  All four wait for the handle's pending work.  The frontier pair refuses a handle without a tsdf_volume_find_frontiers, the
 *     cluster pair one not clustered since its last tsdf_volume_find_frontiers.
 *   Refused (TSDF_ERR_INVALID, with a message naming the entry point): NULL handles or volumes; a Z-slab volume; a materialised
 *     deformation-node array; unknown flags; a connectivity other than 6 or 26; clustering before any tsdf_volume_find_frontiers; NULL
 *     origins or directions with n > 0; all four outputs NULL; more rays than a launch holds (n > (2^31 - 1) * 256); a view gain with
 *     a handle whose geometry (sizes, voxel sizes, offset) is not the volume's, unless the handle is fresh -- it then adopts the volume's.
 *   Out of scope: frontiers inside the pipeline step or the tracker, Z-slabs, incremental updates, and planning itself. */
typedef struct tsdf_explorer tsdf_explorer;
#define TSDF_GAIN_KEEP_MASK 1u
typedef struct tsdf_explorer_info {
    uint32_t size[3];
    uint32_t connectivity;   /* of the last clustering; 0: not clustered since the last tsdf_volume_find_frontiers */
    float voxel_size[3];
    float offset[3];         /* the volume's current offset when the geometry was taken */
    uint64_t n_unknown, n_free, n_occupied, n_frontiers;
    uint64_t n_clusters, n_listed_clusters;
} tsdf_explorer_info;
typedef struct tsdf_frontier_cluster {
    uint32_t label, size;
    uint32_t lo[3], hi[3];
    uint64_t sum[3];
} tsdf_frontier_cluster;
int tsdf_explorer_create(tsdf_explorer **out);   /* on the current device */
void tsdf_explorer_destroy(tsdf_explorer *explorer);
int tsdf_volume_find_frontiers(const tsdf_volume *volume, uint32_t flags /* none defined: 0 */, tsdf_explorer *explorer);
int tsdf_explorer_get_info(const tsdf_explorer *explorer, tsdf_explorer_info *info);
int tsdf_explorer_frontier_buffers(const tsdf_explorer *explorer, const uint32_t **device_voxels, const uint64_t **device_masks,
                                   const uint32_t **device_bases);
int tsdf_explorer_frontier_download(const tsdf_explorer *explorer, uint32_t *host_voxels);
/* Device bytes the handle holds besides the list, the labels and the table. */
int tsdf_explorer_scratch_bytes(const tsdf_explorer *explorer, uint64_t *bytes);
int tsdf_explorer_cluster_frontiers(tsdf_explorer *explorer, uint32_t connectivity, uint32_t min_size, void *hip_stream);
int tsdf_explorer_cluster_buffers(const tsdf_explorer *explorer, const uint32_t **device_labels,
                                  const tsdf_frontier_cluster **device_clusters);
int tsdf_explorer_cluster_download(const tsdf_explorer *explorer, uint32_t *host_labels, tsdf_frontier_cluster *host_clusters);
/* Device arrays for the rays and the per-ray outputs; host_gain is a host pointer. */
int tsdf_volume_view_gain_device(const tsdf_volume *volume, tsdf_explorer *explorer, uint64_t n, const float *device_origins,
                                 const float *device_directions, const float *device_t_max /* n floats, or NULL = no limit */,
                                 uint32_t flags, uint32_t *device_unknown, uint32_t *device_free, uint8_t *device_stop,
                                 uint64_t *host_gain);
/* The same on host arrays, on the volume's stream; blocking. */
int tsdf_volume_view_gain(const tsdf_volume *volume, tsdf_explorer *explorer, uint64_t n, const float *host_origins,
                          const float *host_directions, const float *host_t_max, uint32_t flags, uint32_t *host_unknown,
                          uint32_t *host_free, uint8_t *host_stop, uint64_t *host_gain);

/* ---- reachability (no reference counterpart: the reference's volume is asked about its surface only) ------------------------------- */
/* Can I get there, how far is it, and along which voxels?  The travel cost from seed points through free space to every voxel, the
 * voxel path from any goal back to a seed, and the nearest voxel of every frontier cluster -- what a robot asks between "which frontier?"
 * (group "exploration") and "go".  Opt-in by being called: no other entry point, launch or result changes; nothing of a volume, an ESDF
 * or an explorer is written.  Results are integers and sets only (unique values, whatever computes them); two runs give the same bytes.
 *   1. Grid, ids and voxel states are those of "exploration" rule 1: voxel (x, y, z) has id (z * Y + y) * X + x (uint32: more than
 *      2^32 - 1 voxels are refused), and UNKNOWN / OCCUPIED / FREE are as defined there.
 *   2. TRAVERSABLE(v): FREE(v) -- with TSDF_REACH_THROUGH_UNKNOWN also UNKNOWN(v) -- and, if an ESDF handle is given, its value at v
 *      satisfies e(v) >= clearance (an fp32 compare: NaN fails, so a planner that is optimistic about unseen space passes an ESDF
 *      computed with TSDF_ESDF_FILL_UNKNOWN).  Without an ESDF handle clearance must be 0.
 *   3. Steps.  Two voxels u != v are neighbours when their coordinates differ by at most 1 on every axis; the step is a face, edge or
 *      corner step for a difference on 1, 2 or 3 axes.  At connectivity 6 only face steps exist, at 26 all three.  A step u <-> v is
 *      ADMISSIBLE iff every voxel w with w_k in {u_k, v_k} on each axis k is TRAVERSABLE -- 2, 4 or 8 voxels, all inside the grid by
 *      construction: no corner cutting, a diagonal never squeezes between two blocked voxels.  The graph is undirected.  A step costs
 *      TSDF_REACH_COST_FACE 10, TSDF_REACH_COST_EDGE 14 or TSDF_REACH_COST_CORNER 17: tenths of a voxel step in the 10-14-17 chamfer
 *      metric.  For isotropic voxels cost * voxel_size / 10 is a length in mm.  Its error, derived: a path's cost is its own polyline's
 *      length with 14 for 10 sqrt 2 and 17 for 10 sqrt 3, so cost / 10 lies in [17 / (10 sqrt 3), 1] = [0.9815, 1] times that length in
 *      voxels; and a straight run in free space along a direction with sorted components a >= b >= c >= 0 costs 10 a + 4 b + 3 c against
 *      10 sqrt(a^2 + b^2 + c^2), a ratio between 0.9815 (at (1, 1, 1); the minimum over the cone is on an extreme ray: 1, 0.98995, 0.9815)
 *      and sqrt(1 + 0.16 + 0.09) = 1.1180 (Cauchy-Schwarz, at (1, 0.4, 0.3)): -1.9 % .. +11.8 % of the Euclidean distance.  For
 *      anisotropic voxels the cost is a step count only.
 *   4. Seeds: n world points (3 n floats) in the frame of view-gain rays ("exploration" rule 4b).  Seed voxel i_k =
 *      floorf((p_k - offset_k) / vs_k) with the volume's CURRENT offset, every fp32 operation rounded on its own.  A seed is ignored if a
 *      coordinate is not finite, an index is off the grid, or its voxel is not TRAVERSABLE.  n == 0, or all seeds ignored, is TSDF_OK:
 *      nothing is then reached.
 *   5. Cost field.  D(v) = the minimum over all paths of admissible steps from any seed voxel to v of the sum of the step costs; D = 0 at
 *      seed voxels.  cap = max_cost if nonzero, else 0xFFFFFFFE.  The output, one uint32 per voxel id, is D(v) if v is reachable and
 *      D(v) <= cap, otherwise TSDF_REACH_UNREACHED (0xFFFFFFFF).  The cap never changes a value at or below it.
 *   6. tsdf_reach_info: sizes, voxel sizes and offset as tsdf_explorer_info has them; connectivity, flags, clearance and max_cost as
 *      given; n_traversable; n_reached (voxels with an output other than UNREACHED); n_seed_voxels (voxels with output 0);
 *      max_cost_reached (the largest output other than UNREACHED, 0 if none); rounds.  All are unique integers except rounds: a
 *      diagnostic of the implementation that may differ from run to run and is excluded from every byte comparison.
 *   7. Lookup: n world points, each resolved to a voxel by rule 4's expression with the handle's remembered geometry; the output is
 *      that voxel's value, UNREACHED for a coordinate that is not finite or an index off the grid.  n == 0 launches nothing.
 *   8. Paths: n goal points, each mapped to a voxel as in rule 7, and a row capacity max_len.  For goal i: if its voxel is off the
 *      grid or UNREACHED, length[i] = 0.  Otherwise, starting at v = the goal voxel, while out(v) != 0, move to the FIRST neighbour u such
 *      that the step is admissible and out(u) + cost(u, v) == out(v), in the fixed neighbour order dz = -1, 0, 1 outermost, then dy,
 *      then dx innermost, (0, 0, 0) skipped, at connectivity 6 only the face offsets.  length[i] is the number of voxels of the whole
 *      path, goal and seed voxel included; the first min(length[i], max_len) ids, goal first, are written to row i (max_len words a
 *      row) and the rest of the row is left as it was.  Such a neighbour always exists for a reached voxel that is no seed, and the
 *      walk takes at most out(goal) / 10 steps.  The connectivity is that of the computation.
 *   9. Ranking frontier clusters: an explorer handle that has been clustered (tsdf_explorer_cluster_frontiers) and whose geometry
 *      equals the reach handle's.  For each row of its cluster table, in table order, one 16-byte tsdf_reach_cluster {label, cost,
 *      voxel, reserved = 0}: (cost, voxel) is the lexicographic minimum over the cluster's member voxels of (out(id), id), and
 *      (UNREACHED, 0xFFFFFFFF) when no member was reached.  What a next-best-view loop sorts by; one paths call on the centres of the
 *      `voxel`s then gives the routes.
 *  10. The handle (tsdf_reach_create, on the current device) owns the cost array (4 bytes a voxel) and its scratch, keeps them between
 *      calls and only grows them: a warm second computation allocates nothing and leaves tsdf_reach_scratch_bytes unchanged.  Scratch:
 *      1 bit a voxel (the traversable mask), 8 bytes per brick of 8^3 voxels, 8 bytes per ranked cluster row, 160 bytes of counters.
 *      It snapshots the geometry, so lookup, paths and ranking need no volume.  A handle is used by one thread at a time.
 *      tsdf_reach_destroy(NULL) is ignored.
 *  11. Stream order: tsdf_volume_compute_reach[_device] runs on the volume's stream -- a tsdf_volume_compute_esdf enqueued before it is
 *      therefore ordered -- and returns when the field is final (it reads a convergence word anyway).  The _device lookup / paths / rank
 *      calls order their stream behind the handle's event; ranking waits for the explorer's pending work first.  Host variants block.
 *  12. Refused (TSDF_ERR_INVALID, with a message naming the entry point, before any device work where possible): NULL handle or volume;
 *      NULL seeds with n > 0; a Z-slab volume; a materialised deformation-node array; connectivity other than 6 or 26; unknown flags;
 *      a clearance that is negative, not finite, or nonzero without an ESDF; an ESDF never computed, or one whose sizes, voxel sizes or
 *      offset are not the volume's; lookup / paths / rank / download on a handle never computed; max_len == 0 with n > 0; NULL outputs;
 *      an explorer that is not clustered or has another geometry.  A computation that has not converged after n_traversable + 1 rounds
 *      -- it cannot -- fails with TSDF_ERR_DEVICE rather than loop.
 *   Out of scope: Z-slabs, incremental updates, costs other than the chamfer metric (a clearance-weighted cost), and planning itself:
 *     this is the cost field and the read-out of voxel paths, not a trajectory planner. */
typedef struct tsdf_reach tsdf_reach;
#define TSDF_REACH_THROUGH_UNKNOWN 1u
#define TSDF_REACH_UNREACHED 0xFFFFFFFFu
#define TSDF_REACH_COST_FACE 10u
#define TSDF_REACH_COST_EDGE 14u
#define TSDF_REACH_COST_CORNER 17u
typedef struct tsdf_reach_info {
    uint32_t size[3];
    uint32_t connectivity;
    float voxel_size[3];
    float offset[3];         /* the volume's current offset when computed */
    uint32_t flags;
    float clearance;
    uint32_t max_cost;
    uint32_t max_cost_reached;
    uint64_t n_traversable, n_reached, n_seed_voxels;
    uint64_t rounds;         /* a diagnostic: not a unique value */
} tsdf_reach_info;
typedef struct tsdf_reach_cluster {
    uint32_t label, cost, voxel, reserved;
} tsdf_reach_cluster;
int tsdf_reach_create(tsdf_reach **out);   /* on the current device */
void tsdf_reach_destroy(tsdf_reach *reach);
/* n seeds (3 floats each) on the host; esdf may be NULL (clearance then 0); max_cost 0: no cap.  Blocking. */
int tsdf_volume_compute_reach(const tsdf_volume *volume, uint64_t n, const float *host_seeds, uint32_t connectivity,
                              const tsdf_esdf *esdf, float clearance, uint32_t max_cost, uint32_t flags, tsdf_reach *reach);
/* The same with the seeds in device memory. */
int tsdf_volume_compute_reach_device(const tsdf_volume *volume, uint64_t n, const float *device_seeds, uint32_t connectivity,
                                     const tsdf_esdf *esdf, float clearance, uint32_t max_cost, uint32_t flags, tsdf_reach *reach);
int tsdf_reach_get_info(const tsdf_reach *reach, tsdf_reach_info *info);
/* The device array of the last computation (NULL before the first); valid until the next computation into the handle. */
int tsdf_reach_buffer(const tsdf_reach *reach, const uint32_t **device_costs);
/* Blocking copy to size[0] * size[1] * size[2] words. */
int tsdf_reach_download(const tsdf_reach *reach, uint32_t *host_costs);
/* Device bytes the handle holds besides the cost array. */
int tsdf_reach_scratch_bytes(const tsdf_reach *reach, uint64_t *bytes);
/* n points (3 floats each) -> n costs. */
int tsdf_reach_lookup_device(const tsdf_reach *reach, uint64_t n, const float *device_points, uint32_t *device_costs, void *hip_stream);
int tsdf_reach_lookup(const tsdf_reach *reach, uint64_t n, const float *host_points, uint32_t *host_costs);
/* n goals (3 floats each) -> n lengths and n rows of max_len voxel ids. */
int tsdf_reach_paths_device(const tsdf_reach *reach, uint64_t n, const float *device_goals, uint32_t max_len, uint32_t *device_lengths,
                            uint32_t *device_rows, void *hip_stream);
int tsdf_reach_paths(const tsdf_reach *reach, uint64_t n, const float *host_goals, uint32_t max_len, uint32_t *host_lengths,
                     uint32_t *host_rows);
/* One row per row of the explorer's cluster table (tsdf_explorer_info.n_listed_clusters). */
int tsdf_reach_rank_frontiers_device(tsdf_reach *reach, const tsdf_explorer *explorer, tsdf_reach_cluster *device_rows, void *hip_stream);
int tsdf_reach_rank_frontiers(tsdf_reach *reach, const tsdf_explorer *explorer, tsdf_reach_cluster *host_rows);

/* ---- class objects (no reference counterpart; the per-object maps of Voxblox++, Kimera and SemanticFusion) -------------------------- */
/* Which objects are in the scene, where is each, how big is it, and which object did this ray or pixel hit?  The connected pieces of
 * each fused class (group "class fusion"), on the device.  Opt-in by being called: no other entry point, launch or result changes.
 * Only the class words are read; distances, weights and colours are never read, and nothing of the volume is written.
 *   1. Labelled voxels.  Grid and voxel ids as in "exploration": X x Y x Z voxels, voxel (x, y, z) has id (z * Y + y) * X + x (uint32:
 *      more than 2^32 - 1 voxels are refused).  The word (c, n) of a voxel -- class c in bits 0-15, votes n in bits 16-31 -- is what
 *      tsdf_volume_get_class_data reports.  A voxel is LABELLED iff
 *        n >= max(min_votes, 1), and
 *        the selection admits c: host_select == NULL admits every class; otherwise host_select is n_select bytes and admits c iff
 *          c < n_select && host_select[c] != 0.
 *      A word with n == 0 is unlabelled whatever its class bits are.
 *   2. List.  The handle holds the ids of all labelled voxels in ascending order; n_labelled is the list's length.  Per 64 consecutive
 *      voxel ids it keeps the 64-bit mask of the labelled voxels among them (bit l: id 64 c + l) and the list index of the chunk's
 *      first labelled voxel (the base), exactly as the explorer keeps them: a listed voxel's list index is
 *      base[id / 64] + popcount(mask[id / 64] & ((1 << id % 64) - 1)), and a voxel is listed iff its mask bit is set.
 *   3. Objects.  Two listed voxels are adjacent iff they are neighbours at the chosen connectivity -- 6 or 26, as in "exploration"
 *      rule 3: their coordinates differ by at most 1 on every axis and, at 6, on exactly one axis -- AND their class ids are equal.
 *      An object is a connected set of that graph.
 *        L[i] (uint32, one per listed voxel): the smallest LIST INDEX in the object of list entry i.
 *        Per object a tsdf_class_object row (72 bytes): label = that smallest index, size = its number of voxels, lo[k] / hi[k] =
 *          the smallest / largest coordinate on axis k (the inclusive box; k = 0, 1, 2 for x, y, z), sum[k] = the integer sum of the
 *          coordinates on axis k, votes = the sum of the members' vote counts, class_id = the class all members share, reserved = 0.
 *          The centroid's world position is offset[k] + (sum[k] / size + 0.5) * voxel_size[k], as for a frontier cluster.
 *        The table holds the rows with size >= min_size, in ascending label.  info.n_objects counts all objects,
 *          info.n_listed_objects the rows.
 *   4. Lookup.  tsdf_objects_lookup_device resolves n world points (3 floats each) to table rows.  For each point it takes the voxel
 *      tsdf_volume_sample_classes_device reads for that point -- the same frame (offset_at_clear subtracted), the same index
 *      expression -- with the geometry (sizes, voxel sizes, offset, offset_at_clear) the handle remembers from the last
 *      tsdf_volume_find_objects.  rows[i] is the 0-based index in the table of the object that holds the voxel, or TSDF_OBJECT_NONE
 *      for a NaN coordinate, an off-grid index, an unlisted voxel, or an object below min_size.  The row is found through a second
 *      mask and base pair over list indices (bit l of row_mask[j]: list index 64 j + l is the label of a listed row): the row of list
 *      entry i is row_base[L[i] / 64] + popcount(row_mask[L[i] / 64] & ((1 << L[i] % 64) - 1)).  n == 0 is TSDF_OK and launches nothing.
 *      An instance-segmentation image is this lookup on a ray cast's vertices (misses are NaN: TSDF_OBJECT_NONE).
 *      tsdf_objects_lookup_device enqueues on hip_stream behind the handle's pending work; tsdf_objects_lookup is the same on host
 *      arrays, on the null stream, blocking.
 *   5. Uniqueness.  Everything is a set, an integer sum, a minimum or a maximum: two runs give the same bytes, whatever order the
 *      waves run in.  No float atomics.  No lane ever waits for another: no spin loops, locks or flags.  Every loop has a stated
 *      bound: a lane's hook makes 13 trips, a wave's root loop 64, and the union-find's walks are bounded as DESIGN.md 20 argues.
 *   tsdf_volume_find_objects runs list, labels and table on the volume's stream and waits for it twice, once to size the list and once
 *     to size the table (once when the list is empty).  flags: none defined, 0.
 *   The handle (tsdf_objects_create, on the current device) owns the list, the masks and bases, the labels and the table, keeps them
 *     between calls and only grows them: a warm second call allocates nothing and leaves tsdf_objects_scratch_bytes unchanged.
 *     Scratch (tsdf_objects_scratch_bytes: everything but the list, the labels and the table): 12 bytes per 64 voxels for masks and
 *     bases (3/16 byte a voxel), the chunk scan's sums, the device copy of the selection (n_select bytes), 72 bytes per listed voxel
 *     for the accumulator rows and 12 per 64 of them for the row masks and bases.  A handle is used by one thread at a time.
 *     tsdf_objects_destroy(NULL) is ignored.
 *   tsdf_objects_buffers: the device arrays -- the list and the labels (n_labelled words each), the masks and bases (one per 64 voxel
 *     ids), the table (n_listed_objects rows); any pointer may be NULL, a buffer is NULL where it is empty.  tsdf_objects_download
 *     copies list, labels and table (any pointer may be NULL).  Both wait for the handle's pending work.
 *   Refused (TSDF_ERR_INVALID, with a message naming the entry point, nothing written): NULL handles or volumes; a volume without
 *     classes enabled; more than 2^32 - 1 voxels; a connectivity other than 6 or 26; unknown flags; host_select == NULL with
 *     n_select > 0, or n_select > 65535; buffers, download or lookup before any tsdf_volume_find_objects; NULL points or rows with n > 0.
 *   Out of scope: objects in the pipeline step or the tracker; labels that stay stable across calls; per-object meshes (a row's box
 *     feeds tsdf_volume_extract_mesh); merging objects across classes; classes through fuse, snapshots and files. */
typedef struct tsdf_objects tsdf_objects;
#define TSDF_OBJECT_NONE 0xFFFFFFFFu
typedef struct tsdf_objects_info {
    uint32_t size[3];
    uint32_t connectivity;
    float voxel_size[3];
    float offset[3];         /* the volume's current offset at the last tsdf_volume_find_objects */
    uint32_t min_votes, min_size;   /* as given */
    uint64_t n_labelled, n_objects, n_listed_objects;
} tsdf_objects_info;         /* 72 bytes, n_labelled at 48 */
typedef struct tsdf_class_object {
    uint32_t label, size;
    uint32_t lo[3], hi[3];
    uint64_t sum[3];
    uint64_t votes;
    uint32_t class_id, reserved;
} tsdf_class_object;         /* 72 bytes, sum at 32, votes at 56, class_id at 64 */
int tsdf_objects_create(tsdf_objects **out);   /* on the current device */
void tsdf_objects_destroy(tsdf_objects *objects);
int tsdf_volume_find_objects(const tsdf_volume *volume, uint32_t min_votes, const uint8_t *host_select /* or NULL: every class */,
                             uint32_t n_select, uint32_t connectivity, uint32_t min_size, uint32_t flags /* none defined: 0 */,
                             tsdf_objects *objects);
int tsdf_objects_get_info(const tsdf_objects *objects, tsdf_objects_info *info);
int tsdf_objects_buffers(const tsdf_objects *objects, const uint32_t **device_voxels, const uint64_t **device_masks,
                         const uint32_t **device_bases, const uint32_t **device_labels, const tsdf_class_object **device_rows);
int tsdf_objects_download(const tsdf_objects *objects, uint32_t *host_voxels, uint32_t *host_labels, tsdf_class_object *host_rows);
/* n points (3 floats each) -> the table row of the object each lies in, or TSDF_OBJECT_NONE. */
int tsdf_objects_lookup_device(const tsdf_objects *objects, uint64_t n, const float *device_points, uint32_t *device_rows,
                               void *hip_stream);
int tsdf_objects_lookup(const tsdf_objects *objects, uint64_t n, const float *host_points, uint32_t *host_rows);
/* Device bytes the handle holds besides the list, the labels and the table. */
int tsdf_objects_scratch_bytes(const tsdf_objects *objects, uint64_t *bytes);

/* ---- sparse snapshot (no reference counterpart: the reference saves a volume densely, and cannot load one) ------------------------ */
/* The state of a whole volume as the bricks that hold anything but what clear() leaves: taken out of the dense arrays on the device,
 * put back, downloaded and uploaded.  What it is for: checkpoint and resume, rolling back after a lost track, parking a finished
 * sub-map.  Lossless: every word is carried as its bits.  Opt-in by being called.
 *   The value (a unique set of bytes, whatever computes it): the grid is X x Y x Z; bricks are 8 x 8 x 8 voxels aligned to multiples
 *     of 8, nb[a] = ceil(size[a] / 8) per axis, brick id b = bx + by nb[0] + bz nb[0] nb[1].
 *     fill = the volume's truncation distance when the snapshot is taken.  A voxel is CLEARED iff its distance has exactly the bits of
 *       fill, its weight is zero -- a packed count of 0; in fp32 storage the bits 0x00000000, so -0.0 and NaN are not cleared -- and,
 *       when colour is enabled, its colour word is 0.
 *     A brick is LIVE iff one of its voxels inside the grid is not cleared.  The snapshot holds the live brick ids in ascending order
 *       and, per brick in list order, 512 distances (fp32, the volume's bits), 512 weights in the volume's own element type when taken
 *       (uint8 for 8-bit storage, uint16 for 16-bit, the fp32 bits for fp32) and, with colour, 512 colour words {r, g, b, n}.  Voxel
 *       (lx, ly, lz) of a brick sits at lx + 8 ly + 64 lz; positions of a partial brick beyond the grid hold fill, 0 and 0.
 *     The handle also records weight_bound (the volume's own upper bound of every count; 0 for fp32), the geometry (size, voxel size,
 *       current offset) and fill.
 *   tsdf_volume_snapshot writes nothing of the volume: no distance, weight, storage mode, occupancy flag, dirty mark, prepared cull or
 *     ray-cast state.  It enqueues on the volume's stream and synchronises once, to learn n_bricks and size the arrays.  The handle keeps
 *     its arrays and scratch between calls and only grows them: a warm handle that is large enough allocates nothing.  Scratch beyond
 *     the four arrays: 8 bytes a brick of the grid and 16 bytes per 1024 bricks (tsdf_snapshot_scratch_bytes).
 *   tsdf_volume_restore: afterwards every accessor reports the state the volume had when the snapshot was taken, bit for bit; voxels
 *     of bricks that are not stored get fill, weight 0 and colour 0.  The grid size must equal the snapshot's.  Header fields, offsets,
 *     offset_at_clear, the weight cap, the stream and attachments are not touched (a caller who wants the snapshot's offset sets it).
 *     Weight storage: an unpinned volume ends in the wider of its present mode and the snapshot's weight_bits, a pinned one stays fp32;
 *     counts are converted exactly, never narrowed; weight_bound becomes the snapshot's.  A snapshot with colour enables colour on the
 *     volume, one without zeroes an enabled colour array.  The occupancy flags are rebuilt from everything before the next ray cast and
 *     a prepared brick list is discarded, as after tsdf_volume_set_distance_data and tsdf_volume_set_weight_data.  Asynchronous on the
 *     volume's stream unless the storage has to change.
 *   Stream order: the handle records an event behind whatever was enqueued last on it; tsdf_snapshot_get_info, tsdf_snapshot_download
 *     and tsdf_snapshot_buffers wait for it, a snapshot or restore from a volume on another stream orders itself behind it.  A handle
 *     is used by one thread at a time, on the device it was made on.
 *   tsdf_snapshot_upload: the host arrays of a download (or of a file) into a handle.  From info it takes size, flags, weight_bits,
 *     fill_distance, voxel_size, offset and n_bricks; for counts it sets weight_bound to the largest weight in the array.  Checked on
 *     the host before a device is touched: sizes in 1 .. 65535, weight_bits 8, 16 or 32, n_bricks at most the brick count, ids strictly
 *     ascending and below the brick count.
 *   Refused (TSDF_ERR_INVALID, with a message naming the function): NULL arguments (host_colours / device_colours results aside when
 *     there is no colour); flags other than 0; a Z-slab volume; a materialised deformation-node array; restore into a grid of another
 *     size; restore, download or buffers from a handle that was never filled.  tsdf_snapshot_destroy(NULL) is ignored.
 *   Out of scope: merging into live data (tsdf_volume_fuse), Z-slabs, deformation nodes, compression, incremental snapshots.
 *     (Shifting bricks on restore and a box of the list are the next group, "rolling volume".) */
typedef struct tsdf_snapshot tsdf_snapshot;
#define TSDF_SNAPSHOT_BRICK 8
#define TSDF_SNAPSHOT_COLOUR 1u            /* info.flags: colour words are carried */
typedef struct tsdf_snapshot_info {
    uint32_t size[3];
    uint32_t bricks[3];
    uint32_t flags;
    uint32_t weight_bits;                  /* 8, 16 or 32 */
    uint32_t weight_bound;
    float fill_distance;
    float voxel_size[3];
    float offset[3];
    uint64_t n_bricks;
    uint64_t bytes;                        /* device bytes of the id, distance, weight and colour arrays */
} tsdf_snapshot_info;                      /* 80 bytes, n_bricks at 64 */
int tsdf_snapshot_create(tsdf_snapshot **out);   /* on the current device */
void tsdf_snapshot_destroy(tsdf_snapshot *snapshot);
int tsdf_volume_snapshot(const tsdf_volume *volume, uint32_t flags, tsdf_snapshot *snapshot);   /* flags: 0 */
int tsdf_volume_restore(tsdf_volume *volume, const tsdf_snapshot *snapshot);
int tsdf_snapshot_get_info(const tsdf_snapshot *snapshot, tsdf_snapshot_info *info);
/* The device arrays (NULL for an empty snapshot, device_colours also without colour); valid until the handle is filled again. */
int tsdf_snapshot_buffers(const tsdf_snapshot *snapshot, const uint32_t **device_bricks, const float **device_distances,
                          const void **device_weights, const uint32_t **device_colours);
/* Blocking copies: n_bricks ids, and 512 n_bricks distances, weights (weight_bits / 8 bytes each) and colour words. */
int tsdf_snapshot_download(const tsdf_snapshot *snapshot, uint32_t *host_bricks, float *host_distances, void *host_weights,
                           uint32_t *host_colours);
int tsdf_snapshot_upload(tsdf_snapshot *snapshot, const tsdf_snapshot_info *info, const uint32_t *host_bricks,
                         const float *host_distances, const void *host_weights, const uint32_t *host_colours);
/* Device bytes the handle holds besides the four arrays. */
int tsdf_snapshot_scratch_bytes(const tsdf_snapshot *snapshot, uint64_t *bytes);

/* ---- rolling volume (no reference counterpart: the reference's volume stays where it was made) ------------------------------------ */
/* A volume that follows the camera: a shift by whole bricks is a snapshot put back at other brick coordinates, the bricks that fall out
 * are themselves a snapshot (to keep on the host, write to a .tsdfs file, mesh later, or page back in when the camera returns).  No
 * voxel is resampled: whole words move, there are no atomics, every output word has one writer, every run gives the same bytes.
 *   tsdf_volume_restore_shifted: nbS is the snapshot's brick grid, nbD the volume's.  Destination brick bD takes source brick
 *     bS = bD - brick_shift per axis (formed in 64 bits: every int32 shift is served).  The copy happens iff bS lies in [0, nbS) on every
 *     axis and is stored in the snapshot; then every voxel of bD inside the destination grid takes the snapshot's word at the same local
 *     position lx + 8 ly + 64 lz -- positions of a partial source brick beyond the source grid hold fill, 0 and 0 and are written as
 *     such -- and voxels of bD beyond the destination grid are not written.  Without flags every other voxel of the volume gets the
 *     cleared state (the snapshot's fill_distance, weight 0, colour 0), as after tsdf_volume_restore; with TSDF_RESTORE_KEEP_OTHERS every
 *     other voxel keeps its bits (paging in), and the launch is over the snapshot's list, not over the grid.  The two grid sizes need
 *     not be equal: a shifted restore into a smaller or larger grid crops or grows a volume.  Voxel sizes and offsets are neither
 *     compared nor touched.  Storage, colour and flags follow tsdf_volume_restore: weight storage widens and never narrows, a snapshot
 *     with colour enables colour, the occupancy flags are rebuilt from everything and a prepared brick list is discarded.  Under
 *     KEEP_OTHERS widening carries the data already in the volume, weight_bound becomes the larger of the two, and a snapshot without
 *     colour writes colour 0 on the bricks it writes only.  A zero shift into a grid of the snapshot's size without flags leaves the
 *     state tsdf_volume_restore leaves.
 *   tsdf_snapshot_select: dst becomes the snapshot of those bricks of src whose brick coordinates lie inside the box [lo, hi) -- with
 *     TSDF_SELECT_OUTSIDE, outside it.  Ids are unchanged and still ascending, each brick's 512-word rows are copied; geometry, flags,
 *     weight_bits, fill_distance and weight_bound are src's, n_bricks and bytes are new; an empty result is a filled handle with
 *     n_bricks == 0.  Runs on the null stream, ordered against both handles by their events, and synchronises once, to size dst; a warm
 *     dst that is large enough allocates nothing.
 *   tsdf_volume_shift: the box moves by box_shift bricks in the world, the content stays where it is in the world.  In order: the
 *     volume is snapshotted into work; leaving (if not NULL) gets the bricks b of work for which b - box_shift is outside [0, nb) on some
 *     axis, its info.offset the old offset, so that brick b sits at offset + 8 b voxel_size; tsdf_volume_restore_shifted(volume, work,
 *     -box_shift, 0); offset[k] = offset[k] + (float)(8 * box_shift[k]) * voxel_size[k] in fp32, with the effects of
 *     tsdf_volume_set_offset.  offset_at_clear is not touched: integrate forms a centre as (((i + 0.5f) vs) + offset_at_clear) + offset,
 *     the ray cast and the queries use offset, so moving offset alone moves every frame together.  An all-zero shift writes nothing of
 *     the volume (leaving, if given, is filled empty).
 *   Refused (TSDF_ERR_INVALID, with a message naming the function): NULL arguments (leaving aside); unknown flags; a Z-slab volume; a
 *     materialised deformation-node array; handles on other devices; a handle that was never filled; dst == src; leaving == work;
 *     tsdf_volume_shift of a grid whose size is not a multiple of 8 on every axis (voxels cut off at a partial border would be lost
 *     without appearing in leaving; tsdf_volume_restore_shifted still serves such grids) or of a volume with classes enabled
 *     (snapshots do not carry class words: they would stay behind while the geometry moves).
 *   Out of scope: the tracker and tsdf_pipeline_*, kinfu_stream, class words, Z-slabs, shifts by less than a brick, a shift in place
 *     without the snapshot round trip. */
#define TSDF_RESTORE_KEEP_OTHERS 1u        /* tsdf_volume_restore_shifted: voxels of bricks that are not written keep their bits */
#define TSDF_SELECT_OUTSIDE 1u             /* tsdf_snapshot_select: the bricks outside the box */
int tsdf_volume_restore_shifted(tsdf_volume *volume, const tsdf_snapshot *snapshot, const int32_t brick_shift[3], uint32_t flags);
int tsdf_snapshot_select(const tsdf_snapshot *src, const int32_t lo[3], const int32_t hi[3], uint32_t flags, tsdf_snapshot *dst);
/* leaving may be NULL */
int tsdf_volume_shift(tsdf_volume *volume, const int32_t box_shift[3], tsdf_snapshot *work, tsdf_snapshot *leaving);

/* ---- column maps (no reference counterpart: the reference's volume is asked about its surface only) -------------------------------- */
/* Where is the floor and how high is it, is this cell of the floor plan free, occupied or unseen, how much headroom is above the
 * ground, how close is the nearest obstacle in my height range?  Every column of voxels along one axis of the grid is reduced to one
 * small row of a 2-D map -- what a ground robot's planner, a drone's altitude hold or a map viewer asks before anything in 3-D.  Opt-in
 * by being called: no other entry point, launch or result changes; nothing of a volume or an ESDF is written.  Every result is an
 * integer, a set, a minimum or the outcome of a fixed fp32 expression: two runs give the same bytes.
 *   1. Grid, ids and voxel states are those of "exploration" rule 1: voxel (x, y, z) has id (z * Y + y) * X + x (uint32: more than
 *      2^32 - 1 voxels are refused), and UNKNOWN / FREE / OCCUPIED are as defined there.  Weights are read in place from all three
 *      storages; a distance d(v) is read only where the voxel is observed.
 *   2. Axis and map.  axis in {0, 1, 2} (x, y, z) is the axis reduced.  The map's axes (a_u, a_v) are the two others in ascending
 *      order: axis 0 -> (y, z); axis 1 -> (x, z); axis 2 -> (x, y).  The map has U x V cells, U = N[a_u], V = N[a_v]; cell (u, v) has
 *      index v * U + u.
 *   3. Band and walk.  lo, hi are voxel indices on `axis` with 0 <= lo < hi <= N_axis; hi == 0 means N_axis.  L = hi - lo.  The
 *      column of a cell is the sequence c_0 .. c_{L-1}; c_p is the voxel with axis index lo + p -- with TSDF_COLUMNS_REVERSED, with
 *      axis index hi - 1 - p.  "Up" is increasing p: a volume whose gravity axis points down the index is served by the flag, not by
 *      a second definition.
 *   4. Row.  One 32-byte tsdf_column per cell:
 *        n_unknown, n_free, n_occupied: the counts over the column; they sum to L.
 *        top: the largest p with OCCUPIED(c_p), or -1 if there is none.  bottom: the smallest such p, or -1.
 *        headroom: 0 if top == -1; otherwise the number of consecutive FREE voxels at p = top + 1, top + 2, ...: the count ends at
 *          the first voxel that is not FREE, or at L.
 *        height, in voxels of the walk, measured from the band's start: NaN if top == -1.  The fallback is (float)top + 1.0f, the
 *          voxel's upper face.  If top + 1 < L and c_{top+1} is FREE, let d0 = d(c_top), d1 = d(c_{top+1}) and f = d0 / (d0 - d1),
 *          every fp32 operation rounded on its own.  If f >= 0.0f and f <= 1.0f (NaN fails both), height = ((float)top + 0.5f) + f:
 *          the zero crossing between the two voxel centres.  Otherwise it is the fallback.  In the world the surface is at
 *          offset[axis] + ((float)lo + height) * voxel_size[axis] forward, offset[axis] + ((float)hi - height) * voxel_size[axis]
 *          reversed.
 *        min_distance: with an ESDF handle, the minimum over the column of the ESDF values that are not NaN; NaN if all of them are
 *          NaN.  A minimum that compares equal to zero is stored as +0.0f, so the order of the reduction never shows.  Without an
 *          ESDF handle it is NaN.
 *      Every NaN of height and min_distance is the canonical quiet NaN 0x7FC00000.
 *   5. tsdf_columns_info: the volume's sizes, voxel sizes and offset as tsdf_explorer_info has them; axis, lo, hi (resolved), flags,
 *      map_size = {U, V}, map_axes = {a_u, a_v}, has_esdf; the totals n_unknown, n_free, n_occupied over all rows (they sum to
 *      U * V * L) and n_ground, the cells with top >= 0.  After a classification n_no_ground, n_traversable, n_blocked and the
 *      max_step and min_headroom given; zero before one, and again after the next projection.  All are unique integers: integer
 *      atomics, one per counter and workgroup.
 *   6. Classification: tsdf_columns_classify[_device](map, max_step, min_headroom, flags = 0, uint8 out[U * V], stream), 2.5-D
 *      traversability from the rows alone, one byte per cell in cell order:
 *        TSDF_CELL_NO_GROUND 0:   top == -1.
 *        TSDF_CELL_BLOCKED 2:     top >= 0 and headroom < min_headroom, or some 4-neighbour cell (u -+ 1, v), (u, v -+ 1) inside the
 *                                 map with top_nb >= 0 has |top - top_nb| > max_step (an integer compare).  A neighbour without ground
 *                                 blocks nothing.
 *        TSDF_CELL_TRAVERSABLE 1: every other cell with top >= 0.
 *   7. The handle (tsdf_columns_create, on the current device) owns the rows and eight counter words, keeps them between calls and
 *      only grows them: a warm second call allocates nothing.  It snapshots the geometry, so classification and downloads need no
 *      volume.  tsdf_volume_project_columns runs on the volume's stream and does not synchronise (an ESDF handle's own pending work is
 *      waited for first, as "reachability" does); tsdf_columns_classify_device runs on hip_stream behind the handle's pending work;
 *      tsdf_columns_classify blocks.  tsdf_columns_get_info, tsdf_columns_buffer and tsdf_columns_download wait for the handle's
 *      pending work.  tsdf_columns_scratch_bytes: the device bytes the handle holds, rows (32 a cell of the largest map so far) and
 *      counters (64).  A handle is used by one thread at a time.  tsdf_columns_destroy(NULL) is ignored.
 *   8. Refused (TSDF_ERR_INVALID, with a message naming the entry point, before any device work): NULL handle or volume; a Z-slab
 *      volume; a materialised deformation-node array; axis > 2; lo >= hi after resolving hi == 0; hi > N_axis; an axis of more than
 *      2^31 - 1 voxels (top is an int32); unknown flags; an ESDF that was never computed, or whose sizes, voxel sizes or offset are not
 *      the volume's; classification, buffer or download on a handle that was never projected; a NULL output.
 *   How: a lane per cell, consecutive lanes along the map's u axis, walking its column in strides (columns_walk_kernel).  For axes 1
 *     and 2 u is x, so every step of the walk reads 64 consecutive words of a row; for axis 0 the lanes lie X words apart.  A second
 *     kernel for axis 0 -- a wave per column, 64 voxels a step, ballots and popcounts -- was measured against the walk and was slower;
 *     it is not in the library.
 *   Out of scope: several surfaces per column (multi-level maps), a 2-D reachability over the classified map, maps inside the pipeline
 *     step or the tracker, Z-slabs, incremental updates. */
typedef struct tsdf_columns tsdf_columns;
#define TSDF_COLUMNS_REVERSED 1u
#define TSDF_CELL_NO_GROUND 0u
#define TSDF_CELL_TRAVERSABLE 1u
#define TSDF_CELL_BLOCKED 2u
typedef struct tsdf_column {
    uint32_t n_unknown, n_free, n_occupied;
    int32_t top, bottom;
    uint32_t headroom;
    float height;
    float min_distance;
} tsdf_column;
typedef struct tsdf_columns_info {
    uint32_t size[3];
    uint32_t axis;
    float voxel_size[3];
    float offset[3];         /* the volume's current offset when projected */
    uint32_t lo, hi;         /* the band, hi resolved */
    uint32_t flags;
    uint32_t has_esdf;
    uint32_t map_size[2];    /* U, V */
    uint32_t map_axes[2];    /* a_u, a_v */
    uint64_t n_unknown, n_free, n_occupied, n_ground;
    uint64_t n_no_ground, n_traversable, n_blocked;
    uint32_t max_step, min_headroom;
} tsdf_columns_info;
int tsdf_columns_create(tsdf_columns **out);   /* on the current device */
void tsdf_columns_destroy(tsdf_columns *columns);
/* esdf may be NULL (min_distance is then NaN); hi == 0: the whole axis from lo. */
int tsdf_volume_project_columns(const tsdf_volume *volume, uint32_t axis, uint32_t lo, uint32_t hi, const tsdf_esdf *esdf, uint32_t flags,
                                tsdf_columns *columns);
int tsdf_columns_get_info(const tsdf_columns *columns, tsdf_columns_info *info);
/* The device rows of the last projection, map_size[0] * map_size[1] of them; valid until the next projection into the handle. */
int tsdf_columns_buffer(const tsdf_columns *columns, const tsdf_column **device_rows);
/* Blocking copy of the rows. */
int tsdf_columns_download(const tsdf_columns *columns, tsdf_column *host_rows);
int tsdf_columns_scratch_bytes(const tsdf_columns *columns, uint64_t *bytes);
/* One byte per cell into a device array, on hip_stream. */
int tsdf_columns_classify_device(tsdf_columns *columns, uint32_t max_step, uint32_t min_headroom, uint32_t flags /* none defined: 0 */,
                                 uint8_t *device_cells, void *hip_stream);
/* The same into a host array; blocking. */
int tsdf_columns_classify(tsdf_columns *columns, uint32_t max_step, uint32_t min_headroom, uint32_t flags, uint8_t *host_cells);

/* Multi-GPU raycast: a slab evaluates only the samples whose lower trilinear tap plane it owns and writes
 * one 8-byte record per pixel: k = index of the first owned sample with tsdf <= 0 (TSDF_NO_HIT if none), t = that sample's
 * refined ray parameter (src/RayCaster/GPURaycaster.cu:338-341).  After an all-gather of the records (layout
 * [slab][pixel]), tsdf_merge_hits_device keeps, per pixel, the record with the smallest k and forms the vertex
 * space_min + (start + t * dir) with the reference's expressions (:306, :344-347): start and dir are functions of the pixel
 * and the pose, which every rank computes bit-identically -- so the record needs neither of them.  (Up to round 2 the record
 * was {k, x, y, z}, 16 bytes.)  `volume` supplies the grid's offset and physical size (any slab of the grid, or the whole). */
#define TSDF_NO_HIT 0xffffffffu
typedef struct tsdf_hit_record {
    uint32_t k;
    float t;
} tsdf_hit_record;
int tsdf_raycast_slab_device(const tsdf_volume *volume, uint32_t width, uint32_t height,
                             const float pose[16], const float kinv[9], tsdf_hit_record *device_hits);
int tsdf_merge_hits_device(const tsdf_volume *volume, const tsdf_hit_record *device_hits_all, uint32_t n_slabs,
                           uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                           float *device_vertices, void *hip_stream);
/* The same select and compute_normals (src/RayCaster/GPURaycaster.cu:393-427) on the merged map in one launch. */
int tsdf_merge_hits_normals_device(const tsdf_volume *volume, const tsdf_hit_record *device_hits_all, uint32_t n_slabs,
                                   uint32_t width, uint32_t height, const float pose[16], const float kinv[9],
                                   float *device_vertices, float *device_normals, void *hip_stream);

/* ---- frame differences (no reference counterpart; the dynamic masks of nvblox, StaticFusion and Co-Fusion) ------------------------- */
/* Does a depth frame agree with the model, which pixels do not, and how do those hang together?  A frame (the tracker's filtered
 * frame, say) is compared with the model's depth image from the same camera (tsdf_raycast_depth_device, or the mesh renderer's depth
 * target); the pixels that lie in front of the model are listed, clustered into blobs, and the blobs that are large enough become a
 * dilated mask under which a frame's depths are set to 0, which every integrate reads as "no measurement".  Opt-in by being called: no
 * other entry point, launch or result changes.  Everything is integers and sets (unique values, whatever computes them): two runs give
 * the same bytes, and a host reference can match them byte for byte.
 *   1. Compare.  frame and model are width x height uint16 millimetres, row major; pixel (x, y) has id y * width + x (uint32).  With f
 *      the frame's and m the model's value of a pixel, and params {tolerance (mm), quadratic}:
 *        tol = tolerance + ((quadratic * m * m) >> 32), product and sum formed in 64 bits (65535^2 * (2^32 - 1) < 2^64), then saturated
 *              to 65535: quadratic = 2^32 * c gives a tolerance that grows by c mm per mm^2 of model depth, as a depth sensor's noise does.
 *        TSDF_DIFF_NO_FRAME (0): f == 0.
 *        TSDF_DIFF_NO_MODEL (1): f > 0 and m == 0.
 *        TSDF_DIFF_NEARER   (4): f + tol < m.
 *        TSDF_DIFF_FARTHER  (3): f > m + tol.
 *        TSDF_DIFF_SAME     (2): otherwise.       (the first that holds, in this order; the sums cannot overflow 32 bits)
 *      info.counts[state] is the number of pixels in each state (they sum to width * height); device_states, when given, takes the
 *      state of every pixel, one uint8 each.  The LISTED pixels are the NEARER ones, their ids in ascending order, with the per-64-ids
 *      masks and bases of "exploration" (2.).  NO_MODEL and FARTHER are reported and never listed: something seen where the model is
 *      empty, or behind where it was, is unexplored space or a surface that has left, not a thing in front of the scene.  The handle
 *      keeps a copy of the frame (2 bytes a pixel): the caller's arrays are free again when the call returns.  Runs on hip_stream
 *      behind the handle's pending work and waits for it once, to size the list.
 *   2. Cluster.  Two listed pixels are joined iff they are neighbours IN THE IMAGE -- x and y differ by at most 1, at connectivity 4 on
 *      one axis only; the last pixel of a row and the first of the next are not neighbours -- and their FRAME depths differ by at most
 *      depth_step (depth_step >= 65535 joins any neighbours): a hand in front of a body comes out as two blobs.  A blob is a connected
 *      set of that graph.
 *        L[i] (uint32, one per listed pixel): the smallest LIST INDEX in the blob of list entry i.
 *        Per blob: label = that index, size = its pixels, lo / hi = the inclusive pixel box (x, y), min_depth / max_depth of the frame,
 *          sum_x, sum_y, sum_depth = integer sums over its pixels (centroid and mean depth are sum / size, exact for whoever divides).
 *        The table holds one tsdf_diff_blob row per blob of at least max(min_pixels, 1) pixels -- the KEPT blobs -- in ascending label.
 *          info.n_blobs counts all blobs, info.n_kept_blobs the rows.
 *      Runs on hip_stream and waits for it once, to size the table.  How: the chain of "exploration" (3.) over a width x height x 1
 *      grid with the policy "near in depth"; sums, minima and maxima by integer atomics, one set per wave and blob.
 *   3. Mask, with dilate in 0 .. 32 pixels; every output is optional.
 *        blob_index[p] (uint32) = the row of the kept blob that listed pixel p belongs to, TSDF_DIFF_NO_BLOB everywhere else.  Not
 *          dilated: an instance image of what moved.
 *        mask[p] (uint8) = 1 iff some pixel q of a kept blob has max(|px - qx|, |py - qy|) <= dilate, else 0.  The window is clipped at
 *          the image's border.
 *        frame_out[p] = mask[p] ? 0 : frame_in[p] (uint16; frame_out == frame_in is allowed; both or neither).
 *      How: diff_paint_kernel looks every pixel up (mask and base to the list index, its label, the table's keep mask to the row) and
 *      writes one bit per pixel by ballot; diff_dilate_kernel tests the row window as a range of ids in that bit mask, keeps the result
 *      of a tile's rows with a halo of `dilate` rows in LDS, and ORs the column window from there.  One writer per output, no atomics.
 *      Asynchronous on hip_stream.
 *   The handle (tsdf_frame_diff_create, on the current device) owns the frame copy, the list, the masks and bases, the labels, the
 *     table and the kept-pixel mask, keeps them between calls and only grows them: a warm call of no larger an image allocates
 *     nothing.  Scratch (tsdf_frame_diff_scratch_bytes: everything but the list, the labels and the table): 2 bytes a pixel for the
 *     frame copy, 20 bytes per 64 pixels for the masks and bases, 56 bytes per listed pixel and 12 per 64 of them once clustered.
 *     A handle is used by one thread at a time.  tsdf_frame_diff_destroy(NULL) is ignored.
 *   tsdf_frame_diff_buffers: the device arrays (any pointer may be NULL; list, labels and table are NULL where empty);
 *     tsdf_frame_diff_download copies list and labels (counts[TSDF_DIFF_NEARER] words each) and the table (n_kept_blobs rows); any
 *     pointer may be NULL.  Both wait for the handle's pending work and refuse a handle that has not been clustered since its last
 *     compare.
 *   Refused (TSDF_ERR_INVALID, with a message naming the entry point): NULL handles, params, frame or model; width * height of 0 or
 *     above 2^32 - 1, or a side above 65535; a connectivity other than 4 or 8; clustering before a compare; a mask before a cluster call;
 *     dilate > 32; only one of frame_in and frame_out.
 *   In the tracked loop: tsdf_tracker_set_dynamic_rejection ("the tracked loop").
 *   Out of scope: masks inside tsdf_pipeline_step, masked ICP and aligner inputs, blob tracking across frames, carving from FARTHER,
 *     general cameras. */
typedef struct tsdf_frame_diff tsdf_frame_diff;
#define TSDF_DIFF_NO_FRAME 0u
#define TSDF_DIFF_NO_MODEL 1u
#define TSDF_DIFF_SAME 2u
#define TSDF_DIFF_FARTHER 3u
#define TSDF_DIFF_NEARER 4u
#define TSDF_DIFF_NO_BLOB 0xffffffffu
typedef struct tsdf_diff_params {
    uint32_t tolerance;   /* mm */
    uint32_t quadratic;   /* 2^32 * mm per mm^2 of model depth */
} tsdf_diff_params;
typedef struct tsdf_frame_diff_info {
    uint32_t width, height;          /* of the last compare */
    uint32_t tolerance, quadratic;
    uint32_t connectivity;           /* of the last clustering; 0: not clustered since the last compare */
    uint32_t depth_step, min_pixels;
    uint32_t reserved;
    uint64_t counts[5];              /* by state */
    uint64_t n_blobs, n_kept_blobs;
} tsdf_frame_diff_info;
typedef struct tsdf_diff_blob {   /* 56 bytes */
    uint32_t label, size;
    uint32_t lo[2], hi[2];        /* pixel box, inclusive */
    uint32_t min_depth, max_depth;/* of the frame, mm */
    uint64_t sum_x, sum_y, sum_depth;
} tsdf_diff_blob;
int tsdf_frame_diff_create(tsdf_frame_diff **out);   /* on the current device */
void tsdf_frame_diff_destroy(tsdf_frame_diff *diff);
int tsdf_frame_diff_get_info(const tsdf_frame_diff *diff, tsdf_frame_diff_info *info);
/* Device bytes the handle holds besides the list, the labels and the table. */
int tsdf_frame_diff_scratch_bytes(const tsdf_frame_diff *diff, uint64_t *bytes);
int tsdf_frame_diff_compare_device(tsdf_frame_diff *diff, const uint16_t *device_frame, const uint16_t *device_model, uint32_t width,
                                   uint32_t height, const tsdf_diff_params *params, uint8_t *device_states /* or NULL */,
                                   void *hip_stream);
int tsdf_frame_diff_cluster(tsdf_frame_diff *diff, uint32_t connectivity /* 4 or 8 */, uint32_t depth_step /* mm */,
                            uint32_t min_pixels, void *hip_stream);
int tsdf_frame_diff_buffers(const tsdf_frame_diff *diff, const uint32_t **device_pixels, const uint64_t **device_masks,
                            const uint32_t **device_bases, const uint32_t **device_labels, const tsdf_diff_blob **device_blobs);
int tsdf_frame_diff_download(const tsdf_frame_diff *diff, uint32_t *host_pixels, uint32_t *host_labels, tsdf_diff_blob *host_blobs);
int tsdf_frame_diff_mask_device(tsdf_frame_diff *diff, uint32_t dilate /* 0..32 pixels */, uint8_t *device_mask /* or NULL */,
                                uint32_t *device_blob_index /* or NULL */, const uint16_t *device_frame_in /* or NULL */,
                                uint16_t *device_frame_out /* or NULL */, void *hip_stream);

/* ---- slab exchange: the one collective of a sharded frame (no reference counterpart) ------------------------- */
/* ncclAllGather of the ranks' hit records by RCCL ON THE CALLER'S HIP STREAM: one more launch between the slab ray cast and the
 * merge kernel, no event, no second stream.  librccl is opened at run time: rccl_library = path of the library to use (a process
 * that already holds one, e.g. torch's, passes that path), NULL = the one already loaded if any, else the ROCm installation's.
 * Rank 0 makes the 128-byte id (tsdf_slab_exchange_unique_id) and hands it to the other ranks by whatever means the caller has
 * (torch.distributed, MPI, a file); then EVERY rank calls tsdf_slab_exchange_create (it is collective: ncclCommInitRank). */
typedef struct tsdf_slab_exchange tsdf_slab_exchange;
#define TSDF_EXCHANGE_ID_BYTES 128
int tsdf_slab_exchange_unique_id(uint8_t id[TSDF_EXCHANGE_ID_BYTES], const char *rccl_library);
int tsdf_slab_exchange_create(int rank, int world, const uint8_t id[TSDF_EXCHANGE_ID_BYTES], const char *rccl_library,
                              tsdf_slab_exchange **out);
/* The same object over the caller's own collective (MPI, torch.distributed, a test double): all_gather must leave rank r's
 * n_pixels records at device_all + r * n_pixels on every rank, enqueued on or ordered behind hip_stream; returns TSDF_OK. */
typedef int (*tsdf_exchange_fn)(void *user, const tsdf_hit_record *device_mine, tsdf_hit_record *device_all, uint32_t n_pixels,
                                void *hip_stream);
int tsdf_slab_exchange_create_callback(int rank, int world, tsdf_exchange_fn all_gather, void *user, tsdf_slab_exchange **out);
/* A stand-in for the collective on a box with one GPU (emulation and tests; no reference counterpart): "rank `rank` of `world`" whose
 * all-gather copies this rank's own records into every rank's place, device to device on the caller's stream -- the launches, the
 * bytes landing in this GPU's memory and the merge over `world` record buffers cost what they cost on a node; the wire does not run. */
int tsdf_slab_exchange_create_loopback(int rank, int world, tsdf_slab_exchange **out);
int tsdf_slab_exchange_world(const tsdf_slab_exchange *exchange, int *rank, int *world);
/* How many ranks the communicator itself reports (ncclCommCount; the world handed in at creation for a caller's own collective):
 * what a driver prints beside its timings, so that nobody takes a run of one rank for a scaling point. */
int tsdf_slab_exchange_ranks_seen(const tsdf_slab_exchange *exchange, int *ranks);
/* SURVEY.md 8e, mode B -- the cross-rank validator of the merge path (no reference counterpart: the reference has one GPU).  Every
 * rank gathers every rank's DISTANCE slab through the exchange, assembles the whole volume, casts it the ordinary single-volume way
 * and counts the words in which that picture differs from the merged one (device_merged_*: what tsdf_pipeline_step or
 * tsdf_merge_hits_normals_device left; normals may be NULL); NaN equals NaN.  0 differing words on every rank = the 8-byte {k, t}
 * records + min-k merge reproduce the whole volume's cast bit for bit.  Collective (every rank calls it, on its slab's stream),
 * blocking, and expensive by design: 4 N bytes per rank through the collective and a whole volume resident on every rank. */
int tsdf_slab_validate_merge(tsdf_volume *slab_volume, tsdf_slab_exchange *exchange, uint32_t width, uint32_t height,
                             const float pose[16], const float kinv[9], const float *device_merged_vertices,
                             const float *device_merged_normals, uint64_t *differing_words);
/* device_all: world x n_pixels records, rank r's at [r * n_pixels, (r + 1) * n_pixels).  Asynchronous on hip_stream. */
int tsdf_slab_exchange_all_gather(tsdf_slab_exchange *exchange, const tsdf_hit_record *device_mine, tsdf_hit_record *device_all,
                                  uint32_t n_pixels, void *hip_stream);
int tsdf_slab_exchange_destroy(tsdf_slab_exchange *exchange);

/* ---- the per-frame loop ------------------------------------------------------------------------------------------------- */
/* Replaces the body of the reference's frame loop (src/Tools/kinfu.cpp:32-56: load, integrate, one blocking call each; BASELINE
 * configs[2] adds the bilateral filter and a ray cast per frame) on frames that live in HBM: filter -> integrate -> ray cast +
 * normals per step on a HIP stream of the pipeline's own, and -- with TSDF_PIPELINE_OVERLAP -- the NEXT frame's filter (and its
 * brick culling, when next_camera is given: ground-truth trajectories; not when the pose comes from tracking against this
 * frame's ray cast) on a second stream of lower priority, released by this frame's integrate and awaited by the next step.
 * Same results as the three calls one after the other (tests/test_pipeline.py, tests/cpp/test_stream.cpp); 0.345 -> 0.325 ms per
 * step at 512^3.  With a slab exchange the volume is one rank's Z-slab: a step ray casts the slab, all-gathers the ranks' records
 * on the step's stream and merges them (vertices + normals on every rank); TSDF_PIPELINE_EXCHANGE_STREAM moves the all-gather
 * and the merge to a third stream so that the next frame's integrate need not wait for the collective (results are then
 * ordered behind tsdf_pipeline_synchronize only).  The pipeline owns its streams, events, the two filtered frames + tile
 * maxima and the record buffers; while it lives the volume's stream is the pipeline's (tsdf_pipeline_streams), restored
 * by tsdf_pipeline_destroy.  A volume takes ONE pipeline or tracker at a time: tsdf_pipeline_create / tsdf_tracker_create on a
 * volume that is still attached return TSDF_ERR_INVALID (destroy the previous one first).  A frame announced as `next` is
 * recognised in the following step BY ITS DEVICE POINTER: every frame in flight needs a buffer of its own -- refilling one staging
 * buffer between the announcement and the step integrates the image that was filtered ahead, not the new contents.  All pointers are device pointers: width * height uint16 depth (it must stay valid until the step
 * after the one it was announced to has run), 3 * width * height floats per map (device_normals may be NULL). */
typedef struct tsdf_pipeline tsdf_pipeline;
typedef struct tsdf_camera_matrices {   /* camera.pose(), inverse_pose(), k(), kinv(): column-major, as everywhere in this header */
    float pose[16], inv_pose[16], k[9], kinv[9];
} tsdf_camera_matrices;
#define TSDF_PIPELINE_OVERLAP 1          /* the next frame's filter / culling on a second, lower-priority stream                */
#define TSDF_PIPELINE_EQUAL_PRIORITY 2   /* diagnostics: both streams at the same priority (always so with a slab exchange)      */
#define TSDF_PIPELINE_EXCHANGE_STREAM 4  /* slab exchange + merge on a third stream                                            */
#define TSDF_PIPELINE_NO_TIGHTEN_AHEAD 8 /* diagnostics: the periodic tightening of the ray caster's flags stays in front of the ray cast */
int tsdf_pipeline_create(tsdf_volume *volume, const tsdf_bilateral *filter, uint32_t width, uint32_t height, int flags,
                         tsdf_slab_exchange *exchange /* NULL: a whole volume */, tsdf_pipeline **out);
int tsdf_pipeline_step(tsdf_pipeline *pipeline, const uint16_t *device_depth, const tsdf_camera_matrices *camera,
                       float *device_vertices, float *device_normals, const uint16_t *next_device_depth /* or NULL */,
                       const tsdf_camera_matrices *next_camera /* or NULL */);
/* tsdf_pipeline_step with a colour integrate of the FILTERED frame and device_rgb (3 * width * height bytes, registered to the depth
 * image; it must stay valid until this step's integrate has run on the step's stream: nothing of it is read ahead).  device_colours
 * (3 * width * height bytes, or NULL): the colour of the voxel every vertex of the ray cast lies in, sampled on the step's stream as
 * tsdf_raycast_colour_device samples it.  Distances, weights, vertices and normals are those of tsdf_pipeline_step.  Refused
 * (TSDF_ERR_INVALID, with a message): a volume without colour enabled, a sharded pipeline, a NULL rgb frame. */
int tsdf_pipeline_step_colour(tsdf_pipeline *pipeline, const uint16_t *device_depth, const uint8_t *device_rgb,
                              const tsdf_camera_matrices *camera, float *device_vertices, float *device_normals,
                              uint8_t *device_colours /* or NULL */, const uint16_t *next_device_depth /* or NULL */,
                              const tsdf_camera_matrices *next_camera /* or NULL */);
int tsdf_pipeline_synchronize(tsdf_pipeline *pipeline);
/* The pipeline's hipStream_t handles (side_stream is NULL without TSDF_PIPELINE_OVERLAP), e.g. to order the caller's own work. */
int tsdf_pipeline_streams(const tsdf_pipeline *pipeline, void **main_stream, void **side_stream);
/* The record buffers of a sharded pipeline (NULL for a whole volume): this rank's n_pixels records, all ranks' world x n_pixels. */
int tsdf_pipeline_hit_buffers(const tsdf_pipeline *pipeline, tsdf_hit_record **device_mine, tsdf_hit_record **device_all);
int tsdf_pipeline_destroy(tsdf_pipeline *pipeline);

/* ---- the tracked loop (BASELINE configs[4]) ------------------------------------------------------------------------------- */
/* Frame-to-model tracking: what src/Tools/tsdf_icp.cpp:115-198 does for one frame (render the volume to a depth image from a pose,
 * ICPOdometry against the new frame) composed with kinfu.cpp's integrate, frame after frame on device buffers:
 *     tsdf_tracker_filter(depth)                      bilateral filter (+ tile maxima) and, from the second frame on, initICP of
 *                                                     the filtered frame -- on a second, lower-priority stream (TSDF_PIPELINE_OVERLAP)
 *     tsdf_tracker_align(previous camera, T, ...)     ray cast from the previous pose, render_to_depth_image, initICPModel,
 *                                                     getIncrementalTransformation; blocks for T (current camera -> previous
 *                                                     camera, metres, column-major double as tsdf_icp_get_incremental_transformation)
 *     tsdf_tracker_integrate(camera)                  the filtered frame at the pose the caller composed (asynchronous)
 * The first frame is only filtered and integrated.  The tracker owns its streams, events and frame buffers; while it lives the
 * volume's and the ICP object's stream are its own. */
typedef struct tsdf_tracker tsdf_tracker;
int tsdf_tracker_create(tsdf_volume *volume, const tsdf_bilateral *filter, tsdf_icp *icp, uint32_t width, uint32_t height,
                        float depth_cutoff, int flags /* TSDF_PIPELINE_OVERLAP or 0 */, tsdf_tracker **out);
int tsdf_tracker_filter(tsdf_tracker *tracker, const uint16_t *device_depth);
int tsdf_tracker_align(tsdf_tracker *tracker, const tsdf_camera_matrices *previous, double T_prev_curr[16] /* in: start, out */,
                       float *last_error, float *last_inliers);
/* tsdf_tracker_align without the ray cast ("field alignment"): the filtered current frame becomes camera-frame points through
 * tsdf_depth_to_points_device (kinv; the tracker's depth cutoff) at steps 4, 2 and 1, then tsdf_aligner_run with ICP's 4 / 5 / 10
 * iterations, coarse to fine, on the tracker's main stream, the gate at the volume's truncation distance.  T_world_cam: camera ->
 * world in volume units (what tsdf_camera_matrices::pose holds, as doubles), in: the prediction (e.g. the previous pose), out: the
 * aligned pose; residual / inliers as tsdf_aligner_run.  Blocks for the result.  The aligner and the three point buffers are created
 * on the first call: a tracker that never calls this allocates and launches nothing new.  tsdf_tracker_filter still runs ICP's
 * initICP for the new frame whichever align follows (no existing behaviour changes; dropping it for field-only users is a later
 * change). */
int tsdf_tracker_align_field(tsdf_tracker *tracker, const float kinv[9], double T_world_cam[16] /* in: prediction, out */,
                             float *residual, float *inliers);
/* tsdf_tracker_align_field with the colour term ("colour alignment"): the same points at steps 4, 2 and 1 with 4 / 5 / 10 iterations,
 * the intensities of device_rgb (3 * width * height bytes, registered to the depth image) at the same steps through
 * tsdf_rgb_to_intensity_device, then tsdf_aligner_run_colour.  residual / inliers (either may be NULL): {geometric, colour}.  The three
 * intensity buffers are created on the first call.  Refused as tsdf_aligner_run_colour refuses, and with a NULL rgb frame. */
int tsdf_tracker_align_field_colour(tsdf_tracker *tracker, const float kinv[9], const uint8_t *device_rgb, float colour_gate,
                                    float colour_weight, double T_world_cam[16] /* in: prediction, out */, float residual[2],
                                    float inliers[2]);
int tsdf_tracker_integrate(tsdf_tracker *tracker, const tsdf_camera_matrices *camera);
/* tsdf_tracker_integrate plus the colour of device_rgb (as tsdf_pipeline_step_colour: the filtered frame, rgb valid until the
 * integrate has run on the tracker's stream; refused without colour enabled or with a NULL rgb frame). */
int tsdf_tracker_integrate_colour(tsdf_tracker *tracker, const tsdf_camera_matrices *camera, const uint8_t *device_rgb);
/* Windowed tracking: n = 0 (the default) is off -- nothing is kept, nothing allocated.  n >= 1 makes the tracker keep device copies of
 * the last n filtered frames it integrated with their camera matrices (n * width * height * 2 bytes); tsdf_tracker_integrate and
 * tsdf_tracker_integrate_colour then integrate the new frame and, once n frames are kept, take the oldest back out on the same stream
 * (tsdf_deintegrate_device; colour words stay): the volume holds exactly the last n frames.  Refused with a message when the volume has
 * a weight cap (TSDF_ERR_INVALID), when the ring cannot be allocated (TSDF_ERR_NOMEM) and between tsdf_tracker_filter and the integrate
 * of that frame (TSDF_ERR_INVALID).  Setting n again, to the same value too, resizes the ring and forgets the frames it held; the volume
 * is left as it is. */
int tsdf_tracker_set_window(tsdf_tracker *tracker, uint32_t n);
int tsdf_tracker_window(const tsdf_tracker *tracker, uint32_t *n);
/* Weighted tracking ("weighted integration"): flags = 0 (the default) is off -- the plain integrate, nothing allocated.  With flags a
 * combination of TSDF_WEIGHTS_*, tsdf_tracker_integrate and tsdf_tracker_integrate_colour compute that model's weights from the filtered
 * frame they hold (tsdf_depth_weights_device with the camera's kinv and z_ref, on the tracker's main stream, into a buffer made on the
 * first such frame) and fuse it with tsdf_integrate_weighted_device: the volume goes to fp32 weights.  Refused with a message
 * (TSDF_ERR_INVALID) as tsdf_depth_weights refuses flags and z_ref, and together with a window, in either order: there is no weighted
 * removal. */
int tsdf_tracker_set_weighting(tsdf_tracker *tracker, uint32_t flags, float z_ref);
int tsdf_tracker_weighting(const tsdf_tracker *tracker, uint32_t *flags, float *z_ref /* or NULL */);
/* Dynamic rejection ("frame differences"): params = NULL (the default) is off -- nothing is allocated or launched, and every path is bit
 * for bit what it is without this call.  With params, tsdf_tracker_integrate and tsdf_tracker_integrate_colour run, before they fuse and
 * on the tracker's main stream:
 *     1. tsdf_raycast_depth_device at the camera they are given, into a buffer of the tracker's own (the cast's bits do not depend on
 *        its scheduling);
 *     2. tsdf_frame_diff_compare_device of the filtered frame with it (tolerance, quadratic);
 *     3. tsdf_frame_diff_cluster (connectivity, depth_step, min_pixels);
 *     4. tsdf_frame_diff_mask_device (dilate) into a mask and a masked frame of the tracker's own;
 *     5. the integrate they would have run, of the MASKED frame.
 * The first frame fuses unmasked: the model is empty, every pixel is NO_MODEL or NO_FRAME and nothing is listed.  With a window the
 * ring keeps the masked frame (de-integration needs the frame exactly as it was fused); with weighting the weights are computed from
 * the masked frame.  The frame differences handle and the three buffers (5 bytes a pixel) are made by this call and freed by the call
 * that turns it off.  Cost per frame: one more ray cast and two host synchronisations (the list's and the table's), so the integrate
 * is no longer asynchronous (measured at 512^3 and 640 x 480: 1.03 ms a frame against 0.44 ms with rejection off).  Out of scope: ICP and the field aligners still see the unmasked frame; feeding the previous frame's mask
 * to the next align is a later change.  Z-slab volumes are refused as tsdf_tracker_create refuses them.
 * Refused (TSDF_ERR_INVALID) with a connectivity other than 4 or 8 or a dilate above 32, and between tsdf_tracker_filter and the
 * integrate of that frame.
 * tsdf_tracker_last_rejection: the result of the last integrated frame -- counts[5] by state, the number of kept blobs, the device mask
 * (width * height uint8, the tracker's own, valid until the next integrate); any pointer may be NULL.  Waits for the main stream.
 * Refused while rejection is off and before the first frame has been integrated with it. */
typedef struct tsdf_diff_rejection {
    uint32_t tolerance, quadratic;   /* tsdf_diff_params */
    uint32_t connectivity;           /* 4 or 8 */
    uint32_t depth_step, min_pixels;
    uint32_t dilate;                 /* 0..32 */
} tsdf_diff_rejection;
int tsdf_tracker_set_dynamic_rejection(tsdf_tracker *tracker, const tsdf_diff_rejection *params /* NULL: off, the default */);
int tsdf_tracker_dynamic_rejection(const tsdf_tracker *tracker, int *on, tsdf_diff_rejection *params /* or NULL */);
int tsdf_tracker_last_rejection(const tsdf_tracker *tracker, uint64_t counts[5], uint64_t *n_blobs, const uint8_t **device_mask);
int tsdf_tracker_synchronize(tsdf_tracker *tracker);
int tsdf_tracker_streams(const tsdf_tracker *tracker, void **main_stream, void **side_stream);
/* The ICP inputs of the last aligned frame: the rendered model depth and the filtered frame (width * height uint16, device). */
int tsdf_tracker_buffers(const tsdf_tracker *tracker, const uint16_t **device_model, const uint16_t **device_filtered);
int tsdf_tracker_destroy(tsdf_tracker *tracker);

/* ---- ICP tracking: replaces third_party/ICP_CUDA ------------------------------------------ */
/* ICPOdometry::ICPOdometry (third_party/ICP_CUDA/ICPOdometry.cpp:10-57): three pyramid levels of vertex / normal maps for
 * the model ("prev") and the current frame; angle_thresh is the sine of the angle gate. */
int tsdf_icp_create(int width, int height, float cx, float cy, float fx, float fy, float dist_thresh, float angle_thresh,
                    tsdf_icp **out);
void tsdf_icp_destroy(tsdf_icp *icp);
int tsdf_icp_set_stream(tsdf_icp *icp, void *hip_stream);
int tsdf_icp_stream(const tsdf_icp *icp, void **hip_stream);   /* the stream its kernels are enqueued on now */
/* ICPOdometry::initICP (model = 0, ICPOdometry.cpp:64-78) / initICPModel (model = 1, :80-95): upload the depth (uint16 mm),
 * pyrDown twice, createVMap + createNMap per level (Cuda/pyrdown.cu).  The host variant synchronises like the reference;
 * the _device variant takes a device pointer and does not. */
int tsdf_icp_init(tsdf_icp *icp, int model, const uint16_t *host_depth, float depth_cutoff);
int tsdf_icp_init_device(tsdf_icp *icp, int model, const uint16_t *device_depth, float depth_cutoff);
/* estimateStep (Cuda/estimate.cu:215-281) for one pyramid level: R (3x3 column-major, Eigen's data()) and t map current-frame
 * points into the model frame; returns the 6x6 normal matrix A, b, {sum of squared residuals, inliers}. */
int tsdf_icp_estimate_step(tsdf_icp *icp, int level, const float R[9], const float t[3], float A[36], float b[6],
                           float residual_inliers[2]);
/* ICPOdometry::getIncrementalTransformation (ICPOdometry.cpp:97-136): 4/5/10 iterations from the coarsest level down,
 * T <- exp(A^-1 b) * T each (the solve and the exponential run on the device, the pose never leaves it between
 * iterations).  T_prev_curr: 4x4 column-major double (Sophus::SE3d::matrix().data()), in/out. */
int tsdf_icp_get_incremental_transformation(tsdf_icp *icp, double T_prev_curr[16], float *last_error, float *last_inliers);
/* Tests / diagnostics: which = 0 vmap_prev, 1 nmap_prev, 2 vmap_curr, 3 nmap_curr (3*rows x cols floats of the level);
 * the depth pyramid of the last init call. */
int tsdf_icp_get_map(const tsdf_icp *icp, int which, int level, float *host_map);
int tsdf_icp_get_depth_level(const tsdf_icp *icp, int level, uint16_t *host_depth);

/* ---- bilateral filter -------------------------------------------------------------------- */
/* Replaces BilateralFilter::BilateralFilter / ~BilateralFilter (src/BilateralFilter.cpp:15-51):
 * builds the spatial kernel and the similarity table on the host exactly as the reference
 * does and uploads them. */
int tsdf_bilateral_create(float sigma_colour, float sigma_space, tsdf_bilateral **out);
int tsdf_bilateral_destroy(tsdf_bilateral *filter);
/* Replace BilateralFilter::filter (src/BilateralFilter.cpp:124-130, 53-121): in place on a host
 * image, blocking.  8 bit: bit-identical to the reference.  16 bit: the reference's path is
 * undefined behaviour; the semantics implemented are stated in DESIGN.md. */
int tsdf_bilateral_filter_u8(const tsdf_bilateral *filter, uint8_t *host_image, int width, int height);
int tsdf_bilateral_filter_u16(const tsdf_bilateral *filter, uint16_t *host_image, int width, int height);
/* Device variants: in != out, asynchronous on hip_stream. */
int tsdf_bilateral_filter_u8_device(const tsdf_bilateral *filter, const uint8_t *device_in,
                                    uint8_t *device_out, int width, int height, void *hip_stream);
int tsdf_bilateral_filter_u16_device(const tsdf_bilateral *filter, const uint16_t *device_in,
                                     uint16_t *device_out, int width, int height, void *hip_stream);
/* The same filter; each workgroup also leaves the largest filtered value of its TSDF_DEPTH_TILE x TSDF_DEPTH_TILE pixel
 * tile in device_tile_max[tile_y * ceil(width / TSDF_DEPTH_TILE) + tile_x] (0 = the tile holds no valid depth).  Hand the
 * array to tsdf_integrate_device_tiles with the filtered image: integrate's culling then skips its own pass over the image.
 * (No reference counterpart: the reference filters on the host and integrates every voxel.) */
#define TSDF_DEPTH_TILE 16
int tsdf_bilateral_filter_u16_device_tiles(const tsdf_bilateral *filter, const uint16_t *device_in,
                                           uint16_t *device_out, int width, int height,
                                           uint16_t *device_tile_max, void *hip_stream);

/* ---- measurement aid (no reference counterpart) ------------------------------------------ */
/* Device-to-device copy of `bytes` (a multiple of 16; two internal buffers) with a float4 copy kernel, `reps` times on
 * `hip_stream`, timed with HIP events on that stream: *gb_per_s = read + write bytes per second of the best repetition / 1e9.
 * bench.py reports it beside the nominal HBM peak as the practical ceiling of a streaming kernel on this box. */
int tsdf_measure_copy_bandwidth(size_t bytes, int reps, void *hip_stream, double *gb_per_s);
/* The same for the access shape of integrate: two arrays of a 512^3 float grid updated IN PLACE (read, modify, write back)
 * brick by brick -- workgroups of 4 waves walking 32 planes of a 64 x 4 x 32 voxel brick, a wave per 256-byte row segment, 4
 * planes in flight -- with no projection work at all: *gb_per_s = (read + write bytes of both arrays) per second / 1e9, best of
 * `reps`.  The ceiling an in-place update of every voxel could reach with integrate's memory walk. */
int tsdf_measure_update_bandwidth(int reps, void *hip_stream, double *gb_per_s);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_AMD_H */
