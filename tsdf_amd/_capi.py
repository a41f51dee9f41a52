"""ctypes binding of the C ABI declared in include/tsdf_amd.h (tsdf_amd/lib/libtsdf_hip.so).

There is no fallback: if the HIP library is missing or fails to load, importing this module
raises.  The CPU checker used by the tests lives outside this package and is never loaded from here.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (TSDF_HIP_LIB: another build of the same library, for A/B timing of kernel variants on one box -- tools/ab_variants.sh)
LIB_PATH = os.environ.get("TSDF_HIP_LIB") or os.path.join(_HERE, "lib", "libtsdf_hip.so")

TSDF_OK, TSDF_ERR_INVALID, TSDF_ERR_DEVICE, TSDF_ERR_NOMEM = 0, 1, 2, 3
TSDF_FIELD_UNIT_GRADIENT = 1
TSDF_RAYS_BAND_ONLY = 1
TSDF_MESH_NORMALS, TSDF_MESH_COLOURS = 1, 2
TSDF_MESH_KEEP_LARGEST = 1
TSDF_CLASS_VOID = 0xFFFF
TSDF_SMOOTH_PIN_BOUNDARY, TSDF_SMOOTH_NORMALS = 1, 2
TSDF_ESDF_FILL_UNKNOWN = 1
TSDF_GAIN_KEEP_MASK = 1
TSDF_REACH_THROUGH_UNKNOWN = 1
TSDF_REACH_UNREACHED = 0xFFFFFFFF
TSDF_REACH_COST_FACE, TSDF_REACH_COST_EDGE, TSDF_REACH_COST_CORNER = 10, 14, 17
TSDF_OBJECT_NONE = 0xFFFFFFFF
TSDF_SCENE_FLOW_DEFORMED = 1
TSDF_SNAPSHOT_BRICK, TSDF_SNAPSHOT_COLOUR = 8, 1
TSDF_RESTORE_KEEP_OTHERS, TSDF_SELECT_OUTSIDE = 1, 1
TSDF_WEIGHTS_INVERSE_SQUARE, TSDF_WEIGHTS_COSINE = 1, 2
TSDF_COLUMNS_REVERSED = 1
TSDF_CELL_NO_GROUND, TSDF_CELL_TRAVERSABLE, TSDF_CELL_BLOCKED = 0, 1, 2
TSDF_RENDER_CULL_BACK = 1
TSDF_RENDER_LARGE_BOX = 256
TSDF_RENDER_MISS = 0xFFFFFFFF


class TsdfError(RuntimeError):
    """A C-ABI call failed with TSDF_ERR_DEVICE / TSDF_ERR_NOMEM."""


class VolumeInfo(C.Structure):
    """struct tsdf_volume_info (include/tsdf_amd.h)."""
    _fields_ = [("size", C.c_uint32 * 3), ("z_begin", C.c_uint32), ("z_end", C.c_uint32),
                ("z_store_begin", C.c_uint32), ("z_store_end", C.c_uint32),
                ("physical_size", C.c_float * 3), ("voxel_size", C.c_float * 3), ("offset", C.c_float * 3),
                ("offset_at_clear", C.c_float * 3), ("truncation_distance", C.c_float),
                ("max_weight", C.c_float), ("global_translation", C.c_float * 3),
                ("global_rotation", C.c_float * 3), ("deformation_materialised", C.c_int32),
                ("fast_division_verified", C.c_int32)]


class MeshInfo(C.Structure):
    """struct tsdf_mesh_info (include/tsdf_amd.h)."""
    _fields_ = [("n_vertices", C.c_uint64), ("n_indices", C.c_uint64), ("flags", C.c_uint32), ("box", C.c_uint32 * 6)]


class ComponentsInfo(C.Structure):
    """struct tsdf_components_info (include/tsdf_amd.h)."""
    _fields_ = [("n_components", C.c_uint64), ("n_triangles", C.c_uint64), ("largest_triangles", C.c_uint64),
                ("largest_label", C.c_uint32)]


class SceneFlowInfo(C.Structure):
    """struct tsdf_scene_flow_info (include/tsdf_amd.h)."""
    _fields_ = [("n_vertices", C.c_uint64), ("n_correspondences", C.c_uint64), ("n_nodes_moved", C.c_uint64)]


class EsdfInfo(C.Structure):
    """struct tsdf_esdf_info (include/tsdf_amd.h)."""
    _fields_ = [("size", C.c_uint32 * 3), ("flags", C.c_uint32), ("voxel_size", C.c_float * 3), ("offset", C.c_float * 3),
                ("max_distance", C.c_float), ("n_sites", C.c_uint64)]


class ExplorerInfo(C.Structure):
    """struct tsdf_explorer_info (include/tsdf_amd.h)."""
    _fields_ = [("size", C.c_uint32 * 3), ("connectivity", C.c_uint32), ("voxel_size", C.c_float * 3), ("offset", C.c_float * 3),
                ("n_unknown", C.c_uint64), ("n_free", C.c_uint64), ("n_occupied", C.c_uint64), ("n_frontiers", C.c_uint64),
                ("n_clusters", C.c_uint64), ("n_listed_clusters", C.c_uint64)]


class FrontierCluster(C.Structure):
    """struct tsdf_frontier_cluster (include/tsdf_amd.h): 56 bytes, sum at offset 32."""
    _fields_ = [("label", C.c_uint32), ("size", C.c_uint32), ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("sum", C.c_uint64 * 3)]


class DiffParams(C.Structure):
    """struct tsdf_diff_params (include/tsdf_amd.h)."""
    _fields_ = [("tolerance", C.c_uint32), ("quadratic", C.c_uint32)]


class FrameDiffInfo(C.Structure):
    """struct tsdf_frame_diff_info (include/tsdf_amd.h): 88 bytes, counts at offset 32."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("tolerance", C.c_uint32), ("quadratic", C.c_uint32),
                ("connectivity", C.c_uint32), ("depth_step", C.c_uint32), ("min_pixels", C.c_uint32), ("reserved", C.c_uint32),
                ("counts", C.c_uint64 * 5), ("n_blobs", C.c_uint64), ("n_kept_blobs", C.c_uint64)]


class DiffBlob(C.Structure):
    """struct tsdf_diff_blob (include/tsdf_amd.h): 56 bytes, sum_x at offset 32."""
    _fields_ = [("label", C.c_uint32), ("size", C.c_uint32), ("lo", C.c_uint32 * 2), ("hi", C.c_uint32 * 2), ("min_depth", C.c_uint32),
                ("max_depth", C.c_uint32), ("sum_x", C.c_uint64), ("sum_y", C.c_uint64), ("sum_depth", C.c_uint64)]


class DiffRejection(C.Structure):
    """struct tsdf_diff_rejection (include/tsdf_amd.h)."""
    _fields_ = [("tolerance", C.c_uint32), ("quadratic", C.c_uint32), ("connectivity", C.c_uint32), ("depth_step", C.c_uint32),
                ("min_pixels", C.c_uint32), ("dilate", C.c_uint32)]


class ReachInfo(C.Structure):
    """struct tsdf_reach_info (include/tsdf_amd.h): 88 bytes, n_traversable at offset 56, rounds at 80."""
    _fields_ = [("size", C.c_uint32 * 3), ("connectivity", C.c_uint32), ("voxel_size", C.c_float * 3), ("offset", C.c_float * 3),
                ("flags", C.c_uint32), ("clearance", C.c_float), ("max_cost", C.c_uint32), ("max_cost_reached", C.c_uint32),
                ("n_traversable", C.c_uint64), ("n_reached", C.c_uint64), ("n_seed_voxels", C.c_uint64), ("rounds", C.c_uint64)]


class ReachCluster(C.Structure):
    """struct tsdf_reach_cluster (include/tsdf_amd.h): 16 bytes."""
    _fields_ = [("label", C.c_uint32), ("cost", C.c_uint32), ("voxel", C.c_uint32), ("reserved", C.c_uint32)]


class Column(C.Structure):
    """struct tsdf_column (include/tsdf_amd.h): 32 bytes, top at offset 12, height at 24."""
    _fields_ = [("n_unknown", C.c_uint32), ("n_free", C.c_uint32), ("n_occupied", C.c_uint32), ("top", C.c_int32), ("bottom", C.c_int32),
                ("headroom", C.c_uint32), ("height", C.c_float), ("min_distance", C.c_float)]


class ColumnsInfo(C.Structure):
    """struct tsdf_columns_info (include/tsdf_amd.h): 136 bytes, lo at offset 40, n_unknown at 72, max_step at 128."""
    _fields_ = [("size", C.c_uint32 * 3), ("axis", C.c_uint32), ("voxel_size", C.c_float * 3), ("offset", C.c_float * 3),
                ("lo", C.c_uint32), ("hi", C.c_uint32), ("flags", C.c_uint32), ("has_esdf", C.c_uint32), ("map_size", C.c_uint32 * 2),
                ("map_axes", C.c_uint32 * 2), ("n_unknown", C.c_uint64), ("n_free", C.c_uint64), ("n_occupied", C.c_uint64),
                ("n_ground", C.c_uint64), ("n_no_ground", C.c_uint64), ("n_traversable", C.c_uint64), ("n_blocked", C.c_uint64),
                ("max_step", C.c_uint32), ("min_headroom", C.c_uint32)]


class RenderTargets(C.Structure):
    """struct tsdf_render_targets (include/tsdf_amd.h): 48 bytes, six optional pointers."""
    _fields_ = [("triangle", C.c_void_p), ("z", C.c_void_p), ("depth", C.c_void_p), ("vertices", C.c_void_p), ("normals", C.c_void_p),
                ("rgb", C.c_void_p)]


class RenderInfo(C.Structure):
    """struct tsdf_render_info (include/tsdf_amd.h): 40 bytes."""
    _fields_ = [("n_triangles", C.c_uint64), ("n_live", C.c_uint64), ("n_dropped", C.c_uint64), ("n_large", C.c_uint64),
                ("n_pixels_hit", C.c_uint64)]


class ObjectsInfo(C.Structure):
    """struct tsdf_objects_info (include/tsdf_amd.h): 72 bytes, n_labelled at offset 48."""
    _fields_ = [("size", C.c_uint32 * 3), ("connectivity", C.c_uint32), ("voxel_size", C.c_float * 3), ("offset", C.c_float * 3),
                ("min_votes", C.c_uint32), ("min_size", C.c_uint32), ("n_labelled", C.c_uint64), ("n_objects", C.c_uint64),
                ("n_listed_objects", C.c_uint64)]


class ClassObject(C.Structure):
    """struct tsdf_class_object (include/tsdf_amd.h): 72 bytes, sum at offset 32, votes at 56, class_id at 64."""
    _fields_ = [("label", C.c_uint32), ("size", C.c_uint32), ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("sum", C.c_uint64 * 3),
                ("votes", C.c_uint64), ("class_id", C.c_uint32), ("reserved", C.c_uint32)]


class SnapshotInfo(C.Structure):
    """struct tsdf_snapshot_info (include/tsdf_amd.h)."""
    _fields_ = [("size", C.c_uint32 * 3), ("bricks", C.c_uint32 * 3), ("flags", C.c_uint32), ("weight_bits", C.c_uint32),
                ("weight_bound", C.c_uint32), ("fill_distance", C.c_float), ("voxel_size", C.c_float * 3), ("offset", C.c_float * 3),
                ("n_bricks", C.c_uint64), ("bytes", C.c_uint64)]


class HostSparseInfo(C.Structure):
    """struct tsdf_host_sparse_info (tsdf_amd/host/src/host_capi.cpp): the header of a .tsdfs file."""
    _fields_ = [("size", C.c_uint32 * 3), ("physical_size", C.c_float * 3), ("offset", C.c_float * 3), ("truncation_distance", C.c_float),
                ("max_weight", C.c_float), ("global_translation", C.c_float * 3), ("global_rotation", C.c_float * 3), ("brick", C.c_uint32),
                ("flags", C.c_uint32), ("weight_bits", C.c_uint32), ("weight_bound", C.c_uint32), ("fill_distance", C.c_float),
                ("reserved", C.c_uint32), ("n_bricks", C.c_uint64)]


class AlignStage(C.Structure):
    """struct tsdf_align_stage (include/tsdf_amd.h)."""
    _fields_ = [("device_points", C.c_void_p), ("n", C.c_uint32), ("iterations", C.c_uint32)]


class AlignColourStage(C.Structure):
    """struct tsdf_align_colour_stage (include/tsdf_amd.h)."""
    _fields_ = [("device_points", C.c_void_p), ("device_intensity", C.c_void_p), ("n", C.c_uint32), ("iterations", C.c_uint32)]


class CameraMatrices(C.Structure):
    """struct tsdf_camera_matrices (include/tsdf_amd.h)."""
    _fields_ = [("pose", C.c_float * 16), ("inv_pose", C.c_float * 16), ("k", C.c_float * 9), ("kinv", C.c_float * 9)]


#: tsdf_exchange_fn (include/tsdf_amd.h): int (*)(void *user, const record *mine, record *all, uint32_t n_pixels, void *stream)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "tsdf_amd: %s is missing -- build it with `make hip` (or `python -c 'import __graft_entry__ as g; "
            "g.build()'`). There is no CPU fallback." % LIB_PATH)
    # RTLD_GLOBAL on purpose: torch ships its own libamdhip64 under a different NEEDED name, so a process can hold
    # two HIP runtimes; with the first-loaded one in the global scope everything binds to that single runtime
    # whichever of torch / this library is imported first.  (Only tsdf_* and tsdf:: symbols are exported here.)
    return C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)


lib = _load()

_vp, _fp = C.c_void_p, C.POINTER(C.c_float)
_u32, _f, _i = C.c_uint32, C.c_float, C.c_int
_SIGS = {
    "tsdf_last_error": (C.c_char_p, []),
    "tsdf_build_arch": (C.c_char_p, []),
    "tsdf_device_count": (_i, [C.POINTER(_i)]),
    "tsdf_set_device": (_i, [_i]),
    "tsdf_get_device": (_i, [C.POINTER(_i)]),
    "tsdf_device_alloc": (_i, [C.c_size_t, C.POINTER(_vp)]),
    "tsdf_device_free": (_i, [_vp]),
    "tsdf_device_upload": (_i, [_vp, _vp, C.c_size_t]),
    "tsdf_device_download": (_i, [_vp, _vp, C.c_size_t]),
    "tsdf_stream_synchronize": (_i, [_vp]),
    "tsdf_volume_create": (_i, [_u32, _u32, _u32, _f, _f, _f, C.POINTER(_vp)]),
    "tsdf_volume_create_slab": (_i, [_u32, _u32, _u32, _f, _f, _f, _u32, _u32, C.POINTER(_vp)]),
    "tsdf_volume_destroy": (_i, [_vp]),
    "tsdf_volume_set_stream": (_i, [_vp, _vp]),
    "tsdf_volume_stream": (_i, [_vp, C.POINTER(_vp)]),
    "tsdf_volume_synchronize": (_i, [_vp]),
    "tsdf_volume_clear": (_i, [_vp]),
    "tsdf_volume_get_info": (_i, [_vp, C.POINTER(VolumeInfo)]),
    "tsdf_volume_set_offset": (_i, [_vp, _f, _f, _f]),
    "tsdf_volume_set_header": (_i, [_vp, _fp, _f, _f, _fp, _fp]),
    "tsdf_volume_mark_dirty": (_i, [_vp]),
    "tsdf_volume_distances": (_i, [_vp, C.POINTER(_vp)]),
    "tsdf_volume_weights": (_i, [_vp, C.POINTER(_vp)]),
    "tsdf_volume_weight_storage": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "tsdf_volume_last_raycast_kind": (_i, [_vp, C.POINTER(_i)]),
    "tsdf_volume_last_cell_list": (_i, [_vp, C.POINTER(C.c_uint32)]),
    "tsdf_volume_set_weight_storage": (_i, [_vp, _i]),
    "tsdf_volume_set_weight_cap": (_i, [_vp, C.c_uint32]),
    "tsdf_volume_weight_cap": (_i, [_vp, C.POINTER(C.c_uint32)]),
    "tsdf_selftest_count_division": (_i, [_u32, _u32, C.POINTER(C.c_uint64)]),
    "tsdf_selftest_bilateral_chain_taps": (_i, [C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tsdf_selftest_bilateral_chain_image": (_i, [_f, _f, _vp, _i, _i, _i, _vp, C.POINTER(C.c_uint64)]),
    "tsdf_selftest_cell_boxes": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _f, _f, C.c_size_t, _vp, _i, _vp, _vp]),
    "tsdf_selftest_cell_owner": (_i, [_vp, _vp, _i, C.c_size_t, _vp, _vp, _vp, _vp]),
    "tsdf_selftest_gn_finish": (_i, [_vp, _i, _vp, _i, _vp]),
    "tsdf_volume_deformation": (_i, [_vp, C.POINTER(_vp)]),
    "tsdf_volume_set_distance_data": (_i, [_vp, _vp]),
    "tsdf_volume_set_weight_data": (_i, [_vp, _vp]),
    "tsdf_volume_set_deformation": (_i, [_vp, _vp]),
    "tsdf_volume_get_distance_data": (_i, [_vp, _vp]),
    "tsdf_measure_copy_bandwidth": (_i, [C.c_size_t, _i, _vp, C.POINTER(C.c_double)]),
    "tsdf_measure_update_bandwidth": (_i, [_i, _vp, C.POINTER(C.c_double)]),
    "tsdf_volume_get_weight_data": (_i, [_vp, _vp]),
    "tsdf_volume_get_deformation_planes": (_i, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "tsdf_volume_set_offset_at_clear": (_i, [_vp, _vp]),
    "tsdf_integrate": (_i, [_vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp]),
    "tsdf_integrate_device": (_i, [_vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp]),
    "tsdf_deintegrate": (_i, [_vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp]),
    "tsdf_deintegrate_device": (_i, [_vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp]),
    "tsdf_integrate_weighted": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp]),
    "tsdf_integrate_weighted_device": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp]),
    "tsdf_depth_weights": (_i, [_u32, _u32, _vp, _fp, _u32, _f, _vp]),
    "tsdf_depth_weights_device": (_i, [_u32, _u32, _vp, _fp, _u32, _f, _vp, _vp]),
    "tsdf_integrate_device_tiles": (_i, [_vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp, _vp]),
    "tsdf_integrate_prepare_device_tiles": (_i, [_vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp, _vp, _vp]),
    "tsdf_integrate_discard_prepared": (_i, [_vp]),
    "tsdf_volume_set_timing": (_i, [_vp, _i]),
    "tsdf_volume_kernel_time": (_i, [_vp, _i, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "tsdf_volume_set_counting": (_i, [_vp, _i]),
    "tsdf_volume_last_updated_voxels": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_volume_last_distance_stores": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_volume_enable_colour": (_i, [_vp, _i]),
    "tsdf_volume_colour_enabled": (_i, [_vp, C.POINTER(_i)]),
    "tsdf_volume_colours": (_i, [_vp, C.POINTER(_vp)]),
    "tsdf_volume_get_colour_data": (_i, [_vp, _vp]),
    "tsdf_volume_set_colour_data": (_i, [_vp, _vp]),
    "tsdf_integrate_colour": (_i, [_vp, _vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp]),
    "tsdf_integrate_colour_device": (_i, [_vp, _vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp]),
    "tsdf_volume_sample_colours_device": (_i, [_vp, C.c_uint64, _vp, _vp, _vp]),
    "tsdf_raycast_colour": (_i, [_vp, _u32, _u32, _fp, _fp, _vp, _vp, _vp]),
    "tsdf_raycast_colour_device": (_i, [_vp, _u32, _u32, _fp, _fp, _vp, _vp, _vp]),
    "tsdf_volume_enable_classes": (_i, [_vp, _i]),
    "tsdf_volume_classes_enabled": (_i, [_vp, C.POINTER(_i)]),
    "tsdf_volume_classes": (_i, [_vp, C.POINTER(_vp)]),
    "tsdf_volume_get_class_data": (_i, [_vp, _vp]),
    "tsdf_volume_set_class_data": (_i, [_vp, _vp]),
    "tsdf_integrate_classes": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp]),
    "tsdf_integrate_classes_device": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp]),
    "tsdf_volume_sample_classes_device": (_i, [_vp, C.c_uint64, _vp, _vp, _vp, _vp]),
    "tsdf_raycast_classes": (_i, [_vp, _u32, _u32, _fp, _fp, _vp, _vp, _vp, _vp]),
    "tsdf_raycast_classes_device": (_i, [_vp, _u32, _u32, _fp, _fp, _vp, _vp, _vp, _vp]),
    "tsdf_volume_class_counts": (_i, [_vp, _u32, _u32, _vp]),
    "tsdf_volume_class_counts_device": (_i, [_vp, _u32, _u32, _vp, _vp]),
    "tsdf_volume_sample_field_device": (_i, [_vp, C.c_uint64, _vp, _vp, _vp, _vp, _i, _vp]),
    "tsdf_volume_sample_field": (_i, [_vp, C.c_uint64, _vp, _vp, _vp, _vp, _i]),
    "tsdf_raycast_gradient_normals_device": (_i, [_vp, _u32, _u32, _fp, _fp, _vp, _vp]),
    "tsdf_volume_cast_rays_device": (_i, [_vp, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tsdf_volume_cast_rays": (_i, [_vp, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tsdf_volume_cast_rays_colour_device": (_i, [_vp, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tsdf_volume_cast_rays_colour": (_i, [_vp, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tsdf_volume_fuse": (_i, [_vp, _vp, _fp, C.POINTER(C.c_uint64)]),
    "tsdf_volume_last_fuse_bricks": (_i, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "tsdf_integrate_rays_device": (_i, [_vp, C.c_uint64, _vp, C.c_uint64, _vp, _f, _f, _i, C.POINTER(C.c_uint64)]),
    "tsdf_integrate_rays": (_i, [_vp, C.c_uint64, _vp, C.c_uint64, _vp, _f, _f, _i, C.POINTER(C.c_uint64)]),
    "tsdf_volume_release_ray_scratch": (_i, [_vp]),
    "tsdf_integrate_rays_colour_device": (_i, [_vp, C.c_uint64, _vp, C.c_uint64, _vp, _vp, _f, _f, _i, C.POINTER(C.c_uint64)]),
    "tsdf_integrate_rays_colour": (_i, [_vp, C.c_uint64, _vp, C.c_uint64, _vp, _vp, _f, _f, _i, C.POINTER(C.c_uint64)]),
    "tsdf_volume_ray_scratch_bytes": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_aligner_create": (_i, [C.POINTER(_vp)]),
    "tsdf_aligner_destroy": (None, [_vp]),
    "tsdf_aligner_set_stream": (_i, [_vp, _vp]),
    "tsdf_aligner_stream": (_i, [_vp, C.POINTER(_vp)]),
    "tsdf_aligner_step": (_i, [_vp, _vp, _u32, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    "tsdf_aligner_run": (_i, [_vp, _vp, _u32, _vp, _f, _vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "tsdf_depth_to_points_device": (_i, [_u32, _u32, _vp, _vp, _u32, _f, _vp, _vp]),
    "tsdf_volume_sample_intensity_device": (_i, [_vp, C.c_uint64, _vp, _vp, _vp, _vp]),
    "tsdf_volume_sample_intensity": (_i, [_vp, C.c_uint64, _vp, _vp, _vp]),
    "tsdf_rgb_to_intensity_device": (_i, [_u32, _u32, _vp, _u32, _vp, _vp]),
    "tsdf_aligner_step_colour": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp]),
    "tsdf_aligner_run_colour": (_i, [_vp, _vp, _u32, _vp, _f, _f, _f, _vp, _vp, _vp]),
    "tsdf_raycast": (_i, [_vp, _u32, _u32, _fp, _fp, _vp, _vp]),
    "tsdf_raycast_device": (_i, [_vp, _u32, _u32, _fp, _fp, _vp, _vp]),
    "tsdf_normals_device": (_i, [_u32, _u32, _vp, _vp, _vp]),
    "tsdf_raycast_stats": (_i, [_vp, _u32, _u32, _fp, _fp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                C.POINTER(C.c_uint64)]),
    "tsdf_raycast_evaluated_samples": (_i, [_vp, _u32, _u32, _fp, _fp, C.POINTER(C.c_uint64), _vp]),
    "tsdf_volume_deform_points": (_i, [_vp, _i, _vp]),
    "tsdf_volume_deform_points_device": (_i, [_vp, _i, _vp]),
    "tsdf_volume_occupancy": (_i, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "tsdf_volume_get_occupancy_data": (_i, [_vp, C.c_int, _vp, _vp, _vp]),
    "tsdf_raycast_slab_device": (_i, [_vp, _u32, _u32, _fp, _fp, _vp]),
    "tsdf_vertices_to_depth_device": (_i, [_u32, _u32, _vp, _vp, _vp, _vp]),
    "tsdf_raycast_depth_device": (_i, [_vp, _u32, _u32, _fp, _fp, _fp, _vp, _vp]),
    "tsdf_volume_marching_cubes": (_i, [_vp, _vp, _vp, _vp, C.c_uint64]),
    "tsdf_mesh_create": (_i, [C.POINTER(_vp)]),
    "tsdf_mesh_destroy": (None, [_vp]),
    "tsdf_volume_extract_mesh": (_i, [_vp, _vp, C.POINTER(_u32), _u32, _vp]),
    "tsdf_mesh_get_info": (_i, [_vp, C.POINTER(MeshInfo)]),
    "tsdf_mesh_buffers": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "tsdf_mesh_download": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "tsdf_mesh_scratch_bytes": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_label_components_device": (_i, [C.c_uint64, C.c_uint64, _vp, _vp, _vp, C.POINTER(ComponentsInfo), _vp]),
    "tsdf_mesh_label_components": (_i, [_vp, C.POINTER(ComponentsInfo), _vp]),
    "tsdf_mesh_component_buffers": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "tsdf_mesh_component_download": (_i, [_vp, _vp, _vp]),
    "tsdf_mesh_filter_components": (_i, [_vp, C.c_uint64, _u32, _vp, _vp]),
    "tsdf_simplify_mesh_device": (_i, [C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp, C.c_float, _u32, _vp, _vp]),
    "tsdf_mesh_simplify": (_i, [_vp, C.c_float, _u32, _vp, _vp]),
    "tsdf_smooth_mesh_device": (_i, [C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp, _u32, C.c_float, C.c_float, _u32, _vp, _vp]),
    "tsdf_mesh_smooth": (_i, [_vp, _u32, C.c_float, C.c_float, _u32, _vp, _vp]),
    "tsdf_vertex_normals_device": (_i, [C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp]),
    "tsdf_mesh_compute_normals": (_i, [_vp, _vp]),
    "tsdf_render_create": (_i, [C.POINTER(_vp)]),
    "tsdf_render_destroy": (None, [_vp]),
    "tsdf_render_scratch_bytes": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_render_get_info": (_i, [_vp, C.POINTER(RenderInfo)]),
    "tsdf_render_set_large_box": (_i, [_vp, _u32]),
    "tsdf_render_mesh_device": (_i, [_vp, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp, _u32, _u32, _fp, _fp, _f, _f, _u32, C.POINTER(RenderTargets),
                                     C.POINTER(RenderInfo), _vp]),
    "tsdf_mesh_render_device": (_i, [_vp, _vp, _u32, _u32, _fp, _fp, _f, _f, _u32, C.POINTER(RenderTargets), C.POINTER(RenderInfo), _vp]),
    "tsdf_mesh_render": (_i, [_vp, _vp, _u32, _u32, _fp, _fp, _f, _f, _u32, C.POINTER(RenderTargets), C.POINTER(RenderInfo)]),
    "tsdf_volume_apply_scene_flow": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp, _f, _u32, C.POINTER(SceneFlowInfo)]),
    "tsdf_volume_apply_scene_flow_device": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _fp, _fp, _fp, _fp, _f, _u32, C.POINTER(SceneFlowInfo), _vp]),
    "tsdf_esdf_create": (_i, [C.POINTER(_vp)]),
    "tsdf_esdf_destroy": (None, [_vp]),
    "tsdf_volume_compute_esdf": (_i, [_vp, _f, _u32, _vp]),
    "tsdf_esdf_get_info": (_i, [_vp, C.POINTER(EsdfInfo)]),
    "tsdf_esdf_buffer": (_i, [_vp, C.POINTER(_vp)]),
    "tsdf_esdf_download": (_i, [_vp, _vp]),
    "tsdf_esdf_sample_device": (_i, [_vp, C.c_uint64, _vp, _vp, _vp, _i, _vp]),
    "tsdf_esdf_sample": (_i, [_vp, C.c_uint64, _vp, _vp, _vp, _i]),
    "tsdf_esdf_scratch_bytes": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_explorer_create": (_i, [C.POINTER(_vp)]),
    "tsdf_explorer_destroy": (None, [_vp]),
    "tsdf_volume_find_frontiers": (_i, [_vp, _u32, _vp]),
    "tsdf_explorer_get_info": (_i, [_vp, C.POINTER(ExplorerInfo)]),
    "tsdf_explorer_frontier_buffers": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "tsdf_explorer_frontier_download": (_i, [_vp, _vp]),
    "tsdf_explorer_scratch_bytes": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_explorer_cluster_frontiers": (_i, [_vp, _u32, _u32, _vp]),
    "tsdf_explorer_cluster_buffers": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "tsdf_explorer_cluster_download": (_i, [_vp, _vp, _vp]),
    "tsdf_volume_view_gain_device": (_i, [_vp, _vp, C.c_uint64, _vp, _vp, _vp, _u32, _vp, _vp, _vp, C.POINTER(C.c_uint64)]),
    "tsdf_volume_view_gain": (_i, [_vp, _vp, C.c_uint64, _vp, _vp, _vp, _u32, _vp, _vp, _vp, C.POINTER(C.c_uint64)]),
    "tsdf_reach_create": (_i, [C.POINTER(_vp)]),
    "tsdf_reach_destroy": (None, [_vp]),
    "tsdf_volume_compute_reach": (_i, [_vp, C.c_uint64, _vp, _u32, _vp, _f, _u32, _u32, _vp]),
    "tsdf_volume_compute_reach_device": (_i, [_vp, C.c_uint64, _vp, _u32, _vp, _f, _u32, _u32, _vp]),
    "tsdf_reach_get_info": (_i, [_vp, C.POINTER(ReachInfo)]),
    "tsdf_reach_buffer": (_i, [_vp, C.POINTER(_vp)]),
    "tsdf_reach_download": (_i, [_vp, _vp]),
    "tsdf_reach_scratch_bytes": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_reach_lookup_device": (_i, [_vp, C.c_uint64, _vp, _vp, _vp]),
    "tsdf_reach_lookup": (_i, [_vp, C.c_uint64, _vp, _vp]),
    "tsdf_reach_paths_device": (_i, [_vp, C.c_uint64, _vp, _u32, _vp, _vp, _vp]),
    "tsdf_reach_paths": (_i, [_vp, C.c_uint64, _vp, _u32, _vp, _vp]),
    "tsdf_reach_rank_frontiers_device": (_i, [_vp, _vp, _vp, _vp]),
    "tsdf_reach_rank_frontiers": (_i, [_vp, _vp, _vp]),
    "tsdf_objects_create": (_i, [C.POINTER(_vp)]),
    "tsdf_objects_destroy": (None, [_vp]),
    "tsdf_volume_find_objects": (_i, [_vp, _u32, _vp, _u32, _u32, _u32, _u32, _vp]),
    "tsdf_objects_get_info": (_i, [_vp, C.POINTER(ObjectsInfo)]),
    "tsdf_objects_buffers": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "tsdf_objects_download": (_i, [_vp, _vp, _vp, _vp]),
    "tsdf_objects_lookup_device": (_i, [_vp, C.c_uint64, _vp, _vp, _vp]),
    "tsdf_objects_lookup": (_i, [_vp, C.c_uint64, _vp, _vp]),
    "tsdf_objects_scratch_bytes": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_snapshot_create": (_i, [C.POINTER(_vp)]),
    "tsdf_snapshot_destroy": (None, [_vp]),
    "tsdf_volume_snapshot": (_i, [_vp, _u32, _vp]),
    "tsdf_volume_restore": (_i, [_vp, _vp]),
    "tsdf_snapshot_get_info": (_i, [_vp, C.POINTER(SnapshotInfo)]),
    "tsdf_snapshot_buffers": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "tsdf_snapshot_download": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "tsdf_snapshot_upload": (_i, [_vp, C.POINTER(SnapshotInfo), _vp, _vp, _vp, _vp]),
    "tsdf_snapshot_scratch_bytes": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_volume_restore_shifted": (_i, [_vp, _vp, C.POINTER(C.c_int32), _u32]),
    "tsdf_snapshot_select": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _u32, _vp]),
    "tsdf_volume_shift": (_i, [_vp, C.POINTER(C.c_int32), _vp, _vp]),
    "tsdf_columns_create": (_i, [C.POINTER(_vp)]),
    "tsdf_columns_destroy": (None, [_vp]),
    "tsdf_volume_project_columns": (_i, [_vp, _u32, _u32, _u32, _vp, _u32, _vp]),
    "tsdf_columns_get_info": (_i, [_vp, C.POINTER(ColumnsInfo)]),
    "tsdf_columns_buffer": (_i, [_vp, C.POINTER(_vp)]),
    "tsdf_columns_download": (_i, [_vp, _vp]),
    "tsdf_columns_scratch_bytes": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_columns_classify_device": (_i, [_vp, _u32, _u32, _u32, _vp, _vp]),
    "tsdf_columns_classify": (_i, [_vp, _u32, _u32, _u32, _vp]),
    "tsdf_merge_hits_device": (_i, [_vp, _vp, _u32, _u32, _u32, _fp, _fp, _vp, _vp]),
    "tsdf_merge_hits_normals_device": (_i, [_vp, _vp, _u32, _u32, _u32, _fp, _fp, _vp, _vp, _vp]),
    "tsdf_slab_exchange_unique_id": (_i, [_vp, C.c_char_p]),
    "tsdf_slab_exchange_create": (_i, [_i, _i, _vp, C.c_char_p, C.POINTER(_vp)]),
    "tsdf_slab_exchange_create_callback": (_i, [_i, _i, EXCHANGE_FN, _vp, C.POINTER(_vp)]),
    "tsdf_slab_exchange_create_loopback": (_i, [_i, _i, C.POINTER(_vp)]),
    "tsdf_slab_exchange_world": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "tsdf_slab_exchange_ranks_seen": (_i, [_vp, C.POINTER(_i)]),
    "tsdf_slab_validate_merge": (_i, [_vp, _vp, _u32, _u32, _fp, _fp, _vp, _vp, C.POINTER(C.c_uint64)]),
    "tsdf_slab_exchange_all_gather": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "tsdf_slab_exchange_destroy": (_i, [_vp]),
    "tsdf_pipeline_create": (_i, [_vp, _vp, _u32, _u32, _i, _vp, C.POINTER(_vp)]),
    "tsdf_pipeline_step": (_i, [_vp, _vp, C.POINTER(CameraMatrices), _vp, _vp, _vp, C.POINTER(CameraMatrices)]),
    "tsdf_pipeline_step_colour": (_i, [_vp, _vp, _vp, C.POINTER(CameraMatrices), _vp, _vp, _vp, _vp, C.POINTER(CameraMatrices)]),
    "tsdf_pipeline_synchronize": (_i, [_vp]),
    "tsdf_pipeline_streams": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "tsdf_pipeline_hit_buffers": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "tsdf_pipeline_destroy": (_i, [_vp]),
    "tsdf_tracker_create": (_i, [_vp, _vp, _vp, _u32, _u32, _f, _i, C.POINTER(_vp)]),
    "tsdf_tracker_filter": (_i, [_vp, _vp]),
    "tsdf_tracker_align": (_i, [_vp, C.POINTER(CameraMatrices), _vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "tsdf_tracker_align_field": (_i, [_vp, _vp, _vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "tsdf_tracker_align_field_colour": (_i, [_vp, _vp, _vp, _f, _f, _vp, _vp, _vp]),
    "tsdf_tracker_integrate": (_i, [_vp, C.POINTER(CameraMatrices)]),
    "tsdf_tracker_integrate_colour": (_i, [_vp, C.POINTER(CameraMatrices), _vp]),
    "tsdf_tracker_set_window": (_i, [_vp, _u32]),
    "tsdf_tracker_window": (_i, [_vp, C.POINTER(C.c_uint32)]),
    "tsdf_tracker_set_weighting": (_i, [_vp, _u32, _f]),
    "tsdf_tracker_weighting": (_i, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "tsdf_tracker_set_dynamic_rejection": (_i, [_vp, C.POINTER(DiffRejection)]),
    "tsdf_tracker_dynamic_rejection": (_i, [_vp, C.POINTER(_i), C.POINTER(DiffRejection)]),
    "tsdf_tracker_last_rejection": (_i, [_vp, C.POINTER(C.c_uint64 * 5), C.POINTER(C.c_uint64), C.POINTER(_vp)]),
    "tsdf_frame_diff_create": (_i, [C.POINTER(_vp)]),
    "tsdf_frame_diff_destroy": (None, [_vp]),
    "tsdf_frame_diff_get_info": (_i, [_vp, C.POINTER(FrameDiffInfo)]),
    "tsdf_frame_diff_scratch_bytes": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "tsdf_frame_diff_compare_device": (_i, [_vp, _vp, _vp, _u32, _u32, C.POINTER(DiffParams), _vp, _vp]),
    "tsdf_frame_diff_cluster": (_i, [_vp, _u32, _u32, _u32, _vp]),
    "tsdf_frame_diff_buffers": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "tsdf_frame_diff_download": (_i, [_vp, _vp, _vp, _vp]),
    "tsdf_frame_diff_mask_device": (_i, [_vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "tsdf_tracker_synchronize": (_i, [_vp]),
    "tsdf_tracker_streams": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "tsdf_tracker_buffers": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "tsdf_tracker_destroy": (_i, [_vp]),
    "tsdf_icp_create": (_i, [_i, _i, _f, _f, _f, _f, _f, _f, C.POINTER(_vp)]),
    "tsdf_icp_destroy": (None, [_vp]),
    "tsdf_icp_set_stream": (_i, [_vp, _vp]),
    "tsdf_icp_stream": (_i, [_vp, C.POINTER(_vp)]),
    "tsdf_icp_init": (_i, [_vp, _i, _vp, _f]),
    "tsdf_icp_init_device": (_i, [_vp, _i, _vp, _f]),
    "tsdf_icp_estimate_step": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "tsdf_icp_get_incremental_transformation": (_i, [_vp, _vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "tsdf_icp_get_map": (_i, [_vp, _i, _i, _vp]),
    "tsdf_icp_get_depth_level": (_i, [_vp, _i, _vp]),
    "tsdf_bilateral_create": (_i, [_f, _f, C.POINTER(_vp)]),
    "tsdf_bilateral_destroy": (_i, [_vp]),
    "tsdf_bilateral_filter_u8": (_i, [_vp, _vp, _i, _i]),
    "tsdf_bilateral_filter_u16": (_i, [_vp, _vp, _i, _i]),
    "tsdf_bilateral_filter_u8_device": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "tsdf_bilateral_filter_u16_device": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "tsdf_bilateral_filter_u16_device_tiles": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
}
#: every symbol include/tsdf_amd.h declares
EXPORTS = tuple(_SIGS)
for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(lib, _name)   # AttributeError here = the library does not export a declared symbol
    _fn.restype = _res
    _fn.argtypes = _args


def last_error():
    return lib.tsdf_last_error().decode("utf-8", "replace")


def check(rc):
    """Map a C-ABI status to the reference's error behaviour: invalid argument -> ValueError
    (std::invalid_argument in the C++ surface), anything else -> TsdfError."""
    if rc == TSDF_OK:
        return
    msg = last_error()
    if rc == TSDF_ERR_INVALID:
        raise ValueError(msg)
    if rc == TSDF_ERR_NOMEM:
        raise MemoryError(msg)
    raise TsdfError(msg)

# ---- host library (C++ class surface; Camera is exposed to Python through it) ------------------
HOST_LIB_PATH = os.path.join(_HERE, "lib", "libtsdf_host.so")
if not os.path.exists(HOST_LIB_PATH):
    raise ImportError("tsdf_amd: %s is missing -- build it with `make host`." % HOST_LIB_PATH)
# RTLD_LOCAL: this library defines the reference's class names (BilateralFilter, Camera, ...); they must not
# interpose the same names inside other shared objects (e.g. the reference build the tests compare against).
host = C.CDLL(HOST_LIB_PATH)
_ip = C.POINTER(C.c_int)
_HOST_SIGS = {
    "tsdf_camera_create": (_vp, [_f, _f, _f, _f]),
    "tsdf_camera_destroy": (None, [_vp]),
    "tsdf_camera_get": (None, [_vp, _fp, _fp, _fp, _fp]),
    "tsdf_camera_set_pose": (None, [_vp, _fp]),
    "tsdf_camera_set_pose_tum": (None, [_vp, _fp]),
    "tsdf_camera_move_to": (None, [_vp, _f, _f, _f]),
    "tsdf_camera_look_at": (None, [_vp, _f, _f, _f]),
    "tsdf_camera_world_to_camera": (None, [_vp, _fp, _fp]),
    "tsdf_camera_camera_to_world": (None, [_vp, _fp, _fp]),
    "tsdf_camera_world_to_pixel": (None, [_vp, _fp, _ip]),
    "tsdf_camera_pixel_to_image_plane": (None, [_vp, C.c_uint16, C.c_uint16, _fp]),
    "tsdf_camera_image_plane_to_pixel": (None, [_vp, _fp, _ip]),
    "tsdf_host_marching_cubes_c": (C.c_size_t, [_vp, C.c_uint, C.c_uint, C.c_uint, _vp, _vp, _vp, C.c_size_t]),
    "tsdf_host_mc_table": (None, [_vp]),
    "tsdf_host_tum_open": (_vp, [C.c_char_p]),
    "tsdf_host_tum_next": (_i, [_vp, _vp, C.c_size_t, C.POINTER(C.c_uint), _fp]),
    "tsdf_host_tum_close": (None, [_vp]),
    "tsdf_host_tum_next_rgb": (_i, [_vp, _vp, C.c_size_t, C.POINTER(C.c_uint), _fp, _vp, C.c_size_t]),
    "tsdf_host_block_loader_parse": (_i, [C.c_char_p, _vp, _vp, _vp, _vp, C.c_size_t]),
    "tsdf_host_write_ply": (None, [C.c_char_p, _vp, C.c_size_t, _vp, C.c_size_t]),
    "tsdf_host_write_ply_coloured": (_i, [C.c_char_p, _vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    "tsdf_host_write_ply_normals": (_i, [C.c_char_p, _vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    "tsdf_host_write_ply_normals_coloured": (_i, [C.c_char_p, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp]),
    "tsdf_host_read_nyu_depth_map": (C.c_size_t, [C.c_char_p, C.POINTER(C.c_uint), _vp, C.c_size_t]),
    "tsdf_host_match_file_name": (_i, [C.c_char_p, _i, C.c_char_p, C.c_char_p, C.c_char_p]),
    "tsdf_host_process_file_by_lines": (C.c_size_t, [C.c_char_p, C.POINTER(_i), C.c_char_p, C.c_size_t]),
    "tsdf_host_read_last_line": (C.c_size_t, [C.c_char_p, C.c_char_p, C.POINTER(_i), C.c_char_p, C.c_size_t]),
    "tsdf_host_files_in_directory": (C.c_size_t, [C.c_char_p, C.c_char_p, _i, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "tsdf_host_file_exists": (_i, [C.c_char_p, C.POINTER(_i)]),
    "tsdf_host_read_sparse_info": (_i, [C.c_char_p, C.POINTER(HostSparseInfo), C.c_char_p, C.c_size_t]),
}
for _name, (_res, _args) in _HOST_SIGS.items():
    _fn = getattr(host, _name)
    _fn.restype = _res
    _fn.argtypes = _args
