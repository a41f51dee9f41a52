"""tsdf_amd -- MI355X (gfx950) implementation of the TSDF integrate / raycast / bilateral hot path
of Scoobadood/TSDF behind the reference's class surface.  See DESIGN.md and include/tsdf_amd.h."""
from ._capi import TsdfError, last_error, LIB_PATH  # noqa: F401  (import fails loudly without the HIP library)
from .api import (TSDFVolume, GPURaycaster, BilateralFilter, Camera, ICPOdometry, compute_normals_device,  # noqa: F401
                  merge_hits_device, merge_hits_normals_device, HIT_RECORD_BYTES, vertices_to_depth_device, marching_cubes, marching_cubes_table, load_block_tsdf, load_tum_directory,
                  FieldAligner, depth_to_points, depth_to_points_device, Mesh, ESDF, Explorer, pixel_rays, Snapshot, label_components, label_components_device, simplify_mesh,
                  simplify_mesh_device, smooth_mesh, smooth_mesh_device, vertex_normals, rgb_to_intensity, rgb_to_intensity_device,
                  depth_weights, depth_weights_device, WEIGHTS_INVERSE_SQUARE, WEIGHTS_COSINE, CLASS_VOID, Objects, OBJECT_DTYPE,
                  OBJECT_NONE, Reach, REACH_CLUSTER_DTYPE, REACH_UNREACHED, REACH_COST_FACE, REACH_COST_EDGE, REACH_COST_CORNER,
                  TSDF_REACH_THROUGH_UNKNOWN, ColumnMap, COLUMN_DTYPE, CELL_NO_GROUND, CELL_TRAVERSABLE, CELL_BLOCKED, Renderer, render_mesh,
                  render_mesh_device, RENDER_TARGETS, RENDER_CULL_BACK, RENDER_MISS, FrameDiff, DIFF_BLOB_DTYPE, DIFF_NO_FRAME, DIFF_NO_MODEL, DIFF_SAME,
                  DIFF_FARTHER, DIFF_NEARER, DIFF_NO_BLOB, DIFF_DEFAULTS)
from .rolling import BrickStore, RollingVolume  # noqa: F401
