// Iso-surface extraction from a TSDFVolume (zero level set of the distance field), on the HOST.
// Same entry point as the reference's extract_surface (src/include/MarkAndSweepMC.hpp:8).  The reference runs
// marching cubes on the GPU; here the distance array is copied to the host and triangulated there, cube by cube in the
// reference's order (BASELINE north_star: "src/MarchingCubes stays host-side").
#ifndef TSDF_AMD_HOST_MARK_AND_SWEEPMC_INCLUDED
#define TSDF_AMD_HOST_MARK_AND_SWEEPMC_INCLUDED

#include <vector>

#include "TSDFVolume.hpp"

void extract_surface(const TSDFVolume *volume, std::vector<float3> &vertices, std::vector<int3> &triangles);
// the same with the colour of the voxel each vertex lies in (tsdf_volume_sample_colours_device); the volume must have colour
// enabled (not in the reference)
void extract_surface(const TSDFVolume *volume, std::vector<float3> &vertices, std::vector<int3> &triangles,
                     std::vector<uchar3> &colours);
// with a normal per vertex: the unit gradient of the fused field there (tsdf_volume_sample_field, TSDF_FIELD_UNIT_GRADIENT), which
// points out of the surface; the NaN triple within one voxel of the grid's faces and where the gradient vanishes.  Alone, or with
// the colours as above (not in the reference)
void extract_surface(const TSDFVolume *volume, std::vector<float3> &vertices, std::vector<int3> &triangles,
                     std::vector<float3> &normals);
void extract_surface(const TSDFVolume *volume, std::vector<float3> &vertices, std::vector<int3> &triangles,
                     std::vector<float3> &normals, std::vector<uchar3> &colours);

// The surface as an INDEXED mesh (tsdf_volume_extract_mesh, include/tsdf_amd.h "indexed mesh"; not in the reference): one vertex per
// lattice edge the surface crosses, shared by the triangles round it, sorted by ((z * Y + y) * X + x) * 3 + axis of the edge's lower
// voxel; triangles wired (I[3t], I[3t+2], I[3t+1]) like extract_surface's, so that vertices[triangle corner] are extract_surface's
// vertices bit for bit.  Welding is by lattice edge, not by position: where a voxel is exactly 0 several vertices coincide and stay
// distinct.  Normals (the unit gradient) and colours are sampled once per shared vertex, on the device.  The results go straight into
// the write_to_ply overloads.
void extract_surface_indexed(const TSDFVolume *volume, std::vector<float3> &vertices, std::vector<int3> &triangles);
void extract_surface_indexed(const TSDFVolume *volume, std::vector<float3> &vertices, std::vector<int3> &triangles,
                             std::vector<float3> &normals);
void extract_surface_indexed(const TSDFVolume *volume, std::vector<float3> &vertices, std::vector<int3> &triangles,
                             std::vector<uchar3> &colours);
void extract_surface_indexed(const TSDFVolume *volume, std::vector<float3> &vertices, std::vector<int3> &triangles,
                             std::vector<float3> &normals, std::vector<uchar3> &colours);
// ... of the cubes rooted at voxels in [box[0], box[3]) x [box[1], box[4]) x [box[2], box[5]) only (ends clipped to the grid; a begin
// that is not below its end throws std::invalid_argument); normals / colours may be null
void extract_surface_indexed(const TSDFVolume *volume, const unsigned box[6], std::vector<float3> &vertices,
                             std::vector<int3> &triangles, std::vector<float3> *normals = nullptr,
                             std::vector<uchar3> *colours = nullptr);

// The indexed mesh without its small connected pieces -- the floaters that sensor noise leaves in a fused scan (include/tsdf_amd.h
// "mesh components"; not in the reference): extracted, labelled and filtered on the device, downloaded once.  A piece is kept when
// it has at least min_triangles triangles and, with keep_largest, is the one with the most (ties: the one holding the smallest vertex
// index).  Kept vertices and triangles stay in extract_surface_indexed's order, triangles wired (i, i+2, i+1) as there; box, normals
// and colours may be null.  The results go straight into the write_to_ply overloads.
void extract_surface_components(const TSDFVolume *volume, const unsigned box[6], size_t min_triangles, bool keep_largest,
                                std::vector<float3> &vertices, std::vector<int3> &triangles, std::vector<float3> *normals = nullptr,
                                std::vector<uchar3> *colours = nullptr);

// A level of detail of the indexed mesh (include/tsdf_amd.h "mesh simplification"; not in the reference): extracted and clustered on the
// device, downloaded once.  The vertices of each cubic cell of side cell_size (mm) become one vertex -- the mean of their positions,
// normals and colours -- in the order of each cell's first vertex; triangles left with fewer than three corners are dropped, the rest
// stay in extract_surface_indexed's order, wired (i, i+2, i+1) as there.  Vertices that no triangle names any more stay in the
// arrays.  box, normals and colours may be null; a cell_size that is not a finite length above 0 throws std::invalid_argument.  The
// results go straight into the write_to_ply overloads.
void extract_surface_simplified(const TSDFVolume *volume, const unsigned box[6], float cell_size, std::vector<float3> &vertices,
                                std::vector<int3> &triangles, std::vector<float3> *normals = nullptr,
                                std::vector<uchar3> *colours = nullptr);

// The indexed mesh smoothed (include/tsdf_amd.h "mesh smoothing"; not in the reference): extracted and smoothed on the device, downloaded
// once.  `iterations` times a pass with factor lambda, then one with mu (Taubin: 0.5 and -0.53 smooth without shrinking; mu = 0 is the
// plain Laplacian); vertices, triangles and colours stay in extract_surface_indexed's order, only the positions move.  pin_boundary
// keeps the bytes of the open border, so meshes of neighbouring boxes still fit.  Normals, when asked for, are the area-weighted normals
// of the smoothed faces.  box, normals and colours may be null; factors that are not finite and more than 1024 iterations throw
// std::invalid_argument.  The results go straight into the write_to_ply overloads.
void extract_surface_smoothed(const TSDFVolume *volume, const unsigned box[6], unsigned iterations, float lambda, float mu, bool pin_boundary,
                              std::vector<float3> &vertices, std::vector<int3> &triangles, std::vector<float3> *normals = nullptr,
                              std::vector<uchar3> *colours = nullptr);

// The same marching cubes over a host distance array (x fastest, voxel centres at (i + 0.5) * voxel_size + offset):
// appends three vertices per triangle.  extract_surface is this on the volume's distances.
void tsdf_host_marching_cubes(const float *dist, unsigned X, unsigned Y, unsigned Z, const float voxel_size[3],
                              const float offset[3], std::vector<float3> &vertices);

#endif
