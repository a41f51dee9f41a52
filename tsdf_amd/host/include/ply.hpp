// ASCII PLY mesh writer.  Same function as the reference's src/include/ply.hpp.
#ifndef TSDF_AMD_HOST_PLY_INCLUDED
#define TSDF_AMD_HOST_PLY_INCLUDED
#include <string>
#include <vector>
#include "vector_types.h"

// one "x y z" line per vertex, one "3 a b c" line per triangle
void write_to_ply(const std::string &file_name,
                  const std::vector<float3> &vertices,
                  const std::vector<int3> &triangles);

// the same with a colour per vertex: "property uchar red / green / blue" after "property float z", and " r g b" ending each
// vertex line (colours.size() == vertices.size())
void write_to_ply(const std::string &file_name,
                  const std::vector<float3> &vertices,
                  const std::vector<int3> &triangles,
                  const std::vector<uchar3> &colours);

// with a normal per vertex (extract_surface(volume, vertices, triangles, normals)): "property float nx / ny / nz" after
// "property float z" and before the colour properties, " nx ny nz" after the coordinates of each vertex line, printed like them
// (normals.size() == vertices.size(); a missing normal is written as 0 0 0)
void write_to_ply(const std::string &file_name,
                  const std::vector<float3> &vertices,
                  const std::vector<int3> &triangles,
                  const std::vector<float3> &normals);
void write_to_ply(const std::string &file_name,
                  const std::vector<float3> &vertices,
                  const std::vector<int3> &triangles,
                  const std::vector<float3> &normals,
                  const std::vector<uchar3> &colours);
#endif
