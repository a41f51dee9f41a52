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
#endif
