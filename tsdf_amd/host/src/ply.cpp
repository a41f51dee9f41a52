// reference: src/Utilities/ply.cpp:6-30 (same header lines and record layout)
#include "ply.hpp"

#include <fstream>
#include <iostream>

void write_to_ply(const std::string &file_name, const std::vector<float3> &vertices, const std::vector<int3> &triangles) {
    std::ofstream f{file_name};
    if (!f.is_open()) {
        std::cout << "Problem opening file for write " << file_name << std::endl;
        return;
    }
    f << "ply\nformat ascii 1.0\n";
    f << "element vertex " << vertices.size() << "\n";
    f << "property float x\nproperty float y\nproperty float z\n";
    f << "element face " << triangles.size() << "\n";
    f << "property list uchar int vertex_indices\nend_header\n";
    for (size_t v = 0; v < vertices.size(); v++) f << vertices[v].x << " " << vertices[v].y << " " << vertices[v].z << "\n";
    for (size_t t = 0; t < triangles.size(); t++) f << "3 " << triangles[t].x << " " << triangles[t].y << " " << triangles[t].z << "\n";
}

// not in the reference: the coloured mesh of extract_surface(volume, vertices, triangles, colours)
void write_to_ply(const std::string &file_name, const std::vector<float3> &vertices, const std::vector<int3> &triangles,
                  const std::vector<uchar3> &colours) {
    std::ofstream f{file_name};
    if (!f.is_open()) {
        std::cout << "Problem opening file for write " << file_name << std::endl;
        return;
    }
    f << "ply\nformat ascii 1.0\n";
    f << "element vertex " << vertices.size() << "\n";
    f << "property float x\nproperty float y\nproperty float z\n";
    f << "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    f << "element face " << triangles.size() << "\n";
    f << "property list uchar int vertex_indices\nend_header\n";
    for (size_t v = 0; v < vertices.size(); v++) {
        const uchar3 c = v < colours.size() ? colours[v] : uchar3{0, 0, 0};
        f << vertices[v].x << " " << vertices[v].y << " " << vertices[v].z << " " << (int)c.x << " " << (int)c.y << " " << (int)c.z << "\n";
    }
    for (size_t t = 0; t < triangles.size(); t++) f << "3 " << triangles[t].x << " " << triangles[t].y << " " << triangles[t].z << "\n";
}

// not in the reference: normals per vertex, with or without colours (`colours` null: none)
static void write_ply_with_normals(const std::string &file_name, const std::vector<float3> &vertices, const std::vector<int3> &triangles,
                                   const std::vector<float3> &normals, const std::vector<uchar3> *colours) {
    std::ofstream f{file_name};
    if (!f.is_open()) {
        std::cout << "Problem opening file for write " << file_name << std::endl;
        return;
    }
    f << "ply\nformat ascii 1.0\n";
    f << "element vertex " << vertices.size() << "\n";
    f << "property float x\nproperty float y\nproperty float z\n";
    f << "property float nx\nproperty float ny\nproperty float nz\n";
    if (colours) f << "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    f << "element face " << triangles.size() << "\n";
    f << "property list uchar int vertex_indices\nend_header\n";
    for (size_t v = 0; v < vertices.size(); v++) {
        const float3 n = v < normals.size() ? normals[v] : float3{0.0f, 0.0f, 0.0f};
        f << vertices[v].x << " " << vertices[v].y << " " << vertices[v].z << " " << n.x << " " << n.y << " " << n.z;
        if (colours) {
            const uchar3 c = v < colours->size() ? (*colours)[v] : uchar3{0, 0, 0};
            f << " " << (int)c.x << " " << (int)c.y << " " << (int)c.z;
        }
        f << "\n";
    }
    for (size_t t = 0; t < triangles.size(); t++) f << "3 " << triangles[t].x << " " << triangles[t].y << " " << triangles[t].z << "\n";
}

void write_to_ply(const std::string &file_name, const std::vector<float3> &vertices, const std::vector<int3> &triangles,
                  const std::vector<float3> &normals) {
    write_ply_with_normals(file_name, vertices, triangles, normals, nullptr);
}

void write_to_ply(const std::string &file_name, const std::vector<float3> &vertices, const std::vector<int3> &triangles,
                  const std::vector<float3> &normals, const std::vector<uchar3> &colours) {
    write_ply_with_normals(file_name, vertices, triangles, normals, &colours);
}
