// Ray queries through the C++ class surface: F frames of integrate() on a grid^3 volume, TSDFVolume::cast_rays on the rays given
// (points alone; points, t and normals; the same with a range limit per ray), and the pixel rays of the last frame's camera against
// GPURaycaster::raycast.  Dumps the arrays for tests/test_cpp_rays.py.
//
//   test_rays <frames.u16 (F x 640 x 480)> <poses.f32 (F x 16, column-major)> <F> <grid> <origins.f32 (N x 3)> <directions.f32 (N x 3)>
//             <t_max.f32 (N)> <N> <out_dir>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "GPURaycaster.hpp"
#include "TSDFVolume.hpp"
#include "tsdf_amd.h"

static void dump(const std::string &path, const void *p, size_t bytes) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char *)p, (std::streamsize)bytes);
}

template <typename T>
static bool load(const char *path, std::vector<T> &v) {
    std::ifstream f(path, std::ios::binary);
    f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(T)));
    return (bool)f;
}

int main(int argc, char **argv) {
    if (argc < 10) {
        std::cerr << "usage: test_rays frames.u16 poses.f32 F grid origins.f32 directions.f32 t_max.f32 N out_dir" << std::endl;
        return 2;
    }
    const int W = 640, H = 480;
    const size_t F = (size_t)atoi(argv[3]);
    const unsigned n = (unsigned)atoi(argv[4]);
    const size_t N = (size_t)atoi(argv[8]);
    const std::string out = argv[9];
    std::vector<uint16_t> depth(F * W * H);
    std::vector<float> poses(F * 16), t_max(N);
    std::vector<float3> origins(N), directions(N);
    if (!load(argv[1], depth) || !load(argv[2], poses) || !load(argv[5], origins) || !load(argv[6], directions) || !load(argv[7], t_max)) return 3;

    TSDFVolume volume(TSDFVolume::UInt3{n, n, n}, TSDFVolume::Float3{3000.0f, 3000.0f, 3000.0f});
    Camera *camera = Camera::default_depth_camera();
    for (size_t f = 0; f < F; f++) {
        Eigen::Matrix4f pose;
        for (int i = 0; i < 16; i++) pose.data()[i] = poses[f * 16 + i];
        camera->set_pose(pose);
        volume.integrate(depth.data() + f * W * H, W, H, *camera);
    }

    // the points alone; everything; everything under a range limit
    std::vector<float3> points_only, points, normals, points_lim, normals_lim;
    std::vector<float> t, t_lim;
    volume.cast_rays(origins, directions, points_only);
    volume.cast_rays(origins, directions, points, &t, &normals);
    volume.cast_rays(origins, directions, points_lim, &t_lim, &normals_lim, &t_max);
    if (points_only.size() != N || points.size() != N || t.size() != N || normals.size() != N || points_lim.size() != N ||
        t_lim.size() != N || normals_lim.size() != N)
        return 4;
    if (N && memcmp(points_only.data(), points.data(), N * sizeof(float3)) != 0) return 5;
    bool threw = false;
    try {
        std::vector<float3> short_directions(directions.begin(), directions.begin() + (N ? N - 1 : 0));
        if (N) volume.cast_rays(origins, short_directions, points_only); else threw = true;
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    if (!threw) return 6;
    std::vector<float3> none, untouched(3, float3{7.0f, 7.0f, 7.0f});
    volume.cast_rays(none, none, untouched);   // no rays: an empty result
    if (!untouched.empty()) return 7;

    // the pixel rays of the camera, cast as rays of their own: GPURaycaster's vertex map bit for bit
    GPURaycaster caster(W, H);
    Eigen::Matrix<float, 3, Eigen::Dynamic> cast_v, cast_n;
    caster.raycast(volume, *camera, cast_v, cast_n);
    const size_t pixels = (size_t)W * H;
    if ((size_t)cast_v.cols() != pixels) return 8;
    const Eigen::Matrix4f pose = camera->pose();
    const Eigen::Matrix3f kinv = camera->kinv();
    const float *P = pose.data(), *K = kinv.data();   // column-major: P[4 c + r], K[3 c + r]
    std::vector<float3> pixel_origins(pixels), pixel_directions(pixels), pixel_points;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            // compute_ray_direction_at_pixel (src/RayCaster/GPURaycaster.cu:24-44) in the same fp32 order
            const float px = (float)(uint16_t)x, py = (float)(uint16_t)y;
            const float rcx = px * K[0] + py * K[3] + K[6];
            const float rcy = px * K[1] + py * K[4] + K[7];
            const float rcz = px * K[2] + py * K[5] + K[8];
            float3 d;
            d.x = P[0] * rcx + P[4] * rcy + P[8] * rcz;
            d.y = P[1] * rcx + P[5] * rcy + P[9] * rcz;
            d.z = P[2] * rcx + P[6] * rcy + P[10] * rcz;
            pixel_directions[(size_t)y * W + x] = d;
            pixel_origins[(size_t)y * W + x] = float3{P[12], P[13], P[14]};
        }
    volume.cast_rays(pixel_origins, pixel_directions, pixel_points);
    if (pixel_points.size() != pixels) return 9;
    size_t hits = 0;
    const float *A = reinterpret_cast<const float *>(pixel_points.data()), *B = cast_v.data();
    for (size_t i = 0; i < 3 * pixels; i++) {
        const bool nan_a = A[i] != A[i], nan_b = B[i] != B[i];
        if (nan_a != nan_b || (!nan_a && memcmp(A + i, B + i, sizeof(float)) != 0)) return 10;
        hits += (i % 3 == 0 && !nan_a) ? 1 : 0;
    }
    delete camera;

    dump(out + "/points.f32", points.data(), N * sizeof(float3));
    dump(out + "/t.f32", t.data(), N * sizeof(float));
    dump(out + "/normals.f32", normals.data(), N * sizeof(float3));
    dump(out + "/points_lim.f32", points_lim.data(), N * sizeof(float3));
    dump(out + "/t_lim.f32", t_lim.data(), N * sizeof(float));
    dump(out + "/normals_lim.f32", normals_lim.data(), N * sizeof(float3));
    std::printf("ray surface ok: %zu rays, %zu of %zu pixel rays hit\n", N, hits, pixels);
    return 0;
}
