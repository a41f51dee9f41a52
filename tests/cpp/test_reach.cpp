// The reachability group through the C++ class surface: TSDFVolume::reach() into a TSDFVolume::Reach on a 13 x 7 x 5 state field and a
// 24^3 serpentine that tests/test_cpp_reach.py writes, costs(), lookup(), paths(), rank(), info() against the C ABI, and the refusals as
// exceptions.  Dumps the arrays for the Python side to compare with the CPU reference.
//
//   test_reach <dir>     reads <dir>/{a,s}_dist.f32, {a,s}_weight.f32, {a,s}_seeds.f32 (3 floats a seed) and a_goals.f32
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "TSDFVolume.hpp"
#include "tsdf_amd.h"

static void dump(const std::string &path, const void *p, size_t bytes) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char *)p, (std::streamsize)bytes);
}

static std::vector<float> load(const std::string &path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) {
        std::cerr << "cannot read " << path << std::endl;
        exit(3);
    }
    std::vector<float> v((size_t)f.tellg() / sizeof(float));
    f.seekg(0);
    f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(float)));
    return v;
}

static std::vector<float3> points_of(const std::vector<float> &v) {
    std::vector<float3> p(v.size() / 3);
    for (size_t i = 0; i < p.size(); i++) p[i] = float3{v[3 * i], v[3 * i + 1], v[3 * i + 2]};
    return p;
}

// the volume of tests/test_reach.py::volume_of: 10 x 12.5 x 9 mm voxels and an offset
static void fill(TSDFVolume &volume, const std::string &dir, const char *name) {
    volume.offset(100.0f, -50.0f, 25.0f);
    const std::vector<float> d = load(dir + "/" + name + "_dist.f32"), w = load(dir + "/" + name + "_weight.f32");
    const TSDFVolume::UInt3 s = volume.size();
    if (d.size() != (size_t)s.x * s.y * s.z || w.size() != d.size()) exit(4);
    volume.set_distance_data(d.data());
    volume.set_weight_data(w.data());
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::cerr << "usage: test_reach dir" << std::endl;
        return 2;
    }
    const std::string dir = argv[1];
    TSDFVolume::Reach reach;

    // ---- the random field: connectivity 26, through unknown space, a cap of 400
    TSDFVolume a(TSDFVolume::UInt3{13, 7, 5}, TSDFVolume::Float3{130.0f, 87.5f, 45.0f});
    fill(a, dir, "a");
    const std::vector<float3> seeds = points_of(load(dir + "/a_seeds.f32")), goals = points_of(load(dir + "/a_goals.f32"));
    a.reach(seeds, 26, nullptr, 0.0f, 400, TSDF_REACH_THROUGH_UNKNOWN, reach);
    const std::vector<uint32_t> costs = reach.costs();
    const tsdf_reach_info info = reach.info();
    if (costs.size() != 13 * 7 * 5 || info.size[0] != 13 || info.connectivity != 26 || info.max_cost != 400 || info.flags != TSDF_REACH_THROUGH_UNKNOWN) return 5;
    // the class is the C ABI's computation: the same bytes through the handle
    std::vector<uint32_t> through_abi(costs.size());
    if (tsdf_reach_download(reach.handle(), through_abi.data()) != TSDF_OK || memcmp(through_abi.data(), costs.data(), costs.size() * 4) != 0) return 6;
    const std::vector<uint32_t> looked = reach.lookup(goals);
    std::vector<uint32_t> lengths, flat;
    const std::vector<std::vector<uint32_t>> whole = reach.paths(goals, 0, &lengths);
    if (looked.size() != goals.size() || whole.size() != goals.size() || lengths.size() != goals.size()) return 7;
    for (size_t i = 0; i < whole.size(); i++) {
        if (whole[i].size() != lengths[i]) return 8;
        flat.insert(flat.end(), whole[i].begin(), whole[i].end());
    }
    // rows of two: the lengths are the whole paths', the rows their first two voxels
    std::vector<uint32_t> lengths2;
    const std::vector<std::vector<uint32_t>> cut = reach.paths(goals, 2, &lengths2);
    if (lengths2 != lengths) return 9;
    for (size_t i = 0; i < cut.size(); i++)
        if (cut[i].size() != std::min<size_t>(lengths[i], 2) || (cut[i].size() && memcmp(cut[i].data(), whole[i].data(), cut[i].size() * 4) != 0)) return 10;
    // ranking the field's own frontier clusters
    TSDFVolume::Explorer explorer;
    a.find_frontiers(explorer);
    explorer.cluster(26, 1);
    const std::vector<tsdf_reach_cluster> ranked = reach.rank(explorer);
    if (ranked.size() != explorer.clusters().size()) return 11;

    // ---- the refusals arrive as std::invalid_argument
    int threw = 0;
    try {
        a.reach(seeds, 18, nullptr, 0.0f, 0, 0, reach);
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        a.reach(seeds, 26, nullptr, 10.0f, 0, 0, reach);   // a clearance without an ESDF
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        a.reach(seeds, 26, nullptr, 0.0f, 0, 2u, reach);   // unknown flags
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        TSDFVolume::Reach fresh;
        (void)fresh.lookup(goals);   // never computed
    } catch (const std::invalid_argument &) {
        threw++;
    }
    try {
        TSDFVolume::Explorer unclustered;
        a.find_frontiers(unclustered);
        (void)reach.rank(unclustered);
    } catch (const std::invalid_argument &) {
        threw++;
    }
    if (threw != 5) return 12;
    // (a refused computation leaves the handle as it was)
    if (reach.costs() != costs) return 13;

    // ---- the serpentine, into the same handle
    TSDFVolume s(TSDFVolume::UInt3{24, 24, 24}, TSDFVolume::Float3{240.0f, 300.0f, 216.0f});
    fill(s, dir, "s");
    s.reach(points_of(load(dir + "/s_seeds.f32")), 26, nullptr, 0.0f, 0, 0, reach);
    const std::vector<uint32_t> serpentine = reach.costs();
    const tsdf_reach_info si = reach.info();

    dump(dir + "/a_costs.u32", costs.data(), costs.size() * 4);
    dump(dir + "/a_lookup.u32", looked.data(), looked.size() * 4);
    dump(dir + "/a_lengths.u32", lengths.data(), lengths.size() * 4);
    dump(dir + "/a_paths.u32", flat.data(), flat.size() * 4);
    dump(dir + "/a_rank.bin", ranked.data(), ranked.size() * sizeof(tsdf_reach_cluster));
    dump(dir + "/s_costs.u32", serpentine.data(), serpentine.size() * 4);
    std::printf("reach ok: %llu traversable, %llu reached, %llu seed voxels, max %u; serpentine %llu traversable, %llu reached, max %u, rounds %llu\n",
                (unsigned long long)info.n_traversable, (unsigned long long)info.n_reached, (unsigned long long)info.n_seed_voxels,
                info.max_cost_reached, (unsigned long long)si.n_traversable, (unsigned long long)si.n_reached, si.max_cost_reached,
                (unsigned long long)si.rounds);
    return 0;
}
