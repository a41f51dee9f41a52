"""Time of the reachability group (include/tsdf_amd.h, "reachability") on bench.py's scene (640 x 480, seed 0x5EED0003), 25 frames fused
at 512^3.  Prints one JSON line and writes it to profiles/reach_bench.json.

Host wall-clock times of whole calls, each ending in a device synchronise, into warm handles, as the median (and range) of --reps
repetitions after --warmup, the variants alternating inside every repetition, every yardstick in the same run:

  reach26_ms / reach6_ms              compute_reach from the seed (see `seed` below) at connectivity 26 / 6
  reach26_from_camera_ms              compute_reach from the camera position itself, whatever it reaches (on the bench scene the camera
                                      stands outside the grid: the seed is ignored and the call is the flag, init and statistics kernels
                                      and one batch of rounds that find nothing to do)
  reach26_clear_ms / reach6_clear_ms  the same with a 150 mm clearance from an ESDF computed once before (cap 200 mm)
  rank_ms                             rank_frontiers_device over the scene's frontier clusters (connectivity 26, min_size 1)
  paths_ms                            paths_device to the best voxel of every cluster that was reached
  lookup_ms                           lookup_device of the vertices of a 640 x 480 ray cast
  esdf_ms                             yardstick: compute_esdf(100 mm) into a warm handle
  find_frontiers_ms                   yardstick: find_frontiers into a warm handle
  fill_ms                             yardstick: a plain fill of as many bytes as the cost array takes (4 bytes a voxel; torch fill_)

seed: the camera position of the last fused frame; where that lies off the grid or in a voxel that is not free, the first point along
the optical axis (steps of 50 mm) that lies in a free voxel, found by one computation capped at cost 1 and a lookup.  The output says
which.

    python tools/bench_reach.py [--size 512] [--frames 25] [--reps 10] [--warmup 2] [--once] [--only-compute]

--once: one call of each and nothing else (for a kernel trace).  --only-compute: the four compute_reach variants only (for the table
of batch sizes: builds of the library with -DTSDF_REACH_BATCH=N, chosen with TSDF_HIP_LIB).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=25, help="frames fused before the queries")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clearance", type=float, default=150.0)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--only-compute", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reach_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_reach needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    n = a.size
    vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    cam = None
    for i in range(a.frames):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        vol.integrate(d, W, H, cam)
    vol.synchronize()
    reach, esdf, clear_esdf, ex, ex_yardstick = tsdf_amd.Reach(), tsdf_amd.ESDF(), tsdf_amd.ESDF(), tsdf_amd.Explorer(), tsdf_amd.Explorer()
    vol.compute_esdf(200.0, into=clear_esdf)

    # the seed
    pose = np.asarray(cam.pose(), np.float64).reshape(4, 4).T       # (column-major 16 floats: camera -> world)
    position, axis = pose[:3, 3], pose[:3, 2]
    # (one computation capped at cost 1 with every candidate as a seed, then a lookup: a candidate in a free voxel reads 0)
    camera_point = position.astype(np.float32)[None, :]
    candidates = np.stack([position + 50.0 * step * axis for step in range(0, 121)]).astype(np.float32)
    free = np.flatnonzero(vol.reach(candidates, 26, max_cost=1, into=reach).lookup(candidates) == 0)
    assert len(free), "no free voxel along the optical axis"
    seed, along = candidates[free[0]][None, :], 50.0 * int(free[0])

    vol.find_frontiers(into=ex).cluster(26, 1)
    n_rows = int(ex.info.n_listed_clusters)
    rows = torch.zeros(4 * max(n_rows, 1), dtype=torch.int32, device="cuda")
    vertices, _ = vol.raycast(W, H, cam)
    points = torch.from_numpy(np.ascontiguousarray(vertices, np.float32).reshape(-1)).cuda()
    looked = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    fill_like = torch.zeros(n ** 3, dtype=torch.int32, device="cuda")
    kept = {}

    def compute(connectivity, clearance, point=None, key=None):
        def run():
            vol.reach(seed if point is None else point, connectivity, esdf=clear_esdf if clearance else None, clearance=clearance,
                      into=reach)   # (returns when final)
            kept[key or (connectivity, clearance)] = reach.info
        return run

    # the goals of the paths: the best voxel of every cluster the plain connectivity-26 field reaches
    compute(26, 0.0)()
    ranked = reach.rank(ex)
    best = ranked[ranked["cost"] != tsdf_amd.REACH_UNREACHED]
    goals = torch.from_numpy(reach.voxel_centres(best["voxel"]).reshape(-1)).cuda()
    n_goals = len(best)
    max_len = int(best["cost"].max()) // 10 + 1 if n_goals else 1
    max_len = max(1, min(max_len, 2 ** 27 // max(n_goals, 1)))      # (rows of at most 512 MiB in all; the lengths are the whole paths' anyway)
    path_rows = torch.zeros(max(n_goals, 1) * max_len, dtype=torch.int32, device="cuda")
    path_lengths = torch.zeros(max(n_goals, 1), dtype=torch.int32, device="cuda")

    def rank():
        reach.rank_device(ex, rows.data_ptr())
        torch.cuda.synchronize()

    def paths():
        from tsdf_amd import _capi
        _capi.check(_capi.lib.tsdf_reach_paths_device(reach._h, n_goals, goals.data_ptr() if n_goals else None, max_len, path_lengths.data_ptr(),
                                                      path_rows.data_ptr(), None))
        torch.cuda.synchronize()

    def lookup():
        reach.lookup_device(W * H, points.data_ptr(), looked.data_ptr())
        torch.cuda.synchronize()

    def fill():
        fill_like.fill_(-1)
        torch.cuda.synchronize()

    variants = {"reach26": compute(26, 0.0), "reach6": compute(6, 0.0), "reach26_clear": compute(26, a.clearance), "reach6_clear": compute(6, a.clearance)}
    if not a.only_compute:
        # (rank, paths and lookup read the field of the variant before them: reach26 comes back last in every repetition)
        variants.update({"reach26_from_camera": compute(26, 0.0, camera_point, "camera"), "esdf": lambda: esdf.device_buffer() if vol.compute_esdf(100.0, into=esdf) else None,
                         "find_frontiers": lambda: vol.find_frontiers(into=ex_yardstick), "fill": fill,
                         "reach26_again": compute(26, 0.0), "rank": rank, "paths": paths, "lookup": lookup})
    if a.once:
        for fn in variants.values():
            fn()
        vol.synchronize()
        return
    times = {v: [] for v in variants}
    for r in range(a.warmup + a.reps):
        for v, fn in variants.items():
            vol.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                times[v].append(t)
    out = {"tool": "bench_reach", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "size": n, "reps": a.reps,
           "clearance_mm": a.clearance, "device": torch.cuda.get_device_name(0), "library": os.environ.get("TSDF_HIP_LIB", "default"),
           "seed_point": [float(v) for v in seed[0]], "seed_mm_along_the_optical_axis": along, "bricks": ((n + 7) // 8) ** 3,
           "frontier_clusters": n_rows, "clusters_reached": n_goals, "paths_max_len": max_len, "lookup_points": W * H,
           "scratch_bytes": reach.scratch_bytes, "fields": {}}
    out["camera_position"] = [float(v) for v in camera_point[0]]
    for key, i in kept.items():
        out["fields"]["from the camera position, connectivity 26" if key == "camera" else "connectivity %d clearance %g" % key] = {
            "rounds": int(i.rounds), "n_traversable": int(i.n_traversable), "n_reached": int(i.n_reached), "max_cost_reached": int(i.max_cost_reached)}
    for v, ts in times.items():
        out[v + "_ms"] = round(float(np.median(ts)), 3)
        out[v + "_ms_range"] = [round(min(ts), 3), round(max(ts), 3)]
    out["note"] = ("host wall-clock of whole calls that end in a device synchronise, medians with [min, max], variants alternating inside every "
                   "repetition, all in one run; esdf_ms, find_frontiers_ms and fill_ms are yardsticks, not the code under "
                   "test; rounds is a diagnostic of the run; nothing about the speed was known when the feature was specified")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
