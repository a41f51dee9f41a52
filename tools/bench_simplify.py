"""Time of simplifying a mesh on the device (include/tsdf_amd.h, "mesh simplification") against what a user does without it, on
bench.py's scene (640 x 480, seed 0x5EED0003, 24 noisy frames fused with colour) at 256^3 and 512^3, the mesh extracted once with
normals and colours into a warm handle, at cells of 2 and 4 voxels.  Prints one JSON line and writes it to profiles/simplify_bench.json.

Per size and cell, host wall-clock times of whole calls, each ending in a device synchronise, as the median (and range) of --reps
repetitions after --warmup, the variants alternating inside every repetition:

  simplify_ms     Mesh.simplify(cell) into a warm handle, until its arrays are complete: two memsets, nine launches, one synchronise
  host_ms         the yardstick: tsdf_mesh_download of the four arrays and the numpy reference of the contract (np.unique on the keys,
                  np.add.at on int64; host_download_ms and host_reference_ms are its two parts); the result is then on the host

The yardstick's four arrays are compared with the device's bit for bit; any difference fails the run.  Also recorded: vertices and
triangles before and after, the multi-member clusters, the duplicate triangle sets left (out of scope: two triples on the same three
clusters are both kept), the scratch the handle holds.  The per-kernel split comes from a separate rocprofv3 --kernel-trace --stats run
of this tool (profiles/simplify_kernel_stats.txt).

    python tools/bench_simplify.py [--sizes 256 512] [--cells 2 4] [--frames 24] [--reps 10] [--warmup 2]
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0], help="cell sizes in voxels")
    ap.add_argument("--frames", type=int, default=24, help="frames fused before the extraction")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="leave the yardstick out (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tests import simplify_ref
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_simplify needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    out = {"tool": "bench_simplify", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in a.sizes:
        vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        vol.enable_colour()
        for i in range(a.frames):
            d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
            rgb, _ = synth.colour_frame(i, PERIOD, seed=SEED)
            vol.integrate_colour(d, rgb, W, H, cam)
        vol.synchronize()
        mesh, dst = tsdf_amd.Mesh(), tsdf_amd.Mesh()
        vol.extract_mesh(normals=True, colours=True, into=mesh).device_buffers()
        per_size = {"vertices": mesh.n_vertices, "triangles": mesh.n_indices // 3, "cells": {}}
        for voxels in a.cells:
            cell = float(np.float32(voxels * 3000.0 / n))
            kept = {}

            def simplify():
                mesh.simplify(cell, into=dst).device_buffers()

            def host():
                t0 = time.perf_counter()
                V, I, N, C = mesh.vertices, mesh.indices, mesh.normals, mesh.colours
                t1 = time.perf_counter()
                kept["host"] = simplify_ref.simplify(V, I, cell, N, C)
                t2 = time.perf_counter()
                kept.setdefault("parts", []).append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))

            variants = {"simplify": simplify} if a.no_host else {"simplify": simplify, "host": host}
            times = {v: [] for v in variants}
            for r in range(a.warmup + a.reps):
                for v, fn in variants.items():
                    vol.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    t = (time.perf_counter() - t0) * 1e3
                    if r >= a.warmup:
                        times[v].append(t)
            res = {"cell_mm": cell, "kept_vertices": dst.n_vertices, "kept_triangles": dst.n_indices // 3,
                   "vertex_share": round(dst.n_vertices / max(mesh.n_vertices, 1), 4),
                   "triangle_share": round(dst.n_indices / max(mesh.n_indices, 1), 4),
                   "duplicate_triangles": simplify_ref.duplicate_triangles(dst.indices), "dst_scratch_bytes": dst.scratch_bytes}
            if not a.no_host:   # faster and different is not faster
                hV, hI, hN, hC, cluster = kept["host"]
                same = lambda x, y: bool(np.all((x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))))
                assert dst.vertices.tobytes() == hV.tobytes(), "the device's vertices differ from numpy's"
                assert np.array_equal(dst.indices, hI), "the device's indices differ from numpy's"
                assert same(dst.normals, hN), "the device's normals differ from numpy's"
                assert np.array_equal(dst.colours, hC), "the device's colours differ from numpy's"
                counts = np.bincount(cluster)
                res.update(multi_member_clusters=int((counts > 1).sum()), largest_cluster=int(counts.max()),
                           loose_vertices=int(simplify_ref.cells(mesh.vertices, cell)[0].sum()))
                parts = np.array(kept["parts"][a.warmup:])
                res["host_download_ms"] = round(float(np.median(parts[:, 0])), 3)
                res["host_reference_ms"] = round(float(np.median(parts[:, 1])), 3)
            for v, ts in times.items():
                res[v + "_ms"] = round(float(np.median(ts)), 3)
                res[v + "_ms_range"] = [round(min(ts), 3), round(max(ts), 3)]
            if not a.no_host:
                res["host_over_device"] = round(res["host_ms"] / res["simplify_ms"], 2)
            per_size["cells"]["%g" % voxels] = res
        out["sizes"][str(n)] = per_size
        mesh.close()
        dst.close()
        vol.close()
    out["note"] = ("host wall-clock of whole calls that end in a device synchronise, medians with [min, max], variants alternating inside "
                   "every repetition; host_ms is the download of the four arrays from pageable memory and the numpy reference, and leaves "
                   "the result on the host; simplify_ms leaves it on the device")
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
