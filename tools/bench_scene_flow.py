"""Time of one scene-flow frame (include/tsdf_amd.h, "scene flow") on bench.py's scene (640 x 480, seed 0x5EED0003) fused into a 512^3
volume, beside a warm extraction of the indexed mesh of the same volume from the same run.  Prints one JSON line and writes it to
profiles/scene_flow_bench.json.

Host wall-clock times of whole calls, each ending in a device synchronise, as the median (and range) of --reps repetitions after
--warmup, the variants alternating inside every repetition:

  extract_warm_ms     extract_mesh() of the whole grid into a handle that has held this mesh before, until its arrays are complete
  apply_ms            apply_scene_flow_device with that handle: depth and flow already on the device, canonical vertices
  apply_deformed_ms   the same with the vertices pushed through the deformation field first (TSDF_SCENE_FLOW_DEFORMED)
  apply_host_ms       apply_scene_flow from host images (the two uploads included)

The flow is a constant whose sign alternates between repetitions, so that the nodes stay where a sequence would leave them.  The
byte counts are the model of DESIGN.md 22, computed from the counts of this run.

    python tools/bench_scene_flow.py [--size 512] [--frames 24] [--reps 10] [--warmup 2]
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
    ap.add_argument("--frames", type=int, default=24, help="frames fused before the measurements")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_flow_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    from tsdf_amd.api import _DeviceArray
    assert torch.cuda.is_available(), "bench_scene_flow needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    n = a.size
    vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    for i in range(a.frames):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        vol.integrate(d, W, H, cam)
    vol.synchronize()
    depth, cam = synth.depth_frame(a.frames - 1, PERIOD, seed=SEED)
    depth = np.ascontiguousarray(depth, np.uint16).reshape(H, W)
    flows = [np.ascontiguousarray(np.broadcast_to(np.asarray(f, np.float32), (H, W, 3))) for f in ((1.5, -1.0, 2.0), (-1.5, 1.0, -2.0))]
    mesh = vol.extract_mesh()
    vol.deformation()          # (the 24 bytes a voxel of nodes are materialised once, outside the timed calls)
    info = {}

    with _DeviceArray(depth) as dd, _DeviceArray(flows[0]) as f0, _DeviceArray(flows[1]) as f1:
        dflow = [f0.ptr.value, f1.ptr.value]

        def extract_warm(r):
            vol.extract_mesh(into=mesh).device_buffers()

        def apply(r):
            info["apply"] = vol.apply_scene_flow_device(dd.ptr.value, dflow[r % 2], W, H, cam, mesh=mesh)

        def apply_deformed(r):
            info["apply_deformed"] = vol.apply_scene_flow_device(dd.ptr.value, dflow[r % 2], W, H, cam, deformed=True, mesh=mesh)

        def apply_host(r):
            info["apply_host"] = vol.apply_scene_flow(depth, flows[r % 2], cam, mesh=mesh)

        variants = {"extract_warm": extract_warm, "apply": apply, "apply_deformed": apply_deformed, "apply_host": apply_host}
        times = {v: [] for v in variants}
        for r in range(a.warmup + a.reps):
            for v, fn in variants.items():
                vol.synchronize()
                t0 = time.perf_counter()
                fn(r)
                t = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    times[v].append(t)

    nv, ni = mesh.n_vertices, mesh.n_indices
    chunks = (n ** 3 + 63) // 64
    c, moved = info["apply"]["n_correspondences"], info["apply"]["n_nodes_moved"]
    assert nv > 0 and c > 0 and moved > 0, info
    model = {
        # position 12, depth 2 (vertices that land in the image; counted for all), flow 12 per vertex that passes the depth test, 8 written
        "match_bytes": nv * (12 + 2 + 8) + c * 12,
        # one index read and one 4-byte integer atomic per soup vertex
        "multiplicity_bytes": ni * (4 + 4),
        # 32 bytes per 64 voxels whatever the surface; per edge end (two per vertex) 8 bytes of {pixel, multiplicity}, 12 of flow where
        # it corresponds; 12 read and 12 written per node moved
        "apply_bytes": chunks * 32 + 2 * nv * 8 + 2 * c * 12 + moved * 24,
        "extract_bytes_at_least": 3 * 4 * n ** 3,    # the three kernels that read every distance (edges, vertices, triangles), once each
    }
    out = {"tool": "bench_scene_flow", "size": n, "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "threshold": 10.0, "vertices": nv, "indices": ni, "chunks": chunks,
           "info": info, "scratch_bytes": mesh.scratch_bytes, "model": model}
    for v, ts in times.items():
        out[v + "_ms"] = round(float(np.median(ts)), 3)
        out[v + "_ms_range"] = [round(min(ts), 3), round(max(ts), 3)]
    out["apply_over_extract_warm"] = round(out["apply_ms"] / out["extract_warm_ms"], 3)
    out["apply_deformed_over_extract_warm"] = round(out["apply_deformed_ms"] / out["extract_warm_ms"], 3)
    out["note"] = ("host wall-clock of whole calls that end in a device synchronise, medians with [min, max], variants alternating inside "
                   "every repetition; apply_host_ms holds the uploads of both images from pageable memory; the model's bytes are computed "
                   "from this run's counts, not measured")
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)
    mesh.close()
    vol.close()


if __name__ == "__main__":
    main()
