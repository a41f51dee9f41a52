"""Time of a mesh with normals on bench.py's scene (640 x 480, seed 0x5EED0003) at 256^3 and 512^3: the triangle soup with a normal
per soup vertex against the indexed mesh with a normal per shared vertex (include/tsdf_amd.h, "indexed mesh").  Prints one JSON line
and writes it to profiles/mesh_indexed_bench.json.

Per size, host wall-clock times of whole calls, each ending in a device synchronise, as the median (and range) of --reps
repetitions after --warmup, the variants alternating inside every repetition:

  soup_ms            extract_surface() + sample_field(unit gradient) on the soup: what TSDFVolume.extract_surface_with_normals does
                     (marching cubes, the soup to the host, the soup back to the device, one query per soup vertex, the normals to
                     the host)
  indexed_cold_ms    extract_mesh(normals=True) into a NEW handle, until its device arrays are complete (allocations included)
  indexed_warm_ms    the same into a handle that has held this mesh before: nothing is allocated
  indexed_host_ms    indexed_warm plus the download of vertices, indices and normals: the same information on the host as soup_ms

and the counts: soup vertices, unique vertices, their ratio, and the bytes of both results (12 bytes a position or normal, 4 an index).

    python tools/bench_mesh.py [--sizes 256 512] [--frames 24] [--reps 10] [--warmup 2]
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
    ap.add_argument("--frames", type=int, default=24, help="frames fused before the extractions")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_indexed_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_mesh needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    out = {"tool": "bench_mesh", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in a.sizes:
        vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        for i in range(a.frames):
            d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
            vol.integrate(d, W, H, cam)
        vol.synchronize()
        warm = tsdf_amd.Mesh()
        kept = {}

        def soup():
            V = vol.extract_surface()
            kept["soup"] = (V, vol.sample_field(V, weight=False, unit_gradient=True)[1])

        def indexed_cold():
            m = vol.extract_mesh(normals=True)
            m.device_buffers()          # (waits for the kernels that fill the arrays)
            m.close()

        def indexed_warm():
            vol.extract_mesh(normals=True, into=warm).device_buffers()

        def indexed_host():
            m = vol.extract_mesh(normals=True, into=warm)
            kept["indexed"] = (m.vertices, m.indices, m.normals)

        variants = {"soup": soup, "indexed_cold": indexed_cold, "indexed_warm": indexed_warm, "indexed_host": indexed_host}
        times = {v: [] for v in variants}
        for r in range(a.warmup + a.reps):
            for v, fn in variants.items():
                vol.synchronize()
                t0 = time.perf_counter()
                fn()
                t = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    times[v].append(t)
        S, SN = kept["soup"]
        V, I, N = kept["indexed"]
        # faster and different is not faster: the expansion of the indexed mesh is the soup, normals included
        same = lambda p, q: bool(np.all((p.view(np.uint32) == q.view(np.uint32)) | (np.isnan(p) & np.isnan(q))))
        assert same(V[I], S) and same(N[I], SN), "the indexed mesh does not expand to the soup"
        res = {"soup_vertices": int(len(S)), "unique_vertices": int(len(V)), "indices": int(len(I)),
               "soup_to_unique": round(len(S) / max(len(V), 1), 3),
               "soup_bytes": int(len(S) * 24), "indexed_bytes": int(len(V) * 24 + len(I) * 4),
               "scratch_bytes": warm.scratch_bytes, "scratch_bytes_per_voxel": round(warm.scratch_bytes / float(n) ** 3, 4)}
        for v, ts in times.items():
            res[v + "_ms"] = round(float(np.median(ts)), 3)
            res[v + "_ms_range"] = [round(min(ts), 3), round(max(ts), 3)]
        res["soup_over_indexed_warm"] = round(res["soup_ms"] / res["indexed_warm_ms"], 2)
        res["soup_over_indexed_host"] = round(res["soup_ms"] / res["indexed_host_ms"], 2)
        out["sizes"][str(n)] = res
        warm.close()
        vol.close()
    out["note"] = ("host wall-clock of whole calls that end in a device synchronise, medians with [min, max], variants alternating "
                   "inside every repetition; soup_ms holds two device-to-host copies and one host-to-device copy of soup-sized "
                   "arrays from pageable memory, indexed_warm_ms none")
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
