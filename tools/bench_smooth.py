"""Cost of smoothing a mesh on the device (include/tsdf_amd.h, "mesh smoothing"), on bench.py's scene (640 x 480, seed 0x5EED0003, 24
noisy frames fused with colour) at 256^3 and 512^3, the mesh extracted once with normals and colours into a warm handle.  Prints one JSON
line and writes it to profiles/smooth_bench.json.

Per size, host wall-clock times of whole calls, each ending in a device synchronise, as the median (and range) of --reps repetitions
after --warmup, the variants alternating inside every repetition:

  smooth_ms            Mesh.smooth(10, 0.5, -0.53) into a warm handle: the row build, one synchronise, 20 passes
  smooth_pins_ms       ... with pin_boundary: the edge table as well
  smooth_normals_ms    ... with normals: the face normals of the smoothed positions as well
  smooth_both_ms       ... with both
  one_pass_ms          Mesh.smooth(1, 0.5, 0.0): the row build and a single pass
  compute_normals_ms   Mesh.compute_normals() on the smoothed mesh
  extract_ms           the extraction of the same mesh into its warm handle (normals and colours sampled from the field)
  simplify_ms          Mesh.simplify at a cell of 2 voxels into a warm handle

Derived: pass_ms = (smooth_ms - one_pass_ms) / 19, the cost of one more pass; row_build_ms = one_pass_ms - pass_ms, what a call pays before
its first pass (memsets, the count, the scan, the fill, the copies of indices, normals and colours, the synchronise).  gather_bytes_per_vertex
is what a pass reads and writes per vertex by the layout: 8 bytes of row bounds, 12 of its own position, 8 + 24 per pair of its row, 12
written -- requested bytes: a position is asked for by every row that names it (six on average) and mostly served by the caches, so
pass_requested_gb_per_s is no HBM rate.  The plain result is compared with the numpy reference of the contract bit for bit; any difference fails the run.

    python tools/bench_smooth.py [--sizes 256 512] [--frames 24] [--reps 10] [--warmup 2]
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
    ap.add_argument("--frames", type=int, default=24, help="frames fused before the extraction")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="leave the comparison with the numpy reference out (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tests import smooth_ref
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_smooth needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    ITERATIONS, LAM, MU = 10, 0.5, -0.53
    out = {"tool": "bench_smooth", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "reps": a.reps,
           "iterations": ITERATIONS, "lambda": LAM, "mu": MU, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in a.sizes:
        vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        vol.enable_colour()
        for i in range(a.frames):
            d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
            rgb, _ = synth.colour_frame(i, PERIOD, seed=SEED)
            vol.integrate_colour(d, rgb, W, H, cam)
        vol.synchronize()
        mesh, dst, small = tsdf_amd.Mesh(), tsdf_amd.Mesh(), tsdf_amd.Mesh()
        cell = float(np.float32(2.0 * 3000.0 / n))

        def smooth(pins, normals):
            return lambda: mesh.smooth(ITERATIONS, LAM, MU, pin_boundary=pins, normals=normals, into=dst).device_buffers()

        variants = {
            "extract": lambda: vol.extract_mesh(normals=True, colours=True, into=mesh).device_buffers(),
            "simplify": lambda: mesh.simplify(cell, into=small).device_buffers(),
            "one_pass": lambda: mesh.smooth(1, LAM, 0.0, into=dst).device_buffers(),
            "smooth_pins": smooth(True, False),
            "smooth_normals": smooth(False, True),
            "smooth_both": smooth(True, True),
            "smooth": smooth(False, False),
            "compute_normals": lambda: dst.compute_normals().device_buffers(),
        }
        times = {v: [] for v in variants}
        for r in range(a.warmup + a.reps):
            for v, fn in variants.items():
                vol.synchronize()
                t0 = time.perf_counter()
                fn()
                t = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    times[v].append(t)
        V, I = mesh.vertices, mesh.indices
        pairs = smooth_ref.degrees(V, I) // 2
        res = {"vertices": mesh.n_vertices, "triangles": mesh.n_indices // 3, "live_triangles": int(pairs.sum() // 3),
               "loose_vertices": int(smooth_ref.loose_vertices(V).sum()), "longest_row_pairs": int(pairs.max()) if len(pairs) else 0,
               "mean_row_pairs": round(float(pairs.mean()), 3) if len(pairs) else 0.0,
               "gather_bytes_per_vertex": round(float(32 + 32 * pairs.mean()), 1) if len(pairs) else 0.0,
               "dst_scratch_bytes": dst.scratch_bytes}
        if not a.no_host:   # faster and different is not faster
            mesh.smooth(ITERATIONS, LAM, MU, into=dst)
            assert dst.vertices.tobytes() == smooth_ref.smooth(V, I, ITERATIONS, LAM, MU).tobytes(), "the device's vertices differ from numpy's"
            res["pinned_vertices"] = int(smooth_ref.pinned(V, I).sum())
        for v, ts in times.items():
            res[v + "_ms"] = round(float(np.median(ts)), 3)
            res[v + "_ms_range"] = [round(min(ts), 3), round(max(ts), 3)]
        res["pass_ms"] = round((res["smooth_ms"] - res["one_pass_ms"]) / (2 * ITERATIONS - 1), 4)
        res["row_build_ms"] = round(res["one_pass_ms"] - res["pass_ms"], 3)
        # (requested bytes: a vertex's position is asked for by every row that names it and mostly served by the caches, so this is
        # no HBM rate)
        res["pass_requested_gb_per_s"] = round(res["gather_bytes_per_vertex"] * res["vertices"] / max(res["pass_ms"], 1e-9) / 1e6, 1)
        out["sizes"][str(n)] = res
        for m in (mesh, dst, small):
            m.close()
        vol.close()
    out["note"] = ("host wall-clock of whole calls that end in a device synchronise, medians with [min, max], variants alternating inside "
                   "every repetition; pass_ms and row_build_ms are derived from smooth_ms and one_pass_ms; gather_bytes_per_vertex is by "
                   "the layout, not a counter")
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
