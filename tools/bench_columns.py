"""Time of the column maps (include/tsdf_amd.h, "column maps") on bench.py's scene (640 x 480, seed 0x5EED0003), 25 frames fused at
512^3, in each weight storage (8-bit, 16-bit, fp32).  Prints one JSON line and writes it to profiles/columns_bench.json.

Per storage, host wall-clock times of whole calls, each ending in a wait for the handle's work, as the median (and range) of --reps
repetitions after --warmup, the variants alternating inside every repetition, every yardstick in the same run:

  axis0_ms / axis1_ms / axis2_ms   column_map(axis) over the whole band into a warm handle (columns_walk_kernel; on axis 0 its lanes lie
                                   X words apart.  The A/B against a row kernel for axis 0 that was not kept:
                                   profiles/columns_row_kernel_ab.json)
  axis2_esdf_ms         column_map(2, esdf=...) with a warm ESDF of the same volume: 4 more bytes a voxel
  classify_ms           classify_device(1, 2) on a warm axis-2 map, into a device array
  find_frontiers_ms     yardstick: find_frontiers into a warm handle -- the same state for every voxel plus six neighbours and a scan
  stream_read_ms        yardstick: a plain streaming read (torch sum) of as many bytes as the weights take in this storage

    python tools/bench_columns.py [--size 512] [--frames 25] [--reps 10] [--warmup 2] [--once] [--out FILE]

--once: one call of each per storage and nothing else (for a kernel trace).
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
    ap.add_argument("--esdf-cap", type=float, default=100.0)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "columns_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_columns needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    n = a.size
    out = {"tool": "bench_columns", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "size": n, "reps": a.reps,
           "esdf_cap_mm": a.esdf_cap, "device": torch.cuda.get_device_name(0), "storages": {}}
    for bits in (8, 16, 32):
        vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        for i in range(a.frames):
            d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
            vol.integrate(d, W, H, cam)
        if vol.weight_storage()[0] != bits:
            vol.set_weight_storage(bits)
        vol.synchronize()
        cm, classified, ex = tsdf_amd.ColumnMap(), tsdf_amd.ColumnMap(), tsdf_amd.Explorer()
        esdf = vol.compute_esdf(a.esdf_cap)
        esdf.device_buffer()
        vol.column_map(2, into=classified).device_buffer()
        cells = torch.zeros(n * n, dtype=torch.uint8, device="cuda")
        weights_like = torch.zeros(n ** 3 * bits // 32, dtype=torch.int32, device="cuda")
        kept = {}

        def project(axis, **kw):
            def run():
                vol.column_map(axis, into=cm, **kw).device_buffer()   # (waits for the kernel and the counters' copy)
            return run

        def classify():
            classified.classify_device(1, 2, cells.data_ptr())
            kept["info"] = classified.info                             # (waits)

        def stream_read():
            kept["sum"] = int(weights_like.sum().item())

        variants = {"axis0": project(0), "axis1": project(1), "axis2": project(2),
                    "axis2_esdf": project(2, esdf=esdf), "classify": classify, "find_frontiers": lambda: vol.find_frontiers(into=ex),
                    "stream_read": stream_read}
        if a.once:
            for fn in variants.values():
                fn()
            vol.synchronize()
        else:
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
            vol.column_map(0, into=cm)
            i, c, e = cm.info, kept["info"], ex.info
            assert (int(i.n_unknown), int(i.n_free), int(i.n_occupied)) == (int(e.n_unknown), int(e.n_free), int(e.n_occupied))
            res = {"n_unknown": int(i.n_unknown), "n_free": int(i.n_free), "n_occupied": int(i.n_occupied), "n_ground_axis0": int(i.n_ground),
                   "n_ground_axis2": int(c.n_ground), "n_traversable_axis2": int(c.n_traversable), "n_blocked_axis2": int(c.n_blocked),
                   "scratch_bytes": cm.scratch_bytes, "weight_bytes_read_by_stream_read": int(weights_like.numel()) * 4}
            for v, ts in times.items():
                res[v + "_ms"] = round(float(np.median(ts)), 3)
                res[v + "_ms_range"] = [round(min(ts), 3), round(max(ts), 3)]
            out["storages"][str(bits)] = res
        for h in (cm, classified, ex, esdf):
            h.close()
        vol.close()
    if a.once:
        return
    out["note"] = ("host wall-clock of whole calls that end in a wait for the handle, medians with [min, max], variants alternating inside "
                   "every repetition, all in one run; find_frontiers_ms and stream_read_ms are yardsticks, not the code under test; nothing "
                   "about the speed was known when the feature was specified")
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
