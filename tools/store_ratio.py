#!/usr/bin/env python3
"""How many of the voxels an integrate updates get a distance stored (GPU box).

integrate stores a distance only when the blend changes its bits (integrate_packed.hip, blend_and_store); with counting on,
the volume counts both (tsdf_volume_last_updated_voxels / tsdf_volume_last_distance_stores).  This replays bench.py's stream
(config 3: 512^3, 3 m, synthetic frames of its seed, the same bilateral filter) on a cleared volume and prints one JSON line:
per frame the updated voxels, the distances stored and their ratio, then the ratio over the frames bench.py times
(--warmup .. --warmup + --steps).

    python tools/store_ratio.py [--grid 512] [--warmup 5] [--steps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--physical", type=float, default=3000.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--stream-frames", type=int, default=200)
    a = ap.parse_args()

    import tsdf_amd
    from tsdf_amd import synth
    import bench

    W, H = bench.W, bench.H
    n = a.grid
    vol = tsdf_amd.TSDFVolume((n, n, n), (a.physical,) * 3)
    bil = tsdf_amd.BilateralFilter(30.0, 4.5)
    vol.set_counting(True)
    rows = []
    for i in range(a.warmup + a.steps):
        d, cam = synth.depth_frame(i % a.stream_frames, a.stream_frames, seed=bench.SEED)
        bil.filter(d, W, H)
        vol.integrate(d, W, H, cam)
        u, s = vol.last_updated_voxels(), vol.last_distance_stores()
        rows.append({"frame": i, "updated": u, "stores": s, "ratio": round(s / u, 4) if u else None})
    vol.set_counting(False)
    timed = rows[a.warmup:]
    U, S = sum(r["updated"] for r in timed), sum(r["stores"] for r in timed)
    print(json.dumps({"grid": n, "warmup": a.warmup, "steps": a.steps, "weight_storage_bits": vol.weight_storage()[0],
                      "timed_updated": U, "timed_stores": S, "timed_store_ratio": round(S / U, 4) if U else None,
                      "frames": rows}))


if __name__ == "__main__":
    main()
