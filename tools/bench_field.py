"""Rate of the field queries (include/tsdf_amd.h, "field queries") on bench.py's scene: 512^3, 640 x 480, seed 0x5EED0003.  Prints one
JSON line and writes it to profiles/field_query_bench.json.

Two point sets, both already in HBM: the vertex map of one ray cast (640 x 480 points, misses included: they are NaN and cost a
point read and a NaN store) and the vertices of the extracted mesh (cube order).  For each, the device time of one query per output
set -- distance only, weight only, distance + raw gradient, unit gradient only (what normals cost), all three -- as the median of
--reps event-bracketed launches after --warmup, the variants alternating inside every repetition.

  *_mpts_per_s       million points per second of that variant
  *_tap_gbps         bytes of distance taps the lanes asked for (8 or 56 taps x 4 bytes a valid point) per second / 1e9: what the
                     vector L1 served, not HBM traffic (of the gradient's 56 taps 32 are distinct voxels, and neighbouring points
                     share most of those)

    python tools/bench_field.py [--size 512] [--frames 24] [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (distance, gradient, weight, unit) of each variant, and the distance taps a valid point asks for
VARIANTS = {"distance": (True, False, False, False, 8), "weight": (False, False, True, False, 0),
            "distance_gradient": (True, True, False, False, 56), "unit_gradient": (False, True, False, True, 48),
            "all": (True, True, True, False, 56)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=24, help="frames fused before the queries")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_query_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_field needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = a.size
    vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    vol.set_stream(stream.cuda_stream)
    cam = None
    for i in range(a.frames):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        vol.integrate(d, W, H, cam)
    V = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
    tsdf_amd.GPURaycaster(W, H).raycast_device(vol, cam, V.data_ptr())
    vol.synchronize()
    mesh = torch.from_numpy(vol.extract_surface()).to(dev)
    sets = {"vertex_map": V, "mesh": mesh}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    out = {"tool": "bench_field", "size": n, "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames,
           "reps": a.reps, "weight_storage_bits": vol.weight_storage()[0], "device": torch.cuda.get_device_name(0)}
    for name, P in sets.items():
        m = int(P.shape[0])
        D = torch.empty(m, dtype=torch.float32, device=dev)
        G = torch.empty((m, 3), dtype=torch.float32, device=dev)
        Wt = torch.empty(m, dtype=torch.float32, device=dev)

        def query(v):
            d, g, w, unit, _ = VARIANTS[v]
            vol.sample_field_device(m, P.data_ptr(), D.data_ptr() if d else None, G.data_ptr() if g else None,
                                    Wt.data_ptr() if w else None, unit_gradient=unit, stream=stream.cuda_stream)

        times = {v: [] for v in VARIANTS}
        for r in range(a.warmup + a.reps):
            for v in VARIANTS:
                t = timed(lambda: query(v))
                if r >= a.warmup:
                    times[v].append(t)
        torch.cuda.synchronize()
        query("all")
        torch.cuda.synchronize()
        valid = int((~torch.isnan(D)).sum().item())
        with_gradient = int((~torch.isnan(G).any(dim=1)).sum().item())
        out[name] = {"points": m, "valid_points": valid, "points_with_gradient": with_gradient}
        for v, ts in times.items():
            ms = float(np.median(ts))
            taps = VARIANTS[v][4]
            lanes = with_gradient if taps >= 48 else valid
            out[name][v + "_ms"] = round(ms, 4)
            out[name][v + "_ms_range"] = [round(min(ts), 4), round(max(ts), 4)]
            out[name][v + "_mpts_per_s"] = round(m / ms / 1e3, 1)
            if taps:
                extra = 8 * 4 * valid if taps == 56 else 0     # (the distance's own taps beside the gradient's 48)
                out[name][v + "_tap_gbps"] = round(((taps - (8 if taps == 56 else 0)) * 4 * lanes + extra) / ms / 1e6, 1)
    out["note"] = ("medians of event-bracketed launches on one stream, variants alternating; a launch of this size is tens of "
                   "microseconds, so the dispatch itself is part of every figure; tap rates count the loads the lanes issue, not HBM traffic")
    vol.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
