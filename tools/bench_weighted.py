#!/usr/bin/env python
"""What weighted integration costs: one JSON line.

bench.py's scene (512^3 over 3 m, 640x480, its depth stream).  Two volumes with fp32 weights hold the same --frames fused frames; the
next frames are then fused into both, plain integrate (integrate_kernel<false, false, true>: the yardstick) on the one and weighted
integrate with the 1/z^2 model's weights on the other, the two alternating, --reps times each.  Per side: the call on the volume's stream
between two events (depth tile maxima / weight mask, culling, the integrate kernel) and the integrate kernel alone
(tsdf_volume_set_timing: the dispatch's own timestamps), as median, min and max.  tsdf_depth_weights_device is timed alone, for each
flag combination, the same way.

    python tools/bench_weighted.py [--grid 512] [--frames 8] [--reps 10] [--z-ref 2400] [--out profiles/weighted_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED0003            # bench.py's stream
W, H = 640, 480


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--frames", type=int, default=8, help="frames fused into both volumes before the measurement")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stream-frames", type=int, default=200)
    ap.add_argument("--z-ref", type=float, default=2400.0)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    args = ap.parse_args()
    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "needs a GPU"
    n, reps = args.grid, args.reps
    total = args.frames + reps + 2

    made = [synth.depth_frame(j, args.stream_frames, seed=SEED) for j in range(total)]
    depth_dev = torch.from_numpy(np.stack([d for d, _ in made]).view(np.int16)).cuda()
    cams = [c for _, c in made]
    weights = torch.empty((total, H * W), dtype=torch.float32, device="cuda")
    scratch = torch.empty(H * W, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for j in range(total):
        tsdf_amd.depth_weights_device(W, H, depth_dev[j].data_ptr(), cams[j].kinv(), tsdf_amd.WEIGHTS_INVERSE_SQUARE, args.z_ref, weights[j].data_ptr())
    torch.cuda.synchronize()

    plain, weighted = tsdf_amd.TSDFVolume((n, n, n), (3000.0,) * 3), tsdf_amd.TSDFVolume((n, n, n), (3000.0,) * 3)
    plain.set_weight_storage(32)
    weighted.set_weight_storage(32)
    streams = {}
    for name, v in (("plain", plain), ("weighted", weighted)):
        streams[name] = torch.cuda.ExternalStream(v.stream_ptr()) if v.stream_ptr() else torch.cuda.default_stream()

    def step(name, j):
        if name == "plain":
            plain.integrate_device(depth_dev[j].data_ptr(), W, H, cams[j])
        else:
            weighted.integrate_weighted_device(depth_dev[j].data_ptr(), weights[j].data_ptr(), W, H, cams[j])

    for j in range(args.frames + 2):          # (the last two: warm-up of both paths at the measured state)
        step("plain", j)
        step("weighted", j)
    plain.synchronize()
    weighted.synchronize()

    calls = {"plain": [], "weighted": []}
    kernels = {"plain": [], "weighted": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for r in range(reps):
        j = args.frames + 2 + r
        for name, v in (("plain", plain), ("weighted", weighted)):
            v.set_timing(True)
            ev[0].record(streams[name])
            step(name, j)
            ev[1].record(streams[name])
            v.synchronize()
            torch.cuda.synchronize()
            calls[name].append(ev[0].elapsed_time(ev[1]))
            launches, ms = v.kernel_time("integrate")
            assert launches == 1, launches
            kernels[name].append(ms)
            v.set_timing(False)

    models = {}
    s = torch.cuda.current_stream()
    for flags in (0, 1, 2, 3):
        t = []
        for r in range(reps + 2):
            j = args.frames + r
            ev[0].record(s)
            tsdf_amd.depth_weights_device(W, H, depth_dev[j].data_ptr(), cams[j].kinv(), flags, args.z_ref, scratch.data_ptr(), s.cuda_stream)
            ev[1].record(s)
            torch.cuda.synchronize()
            t.append(ev[0].elapsed_time(ev[1]))
        models[str(flags)] = stats(t[2:])

    line = {"tool": "tools/bench_weighted.py", "grid": n, "image": [W, H], "frames_before": args.frames + 2, "reps": reps, "z_ref": args.z_ref,
            "device": torch.cuda.get_device_name(0),
            "plain": {"call": stats(calls["plain"]), "integrate_kernel": stats(kernels["plain"])},
            "weighted": {"call": stats(calls["weighted"]), "integrate_weighted_kernel": stats(kernels["weighted"])},
            "kernel_ratio_weighted_over_plain": float(np.median(kernels["weighted"]) / np.median(kernels["plain"])),
            "depth_weights_device_by_flags": models,
            "storage_bits": [plain.weight_storage()[0], weighted.weight_storage()[0]]}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
