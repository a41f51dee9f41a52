#!/usr/bin/env python
"""What de-integration costs: one JSON line.

1. The removal kernel beside the plain one at 512^3 / 640x480, in the same run: per round a cleared volume takes --frames frames
   (integrate_packed_kernel, every launch bracketed by tsdf_volume_set_timing) and gives them back in the same order
   (integrate_packed_remove_kernel, bracketed the same way); rounds are interleaved by construction (in, out, in, out, ...).  Mean kernel
   time per round, the median over the rounds and the spread (max - min).  There is no threshold.
2. A --steps tracked run (FrameToModelTracker.process_device) with windows 0, 30 and 200: every step closed by one event on the
   tracker's stream, a step's time the interval between two events (a host round trip shows as the gap it leaves); median step, worst
   step and its index, weight_storage() at the end.  weight_bound still counts every integrate, so a windowed run looks at its real
   counts each time the bound reaches 255: that scan is among the worst steps.

    python tools/bench_deintegrate.py [--steps 600] [--rounds 3] [--grid 512] [--out profiles/deintegrate_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--stream-frames", type=int, default=200)
    ap.add_argument("--windows", default="0,30,200")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    args = ap.parse_args()
    import torch
    import tsdf_amd
    from tsdf_amd import synth
    from tsdf_amd.tracking import FrameToModelTracker
    assert torch.cuda.is_available(), "needs a GPU"
    n, K = args.grid, args.steps

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=8) as pool:
        made = list(pool.map(lambda j: synth.depth_frame(j, args.stream_frames, seed=SEED, noise=False), range(args.stream_frames)))
    depth_dev = torch.from_numpy(np.stack([d for d, _ in made]).view(np.int16)).cuda()
    cams = [c for _, c in made]
    F = len(made)
    torch.cuda.synchronize()

    # ---- 1: the two kernels
    vol = tsdf_amd.TSDFVolume((n, n, n), (3000.0,) * 3)
    plain, removal = [], []
    for r in range(args.rounds + 1):                             # (round 0 warms up: allocations; not reported)
        vol.clear()
        for out, call in ((plain, vol.integrate_device), (removal, vol.deintegrate_device)):
            vol.set_timing(1)
            for j in range(args.frames):
                call(depth_dev[j].data_ptr(), W, H, cams[j])
            launches, ms = vol.kernel_time("integrate")
            vol.set_timing(0)
            assert launches == args.frames
            if r:
                out.append(ms)
        assert vol.get_weight_data().max() == 0.0                # everything taken back out
    kernels = {"frames_per_round": args.frames,
               "integrate_packed_kernel_ms": float(np.median(plain)), "integrate_packed_kernel_ms_rounds": plain,
               "integrate_packed_kernel_ms_spread": float(max(plain) - min(plain)),
               "integrate_packed_remove_kernel_ms": float(np.median(removal)), "integrate_packed_remove_kernel_ms_rounds": removal,
               "integrate_packed_remove_kernel_ms_spread": float(max(removal) - min(removal))}
    kernels["ratio"] = kernels["integrate_packed_remove_kernel_ms"] / kernels["integrate_packed_kernel_ms"]
    del vol

    # ---- 2: tracked runs
    tracked = {}
    for window in [int(w) for w in args.windows.split(",")]:
        vol = tsdf_amd.TSDFVolume((n, n, n), (3000.0,) * 3)
        trk = FrameToModelTracker(vol, W, H, window=window)
        events = [torch.cuda.Event(enable_timing=True) for _ in range(K + 1)]
        for e in events:
            e.record(trk.stream)
        torch.cuda.synchronize()
        events[0].record(trk.stream)
        for i in range(K):
            f = i % F
            trk.process_device(depth_dev[f].data_ptr(), initial_pose=cams[0].pose().astype(np.float64).reshape(4, 4).T if i == 0 else None)
            events[i + 1].record(trk.stream)
        trk.synchronize()
        torch.cuda.synchronize()
        t = np.array([events[i].elapsed_time(events[i + 1]) for i in range(K)])
        order = np.argsort(t)[::-1]
        tracked[str(window)] = {"median_step_ms": float(np.median(t[5:])), "worst_step_ms": float(t[5:].max()), "worst_step": int(t[5:].argmax()) + 6,
                                "worst_five": [[int(j) + 1, float(t[j])] for j in order[:5]],
                                "storage_bits": vol.weight_storage()[0], "largest_weight": float(vol.get_weight_data().max())}
        trk.close()
        del trk, vol

    line = {"tool": "tools/bench_deintegrate.py", "grid": n, "image": [W, H], "steps": K, "rounds": args.rounds,
            "device": torch.cuda.get_device_name(0), "kernels": kernels, "tracked": tracked}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
