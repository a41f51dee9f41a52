#!/usr/bin/env python
"""What a weight cap does to a long stream: one JSON line.

The 512^3 / 640x480 config-3 surrogate driven through tsdf_pipeline_step as bench.py drives it, 600 steps on a cleared volume, for
cap 0 (off), 15 and 255, in interleaved rounds (cap 0, 15, 255, cap 0, 15, 255, ...).  Every step is closed by one event on the
pipeline's stream; a step's time is the interval between two consecutive events, so the host round trip of a widening shows as the
gap it leaves.  Per variant: the median step over steps 6-25 and over steps 300-600, the worst single step and its index, the worst
step among the first 150, weight_storage() at the end, and -- from one more pass per variant with tsdf_volume_set_timing on every
4th launch, kept apart because the brackets cost stream time -- the integrate kernel's mean time in both windows.  Each figure comes
with its spread (max - min) over the rounds.

The gate: the capped runs end in 8-bit storage, and none of their steps exceeds the worst step the cap-0 run
shows among its first 150 (before any widening can happen) by more than that figure's spread between rounds.

    python tools/bench_weight_cap.py [--steps 600] [--rounds 3] [--grid 512] [--out profiles/weight_cap_bench.json]
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
EARLY = (5, 25)              # steps 6-25, as indices [5, 25)
LATE_FROM = 299              # steps 300-600


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--stream-frames", type=int, default=200)
    ap.add_argument("--caps", default="0,15,255")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    args = ap.parse_args()
    import torch
    import tsdf_amd
    from tsdf_amd import synth
    from tsdf_amd.pipeline import FusionPipeline
    assert torch.cuda.is_available(), "needs a GPU"
    K, n = args.steps, args.grid
    assert K > LATE_FROM + 10, "--steps must reach the late window (steps 300 and on)"
    caps = [int(c) for c in args.caps.split(",")]

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=8) as pool:
        made = list(pool.map(lambda j: synth.depth_frame(j, args.stream_frames, seed=SEED), range(args.stream_frames)))
    depth_dev = torch.from_numpy(np.stack([d for d, _ in made]).view(np.int16)).cuda()
    cams = [c for _, c in made]
    F = len(made)
    vert = torch.empty((H * W, 3), dtype=torch.float32, device="cuda")
    norm = torch.empty_like(vert)

    vol = tsdf_amd.TSDFVolume((n, n, n), (3000.0,) * 3)
    pipe = FusionPipeline(vol, tsdf_amd.BilateralFilter(30.0, 4.5), tsdf_amd.GPURaycaster(W, H), W, H, overlap=True)
    stream = pipe.main
    events = [torch.cuda.Event(enable_timing=True) for _ in range(K + 1)]
    for e in events:             # (the runtime grows its signal pool in steps: outside every measured interval, as in bench.py)
        e.record(stream)
    torch.cuda.synchronize()

    def run(cap, timing_windows=False):
        vol.clear()
        vol.set_weight_cap(cap)
        kernel = {}
        events[0].record(stream)
        for i in range(K):
            if timing_windows and i in (EARLY[0], LATE_FROM):
                vol.set_timing(4)
            f, nxt = i % F, (i + 1) % F
            pipe.step(depth_dev[f].data_ptr(), cams[f], vert.data_ptr(), norm.data_ptr(),
                      depth_dev[nxt].data_ptr() if i + 1 < K else None, cams[nxt] if i + 1 < K else None)
            events[i + 1].record(stream)
            if timing_windows and i + 1 in (EARLY[1], K):
                launches, ms = vol.kernel_time("integrate")
                kernel["early" if i + 1 == EARLY[1] else "late"] = {"launches": launches, "mean_ms": ms}
                vol.set_timing(0)
        pipe.synchronize()
        torch.cuda.synchronize()
        if timing_windows:
            return kernel
        t = np.array([events[i].elapsed_time(events[i + 1]) for i in range(K)])
        return {"early_median_ms": float(np.median(t[EARLY[0]:EARLY[1]])), "late_median_ms": float(np.median(t[LATE_FROM:])),
                "worst_ms": float(t.max()), "worst_step": int(t.argmax()) + 1, "worst_first_150_ms": float(t[:150].max()),
                "storage_bits": vol.weight_storage()[0]}

    run(0)                       # (warm-up pass: allocations, the ray caster's tables; not reported)
    rounds = {c: [] for c in caps}
    for _ in range(args.rounds):
        for c in caps:
            rounds[c].append(run(c))
    kernels = {c: run(c, timing_windows=True) for c in caps}

    def fold(c):
        out = {}
        for key in ("early_median_ms", "late_median_ms", "worst_ms", "worst_first_150_ms"):
            v = [r[key] for r in rounds[c]]
            out[key] = float(np.median(v))
            out[key + "_spread"] = float(max(v) - min(v))
            out[key + "_rounds"] = v
        out["worst_step_rounds"] = [r["worst_step"] for r in rounds[c]]
        out["storage_bits"] = rounds[c][-1]["storage_bits"]
        out["storage_bits_rounds"] = [r["storage_bits"] for r in rounds[c]]
        out["integrate_kernel"] = kernels[c]
        return out

    variants = {str(c): fold(c) for c in caps}
    gate = None
    if 0 in caps:
        base = variants["0"]
        limit = max(base["worst_first_150_ms_rounds"]) + base["worst_first_150_ms_spread"]
        capped = [c for c in caps if 0 < c <= 255]
        gate = {"limit_ms": limit,
                "storage_is_8_bits": all(b == 8 for c in capped for b in variants[str(c)]["storage_bits_rounds"]),
                "worst_capped_step_ms": max([max(variants[str(c)]["worst_ms_rounds"]) for c in capped] or [0.0])}
        gate["passed"] = bool(gate["storage_is_8_bits"] and gate["worst_capped_step_ms"] <= limit)
    line = {"tool": "tools/bench_weight_cap.py", "grid": n, "image": [W, H], "steps": K, "rounds": args.rounds,
            "stream_frames": args.stream_frames, "device": torch.cuda.get_device_name(0), "variants": variants, "gate": gate}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    pipe.close()
    return 0 if (gate is None or gate["passed"]) else 1


if __name__ == "__main__":
    sys.exit(main())
