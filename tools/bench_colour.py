"""Cost of colour fusion at 512^3, 640 x 480, on bench.py's stream (seed 0x5EED0003): prints one JSON line.

  integrate_ms / integrate_colour_ms   device time of one integrate of a frame already in HBM, plain and with colour
  raycast_ms / raycast_colour_ms       device time of one ray cast (vertices + normals), plain and with the colour sample pass
  coloured_voxels_per_frame            voxels whose colour a frame updated (observation counts summed over the stream / frames)
  pipeline_step_ms / pipeline_step_colour_ms
                                       one step of FusionPipeline (filter, integrate, ray cast + normals; overlap on, the next
                                       frame announced and culled ahead, as bench.py drives it), plain (step) and coloured
                                       (step_colour, with the colours of the cast): per-step time of blocks of --frames steps

Two volumes -- one plain, one with colour -- are fed the same frames; each measured step is bracketed by HIP events on the
volume's stream around work that has been synchronised before, and the two variants alternate, over --rounds rounds.

    python tools/bench_colour.py [--frames 24] [--warmup 8] [--rounds 4]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=24, help="timed frames per round")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--pipeline-rounds", type=int, default=12, help="blocks of --frames steps per pipeline variant")
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n_frames = a.warmup + a.rounds * a.frames
    depth_dev, rgb_dev, cams = [], [], []
    for i in range(n_frames):
        d, cam = synth.depth_frame(i % PERIOD, PERIOD, seed=SEED)
        rgb, _ = synth.colour_frame(i % PERIOD, PERIOD, seed=SEED)
        depth_dev.append(torch.from_numpy(d.astype(np.int16)).to(dev))
        rgb_dev.append(torch.from_numpy(rgb.reshape(-1)).to(dev))
        cams.append(cam)
    n = a.size
    plain = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    colour = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    colour.enable_colour()
    for v in (plain, colour):
        v.set_stream(stream.cuda_stream)
    caster = tsdf_amd.GPURaycaster(W, H)
    V = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
    N = torch.empty_like(V)
    C = torch.empty((W * H, 3), dtype=torch.uint8, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def integrate(i, use_colour):
        if use_colour:
            colour.integrate_colour_device(depth_dev[i].data_ptr(), rgb_dev[i].data_ptr(), W, H, cams[i])
        else:
            plain.integrate_device(depth_dev[i].data_ptr(), W, H, cams[i])

    def cast(i, use_colour):
        if use_colour:
            caster.raycast_colour_device(colour, cams[i], V.data_ptr(), N.data_ptr(), C.data_ptr())
        else:
            caster.raycast_device(plain, cams[i], V.data_ptr(), N.data_ptr())

    for i in range(a.warmup):
        for c in (False, True):
            integrate(i, c)
            cast(i, c)
    torch.cuda.synchronize()
    t = {"int": [], "int_c": [], "ray": [], "ray_c": []}
    i = a.warmup
    for r in range(a.rounds):
        order = (False, True) if r % 2 == 0 else (True, False)   # alternate which variant goes first
        for _ in range(a.frames):
            for c in order:
                t["int_c" if c else "int"].append(timed(lambda: integrate(i, c)))
                t["ray_c" if c else "ray"].append(timed(lambda: cast(i, c)))
            i += 1
    torch.cuda.synchronize()
    words = colour.get_colour_data()
    observations = int((words >> np.uint32(24)).astype(np.int64).sum())
    med = {k: float(np.median(v)) for k, v in t.items()}
    for v in (plain, colour):   # (the pipeline steps below take volumes of their own)
        v.close()
    steps = pipeline_steps(a, torch, tsdf_amd, depth_dev, rgb_dev, cams, W, H, n)
    out = {
        "tool": "bench_colour", "size": n, "width": W, "height": H, "seed": "0x%X" % SEED, "rounds": a.rounds, "frames_per_round": a.frames,
        "integrate_ms": round(med["int"], 4), "integrate_colour_ms": round(med["int_c"], 4),
        "integrate_colour_ratio": round(med["int_c"] / med["int"], 3),
        "raycast_ms": round(med["ray"], 4), "raycast_colour_ms": round(med["ray_c"], 4),
        "raycast_colour_extra_us": round(1000.0 * (med["ray_c"] - med["ray"]), 1),
        "coloured_voxels_per_frame": round(observations / float(n_frames), 1),
        **steps,
        "note": "medians of event-bracketed synchronised steps; coloured voxels per frame = observation counts / frames "
                "(a lower bound once a count saturates at 255); pipeline steps: medians over --pipeline-rounds host-clocked blocks "
                "of --frames steps ending in a synchronise, the two variants alternating (every block's time in the *_samples_ms "
                "lists, the ratio's spread over the paired blocks in pipeline_step_colour_ratio_range)",
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))


def pipeline_steps(a, torch, tsdf_amd, depth_dev, rgb_dev, cams, W, H, n):
    """Plain against coloured FusionPipeline steps, alternated block by block."""
    import time
    from tsdf_amd.pipeline import FusionPipeline
    torch.cuda.synchronize()
    runs = {}
    for use_colour in (False, True):
        vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        if use_colour:
            vol.enable_colour()
        pipe = FusionPipeline(vol, tsdf_amd.BilateralFilter(30.0, 4.5), tsdf_amd.GPURaycaster(W, H), W, H, overlap=True)
        V = torch.empty((W * H, 3), dtype=torch.float32, device=depth_dev[0].device)
        runs[use_colour] = (vol, pipe, V, torch.empty_like(V), torch.empty((W * H, 3), dtype=torch.uint8, device=V.device))
    F = len(depth_dev)

    def steps(use_colour, first, count):
        vol, pipe, V, N, C = runs[use_colour]
        for i in range(first, first + count):
            f, g = i % F, (i + 1) % F
            if use_colour:
                pipe.step_colour(depth_dev[f].data_ptr(), rgb_dev[f].data_ptr(), cams[f], V.data_ptr(), N.data_ptr(), C.data_ptr(),
                                 depth_dev[g].data_ptr(), cams[g])
            else:
                pipe.step(depth_dev[f].data_ptr(), cams[f], V.data_ptr(), N.data_ptr(), depth_dev[g].data_ptr(), cams[g])
        pipe.synchronize()

    for c in (False, True):
        steps(c, 0, a.warmup)
    t = {False: [], True: []}
    i = a.warmup
    for r in range(a.pipeline_rounds):
        for c in ((False, True) if r % 2 == 0 else (True, False)):
            t0 = time.perf_counter()
            steps(c, i, a.frames)
            t[c].append((time.perf_counter() - t0) * 1e3 / a.frames)
        i += a.frames
    for vol, pipe, *_ in runs.values():
        pipe.close()
        vol.close()
    plain, coloured = float(np.median(t[False])), float(np.median(t[True]))
    pair = [c / p for p, c in zip(t[False], t[True])]
    return {"pipeline_step_ms": round(plain, 4), "pipeline_step_colour_ms": round(coloured, 4),
            "pipeline_step_colour_ratio": round(coloured / plain, 3),
            "pipeline_step_colour_ratio_range": [round(min(pair), 3), round(max(pair), 3)],
            "pipeline_step_samples_ms": [round(x, 4) for x in t[False]],
            "pipeline_step_colour_samples_ms": [round(x, 4) for x in t[True]]}


if __name__ == "__main__":
    main()
