"""Cost of colour fusion at 512^3, 640 x 480, on bench.py's stream (seed 0x5EED0003): prints one JSON line.

  integrate_ms / integrate_colour_ms   device time of one integrate of a frame already in HBM, plain and with colour
  raycast_ms / raycast_colour_ms       device time of one ray cast (vertices + normals), plain and with the colour sample pass
  coloured_voxels_per_frame            voxels whose colour a frame updated (observation counts summed over the stream / frames)

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
    out = {
        "tool": "bench_colour", "size": n, "width": W, "height": H, "seed": "0x%X" % SEED, "rounds": a.rounds, "frames_per_round": a.frames,
        "integrate_ms": round(med["int"], 4), "integrate_colour_ms": round(med["int_c"], 4),
        "integrate_colour_ratio": round(med["int_c"] / med["int"], 3),
        "raycast_ms": round(med["ray"], 4), "raycast_colour_ms": round(med["ray_c"], 4),
        "raycast_colour_extra_us": round(1000.0 * (med["ray_c"] - med["ray"]), 1),
        "coloured_voxels_per_frame": round(observations / float(n_frames), 1),
        "note": "medians of event-bracketed synchronised steps; coloured voxels per frame = observation counts / frames "
                "(a lower bound once a count saturates at 255)",
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
