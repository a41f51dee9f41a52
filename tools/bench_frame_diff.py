"""Time of the frame differences (include/tsdf_amd.h, "frame differences") at 640 x 480 on bench.py's scene (seed 0x5EED0003): 25 frames
fused at --size^3, then the next frame with a disc pasted in front of the scene (synth.moving_disc_frame) compared with the model's depth
image from its camera.  Prints one JSON line and writes it to profiles/frame_diff_bench.json.

Host wall-clock times of whole calls, each followed by a device synchronisation inside its timed region (compare and cluster return with
their last kernel, the list's and the rows', still in flight), as the median (and range) of --reps repetitions
after --warmup, the variants alternating inside every repetition, every yardstick in the same run:

  compare_ms        compare_device into a warm handle (the flag walk, the chunk scan, one synchronisation, the list)
  cluster_ms        cluster on that comparison (hook, flatten, stats, keep, scan, one synchronisation, the rows)
  mask_ms           mask_device with the mask and the masked frame (paint, dilate), then a wait
  raycast_depth_ms  yardstick: tsdf_raycast_depth_device of the volume at the same camera, then a wait
  stream_read_ms    yardstick: a plain streaming read (torch sum) of the two uint16 images

    python tools/bench_frame_diff.py [--size 512] [--frames 25] [--reps 10] [--warmup 2] [--out FILE]
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
    ap.add_argument("--frames", type=int, default=25, help="frames fused before the comparison")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_diff_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import api, synth
    assert torch.cuda.is_available(), "bench_frame_diff needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    p = dict(api.DIFF_DEFAULTS)
    vol = tsdf_amd.TSDFVolume((a.size,) * 3, (3000.0,) * 3)
    for i in range(a.frames):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        vol.integrate(d, W, H, cam)
    depth, cam, disc = synth.moving_disc_frame(a.frames, PERIOD, SEED, disc_depth=900, radius=60)
    frame = torch.from_numpy(depth.view(np.int16).copy()).cuda()
    model = torch.zeros(W * H, dtype=torch.int16, device="cuda")
    mask = torch.zeros(W * H, dtype=torch.uint8, device="cuda")
    masked = torch.zeros(W * H, dtype=torch.int16, device="cuda")
    caster = tsdf_amd.GPURaycaster(W, H)
    fd = tsdf_amd.FrameDiff()
    sync = torch.cuda.synchronize

    def cast():
        caster.render_to_depth_device(vol, cam, model.data_ptr())
        sync()

    def compare():
        fd.compare_device(frame.data_ptr(), model.data_ptr(), W, H, p["tolerance"], p["quadratic"])
        sync()

    def cluster():
        fd.cluster(p["connectivity"], p["depth_step"], p["min_pixels"])
        sync()

    def paint():
        fd.mask_device(p["dilate"], mask.data_ptr(), 0, frame.data_ptr(), masked.data_ptr())
        sync()

    def read():
        s = frame.sum() + model.sum()
        sync()
        return s

    steps = [("raycast_depth_ms", cast), ("compare_ms", compare), ("cluster_ms", cluster), ("mask_ms", paint), ("stream_read_ms", read)]
    times = {name: [] for name, _ in steps}
    sync()
    for rep in range(a.warmup + a.reps):
        for name, fn in steps:   # (in this order: a cluster needs its compare, a mask its cluster)
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= a.warmup:
                times[name].append(dt)
    i = fd.info
    out = {"tool": "bench_frame_diff", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "size": a.size, "reps": a.reps,
           "params": p, "device": torch.cuda.get_device_name(0), "counts": [int(c) for c in i.counts], "n_blobs": int(i.n_blobs),
           "n_kept_blobs": int(i.n_kept_blobs), "masked_pixels": int(mask.sum().item()), "disc_pixels": int(disc.sum()),
           "scratch_bytes": fd.scratch_bytes}
    for name, v in times.items():
        out[name] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
