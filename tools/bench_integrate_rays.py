"""Cost of ray integration (include/tsdf_amd.h, "ray integration") on bench.py's scene: 512^3, 640 x 480, seed 0x5EED0003.  Prints one
JSON line and writes it to profiles/integrate_rays_bench.json.

The volume holds --frames fused frames.  The next frame's 307 200 depth pixels become points (tsdf_depth_to_points_device, moved into
the world frame by the camera's pose) and are fused as rays from the camera centre, the single origin:

  rays_ms            tsdf_integrate_rays_device of those rays (scatter + apply + the counter's reset), event-bracketed on the volume's stream
  band_only_ms       the same with TSDF_RAYS_BAND_ONLY
  shuffled_ms        the same rays in a random order
  integrate_ms       the yardstick: tsdf_integrate_device of the same depth frame, in the same run
  visits_per_ray     cells a ray walks (rules 4 - 5 evaluated in float64 on the device: an estimate, ties and roundings aside), over the rays
                     that are not skipped; atomics_per_s = their sum / the scatter kernel's time when --scatter-us gives it (the two
                     kernels are timed apart by a kernel trace of this tool, not by the tool)

Medians of --reps calls, the four variants alternating.  Every call adds an observation to the volume, as a stream of frames does.

--colour: the volume is colour-enabled (the frames before the measurement are fused with their colour frames), every point carries the
colour of its pixel in synth.colour_frame, and two variants join the alternation (default output profiles/integrate_rays_colour_bench.json):

  colour_rays_ms       tsdf_integrate_rays_colour_device of the same rays with those colours, beside rays_ms, the plain call of the same run
  integrate_colour_ms  the second yardstick: tsdf_integrate_colour_device of the same depth and colour frame

    python tools/bench_integrate_rays.py [--colour] [--size 512] [--frames 24] [--reps 30] [--warmup 5] [--scatter-us rays,band,shuffled]
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
    ap.add_argument("--frames", type=int, default=24, help="frames fused before the measurement")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scatter-us", default="", help="rays_scatter_kernel's time per variant from a kernel trace: rays,band_only,shuffled")
    ap.add_argument("--colour", action="store_true", help="a colour-enabled volume; adds the coloured call and the depth colour integrate")
    ap.add_argument("--out", default=None, help="default: profiles/integrate_rays_bench.json, with --colour profiles/integrate_rays_colour_bench.json")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "integrate_rays_colour_bench.json" if a.colour else "integrate_rays_bench.json")

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_integrate_rays needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = a.size
    vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    vol.set_stream(stream.cuda_stream)
    if a.colour:
        vol.enable_colour(True)
    for i in range(a.frames):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        if a.colour:
            vol.integrate_colour(d, synth.colour_frame(i, PERIOD, seed=SEED)[0], W, H, cam)
        else:
            vol.integrate(d, W, H, cam)
    vol.synchronize()
    depth, cam = synth.depth_frame(a.frames, PERIOD, seed=SEED)
    depth_dev = torch.from_numpy(depth.view(np.int16).copy()).to(dev)
    cam_points = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
    with torch.cuda.stream(stream):
        tsdf_amd.depth_to_points_device(W, H, depth_dev.data_ptr(), cam.kinv(), 1, 20000.0, cam_points.data_ptr(), stream.cuda_stream)
        pose = torch.from_numpy(cam.pose().astype(np.float32).reshape(4, 4).T.copy()).to(dev)
        points = (cam_points @ pose[:3, :3].T + pose[:3, 3]).contiguous()
        origin = pose[:3, 3].contiguous()
        shuffled = points[torch.randperm(W * H, device=dev, generator=torch.Generator(device=dev).manual_seed(1))].contiguous()
        if a.colour:
            # point i is pixel i (tsdf_depth_to_points_device with stride 1 keeps the image's order): its colour is that pixel's
            rgb_dev = torch.from_numpy(np.ascontiguousarray(synth.colour_frame(a.frames, PERIOD, seed=SEED)[0], dtype=np.uint8)).to(dev)
    stream.synchronize()

    info = vol.info()
    trunc = float(info.truncation_distance)

    def visits(band):
        """rules 1 - 5 in float64: cells between the clipped ends, per ray that is not skipped"""
        o, p = origin.double(), points.double()
        dvec = p - o
        r = dvec.norm(dim=1)
        ok = torch.isfinite(r) & (r > 0)
        u = dvec / r[:, None]
        vs = torch.tensor(list(info.voxel_size), dtype=torch.float64, device=dev)
        off = torch.tensor(list(info.offset), dtype=torch.float64, device=dev)
        size = torch.tensor([float(s) for s in info.size], dtype=torch.float64, device=dev)
        aa, s = (o - off) / vs, u / vs
        ta, tb = (0.0 - aa) / s, (size - aa) / s
        t0 = torch.maximum(torch.clamp(r - trunc, min=0.0) if band else torch.zeros_like(r), torch.minimum(ta, tb).max(dim=1).values)
        t1 = torch.minimum(r + trunc, torch.maximum(ta, tb).min(dim=1).values)
        ok &= t0 < t1
        c0 = torch.floor(aa + t0[:, None] * s).clamp(min=0)
        c1 = torch.floor(aa + t1[:, None] * s)
        c1 = torch.minimum(c1.clamp(min=0), size - 1)
        per_ray = 1 + (c1 - c0).abs().sum(dim=1)
        return int(ok.sum().item()), float(per_ray[ok].sum().item())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    variants = {
        "rays": lambda: vol.integrate_rays_device(W * H, origin.data_ptr(), 1, points.data_ptr()),
        "band_only": lambda: vol.integrate_rays_device(W * H, origin.data_ptr(), 1, points.data_ptr(), band_only=True),
        "shuffled": lambda: vol.integrate_rays_device(W * H, origin.data_ptr(), 1, shuffled.data_ptr()),
        "integrate": lambda: vol.integrate_device(depth_dev.data_ptr(), W, H, cam),
    }
    if a.colour:
        variants["colour_rays"] = lambda: vol.integrate_rays_device(W * H, origin.data_ptr(), 1, points.data_ptr(), rgb=rgb_dev.data_ptr())
        variants["integrate_colour"] = lambda: vol.integrate_colour_device(depth_dev.data_ptr(), rgb_dev.data_ptr(), W, H, cam)
    times = {k: [] for k in variants}
    for rep in range(a.warmup + a.reps):
        for k, fn in variants.items():
            t = timed(fn)
            if rep >= a.warmup:
                times[k].append(t)

    out = {"tool": "bench_integrate_rays", "size": n, "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames,
           "reps": a.reps, "rays": W * H, "weight_storage_bits": vol.weight_storage()[0], "device": torch.cuda.get_device_name(0),
           "truncation_mm": round(trunc, 3), "scratch_bytes": vol.ray_scratch_bytes(), "colour": bool(a.colour)}
    for k, ts in times.items():
        out[k + "_ms"] = round(float(np.median(ts)), 4)
        out[k + "_ms_range"] = [round(min(ts), 4), round(max(ts), 4)]
    for k in ("rays", "band_only", "shuffled"):
        out[k + "_over_integrate"] = round(out[k + "_ms"] / out["integrate_ms"], 3)
    if a.colour:
        out["colour_rays_over_rays"] = round(out["colour_rays_ms"] / out["rays_ms"], 3)
        out["colour_rays_over_integrate_colour"] = round(out["colour_rays_ms"] / out["integrate_colour_ms"], 3)
        # per repetition the coloured call over the plain call next to it: the observed range of k in "coloured = plain x k"
        ks = [c / p for c, p in zip(times["colour_rays"], times["rays"])]
        out["colour_rays_over_rays_range"] = [round(min(ks), 3), round(max(ks), 3)]
    live, total = visits(False)
    live_b, total_b = visits(True)
    out["rays_not_skipped"] = live
    out["visits_per_ray"] = round(total / max(live, 1), 2)
    out["band_only_visits_per_ray"] = round(total_b / max(live_b, 1), 2)
    if a.scatter_us:
        us = [float(x) for x in a.scatter_us.split(",")]
        out["scatter_us_from_kernel_trace"] = dict(zip(("rays", "band_only", "shuffled"), us))
        out["atomics_per_s"] = {"rays": round(total / (us[0] * 1e-6), -6), "band_only": round(total_b / (us[1] * 1e-6), -6),
                                "shuffled": round(total / (us[2] * 1e-6), -6)}
    out["note"] = ("medians of event-bracketed asynchronous calls on one stream, the variants alternating; the first ray call's "
                   "allocation and zeroing of the scratch is in the warm-up; visits are an estimate in float64 (an upper bound of the "
                   "atomics: a visited voxel more than trunc behind the point adds nothing)")
    vol.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
