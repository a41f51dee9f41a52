"""Cost of class fusion at 256^3 and 512^3, 640 x 480, on bench.py's stream (seed 0x5EED0003): writes profiles/classes_bench.json and
prints it as one JSON line.

Per size and weight storage (8-bit counts: the packed integrate kernel, which makes the colour update itself; fp32: the general path,
where colour is a band pass of its own like the class pass), the device time of one call on a frame already in HBM:

  integrate_ms                  tsdf_integrate_device
  integrate_colour_ms           tsdf_integrate_colour_device
  integrate_classes_ms          tsdf_integrate_classes_device without rgb
  integrate_classes_rgb_ms      tsdf_integrate_classes_device with rgb
  class_counts_ms               tsdf_volume_class_counts_device, 16 classes (the LDS histogram)
  class_counts_global_ms        ... 65535 classes (global atomics)
  raycast_ms / raycast_classes_ms   tsdf_raycast_device / tsdf_raycast_classes_device

Four volumes per storage -- plain, colour, classes, colour + classes -- are fed the same frames, so each holds the same surface.  Every
measured call is bracketed by HIP events on the bench stream around work that was synchronised before; the variants alternate within a
frame and their order rotates from round to round.  Reported: the median over --rounds x --frames calls, and the quartiles beside it.
A 0.1 ms call inside a window of one call measures launch latency with it: the `*_extra_us` figures (a variant minus plain integrate,
medians) are the numbers to read, and the numbers are this machine's at this load.

    python tools/bench_classes.py [--sizes 256 512] [--frames 24] [--warmup 8] [--rounds 4]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(a, torch, tsdf_amd, synth, n, fp32, frames):
    W, H = synth.WIDTH, synth.HEIGHT
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    depth_dev, rgb_dev, class_dev, cams = frames
    vols = {}
    for name, colour, classes in (("plain", False, False), ("colour", True, False), ("classes", False, True), ("both", True, True)):
        v = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        if colour:
            v.enable_colour()
        if classes:
            v.enable_classes()
        if fp32:
            assert v.weight_data()
        v.set_stream(stream.cuda_stream)
        vols[name] = v
    caster = tsdf_amd.GPURaycaster(W, H)
    V = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
    N = torch.empty_like(V)
    K = torch.empty((2, W * H), dtype=torch.int16, device=dev)
    counts = torch.empty(65535, dtype=torch.int64, device=dev)
    lib, check, C = tsdf_amd._capi.lib, tsdf_amd._capi.check, tsdf_amd._capi.C

    def counts_device(n_classes):
        check(lib.tsdf_volume_class_counts_device(vols["classes"]._h, n_classes, 1, C.c_void_p(counts.data_ptr()), C.c_void_p(stream.cuda_stream)))

    calls = {
        "integrate": lambda i: vols["plain"].integrate_device(depth_dev[i].data_ptr(), W, H, cams[i]),
        "integrate_colour": lambda i: vols["colour"].integrate_colour_device(depth_dev[i].data_ptr(), rgb_dev[i].data_ptr(), W, H, cams[i]),
        "integrate_classes": lambda i: vols["classes"].integrate_classes_device(depth_dev[i].data_ptr(), class_dev[i].data_ptr(), W, H, cams[i]),
        "integrate_classes_rgb": lambda i: vols["both"].integrate_classes_device(depth_dev[i].data_ptr(), class_dev[i].data_ptr(), W, H, cams[i],
                                                                                  rgb_ptr=rgb_dev[i].data_ptr()),
        "class_counts": lambda i: counts_device(16),
        "class_counts_global": lambda i: counts_device(65535),
        "raycast": lambda i: caster.raycast_device(vols["plain"], cams[i], V.data_ptr(), N.data_ptr()),
        "raycast_classes": lambda i: caster.raycast_classes_device(vols["classes"], cams[i], V.data_ptr(), N.data_ptr(), K[0].data_ptr(),
                                                                   K[1].data_ptr()),
    }

    def timed(fn, i):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn(i)
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    names = list(calls)
    for i in range(a.warmup):
        for name in names:
            calls[name](i)
    torch.cuda.synchronize()
    t = {name: [] for name in names}
    i = a.warmup
    for r in range(a.rounds):
        order = names[r % len(names):] + names[:r % len(names)]       # rotate which variant goes first
        for _ in range(a.frames):
            for name in order:
                t[name].append(timed(calls[name], i))
            i += 1
    torch.cuda.synchronize()
    words = vols["classes"].get_class_data()
    assert np.array_equal(words, vols["both"].get_class_data()), "class words with and without rgb differ"
    assert np.array_equal(vols["colour"].get_colour_data(), vols["both"].get_colour_data()), "colour words with and without classes differ"
    out = {"size": n, "weight_storage": "fp32" if fp32 else "8-bit counts"}
    for name in names:
        q = np.percentile(t[name], [25, 50, 75])
        out[name + "_ms"] = round(float(q[1]), 4)
        out[name + "_quartiles_ms"] = [round(float(q[0]), 4), round(float(q[2]), 4)]
    base = out["integrate_ms"]
    for name in ("integrate_colour", "integrate_classes", "integrate_classes_rgb"):
        out[name + "_extra_us"] = round(1000.0 * (out[name + "_ms"] - base), 1)
    out["raycast_classes_extra_us"] = round(1000.0 * (out["raycast_classes_ms"] - out["raycast_ms"]), 1)
    out["classified_voxels"] = int((words != 0).sum())
    out["votes_per_frame"] = round(float((words >> np.uint32(16)).astype(np.int64).sum()) / float(i), 1)
    for v in vols.values():
        v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--frames", type=int, default=24, help="timed frames per round")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classes_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_classes needs a GPU"
    SEED, PERIOD = 0x5EED0003, 200
    dev = torch.device("cuda:0")
    depth_dev, rgb_dev, class_dev, cams = [], [], [], []
    for i in range(a.warmup + a.rounds * a.frames):
        d, cam = synth.depth_frame(i % PERIOD, PERIOD, seed=SEED)
        rgb, _ = synth.colour_frame(i % PERIOD, PERIOD, seed=SEED)
        k, _ = synth.class_frame(i % PERIOD, PERIOD, seed=SEED)
        depth_dev.append(torch.from_numpy(d.astype(np.int16)).to(dev))
        rgb_dev.append(torch.from_numpy(rgb.reshape(-1)).to(dev))
        class_dev.append(torch.from_numpy(k.astype(np.int16)).to(dev))
        cams.append(cam)
    frames = (depth_dev, rgb_dev, class_dev, cams)
    runs = [measure(a, torch, tsdf_amd, synth, n, fp32, frames) for n in a.sizes for fp32 in (False, True)]
    out = {
        "tool": "bench_classes", "width": synth.WIDTH, "height": synth.HEIGHT, "seed": "0x%X" % SEED, "rounds": a.rounds,
        "frames_per_round": a.frames, "warmup": a.warmup, "runs": runs,
        "note": "medians (and quartiles) of event-bracketed synchronised calls, variants alternating within a frame; *_extra_us = the "
                "variant's median minus plain integrate's (or the plain ray cast's)",
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
