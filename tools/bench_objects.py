"""Time of the class objects (include/tsdf_amd.h, "class objects") on bench.py's scene (640 x 480, seed 0x5EED0003), 25 frames fused
with their class frames at 512^3.  Prints one JSON line and writes it to profiles/objects_bench.json.

Host wall-clock times of whole calls, each ending in a device synchronise, as the median (and range) of --reps repetitions after
--warmup, the variants alternating inside every repetition, every yardstick in the same run on the same volume:

  find_objects26_ms / find_objects6_ms   find_objects(min_votes 1, every class, min_size 1) into a warm handle: flag kernel, chunk scan,
                                          the count's synchronise, list, hook, flatten, stats, keep, scan, the table's synchronise, rows
  find_objects_selected_ms               the same at connectivity 26 with a selection of one class
  lookup_ms                              lookup_device on the vertices of a 640 x 480 ray cast (an instance-segmentation image)
  class_counts_ms                        yardstick: tsdf_volume_class_counts_device, 16 classes -- it streams the same 4 bytes a voxel once
  frontiers26_ms / frontiers6_ms         yardstick: find_frontiers + cluster(connectivity, 1) into a warm explorer
  sample_classes_ms                      yardstick: tsdf_volume_sample_classes_device on the same vertices

    python tools/bench_objects.py [--size 512] [--frames 25] [--reps 10] [--warmup 2] [--once]

--once: one call of each and nothing else (for a kernel trace: objects_flag_kernel against class_counts_kernel).
"""
import argparse
import ctypes as C
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
    ap.add_argument("--frames", type=int, default=25, help="frames fused before the queries")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import _capi, synth
    assert torch.cuda.is_available(), "bench_objects needs a GPU"
    lib, check = _capi.lib, _capi.check
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    n = a.size
    vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    vol.enable_classes()
    cam = None
    for i in range(a.frames):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        k, _ = synth.class_frame(i, PERIOD, seed=SEED)
        vol.integrate_classes(d, k, W, H, cam)
    vol.synchronize()
    ob, ex = tsdf_amd.Objects(), tsdf_amd.Explorer()
    vertices = torch.from_numpy(np.ascontiguousarray(vol.raycast(W, H, cam)[0], dtype=np.float32)).cuda()
    n_points = W * H
    rows = torch.zeros(n_points, dtype=torch.int32, device="cuda")
    sampled = torch.zeros(n_points, dtype=torch.int32, device="cuda")      # classes, then votes (uint16 each)
    counts = torch.zeros(16, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(vol.stream_ptr() or 0)

    def find(connectivity, classes=None):
        def run():
            vol.find_objects(1, classes, connectivity, 1, into=ob)
            ob.device_buffers()                                # (waits for the rows kernel)
        return run

    def lookup():
        ob.lookup_device(n_points, vertices.data_ptr(), rows.data_ptr(), stream.value or 0)
        vol.synchronize()

    def class_counts():
        check(lib.tsdf_volume_class_counts_device(vol._h, 16, 1, C.c_void_p(counts.data_ptr()), stream))
        vol.synchronize()

    def frontiers(connectivity):
        def run():
            vol.find_frontiers(into=ex).cluster(connectivity, 1)
            ex.device_buffers()
        return run

    def sample():
        vol.sample_classes_device(n_points, vertices.data_ptr(), sampled.data_ptr(), sampled.data_ptr() + 2 * n_points)
        vol.synchronize()

    variants = {"find_objects26": find(26), "class_counts": class_counts, "frontiers26": frontiers(26), "find_objects6": find(6),
                "frontiers6": frontiers(6), "find_objects_selected": find(26, [1]), "sample_classes": sample}
    if a.once:
        for fn in variants.values():
            fn()
        find(26)()
        lookup()
        vol.synchronize()
        return
    times = {v: [] for v in list(variants) + ["lookup"]}
    info = {}
    for r in range(a.warmup + a.reps):
        for v, fn in variants.items():
            vol.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                times[v].append(t)
            if v.startswith("find_objects"):
                i = ob.info
                info[v] = {"n_labelled": int(i.n_labelled), "n_objects": int(i.n_objects)}
            if v == "find_objects26":                          # the lookup reads the table of every class at connectivity 26
                vol.synchronize()
                t0 = time.perf_counter()
                lookup()
                t = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    times["lookup"].append(t)
                info["lookup_points_in_an_object"] = int((rows != -1).sum().item())
    e = ex.info
    out = {"tool": "bench_objects", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "size": n, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "voxels": n ** 3, "lookup_points": n_points, "objects": info,
           "n_frontiers": int(e.n_frontiers), "n_frontier_clusters_6": int(e.n_clusters), "class_counts": [int(c) for c in counts.tolist()],
           "objects_scratch_bytes": ob.scratch_bytes, "explorer_scratch_bytes": ex.scratch_bytes}
    for v, ts in times.items():
        out[v + "_ms"] = round(float(np.median(ts)), 3)
        out[v + "_ms_range"] = [round(min(ts), 3), round(max(ts), 3)]
    out["note"] = ("host wall-clock of whole calls that end in a device synchronise, medians with [min, max], variants alternating inside "
                   "every repetition, all in one run on one volume with a warm handle; class_counts_ms, frontiers*_ms and sample_classes_ms "
                   "are yardsticks, not the code under test; nothing about the speed was known when the feature was specified")
    ob.close()
    ex.close()
    vol.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
