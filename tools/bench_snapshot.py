"""Cost of sparse snapshots (include/tsdf_amd.h, "sparse snapshot") on bench.py's scene (640 x 480, seed 0x5EED0003), 24 colour frames
fused into 8-bit weights, at 256^3 and 512^3.  Prints one JSON line and writes it to profiles/snapshot_bench.json.

Per size: the live share of voxels and of bricks, the bytes of the compact arrays, and host wall-clock times of whole calls, each ending
in a device synchronise, as the median (and range) of --reps repetitions after --warmup, the variants alternating inside every repetition:

  snapshot_ms            snapshot() into a warm handle, until the device arrays are complete
  restore_ms             restore() from that handle, until the volume is written
  snapshot_download_ms   snapshot() plus the download of the four arrays
  dense_get_ms           what a user does without it: get_distance_data + get_weight_data + get_colour_data
  dense_set_ms           ... and the three set_*_data back

and dense_read_once_ms: the time to read the dense arrays (9 bytes a voxel here) once at the copy bandwidth tsdf_measure_copy_bandwidth
measures in the same run -- the floor of any pass over the volume.  At the first size the lengths of the .tsdfs file save_sparse writes and
of the .tsdf file save_to_file would write (68 + 35 bytes a voxel: the format fixes it) are recorded too.  The restored state is compared
with the state before, bit for bit, so that the columns are the same product.  Nothing about the speed was known when the feature was
specified, and no pass mark is fixed.

    python tools/bench_snapshot.py [--sizes 256 512] [--frames 24] [--reps 10] [--warmup 2] [--dense-reps 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--frames", type=int, default=24, help="frames fused before the measurements")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dense-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import _capi, synth
    assert torch.cuda.is_available(), "bench_snapshot needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    frames = [synth.depth_frame(i, PERIOD, seed=SEED) + (synth.colour_frame(i, PERIOD, seed=SEED)[0],) for i in range(a.frames)]
    out = {"tool": "bench_snapshot", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "reps": a.reps,
           "dense_reps": a.dense_reps, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in a.sizes:
        vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        vol.enable_colour()
        for d, cam, rgb in frames:
            vol.integrate_colour(d, rgb, W, H, cam)
        vol.synchronize()
        assert vol.weight_storage() == (8, False)
        D, Wt, Cl = vol.get_distance_data(), vol.get_weight_data(), vol.get_colour_data()
        fill = np.float32(vol.truncation_distance())
        live = (D.view(np.uint32) != fill.reshape(1).view(np.uint32)[0]) | (Wt != 0) | (Cl != 0)
        nb = (n + 7) // 8
        live_bricks = int(np.pad(live.reshape(n, n, n), [(0, 8 * nb - n)] * 3).reshape(nb, 8, nb, 8, nb, 8).any(axis=(1, 3, 5)).sum())
        warm = vol.snapshot()
        assert warm.n_bricks == live_bricks, "the device and the host disagree about the live bricks"
        kept = {}

        def snapshot():
            vol.snapshot(into=warm).device_buffers()          # (waits for the kernels)

        def restore():
            vol.restore(warm)
            vol.synchronize()

        def snapshot_download():
            kept["arrays"] = vol.snapshot(into=warm).download()

        def dense_get():
            kept["dense"] = (vol.get_distance_data(), vol.get_weight_data(), vol.get_colour_data())

        def dense_set():
            vol.set_distance_data(D)
            vol.set_weight_data(Wt)
            vol.set_colour_data(Cl)

        variants = {"snapshot": snapshot, "restore": restore, "snapshot_download": snapshot_download}
        dense = {"dense_get": dense_get, "dense_set": dense_set}
        times = {v: [] for v in list(variants) + list(dense)}
        for r in range(a.warmup + a.reps):
            for v, fn in variants.items():
                vol.synchronize()
                t0 = time.perf_counter()
                fn()
                t = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    times[v].append(t)
        for r in range(a.dense_reps):
            for v, fn in dense.items():
                vol.synchronize()
                t0 = time.perf_counter()
                fn()
                times[v].append((time.perf_counter() - t0) * 1e3)
        # the same product: the volume after all the restores and uploads is the one that was fused
        d2, w2, c2 = vol.get_distance_data(), vol.get_weight_data(), vol.get_colour_data()
        assert d2.tobytes() == D.tobytes() and w2.tobytes() == Wt.tobytes() and c2.tobytes() == Cl.tobytes(), "the restored state differs"
        assert vol.weight_storage() == (8, False)
        gbps = C.c_double()
        _capi.check(_capi.lib.tsdf_measure_copy_bandwidth(256 << 20, 10, None, C.byref(gbps)))
        dense_bytes = 9 * n ** 3
        i = warm.info
        res = {"voxels": n ** 3, "live_voxel_share": round(float(live.mean()), 4), "bricks": nb ** 3, "live_bricks": live_bricks,
               "live_brick_share": round(live_bricks / float(nb ** 3), 4), "bytes": int(i.bytes), "dense_bytes": dense_bytes,
               "scratch_bytes": warm.scratch_bytes, "copy_bandwidth_gb_per_s": round(gbps.value, 1),
               "dense_read_once_ms": round(dense_bytes / (gbps.value * 1e9) * 1e3, 4)}
        for v, ts in times.items():
            res[v + "_ms"] = round(float(np.median(ts)), 3)
            res[v + "_ms_range"] = [round(min(ts), 3), round(max(ts), 3)]
        if n == a.sizes[0]:
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "volume.tsdfs")
                vol.save_sparse(path)
                res["save_sparse_bytes"] = os.path.getsize(path)
            res["save_to_file_bytes"] = 68 + 35 * n ** 3
        out["sizes"][str(n)] = res
        warm.close()
        vol.close()
    out["note"] = ("host wall-clock of whole calls that end in a device synchronise, medians with [min, max], the snapshot variants alternating "
                   "inside every repetition; dense_get_ms / dense_set_ms are the user's path without the feature (three blocking downloads / "
                   "uploads of the dense arrays), timed in the same run; dense_read_once_ms is the dense arrays' 9 bytes a voxel at the copy "
                   "bandwidth measured in the same run; save_to_file_bytes follows from the .tsdf format; no pass mark was fixed")
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
