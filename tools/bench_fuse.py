"""Time of volume fusion (include/tsdf_amd.h, "volume fusion") on bench.py's scene, seed 0x5EED0003.  Prints one JSON line and writes it
to profiles/fuse_bench.json.

For every --sizes entry n, an n^3 source is fused into a cleared n^3 destination of the same box through a 20 degree rotation about
the box's centre, 8-bit counts on both sides:
  shell   the source as --frames frames of the bench stream leave it: weights > 0 in a shell around the surfaces, most destination
          bricks culled;
  full    the same distances with every weight set to 1: nothing is cullable, every voxel whose point lies in the source is blended.
Beside them, the route a caller had before: tsdf_volume_sample_field_device (distance + weight) at the destination's n^3 voxel centres,
already in HBM -- without the blend pass that route still needs.

Each figure is the median of --reps event-bracketed calls after --warmup; the destination is cleared outside the bracket before
every call, so every call does the same work in the same storage.  A fuse is three launches (source summary, cull, main kernel) and
two small memsets; the bracket holds them all.

  *_ms                  median device time of one call
  *_mvox_per_s          million destination voxels (n^3) per second
  *_listed_bricks       64 x 4 x 32-voxel destination bricks the cull kept, of *_total_bricks
  *_fused_voxels        voxels updated

    python tools/bench_fuse.py [--sizes 256 512] [--frames 25] [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rotation_about(centre, axis, degrees):
    """4 x 4 rigid transform, 16 float32 column-major: a rotation about `axis` through `centre`."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    c = np.asarray(centre, np.float64)
    M[:3, 3] = c - M[:3, :3] @ c
    return M.T.astype(np.float32).reshape(-1).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--frames", type=int, default=25, help="frames fused into the source")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--degrees", type=float, default=20.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_fuse needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    frames = [synth.depth_frame(i, PERIOD, seed=SEED) for i in range(a.frames)]
    m = rotation_about((1500.0,) * 3, (1.0, 2.0, 3.0), a.degrees)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    out = {"tool": "bench_fuse", "seed": "0x%X" % SEED, "frames_fused": a.frames, "degrees": a.degrees, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    mp = m.ctypes.data_as(tsdf_amd._capi.C.POINTER(tsdf_amd._capi.C.c_float))
    for n in a.sizes:
        src = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        dst = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        for v in (src, dst):
            v.set_stream(stream.cuda_stream)
        for d, cam in frames:
            src.integrate(d, W, H, cam)
        src.synchronize()
        res = {"voxels": n ** 3}

        def fuse_async():
            tsdf_amd._capi.check(tsdf_amd._capi.lib.tsdf_volume_fuse(dst._h, src._h, mp, None))

        def measure(name):
            assert src.weight_storage()[0] == 8
            ts = []
            for r in range(a.warmup + a.reps):
                dst.clear()
                assert dst.weight_storage()[0] == 8
                t = timed(fuse_async)
                if r >= a.warmup:
                    ts.append(t)
            dst.clear()
            res[name + "_fused_voxels"] = dst.fuse(src, m)
            res[name + "_listed_bricks"], res[name + "_total_bricks"] = dst.last_fuse_bricks()
            ms = float(np.median(ts))
            res[name + "_ms"] = round(ms, 4)
            res[name + "_ms_range"] = [round(min(ts), 4), round(max(ts), 4)]
            res[name + "_mvox_per_s"] = round(n ** 3 / ms / 1e3, 1)

        measure("shell")
        src.set_weight_data(np.ones(n ** 3, np.float32))
        measure("full")

        # the field-query route: distance + weight at the destination's voxel centres (its offset is 0: centre = (i + 0.5) * voxel size)
        vs = float(dst.voxel_size()[0])
        axis = (torch.arange(n, dtype=torch.float32, device=dev) + 0.5) * vs
        P = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1).flip(-1).reshape(-1, 3).contiguous()   # x fastest
        R = torch.from_numpy(m.reshape(4, 4).T.copy()).to(dev)
        P = (P @ R[:3, :3].T + R[:3, 3]).contiguous()
        D = torch.empty(n ** 3, dtype=torch.float32, device=dev)
        Wt = torch.empty(n ** 3, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ts = []
        for r in range(a.warmup + a.reps):
            t = timed(lambda: src.sample_field_device(n ** 3, P.data_ptr(), D.data_ptr(), None, Wt.data_ptr(), stream=stream.cuda_stream))
            if r >= a.warmup:
                ts.append(t)
        ms = float(np.median(ts))
        res["field_query_ms"] = round(ms, 4)
        res["field_query_ms_range"] = [round(min(ts), 4), round(max(ts), 4)]
        res["field_query_mvox_per_s"] = round(n ** 3 / ms / 1e3, 1)
        res["field_query_valid_points"] = int((~torch.isnan(D)).sum().item())
        out["sizes"][str(n)] = res
        del P, D, Wt
        src.close()
        dst.close()
        torch.cuda.empty_cache()
    out["note"] = ("medians of event-bracketed calls on one stream; a fuse is its three launches and two memsets; the field-query figure "
                   "is the sampling alone (full source, transformed centres already in HBM), without the blend pass that route needs")
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
