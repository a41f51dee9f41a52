"""Rate of the ray queries (include/tsdf_amd.h, "ray queries") on bench.py's scene: 512^3, 640 x 480, seed 0x5EED0003.  Prints one JSON
line and writes it to profiles/ray_query_bench.json.

Four ray sets, all already in HBM, each cast with tsdf_volume_cast_rays_device (points + t):
  pixel_order      the 640 x 480 pixel rays of the bench view in pixel order: neighbours in the array are neighbours in space, but a wave
                   is 64 pixels of one row, not the image cast's 8 x 8 tile
  pixel_shuffled   the same rays in a random order: what incoherence costs (idle lanes behind the wave's longest ray, scattered taps)
  random_inside    307 200 random unit directions from origins inside the box
  pixel_normals    pixel_order with the normals fused into the launch; beside it pixel_points_then_field: the same launch without
                   normals followed by tsdf_volume_sample_field_device (unit gradient) at its points on the same stream
With --repeat R (R >= 2; off by default, and not in the recorded profile) the first comparison is made again at R times the rays --
8 gives 2 457 600 rays, 9 600 workgroups: several times what the chip holds at once, where the 1 200 workgroups of one image are
all resident together and a launch is as long as its longest wave however the rays are arranged: pixel_order_xR is the pixel rays
R times over, copy after copy, pixel_shuffled_xR the same rays in one random order.
Beside them, from the same run: the device time of tsdf_raycast_device for the same view (the yardstick: the image cast's
cell-parallel or march kernels, which know the rays are a pinhole image) and tsdf_raycast_evaluated_samples for that view.
Every figure is the median of --reps event-bracketed calls after --warmup, the variants alternating inside every repetition.

    python tools/bench_rays.py [--size 512] [--frames 24] [--reps 30] [--warmup 5] [--repeat R]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pixel_rays(cam, width, height):
    """compute_ray_direction_at_pixel (src/RayCaster/GPURaycaster.cu:24-44) for every pixel, in fp32 and in its order of operations."""
    F = np.float32
    pose = np.asarray(cam.pose(), F).reshape(-1)
    ki = np.asarray(cam.kinv(), F).reshape(-1)
    ys, xs = np.mgrid[0:height, 0:width]
    x, y = xs.reshape(-1).astype(F), ys.reshape(-1).astype(F)
    rc = [(x * ki[r] + y * ki[3 + r]) + ki[6 + r] for r in range(3)]
    d = np.stack([(pose[r] * rc[0] + pose[4 + r] * rc[1]) + pose[8 + r] * rc[2] for r in range(3)], axis=1).astype(F)
    o = np.tile(pose[12:15], (width * height, 1)).astype(F)
    return o, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=24, help="frames fused before the queries")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=0, help="R >= 2: also cast R copies of the pixel rays, ordered and shuffled")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import _capi, api, synth
    assert torch.cuda.is_available(), "bench_rays needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = a.size
    vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    vol.set_stream(stream.cuda_stream)
    cam = None
    for i in range(a.frames):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        vol.integrate(d, W, H, cam)
    caster = tsdf_amd.GPURaycaster(W, H)
    m = W * H
    rng = np.random.RandomState(0x0BE7C4)
    o_pix, d_pix = pixel_rays(cam, W, H)
    perm = rng.permutation(m)
    info = vol.info()
    lo, size = np.array(info.offset, np.float32), np.array(info.physical_size, np.float32)
    d_rand = rng.normal(size=(m, 3))
    d_rand = (d_rand / np.linalg.norm(d_rand, axis=1)[:, None]).astype(np.float32)
    o_rand = (lo + rng.uniform(0.02, 0.98, (m, 3)) * size).astype(np.float32)
    to_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rays = {"pixel_order": (to_dev(o_pix), to_dev(d_pix)), "pixel_shuffled": (to_dev(o_pix[perm]), to_dev(d_pix[perm])),
            "random_inside": (to_dev(o_rand), to_dev(d_rand))}
    R = max(1, a.repeat)
    big = "_x%d" % R
    if R >= 2:
        big_o, big_d = np.tile(o_pix, (R, 1)), np.tile(d_pix, (R, 1))
        big_perm = rng.permutation(m * R)
        rays["pixel_order" + big] = (to_dev(big_o), to_dev(big_d))
        rays["pixel_shuffled" + big] = (to_dev(big_o[big_perm]), to_dev(big_d[big_perm]))
    P = torch.empty((m * R, 3), dtype=torch.float32, device=dev)
    T = torch.empty(m * R, dtype=torch.float32, device=dev)
    N = torch.empty((m, 3), dtype=torch.float32, device=dev)
    V = torch.empty((m, 3), dtype=torch.float32, device=dev)

    def cast(name, normals=False):
        o, d = rays[name]
        vol.cast_rays_device(int(o.shape[0]), o.data_ptr(), d.data_ptr(), None, P.data_ptr(), T.data_ptr(), N.data_ptr() if normals else None)

    def points_then_field():
        cast("pixel_order")
        vol.sample_field_device(m, P.data_ptr(), None, N.data_ptr(), None, unit_gradient=True, stream=stream.cuda_stream)

    variants = {"pixel_order": lambda: cast("pixel_order"), "pixel_shuffled": lambda: cast("pixel_shuffled"),
                "random_inside": lambda: cast("random_inside"), "pixel_normals": lambda: cast("pixel_order", True),
                "pixel_points_then_field": points_then_field,
                "image_cast": lambda: caster.raycast_device(vol, cam, V.data_ptr())}
    if R >= 2:
        variants["pixel_order" + big] = lambda: cast("pixel_order" + big)
        variants["pixel_shuffled" + big] = lambda: cast("pixel_shuffled" + big)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    times = {v: [] for v in variants}
    for r in range(a.warmup + a.reps):
        for v, fn in variants.items():
            t = timed(fn)
            if r >= a.warmup:
                times[v].append(t)
    torch.cuda.synchronize()

    out = {"tool": "bench_rays", "size": n, "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "reps": a.reps,
           "rays": m, "device": torch.cuda.get_device_name(0), "image_cast_cell_parallel": vol.last_raycast_cell_parallel()}
    # the pixel rays cast as rays of their own give the image cast's vertex map, and the hit counts of the sets
    caster.raycast_device(vol, cam, V.data_ptr())
    cast("pixel_order")
    torch.cuda.synchronize()
    same = (P[:m].view(torch.int32) == V.view(torch.int32)) | (torch.isnan(P[:m]) & torch.isnan(V))
    out["pixel_rays_equal_image_cast"] = bool(same.all().item())
    for name in rays:
        cast(name)
        torch.cuda.synchronize()
        out[name + "_hits"] = int((~torch.isnan(T[:int(rays[name][0].shape[0])])).sum().item())
    for v, ts in times.items():
        ms = float(np.median(ts))
        out[v + "_ms"] = round(ms, 4)
        out[v + "_ms_range"] = [round(min(ts), 4), round(max(ts), 4)]
        out[v + "_mrays_per_s"] = round((m * R if (R >= 2 and v.endswith(big)) else m) / ms / 1e3, 1)
    if R >= 2:
        out["repeat"] = R
    pose, _, _, kinv = api._camera_matrices(cam)
    e = C.c_uint64()
    _capi.check(_capi.lib.tsdf_raycast_evaluated_samples(vol._h, W, H, api._fp(pose), api._fp(kinv), C.byref(e), None))
    out["image_cast_evaluated_samples"] = int(e.value)
    out["note"] = ("medians of event-bracketed calls on one stream, variants alternating; image_cast is tsdf_raycast_device of the same "
                   "view (vertices only) and is not a bound for incoherent rays; pixel_points_then_field is two launches")
    vol.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
