"""Time of the distance field (include/tsdf_amd.h, "distance field") on bench.py's scene (640 x 480, seed 0x5EED0003), 24 frames fused,
at 256^3 and 512^3, with caps of 100 mm, 500 mm and none.  Prints one JSON line and writes it to profiles/esdf_bench.json.

Per size, host wall-clock times of whole calls, each ending in a device synchronise, as the median (and range) of --reps repetitions
after --warmup, the variants alternating inside every repetition:

  esdf_cap100_ms / esdf_cap500_ms / esdf_inf_ms   compute_esdf(cap) into a warm handle, until the device array is complete
  esdf_inf_host_ms                                the same plus the download of the array
  host_edt_ms                                     what a user does without it: get_distance_data + get_weight_data + the site mask +
                                                  scipy.ndimage.distance_transform_edt(sampling = voxel size), the sign and the NaNs
                                                  (--host-reps repetitions: it takes seconds at 512^3)

The host transform is the yardstick, not the code under test; its result is compared with the device's (largest relative difference,
printed) so that the two columns are the same product.

    python tools/bench_esdf.py [--sizes 256 512] [--frames 24] [--reps 10] [--warmup 2] [--host-reps 3] [--once]

--once: one computation per size and cap and nothing else (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def site_mask(D, Wt, n):
    """tests/esdf_ref.py::sites, restated here so that the tool stands alone."""
    with np.errstate(invalid="ignore"):
        obs, neg = (Wt > 0).reshape(n, n, n), (D < 0).reshape(n, n, n)
    site = np.zeros((n, n, n), bool)
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = obs[lo] & obs[hi] & (neg[lo] != neg[hi])
        site[lo] |= cross
        site[hi] |= cross
    return site, obs.reshape(-1), neg.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--frames", type=int, default=24, help="frames fused before the computations")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esdf_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_esdf needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    caps = {"cap100": 100.0, "cap500": 500.0, "inf": float("inf")}
    out = {"tool": "bench_esdf", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "reps": a.reps,
           "host_reps": a.host_reps, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in a.sizes:
        vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        for i in range(a.frames):
            d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
            vol.integrate(d, W, H, cam)
        vol.synchronize()
        warm = tsdf_amd.ESDF()
        if a.once:
            for cap in caps.values():
                vol.compute_esdf(cap, into=warm).device_buffer()
            warm.close()
            vol.close()
            continue
        vs = [float(v) for v in vol.voxel_size()]
        kept = {}

        def device(cap):
            def run():
                vol.compute_esdf(cap, into=warm).device_buffer()      # (waits for the kernels)
            return run

        def device_host():
            kept["device"] = vol.compute_esdf(into=warm).distances

        def host_edt():
            from scipy import ndimage
            D, Wt = vol.get_distance_data(), vol.get_weight_data()
            site, obs, neg = site_mask(D, Wt, n)
            e = ndimage.distance_transform_edt(~site, sampling=(vs[2], vs[1], vs[0])).reshape(-1).astype(np.float32)
            kept["host"] = np.where(obs, np.where(neg, -e, e), np.float32(np.nan))
            kept["sites"] = int(site.sum())

        variants = {"esdf_" + k: device(c) for k, c in caps.items()}
        variants["esdf_inf_host"] = device_host
        times = {v: [] for v in variants}
        for r in range(a.warmup + a.reps):
            for v, fn in variants.items():
                vol.synchronize()
                t0 = time.perf_counter()
                fn()
                t = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    times[v].append(t)
        times["host_edt"] = []
        for r in range(a.host_reps):
            t0 = time.perf_counter()
            host_edt()
            times["host_edt"].append((time.perf_counter() - t0) * 1e3)
        g, h = kept["device"], kept["host"]
        assert warm.n_sites == kept["sites"] > 0, "the device and the host disagree about the sites"
        assert np.array_equal(np.isnan(g), np.isnan(h)) and np.array_equal(np.signbit(g), np.signbit(h))
        ok = ~np.isnan(g) & (h != 0)
        rel = float(np.max(np.abs(g[ok].astype(np.float64) - h[ok]) / np.abs(h[ok])))
        assert rel <= 1e-6 and bool((g[~np.isnan(g) & (h == 0)] == 0).all()), "the device field is not the host transform's (%g)" % rel
        res = {"sites": kept["sites"], "observed_voxels": int((~np.isnan(g)).sum()), "largest_distance_mm": float(np.nanmax(np.abs(g))),
               "largest_relative_difference_from_scipy": rel, "scratch_bytes": warm.scratch_bytes,
               "scratch_bytes_per_voxel": round(warm.scratch_bytes / float(n) ** 3, 4)}
        for v, ts in times.items():
            res[v + "_ms"] = round(float(np.median(ts)), 3)
            res[v + "_ms_range"] = [round(min(ts), 3), round(max(ts), 3)]
        res["host_edt_over_esdf_inf_host"] = round(res["host_edt_ms"] / res["esdf_inf_host_ms"], 1)
        out["sizes"][str(n)] = res
        warm.close()
        vol.close()
    if a.once:
        return
    out["note"] = ("host wall-clock of whole calls that end in a device synchronise, medians with [min, max], variants alternating "
                   "inside every repetition; host_edt_ms is the user's path without the feature (two downloads, the site mask in "
                   "numpy, scipy's exact EDT in double precision), timed in the same run; nothing about the speed was known when the "
                   "feature was specified")
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
