"""Time of the exploration queries (include/tsdf_amd.h, "exploration") on bench.py's scene (640 x 480, seed 0x5EED0003), 25 frames
fused at 512^3, in each weight storage (8-bit, 16-bit, fp32).  Prints one JSON line and writes it to profiles/explore_bench.json.

Per storage, host wall-clock times of whole calls, each ending in a device synchronise, as the median (and range) of --reps repetitions
after --warmup, the variants alternating inside every repetition, every yardstick in the same run:

  find_frontiers_ms     find_frontiers into a warm handle (flag kernel, chunk scan, the count's synchronise, list kernel)
  esdf_ms               yardstick: compute_esdf(--esdf-cap) into a warm handle -- its sites pass has the same stencil, its three scan
                        passes come on top (the kernels apart: --once under a kernel trace)
  stream_read_ms        yardstick: a plain streaming read (torch sum) of as many bytes as the weights take in this storage
  cluster26_ms / cluster6_ms   cluster(connectivity, min_size 1) on the warm handle
  label_components_ms   yardstick: tsdf_mesh_label_components on the same scene's indexed mesh
  view_gain_ms          view_gain_device with the count, for the rays of a 160 x 120 pinhole view (every 4th pixel of the bench camera)
  cast_rays_ms          yardstick: tsdf_volume_cast_rays_device on the same rays

    python tools/bench_explore.py [--size 512] [--frames 25] [--reps 10] [--warmup 2] [--once]

--once: one call of each per storage and nothing else (for a kernel trace).
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
    ap.add_argument("--esdf-cap", type=float, default=100.0)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explore_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import _capi, synth
    assert torch.cuda.is_available(), "bench_explore needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    n = a.size
    out = {"tool": "bench_explore", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "size": n, "reps": a.reps,
           "esdf_cap_mm": a.esdf_cap, "device": torch.cuda.get_device_name(0), "storages": {}}
    for bits in (8, 16, 32):
        vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        cam = None
        for i in range(a.frames):
            d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
            vol.integrate(d, W, H, cam)
        if vol.weight_storage()[0] != bits:
            vol.set_weight_storage(bits)
        vol.synchronize()
        ex, esdf = tsdf_amd.Explorer(), tsdf_amd.ESDF()
        mesh = vol.extract_mesh()
        o, d = tsdf_amd.pixel_rays(cam, W, H, 4)
        n_rays = len(o)
        rays = torch.from_numpy(np.concatenate([o.reshape(-1), d.reshape(-1)])).cuda()
        results = torch.zeros(7 * n_rays, dtype=torch.float32, device="cuda")     # points, t, normals
        counts = torch.zeros(3 * n_rays, dtype=torch.int32, device="cuda")        # unknown, free, stop (bytes)
        p_o, p_d, p_r, p_c = rays.data_ptr(), rays.data_ptr() + 12 * n_rays, results.data_ptr(), counts.data_ptr()
        weights_like = torch.zeros(n ** 3 * bits // 32, dtype=torch.int32, device="cuda")
        kept = {}

        def find():
            vol.find_frontiers(into=ex)

        def cluster(connectivity):
            def run():
                ex.cluster(connectivity, 1)
                ex.device_buffers()                                # (waits for the rows kernel)
            return run

        def gain():
            kept["gain"] = vol.view_gain_device(ex, n_rays, p_o, p_d, None, p_c, p_c + 4 * n_rays, p_c + 8 * n_rays)

        def cast():
            vol.cast_rays_device(n_rays, p_o, p_d, None, p_r, p_r + 12 * n_rays, p_r + 16 * n_rays)
            vol.synchronize()

        def stream_read():
            kept["sum"] = int(weights_like.sum().item())

        variants = {"find_frontiers": find, "esdf": lambda: esdf.device_buffer() if vol.compute_esdf(a.esdf_cap, into=esdf) else None,
                    "stream_read": stream_read, "cluster26": cluster(26), "cluster6": cluster(6),
                    "label_components": lambda: kept.update(components=mesh.label_components()), "view_gain": gain, "cast_rays": cast}
        if a.once:
            for fn in variants.values():
                fn()
            vol.synchronize()
        else:
            times = {v: [] for v in variants}
            for r in range(a.warmup + a.reps):
                for v, fn in variants.items():
                    vol.synchronize()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    t = (time.perf_counter() - t0) * 1e3
                    if r >= a.warmup:
                        times[v].append(t)
            i = ex.info
            stop = np.empty(n_rays, np.uint8)
            _capi.check(_capi.lib.tsdf_device_download(stop.ctypes.data, C.c_void_p(p_c + 8 * n_rays), n_rays))
            res = {"n_unknown": int(i.n_unknown), "n_free": int(i.n_free), "n_occupied": int(i.n_occupied), "n_frontiers": int(i.n_frontiers),
                   "n_clusters_6": int(i.n_clusters), "mesh_vertices": mesh.n_vertices, "mesh_components": int(kept["components"]["n_components"]),
                   "rays": n_rays, "rays_skipped_ended_blocked": [int((stop == k).sum()) for k in range(3)], "view_gain_voxels": kept["gain"],
                   "scratch_bytes": ex.scratch_bytes, "weight_bytes_read_by_stream_read": int(weights_like.numel()) * 4}
            for v, ts in times.items():
                res[v + "_ms"] = round(float(np.median(ts)), 3)
                res[v + "_ms_range"] = [round(min(ts), 3), round(max(ts), 3)]
            out["storages"][str(bits)] = res
        mesh.close()
        ex.close()
        esdf.close()
        vol.close()
    if a.once:
        return
    out["note"] = ("host wall-clock of whole calls that end in a device synchronise, medians with [min, max], variants alternating inside "
                   "every repetition, all in one run; esdf_ms, stream_read_ms, label_components_ms and cast_rays_ms are yardsticks, not "
                   "the code under test; nothing about the speed was known when the feature was specified")
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
