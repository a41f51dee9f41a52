"""Time of the mesh renderer (include/tsdf_amd.h, "mesh rendering") on bench.py's scene (640 x 480, seed 0x5EED0003): 25 colour frames
fused at 512^3, the whole-grid mesh (normals and colours) rendered at 640 x 480 from the last pose.  Prints one JSON line and writes it
to profiles/render_bench.json.

Host wall-clock times of whole calls, each ending in a wait for the handle's work, as the median (and range) of --reps repetitions
after --warmup, the variants alternating inside every repetition, every yardstick in the same run:

  depth_ms / all_ms            the mesh into the depth map alone / into all six targets (device arrays), warm handle
  simplified_<cell>_box<T>_ms  the mesh simplified with cells of <cell> mm, all targets, with the large-path threshold T
                               (tsdf_render_set_large_box; "lane": every triangle on the lane path); n_large is recorded beside each
  raycast_ms                   yardstick: tsdf_raycast_device of the same view (vertices and normals)
  extract_mesh_ms              yardstick: tsdf_volume_extract_mesh with normals and colours into a warm handle
  z_difference                 median and maximum |z_render - z_raycast| (mm) over the pixels both hit: how far the mesh's linear crossing
                               lies from the cast's trilinear one; recorded, not asserted

    python tools/bench_render.py [--size 512] [--frames 25] [--reps 10] [--warmup 2] [--once] [--out FILE]

--once: one call of each and nothing else (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESHOLDS = (64, 256, 1024, None)   # None: everything on the lane path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=25, help="frames fused before the renders")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=float, nargs=2, default=(50.0, 200.0), help="the two cell sizes (mm) of the simplified meshes")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_render needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    n = a.size
    vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    vol.enable_colour()
    for i in range(a.frames):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        rgb, _ = synth.colour_frame(i, PERIOD, seed=SEED)
        vol.integrate_colour(d, rgb, W, H, cam)
    vol.synchronize()
    inv_pose, k = np.array(cam.inverse_pose(), np.float32).reshape(-1), np.array(cam.k(), np.float32).reshape(-1)
    near, far = 100.0, 10000.0

    mesh, remesh = tsdf_amd.Mesh(), tsdf_amd.Mesh()
    vol.extract_mesh(normals=True, colours=True, into=mesh).device_buffers()
    simplified = {cell: mesh.simplify(cell) for cell in a.cells}
    renderer, caster = tsdf_amd.Renderer(), tsdf_amd.GPURaycaster(W, H)
    px = W * H
    maps = {"triangle": torch.zeros(px, dtype=torch.int32, device="cuda"), "z": torch.zeros(px, dtype=torch.float32, device="cuda"),
            "depth": torch.zeros(px, dtype=torch.int16, device="cuda"), "vertices": torch.zeros(3 * px, dtype=torch.float32, device="cuda"),
            "normals": torch.zeros(3 * px, dtype=torch.float32, device="cuda"), "rgb": torch.zeros(3 * px, dtype=torch.uint8, device="cuda")}
    every = {name: t.data_ptr() for name, t in maps.items()}
    cast_v, cast_n = torch.zeros(3 * px, dtype=torch.float32, device="cuda"), torch.zeros(3 * px, dtype=torch.float32, device="cuda")
    infos = {}

    def render(which, m, targets, threshold=tsdf_amd._capi.TSDF_RENDER_LARGE_BOX):
        def run():
            renderer.set_large_box(threshold)
            infos[which] = renderer.render_device(m, inv_pose, k, (W, H), near, far, targets=targets, info=True)   # (waits)
        return run

    def raycast():
        caster.raycast_device(vol, cam, cast_v.data_ptr(), cast_n.data_ptr())
        vol.synchronize()

    def extract():
        vol.extract_mesh(normals=True, colours=True, into=remesh).device_buffers()   # (waits)

    variants = {"depth": render("depth", mesh, {"depth": every["depth"]}), "all": render("all", mesh, every)}
    for cell, m in simplified.items():
        for t in THRESHOLDS:
            name = "simplified_%g_box%s" % (cell, "lane" if t is None else t)
            variants[name] = render(name, m, every, t)
    variants["raycast"] = raycast
    variants["extract_mesh"] = extract

    if a.once:
        for fn in variants.values():
            fn()
        vol.synchronize()
        return
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

    # the mesh's depth against the cast's, from the same pose
    variants["all"]()
    raycast()
    torch.cuda.synchronize()
    z_render = maps["z"].cpu().numpy().astype(np.float64)
    V = cast_v.cpu().numpy().astype(np.float64).reshape(-1, 3)
    m4 = inv_pose.astype(np.float64).reshape(4, 4).T
    z_cast = (V @ m4[2, :3] + m4[2, 3]) / (V @ m4[3, :3] + m4[3, 3])
    both = np.isfinite(z_render) & np.isfinite(z_cast)
    dz = np.abs(z_render[both] - z_cast[both])

    mi = mesh.info()
    out = {"tool": "bench_render", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "size": n, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "near": near, "far": far, "mesh_vertices": int(mi.n_vertices), "mesh_triangles": int(mi.n_indices) // 3,
           "scratch_bytes": renderer.scratch_bytes,
           "simplified": {"%g" % cell: {"vertices": m.n_vertices, "triangles": m.n_indices // 3} for cell, m in simplified.items()},
           "z_difference": {"pixels_both_hit": int(both.sum()), "pixels_render_hit": int(np.isfinite(z_render).sum()),
                            "pixels_cast_hit": int(np.isfinite(z_cast).sum()), "median_mm": float(np.median(dz)) if dz.size else None,
                            "max_mm": float(dz.max()) if dz.size else None},
           "variants": {}}
    for v, ts in times.items():
        out["variants"][v] = {"ms": round(float(np.median(ts)), 4), "ms_range": [round(min(ts), 4), round(max(ts), 4)]}
        if v in infos:
            out["variants"][v].update(infos[v])
    out["note"] = ("host wall-clock of whole calls that end in a wait for the handle, medians with [min, max], variants alternating inside every "
                   "repetition, all in one run; raycast and extract_mesh are yardsticks, not the code under test; box<T>: the large-path threshold, "
                   "lane: no triangle takes render_large_kernel")
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
