"""Time of labelling and filtering the connected components of a mesh on the device (include/tsdf_amd.h, "mesh components") against what
a user does without them, on bench.py's scene (640 x 480, seed 0x5EED0003, 24 noisy frames fused) at 256^3 and 512^3, the mesh
extracted once into a warm handle.  Prints one JSON line and writes it to profiles/components_bench.json.

Per size, host wall-clock times of whole calls, each ending in a device synchronise, as the median (and range) of --reps repetitions
after --warmup, the variants alternating inside every repetition:

  label_ms        Mesh.label_components(): five launches and one synchronise; labels and sizes stay on the device
  filter_ms       Mesh.filter_components(min_triangles=100) of the labelled mesh into a warm handle, until its arrays are complete
  host_ms         the yardstick: tsdf_mesh_download of V and I, scipy.sparse.csgraph.connected_components on the edges of the triples,
                  relabelling to the smallest index, np.bincount, the numpy filter (host_download_ms, host_label_ms and host_filter_ms
                  are its three parts); the filtered mesh is then on the host, not on the device

The yardstick's labels, sizes and filtered arrays are compared with the device's; any difference fails the run.  Also recorded: the
component count, the largest component's share of the triangles, what the filter keeps.

    python tools/bench_components.py [--sizes 256 512] [--frames 24] [--reps 10] [--warmup 2] [--min-triangles 100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_label(n, I):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    tri = I.reshape(-1, 3).astype(np.int64)
    rows, cols = np.concatenate([tri[:, 0], tri[:, 0]]), np.concatenate([tri[:, 1], tri[:, 2]])
    count, comp = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n)), directed=False)
    smallest = np.full(count, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    triangles = np.bincount(comp[tri[:, 0]], minlength=count)
    return smallest[comp].astype(np.uint32), triangles[comp].astype(np.uint32), count


def host_filter(V, I, T, min_triangles):
    keep = T >= min_triangles
    new = np.cumsum(keep) - 1
    tri = I.reshape(-1, 3)
    return V[keep], new[tri[keep[tri[:, 0]]]].reshape(-1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--frames", type=int, default=24, help="frames fused before the extraction")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-triangles", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.json"))
    a = ap.parse_args()

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_components needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    out = {"tool": "bench_components", "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "reps": a.reps,
           "min_triangles": a.min_triangles, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in a.sizes:
        vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
        for i in range(a.frames):
            d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
            vol.integrate(d, W, H, cam)
        vol.synchronize()
        mesh, dst = tsdf_amd.Mesh(), tsdf_amd.Mesh()
        vol.extract_mesh(into=mesh).device_buffers()
        kept = {}

        def label():
            kept["info"] = mesh.label_components()

        def filter_():
            mesh.filter_components(a.min_triangles, into=dst).device_buffers()

        def host():
            t0 = time.perf_counter()
            V, I = mesh.vertices, mesh.indices
            t1 = time.perf_counter()
            L, T, count = host_label(len(V), I)
            t2 = time.perf_counter()
            kept["host"] = (L, T, count) + host_filter(V, I, T, a.min_triangles)
            t3 = time.perf_counter()
            kept.setdefault("parts", []).append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))

        variants = {"label": label, "filter": filter_, "host": host}
        times = {v: [] for v in variants}
        for r in range(a.warmup + a.reps):
            for v, fn in variants.items():
                vol.synchronize()
                t0 = time.perf_counter()
                fn()
                t = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    times[v].append(t)
        # faster and different is not faster
        L, T, count, kV, kI = kept["host"]
        info = kept["info"]
        assert np.array_equal(mesh.labels, L) and np.array_equal(mesh.component_triangles, T), "the device's labels differ from scipy's"
        assert info["n_components"] == count and info["largest_triangles"] == int(T.max())
        assert dst.vertices.tobytes() == kV.tobytes() and np.array_equal(dst.indices, kI), "the device's filtered mesh differs from numpy's"
        res = {"vertices": mesh.n_vertices, "triangles": mesh.n_indices // 3, "components": info["n_components"],
               "largest_triangles": info["largest_triangles"],
               "largest_share": round(info["largest_triangles"] / max(info["n_triangles"], 1), 4),
               "kept_vertices": dst.n_vertices, "kept_triangles": dst.n_indices // 3,
               "kept_components": dst.label_components()["n_components"],
               "scratch_bytes": mesh.scratch_bytes, "dst_scratch_bytes": dst.scratch_bytes}
        for v, ts in times.items():
            res[v + "_ms"] = round(float(np.median(ts)), 3)
            res[v + "_ms_range"] = [round(min(ts), 3), round(max(ts), 3)]
        parts = np.array(kept["parts"][a.warmup:])
        for k, name in enumerate(("host_download_ms", "host_label_ms", "host_filter_ms")):
            res[name] = round(float(np.median(parts[:, k])), 3)
        res["host_over_device"] = round(res["host_ms"] / (res["label_ms"] + res["filter_ms"]), 2)
        out["sizes"][str(n)] = res
        mesh.close()
        dst.close()
        vol.close()
    out["note"] = ("host wall-clock of whole calls that end in a device synchronise, medians with [min, max], variants alternating inside "
                   "every repetition; host_ms is the download of V and I from pageable memory, scipy's connected_components and the numpy "
                   "filter, and leaves the result on the host; label_ms + filter_ms leave it on the device")
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
