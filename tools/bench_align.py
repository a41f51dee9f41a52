"""Cost of field alignment (include/tsdf_amd.h, "field alignment") on bench.py's scene: 512^3, 640 x 480, seed 0x5EED0003.  Prints one
JSON line and writes it to profiles/align_bench.json.

The volume holds --frames fused frames; the next frame's depth pixels become camera-frame points (tsdf_depth_to_points_device) at
steps 1, 2 and 4, and the pose of the last fused frame is the prediction, as in the tracked loop.

  step{1,2,4}_us_per_step   one Gauss-Newton step over those points: (a chain of LONG steps - a chain of SHORT steps) / (LONG - SHORT),
                            each chain event-bracketed on the aligner's stream, launches + finish + synchronise included; medians
  chain_19_ms               the tracker's chain: 4 / 5 / 10 steps at steps 4 / 2 / 1, one call, with the three point conversions
  mesh_us_per_step          the same difference over the vertices of the extracted mesh (volume-to-volume registration's points)
  icp_ms                    tsdf_icp_get_incremental_transformation (19 iterations; maps already built) of the same frame against
                            the model rendered from the prediction, in the same run, for comparison; icp_init_ms: the model's and
                            the frame's maps, which field alignment does not need

    python tools/bench_align.py [--size 512] [--frames 24] [--reps 30] [--warmup 5]

--colour: the colour term as well (include/tsdf_amd.h, "colour alignment"), written to profiles/align_colour_bench.json: the frames
are fused with their colour frames, the next frame's RGB becomes intensities at the same steps (tsdf_rgb_to_intensity_device; for the
mesh, the field's own intensity at the vertices), and every figure above is taken twice in the same run -- "plain" (the calls above,
untouched by the colour term) and "colour" (tsdf_aligner_run_colour at COLOUR_GATE / COLOUR_WEIGHT).  --parent FILE...: align_bench
lines of the parent commit taken in the same session (its own tools/bench_align.py), embedded as "parent_plain"; --again FILE...: earlier
lines of this tool from the same session, embedded as "repeats": together they are the run-to-run spread the plain numbers are judged by.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHORT, LONG = 4, 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=24, help="frames fused before the alignment")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--colour", action="store_true", help="measure the colour term beside the plain calls")
    ap.add_argument("--parent", nargs="*", default=[], help="(--colour) align_bench JSON files of the parent commit, same session")
    ap.add_argument("--again", nargs="*", default=[], help="(--colour) earlier JSON files of this tool, same session")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "align_colour_bench.json" if a.colour else "align_bench.json")

    import torch
    import tsdf_amd
    from tsdf_amd import synth
    assert torch.cuda.is_available(), "bench_align needs a GPU"
    W, H, SEED, PERIOD = synth.WIDTH, synth.HEIGHT, 0x5EED0003, 200
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = a.size
    vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    vol.set_stream(stream.cuda_stream)
    cam = None
    if a.colour:
        vol.enable_colour()
    for i in range(a.frames):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        if a.colour:
            vol.integrate_colour(d, synth.colour_frame(i, PERIOD, seed=SEED)[0], W, H, cam)
        else:
            vol.integrate(d, W, H, cam)
    vol.synchronize()
    prediction = cam.pose().astype(np.float64).reshape(4, 4).T
    depth, cam_next = synth.depth_frame(a.frames, PERIOD, seed=SEED)
    depth_dev = torch.from_numpy(depth.view(np.int16).copy()).to(dev)
    kinv = cam_next.kinv()
    points = {}
    for step in (1, 2, 4):
        m = -(-W // step) * -(-H // step)
        points[step] = torch.empty((m, 3), dtype=torch.float32, device=dev)
    mesh = torch.from_numpy(vol.extract_surface()).to(dev)
    torch.cuda.synchronize()
    aligner = tsdf_amd.FieldAligner()
    gate = vol.truncation_distance()

    def convert(step):
        tsdf_amd.depth_to_points_device(W, H, depth_dev.data_ptr(), kinv, step, 20000.0, points[step].data_ptr(), stream.cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            r = fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for step in (1, 2, 4):
        convert(step)
    torch.cuda.synchronize()

    # (--colour) the observed intensity of every point set, by the key its figures are reported under: the next frame's RGB at the
    # same steps, the field's own at the mesh
    intensity, use_colour = {}, False
    if a.colour:
        rgb_dev = torch.from_numpy(synth.colour_frame(a.frames, PERIOD, seed=SEED)[0].reshape(-1).copy()).to(dev)
        for step in (1, 2, 4):
            intensity["step%d" % step] = torch.empty(points[step].shape[0], dtype=torch.float32, device=dev)
        intensity["mesh"] = torch.empty(mesh.shape[0], dtype=torch.float32, device=dev)
        vol.sample_intensity_device(int(mesh.shape[0]), mesh.data_ptr(), intensity["mesh"].data_ptr())
        vol.synchronize()

    def convert_colour(step):
        tsdf_amd.rgb_to_intensity_device(W, H, rgb_dev.data_ptr(), step, intensity["step%d" % step].data_ptr(), stream.cuda_stream)

    if a.colour:
        for step in (1, 2, 4):
            convert_colour(step)
        torch.cuda.synchronize()

    def flat(r):
        # run_colour_device gives pairs (geometric, colour): the geometric figures go where the plain ones go
        return (r[0], r[1][0], r[2][0], r[2][1]) if use_colour else r

    def chain(P, T0, iterations, key):
        if use_colour:
            return flat(aligner.run_colour_device(vol, [(P.data_ptr(), intensity[key].data_ptr(), int(P.shape[0]), iterations)], T0, gate))
        return aligner.run_device(vol, [(P.data_ptr(), int(P.shape[0]), iterations)], T0, gate)

    def tracker_chain():
        for step in (4, 2, 1):
            convert(step)
            if use_colour:
                convert_colour(step)
        if use_colour:
            return flat(aligner.run_colour_device(vol, [(points[s].data_ptr(), intensity["step%d" % s].data_ptr(), int(points[s].shape[0]), it)
                                                        for s, it in ((4, 4), (2, 5), (1, 10))], prediction, gate))
        return aligner.run_device(vol, [(points[4].data_ptr(), int(points[4].shape[0]), 4), (points[2].data_ptr(), int(points[2].shape[0]), 5),
                                        (points[1].data_ptr(), int(points[1].shape[0]), 10)], prediction, gate)

    out = {"tool": "bench_align", "size": n, "width": W, "height": H, "seed": "0x%X" % SEED, "frames_fused": a.frames, "reps": a.reps,
           "weight_storage_bits": vol.weight_storage()[0], "device": torch.cuda.get_device_name(0), "gate_mm": round(gate, 3)}

    def per_step(P, T0, key):
        short, long_ = [], []
        for r in range(a.warmup + a.reps):
            ts, _ = timed(lambda: chain(P, T0, SHORT, key))
            tl, res = timed(lambda: chain(P, T0, LONG, key))
            if r >= a.warmup:
                short.append(ts)
                long_.append(tl)
        us = (float(np.median(long_)) - float(np.median(short))) * 1e3 / (LONG - SHORT)
        out[key + "_points"] = int(P.shape[0])
        out[key + "_us_per_step"] = round(us, 2)
        out[key + "_chain_ms"] = {"%d_steps" % SHORT: round(float(np.median(short)), 4), "%d_steps" % LONG: round(float(np.median(long_)), 4)}
        out[key + "_inliers_last_step"] = res[2]
        if use_colour:
            out[key + "_colour_inliers_last_step"] = res[3]

    truth = cam_next.pose().astype(np.float64).reshape(4, 4).T

    def alignment_figures():
        for step in (1, 2, 4):
            per_step(points[step], prediction, "step%d" % step)
        per_step(mesh, np.eye(4), "mesh")
        ts = []
        for r in range(a.warmup + a.reps):
            t, res = timed(tracker_chain)
            if r >= a.warmup:
                ts.append(t)
        out["chain_19_ms"] = round(float(np.median(ts)), 4)
        out["chain_19_ms_range"] = [round(min(ts), 4), round(max(ts), 4)]
        out["chain_19_inliers"] = res[2]
        if use_colour:
            out["chain_19_colour_inliers"] = res[3]
        out["chain_19_translation_error_mm"] = round(float(np.linalg.norm(res[0][:3, 3] - truth[:3, 3])), 3)

    alignment_figures()
    out["prediction_translation_error_mm"] = round(float(np.linalg.norm(prediction[:3, 3] - truth[:3, 3])), 3)
    if a.colour:
        # the same figures with the colour term, in the same run: `out` collects them under "colour", the plain ones move under "plain"
        head = {k: out.pop(k) for k in list(out) if k.startswith(("step", "mesh", "chain_19"))}
        use_colour = True
        alignment_figures()
        tail = {k: out.pop(k) for k in list(out) if k.startswith(("step", "mesh", "chain_19"))}
        out["tool"] = "bench_align --colour"
        out["colour_gate"], out["colour_weight"] = tsdf_amd.api.COLOUR_GATE, tsdf_amd.api.COLOUR_WEIGHT
        out["plain"], out["colour"] = head, tail
        out["parent_plain"] = [json.load(open(p)) for p in a.parent]
        out["repeats"] = [{k: j[k] for k in ("plain", "colour")} for j in (json.load(open(p)) for p in a.again)]

    # ICP on the same frame: model = the volume rendered from the prediction
    k = cam.k()
    icp = tsdf_amd.ICPOdometry(W, H, float(k[6]), float(k[7]), float(k[0]), float(k[4]))
    icp.set_stream(stream.cuda_stream)
    model = torch.empty(W * H, dtype=torch.int16, device=dev)
    caster = tsdf_amd.GPURaycaster(W, H)

    def icp_init():
        caster.render_to_depth_device(vol, cam, model.data_ptr(), None)
        icp.init_icp_device(model.data_ptr(), model=True)
        icp.init_icp_device(depth_dev.data_ptr(), model=False)

    ti, tt = [], []
    for r in range(a.warmup + a.reps):
        t0, _ = timed(icp_init)
        t1, T = timed(lambda: icp.get_incremental_transformation())
        if r >= a.warmup:
            ti.append(t0)
            tt.append(t1)
    out["icp_ms"] = round(float(np.median(tt)), 4)
    out["icp_ms_range"] = [round(min(tt), 4), round(max(tt), 4)]
    out["icp_init_ms"] = round(float(np.median(ti)), 4)
    out["icp_inliers"] = icp.last_inliers
    Ti = T.copy()
    Ti[:3, 3] *= 1000.0
    out["icp_translation_error_mm"] = round(float(np.linalg.norm((prediction @ Ti)[:3, 3] - truth[:3, 3])), 3)
    out["note"] = ("medians of event-bracketed calls on one stream; every call blocks for its result, so launch, finish and "
                   "synchronise are part of every chain figure and cancel in the per-step difference; the raw frame, not a filtered one")
    icp.close()
    aligner.close()
    vol.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
