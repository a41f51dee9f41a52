#!/usr/bin/env python3
"""CPU model of tests/test_class_fusion.py::test_fused_classes_match_the_analytic_classes, run once to choose the window radius r of
that test: the oracle's Volume.integrate / raycast and tests/classes_ref.py are what the GPU computes bit for bit, so
the share of differing pixels is known before any GPU run.  Prints, per r in 0..6, the compared pixels and the share that differs; the
test takes the smallest r whose share is under 1 %.

    python tools/class_window_model.py [grid=256] [frames=40]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle as O  # noqa: E402
from tests import classes_ref as R  # noqa: E402
from tsdf_amd import synth  # noqa: E402

SEED = 0x5EED0003
W, H = synth.WIDTH, synth.HEIGHT


def uniform_window(image, r):
    """True where every pixel of the (2r+1)^2 window (clipped at the border) has the centre's value."""
    img = image.reshape(H, W)
    ok = np.ones((H, W), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            y0, y1, x0, x1 = max(0, dy), H + min(0, dy), max(0, dx), W + min(0, dx)
            ok[y0 - dy:y1 - dy, x0 - dx:x1 - dx] &= img[y0 - dy:y1 - dy, x0 - dx:x1 - dx] == img[y0:y1, x0:x1]
    return ok.reshape(-1)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    F = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    O.build()
    ov = O.Volume((n,) * 3, (3000.0,) * 3)
    geom = ((n,) * 3, np.array(ov.voxel_size(), np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32),
            np.float32(ov.truncation_distance()))
    words = np.zeros(n ** 3, np.uint32)
    for i in range(F):
        d, cam = synth.depth_frame(i, F, seed=SEED)
        k, _ = synth.class_frame(i, F, seed=SEED)
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=O.max_threads())
        words, _, _ = R.integrate_classes(O, words, geom, d, k, None, W, H, cam)
        print("frame %d: %d classified voxels" % (i, int((words != 0).sum())), flush=True)
    cam = synth.camera_for_frame(0.5, F)
    V, _ = ov.raycast(W, H, cam.pose(), cam.kinv(), nthreads=O.max_threads())
    V = np.asarray(V, np.float32).reshape(-1, 3)
    classes, votes = R.sample(words, geom, V)
    truth = synth.trace_classes(cam)
    seen = ~np.isnan(V[:, 0]) & (votes >= 1)
    for r in range(7):
        sel = seen & uniform_window(truth, r)
        diff = int((classes[sel] != truth[sel]).sum())
        print("r = %d: %d pixels compared, %d differ (%.4f %%)" % (r, int(sel.sum()), diff, 100.0 * diff / max(int(sel.sum()), 1)))


if __name__ == "__main__":
    main()
