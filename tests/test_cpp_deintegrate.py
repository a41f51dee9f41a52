"""kinfu_stream --track --window N (tools/kinfu_stream.cpp: tsdf_tracker_set_window from C++): the dumped volume holds exactly the last N
tracked frames -- bit for bit the reference replay of the filtered frames at the poses the run dumped."""
import json
import os
import subprocess

import numpy as np
import pytest

import tsdf_amd
from tests.deintegrate_ref import oracle_remove
from tests.helpers import H, W, assert_same_floats
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "kinfu_stream")


@pytest.mark.gpu
def test_kinfu_stream_tracks_with_a_window(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/kinfu_stream missing: run `make cpptest` (build() does)")
    n, F, window = 128, 9, 3
    d = tmp_path / "tum"
    synth.write_tum_directory(str(d), F, seed=0x5EED0005, stream_frames=200)
    runs = {}
    for name, extra in (("window", ["--window", str(window)]), ("plain", [])):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([BIN, "-d", str(d), "-n", str(n), "-k", str(F), "--track", "--dump", str(out)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[name] = (json.loads(r.stdout.strip().splitlines()[-1]), np.fromfile(str(out / "distances.f32"), np.float32))
    line, dist = runs["window"]
    assert line["window"] == window and "window" not in runs["plain"][0]
    assert line["frames"] == F and line["last_icp_inliers"] > 0.3 * W * H and line["last_pose_translation_error_mm"] < 25.0
    assert not np.array_equal(dist, runs["plain"][1])             # (other frames in the volume, and from the 4th frame on other poses)
    # the replay: the loader's frames through the oracle's bilateral filter, integrated at the poses the run dumped, the frame of
    # `window` steps back taken out after each integrate (tests/deintegrate_ref.py): the dumped distances bit for bit
    frames, _ = tsdf_amd.load_tum_directory(str(d))
    poses = np.fromfile(str(tmp_path / "window" / "poses.f32"), np.float32).reshape(F, 16)
    ov = oracle.Volume((n, n, n), (3000.0,) * 3)
    used = []
    for i in range(F):
        f = np.asarray(oracle.bilateral_u16(frames[i][0], W, H, 30.0, 4.5, nthreads=oracle.max_threads()), np.uint16).reshape(-1)
        cam = tsdf_amd.Camera.default_depth_camera()
        cam.set_pose(poses[i].copy())
        assert np.array_equal(np.asarray(cam.pose(), np.float32).reshape(-1), poses[i])
        used.append((f, cam))
        ov.integrate(f, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
        if i >= window:
            oracle_remove(oracle, ov, *used[i - window])
    assert ov.weight.max() == float(window)
    assert_same_floats(dist, ov.dist, "kinfu_stream --track --window %d vs the replay: distances" % window)
