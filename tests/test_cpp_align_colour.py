"""Colour alignment through the C++ class surface (libtsdf_host.so: TSDFVolume::sample_intensity and the align_points overload with
intensities): build/test_align_colour (tests/cpp/test_align_colour.cpp) uploads the wall scene of tests/align_colour_ref.py, samples,
aligns from the start pose and checks that the refusals throw; what it dumps must be the Python surface's bit for bit (the same kernels
in the same order).  And tools/kinfu_stream.cpp's --colour-weight: what it refuses (no GPU needed) and a tracked run with it."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import tsdf_amd
from tests import align_colour_ref as CR
from tests.helpers import assert_same_floats
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_align_colour")
STREAM = os.path.join(ROOT, "build", "kinfu_stream")
ITERATIONS, WEIGHT = 8, 0.25


@pytest.mark.gpu
def test_cpp_colour_align_matches_the_python_surface(tmp_path):
    from tests.test_align_colour import wall_volume
    if not os.path.exists(BIN):
        pytest.fail("build/test_align_colour missing: run `make cpptest` (build() does)")
    s = CR.wall_scene()
    for name, a in (("dist.f32", s.dist), ("weight.f32", s.weight), ("colour.u32", s.colour), ("points.f32", s.points), ("intensity.f32", s.intensity)):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    np.ascontiguousarray(s.T0.T.reshape(-1)).tofile(str(tmp_path / "t0.f64"))
    r = subprocess.run([BIN] + [str(tmp_path / n) for n in ("dist.f32", "weight.f32", "colour.u32", "points.f32", "intensity.f32")]
                       + [str(len(s.points)), str(tmp_path / "t0.f64"), str(ITERATIONS), repr(s.gate), repr(s.colour_gate), repr(WEIGHT), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    m = re.search(r"colour align surface ok: residual (\S+) (\S+) inliers (\S+) (\S+)", r.stdout)
    T = np.fromfile(str(tmp_path / "pose.f64"), np.float64).reshape(4, 4).T

    vol = wall_volume(s)
    Tp, res, inl = vol.align_points(s.points, s.T0, iterations=ITERATIONS, gate=s.gate, intensity=s.intensity, colour_gate=s.colour_gate,
                                    colour_weight=WEIGHT)
    c, g = vol.sample_intensity(s.points)
    vol.close()
    assert np.array_equal(T, Tp)
    assert tuple(np.float32(m.group(i)) for i in (1, 2)) == tuple(np.float32(v) for v in res)
    assert (float(m.group(3)), float(m.group(4))) == inl == (len(s.points), len(s.points))
    assert CR.in_plane_error(T) <= 0.25 * CR.in_plane_error(s.T0)
    assert_same_floats(np.fromfile(str(tmp_path / "intensity.f32"), np.float32), c, "C++ sample_intensity")
    assert_same_floats(np.fromfile(str(tmp_path / "gradient.f32"), np.float32), g, "C++ sample_intensity gradient")
    assert np.isfinite(c).all()


def test_kinfu_stream_refuses_a_colour_weight_it_cannot_use(tmp_path):
    assert os.path.exists(STREAM), "build/kinfu_stream missing: run `make cpptest` (build() does)"
    d = str(tmp_path)          # (arguments are checked before the directory is read)
    for args in (["--track", "--colour-weight", "0.1"],                       # without --field
                 ["--colour-weight", "0.1"],
                 ["--field", "--colour-weight", "0.1"],                       # --field itself needs --track
                 ["--track", "--field", "--colour-weight", "-0.5"],
                 ["--track", "--field", "--colour-weight", "nan"],
                 ["--track", "--field", "--colour-weight", "inf"],
                 ["--track", "--field", "--colour-weight"]):                  # no value
        r = subprocess.run([STREAM, "-d", d] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "", (args, r.returncode, r.stdout + r.stderr)
        assert "--colour-weight" in r.stderr or "--field" in r.stderr, (args, r.stderr)
    r = subprocess.run([STREAM, "--bogus"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--colour-weight W]" in r.stderr


@pytest.mark.gpu
def test_kinfu_stream_tracks_with_a_colour_weight(tmp_path):
    n, F = 128, 5
    d = tmp_path / "tum"
    synth.write_tum_directory(str(d), F, seed=0x5EED0005, stream_frames=200, colour=True)
    base = [STREAM, "-d", str(d), "-n", str(n), "-k", str(F), "--track", "--field"]
    r = subprocess.run(base + ["--colour-weight", "0.1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["frames"] == F and line["align"] == "field" and line["colour"] is True and line["colour_weight"] == 0.1
    assert line["last_icp_inliers"] > 0.2 * synth.WIDTH * synth.HEIGHT and line["last_colour_inliers"] > 0.1 * synth.WIDTH * synth.HEIGHT
    assert line["last_pose_translation_error_mm"] < 25.0          # voxels are 23 mm here, depth noise +-3 mm
    # weight 0 is the plain field tracker with colour fused: the same pose error, no colour inliers reported
    zero = subprocess.run(base + ["--colour-weight", "0"], capture_output=True, text=True, timeout=300)
    plain = subprocess.run(base + ["--colour"], capture_output=True, text=True, timeout=300)
    assert zero.returncode == 0 and plain.returncode == 0, zero.stdout + zero.stderr + plain.stdout + plain.stderr
    z, p = json.loads(zero.stdout.strip().splitlines()[-1]), json.loads(plain.stdout.strip().splitlines()[-1])
    assert z["last_pose_translation_error_mm"] == p["last_pose_translation_error_mm"] and z["last_icp_inliers"] == p["last_icp_inliers"]
    assert z["colour"] is True and z["last_colour_inliers"] == 0 and "colour_weight" not in p
