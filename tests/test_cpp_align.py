"""Field alignment through the C++ class surface (libtsdf_host.so: TSDFVolume::align_points): build/test_align (tests/cpp/test_align.cpp)
fuses the scene of tests/align_ref.py, aligns its points from the start pose and checks that the refusals throw; the pose it dumps
must be the Python surface's bit for bit (the same kernels in the same order) and the float64 reference chain's within the tolerance
rule of tests/test_align.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import tsdf_amd
from tests import align_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_align")
ITERATIONS = 10


@pytest.mark.gpu
def test_cpp_align_matches_the_python_surface_and_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_align missing: run `make cpptest` (build() does)")
    s = R.fused_scene(oracle)
    np.concatenate([d.reshape(-1) for d, _ in s.frames]).astype(np.uint16).tofile(str(tmp_path / "frames.u16"))
    np.concatenate([cam.pose().astype(np.float32).reshape(-1) for _, cam in s.frames]).tofile(str(tmp_path / "poses.f32"))
    s.points.tofile(str(tmp_path / "points.f32"))
    np.ascontiguousarray(s.T0.T.reshape(-1)).tofile(str(tmp_path / "t0.f64"))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "poses.f32"), str(len(s.frames)), str(tmp_path / "points.f32"),
                        str(len(s.points)), str(tmp_path / "t0.f64"), str(ITERATIONS), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    m = re.search(r"align surface ok: residual (\S+) inliers (\S+)", r.stdout)
    T = np.fromfile(str(tmp_path / "pose.f64"), np.float64).reshape(4, 4).T

    vol = tsdf_amd.TSDFVolume(R.SIZE, R.PHYS)
    vol.offset(*R.OFFSET)
    for d, cam in s.frames:
        vol.integrate(d, R.W, R.H, cam)
    Tp, res, inl = vol.align_points(s.points, s.T0, iterations=ITERATIONS)
    vol.close()
    assert np.array_equal(T, Tp)
    assert np.float32(m.group(1)) == np.float32(res) and float(m.group(2)) == inl
    assert inl * 2 >= len(s.points)
    stages = [(s.points, ITERATIONS)]
    ref = R.chain(oracle, s, stages, s.T0, s.gate, order="f64")[0]
    tol = 8 * R.pose_distance(ref, R.chain(oracle, s, stages, s.T0, s.gate, order="ascending")[0])
    assert tol > 0 and R.pose_distance(T, ref) <= tol
