"""Weighted integration through the C++ class surface (libtsdf_host.so: TSDFVolume::integrate_weighted, TSDFVolume::depth_weights):
build/test_weighted (tests/cpp/test_weighted.cpp) computes both models' weights of 4 frames, fuses them, checks the refusals and the
storage, and dumps the weights and the volume, which must be the numpy reference's bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import weighted_ref as R
from tests.helpers import H, W, assert_same_floats
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_weighted")


def test_the_program_is_built_and_states_its_usage():
    assert os.path.exists(BIN), "build/test_weighted missing: run `make cpptest` (build() does)"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage: test_weighted" in r.stderr


@pytest.mark.gpu
def test_cpp_weighted_matches_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_weighted missing: run `make cpptest` (build() does)")
    n, F, flags, z_ref = 64, 4, 3, 2400.0
    fr = [synth.depth_frame(i, 200, seed=0x5EED0C04) for i in range(F)]
    np.concatenate([d.reshape(-1) for d, _ in fr]).astype(np.uint16).tofile(str(tmp_path / "frames.u16"))
    np.concatenate([cam.pose().astype(np.float32).reshape(-1) for _, cam in fr]).tofile(str(tmp_path / "poses.f32"))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "poses.f32"), str(F), str(n), str(flags), str(z_ref), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "weighted surface ok" in r.stdout
    ov = oracle.Volume((n, n, n), (3000, 3000, 3000))
    got_p = np.fromfile(str(tmp_path / "pixel_weights.f32"), np.float32).reshape(F, H * W)
    for i, (d, cam) in enumerate(fr):
        p = R.depth_weights(d, W, H, cam.kinv(), flags, z_ref).reshape(-1)
        assert_same_floats(got_p[i], p, "C++ depth_weights, frame %d" % i)
        assert R.integrate(oracle, ov, d, p, cam)[0] > 1000
    assert_same_floats(np.fromfile(str(tmp_path / "weights.f32"), np.float32), ov.weight, "C++ weighted weights")
    assert_same_floats(np.fromfile(str(tmp_path / "distances.f32"), np.float32), ov.dist, "C++ weighted distances")
