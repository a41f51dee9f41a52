"""The weight cap through the C++ class surface (libtsdf_host.so: TSDFVolume::weight_cap): build/test_weight_cap
(tests/cpp/test_weight_cap.cpp) integrates 20 frames under a cap, checks the largest weight and the std::invalid_argument for 65536
itself, and dumps the volume, which must be the clamped oracle's bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import H, W, assert_same_floats
from tests.weight_cap_ref import oracle_step
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_weight_cap")


@pytest.mark.gpu
def test_cpp_weight_cap_matches_the_clamped_oracle(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_weight_cap missing: run `make cpptest` (build() does)")
    n, F, cap = 64, 20, 15
    fr = [synth.depth_frame(i, 200, seed=0x5EED0A03) for i in range(F)]
    np.concatenate([d.reshape(-1) for d, _ in fr]).astype(np.uint16).tofile(str(tmp_path / "frames.u16"))
    np.concatenate([cam.pose().astype(np.float32).reshape(-1) for _, cam in fr]).tofile(str(tmp_path / "poses.f32"))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "poses.f32"), str(F), str(n), str(cap), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "weight cap surface ok" in r.stdout
    ov = oracle.Volume((n, n, n), (3000, 3000, 3000))
    for d, cam in fr:
        oracle_step(oracle, ov, d, cam, cap)
    assert ov.weight.max() == float(cap)
    assert_same_floats(np.fromfile(str(tmp_path / "weights.f32"), np.float32), ov.weight, "C++ capped weights")
    assert_same_floats(np.fromfile(str(tmp_path / "distances.f32"), np.float32), ov.dist, "C++ capped distances")
