"""The distance field through the C++ class surface (libtsdf_host.so: TSDFVolume::compute_esdf): build/test_esdf
(tests/cpp/test_esdf.cpp) fuses three frames on a 64^3 volume, computes the field as a host array and into a caller's handle, checks
both against the C ABI and the refusals as exceptions; its dumps must be the CPU reference's (tests/esdf_ref.py) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import esdf_ref
from tests.helpers import H, W, assert_same_floats
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_esdf")
F32 = np.float32


@pytest.mark.gpu
def test_cpp_distance_field_matches_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_esdf missing: run `make cpptest` (build() does)")
    n, frames, cap = 64, 3, 250.0
    fr = [synth.depth_frame(i * 9, 40, seed=0x5EEDE5D0) for i in range(frames)]
    np.concatenate([d.reshape(-1) for d, _ in fr]).astype(np.uint16).tofile(str(tmp_path / "frames.u16"))
    np.concatenate([cam.pose().astype(F32).reshape(-1) for _, cam in fr]).tofile(str(tmp_path / "poses.f32"))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "poses.f32"), str(frames), str(n), str(cap), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "distance field ok" in r.stdout

    ov = oracle.Volume((n,) * 3, (3000.0,) * 3)
    for d, cam in fr:
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    site = esdf_ref.sites(ov.dist, ov.weight, (n,) * 3)
    assert site.sum() > 1000 and "%d sites" % site.sum() in r.stdout
    q = esdf_ref.squared(site, (n,) * 3, ov.voxel_size())
    load = lambda name: np.fromfile(str(tmp_path / name), F32)
    assert_same_floats(load("capped.f32"), esdf_ref.finish(q, ov.dist, ov.weight, cap), "C++ capped field")
    assert_same_floats(load("filled.f32"), esdf_ref.finish(q, ov.dist, ov.weight, np.inf, True), "C++ uncapped, filled field")
