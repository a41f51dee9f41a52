"""Volume fusion through the C++ class surface (libtsdf_host.so: TSDFVolume::fuse): build/test_fuse (tests/cpp/test_fuse.cpp) fuses two
frames into a 48 x 40 x 36 destination and three into a 40^3 source at another offset, fuses the source into the destination through
the matrix it is given and checks that the refusals throw; its dumps must be the CPU reference's (tests/fuse_ref.py) bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fuse_ref
from tests.helpers import H, W, assert_same_floats
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_fuse")
F32 = np.float32


@pytest.mark.gpu
def test_cpp_fuse_matches_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_fuse missing: run `make cpptest` (build() does)")
    n_dst, n_src = 2, 3
    fr = [synth.depth_frame(i * 7, 40, seed=0x5EEDF05F) for i in range(n_dst + n_src)]
    np.concatenate([d.reshape(-1) for d, _ in fr]).astype(np.uint16).tofile(str(tmp_path / "frames.u16"))
    np.concatenate([cam.pose().astype(F32).reshape(-1) for _, cam in fr]).tofile(str(tmp_path / "poses.f32"))
    m = fuse_ref.rotation((3.0, -1.0, 2.0), 15.0, (350.0, 420.0, -500.0))
    m.tofile(str(tmp_path / "matrix.f32"))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "poses.f32"), str(n_dst), str(n_src),
                        str(tmp_path / "matrix.f32"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    fused = int(re.search(r"fuse surface ok: (\d+) voxels fused", r.stdout).group(1))

    dv, sv = oracle.Volume((48, 40, 36), (3000.0,) * 3), oracle.Volume((40,) * 3, (3000.0,) * 3)
    sv.offset(100.0, -50.0, 80.0)
    for i, (d, cam) in enumerate(fr):
        (dv if i < n_dst else sv).integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    rd, rw, upd = fuse_ref.fuse(oracle, fuse_ref.geometry(dv), dv.g.trunc, dv.dist, dv.weight, fuse_ref.geometry(sv), sv.dist, sv.weight, m)
    assert 0.05 <= upd.mean() <= 0.95
    assert fused == int(upd.sum())
    load = lambda name: np.fromfile(str(tmp_path / name), F32)
    assert_same_floats(load("distances.f32"), rd, "C++ fused distances")
    assert_same_floats(load("weights.f32"), rw, "C++ fused weights")
