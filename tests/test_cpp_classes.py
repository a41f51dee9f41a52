"""Class fusion through the C++ class surface (libtsdf_host.so: TSDFVolume::enable_classes / integrate_classes / sample_classes /
class_counts, GPURaycaster::raycast_classes): build/test_classes (tests/cpp/test_classes.cpp) fuses 4 frames with and without
confidence, checks the refusals, and dumps the class words, the counts and the classed ray cast, which must be the numpy reference's
and the Python path's bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import classes_ref as R
from tests.helpers import H, W, assert_same_floats
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_classes")


def test_the_program_is_built_and_states_its_usage():
    assert os.path.exists(BIN), "build/test_classes missing: run `make cpptest` (build() does)"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage: test_classes" in r.stderr


@pytest.mark.gpu
def test_cpp_classes_match_the_reference(tmp_path, oracle):
    import tsdf_amd
    if not os.path.exists(BIN):
        pytest.fail("build/test_classes missing: run `make cpptest` (build() does)")
    n, F, seed = 64, 4, 0x5EED0003
    rng = np.random.default_rng(5)
    fr = [synth.depth_frame(i, 200, seed=seed) + (synth.class_frame(i, 200, seed=seed)[0],) for i in range(F)]
    conf = rng.integers(0, 256, size=(F, W * H), dtype=np.uint8)
    np.stack([d for d, _, _ in fr]).tofile(str(tmp_path / "frames.u16"))
    np.stack([k for _, _, k in fr]).tofile(str(tmp_path / "classes.u16"))
    conf.tofile(str(tmp_path / "conf.u8"))
    np.stack([cam.pose().astype(np.float32).reshape(-1) for _, cam, _ in fr]).tofile(str(tmp_path / "poses.f32"))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "classes.u16"), str(tmp_path / "conf.u8"), str(tmp_path / "poses.f32"),
                        str(F), str(n), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "class surface ok" in r.stdout
    gv = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    gv.enable_classes()
    geom = R.geometry(gv)
    want = np.zeros(n ** 3, np.uint32)
    for i, (d, cam, k) in enumerate(fr):
        s = conf[i] if i % 2 == 0 else None
        gv.integrate_classes(d, k, W, H, cam, confidence=s)
        want, _, _ = R.integrate_classes(oracle, want, geom, d, k, s, W, H, cam)
    got = np.fromfile(str(tmp_path / "classes.u32"), np.uint32)
    assert np.array_equal(got, want) and np.array_equal(got, gv.get_class_data())
    assert int((got != 0).sum()) > 1000
    assert np.array_equal(np.fromfile(str(tmp_path / "counts.u64"), np.uint64), R.counts(want, 8, 2))
    V, _, classes, votes = tsdf_amd.GPURaycaster(W, H).raycast_classes(gv, fr[-1][1])
    assert_same_floats(np.fromfile(str(tmp_path / "ray_vertices.f32"), np.float32).reshape(-1, 3), V, "ray vertices")
    assert np.array_equal(np.fromfile(str(tmp_path / "ray_classes.u16"), np.uint16), classes)
    assert np.array_equal(np.fromfile(str(tmp_path / "ray_votes.u16"), np.uint16), votes)
