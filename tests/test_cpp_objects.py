"""The class objects through the C++ class surface (libtsdf_host.so: TSDFVolume::find_objects, TSDFVolume::Objects): build/test_objects
(tests/cpp/test_objects.cpp) checks a hand-made class field against values worked out in the file, fuses three frames with their class
frames on a 48^3 volume, finds the objects of two of the three classes, looks points up, checks the class against the C ABI and the
refusals as exceptions; what it dumps must be the CPU reference's (tests/objects_ref.py) on the class words it dumps, byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import objects_ref
from tests.helpers import H, W
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_objects")
F32 = np.float32


@pytest.mark.gpu
def test_cpp_objects_match_the_reference(tmp_path):
    if not os.path.exists(BIN):
        pytest.fail("build/test_objects missing: run `make cpptest` (build() does)")
    n, frames, n_points = 48, 3, 2000
    size = (n,) * 3
    fr = [synth.depth_frame(i * 9, 40, seed=0x5EED0003) for i in range(frames)]
    kl = [synth.class_frame(i * 9, 40, seed=0x5EED0003)[0] for i in range(frames)]
    assert fr[0][0].size == W * H
    np.concatenate([d.reshape(-1) for d, _ in fr]).astype(np.uint16).tofile(str(tmp_path / "frames.u16"))
    np.concatenate([k.reshape(-1) for k in kl]).astype(np.uint16).tofile(str(tmp_path / "classes.u16"))
    np.concatenate([cam.pose().astype(F32).reshape(-1) for _, cam in fr]).tofile(str(tmp_path / "poses.f32"))
    rng = np.random.default_rng(48)
    points = rng.uniform(-100.0, 3100.0, (n_points, 3)).astype(F32)
    points[:3] = np.nan
    points.tofile(str(tmp_path / "points.f32"))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "classes.u16"), str(tmp_path / "poses.f32"), str(frames), str(n),
                        str(tmp_path / "points.f32"), str(n_points), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "class objects ok" in r.stdout

    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    words = load("classes.u32", np.uint32)
    assert words.size == n ** 3
    ids, L, rows, n_objects = objects_ref.find(words, size, 2, [0, 1, 0, 1], 26, 4)
    assert len(ids) > 100 and len(rows) >= 1 and set(rows["class_id"].tolist()) <= {1, 3}
    printed = [int(v) for v in re.findall(r"\d+", r.stdout.split("class objects ok:")[1])]
    assert printed == [len(ids), n_objects, len(rows)], r.stdout
    assert np.array_equal(load("voxels.u32", np.uint32), ids)
    assert np.array_equal(load("labels.u32", np.uint32), L)
    assert load("objects.bin", objects_ref.OBJECT_DTYPE).tobytes() == rows.tobytes()
    vs = (3000.0 / n,) * 3
    want = objects_ref.lookup(points, ids, L, rows, size, vs, (0.0,) * 3, (0.0,) * 3)
    got = load("lookup.u32", np.uint32)
    assert np.array_equal(got, want) and (got[:3] == objects_ref.NONE).all() and (got != objects_ref.NONE).any()
