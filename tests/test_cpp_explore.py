"""The exploration queries through the C++ class surface (libtsdf_host.so: TSDFVolume::find_frontiers, TSDFVolume::Explorer,
TSDFVolume::view_gain): build/test_explore (tests/cpp/test_explore.cpp) fuses three frames on a 48^3 volume, finds and clusters the
frontiers, walks a fan of rays, checks the class against the C ABI and the refusals as exceptions; what it prints and dumps must be
the CPU reference's (tests/explore_ref.py), integer for integer."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import explore_ref
from tests.helpers import H, W
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_explore")
F32 = np.float32


@pytest.mark.gpu
def test_cpp_exploration_matches_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_explore missing: run `make cpptest` (build() does)")
    n, frames, n_rays = 48, 3, 96
    size = (n,) * 3
    fr = [synth.depth_frame(i * 9, 40, seed=0x5EEDE5D0) for i in range(frames)]
    np.concatenate([d.reshape(-1) for d, _ in fr]).astype(np.uint16).tofile(str(tmp_path / "frames.u16"))
    np.concatenate([cam.pose().astype(F32).reshape(-1) for _, cam in fr]).tofile(str(tmp_path / "poses.f32"))
    rng = np.random.default_rng(48)
    rays = np.concatenate([rng.uniform(-500.0, 3500.0, (n_rays, 3)), rng.normal(size=(n_rays, 3))], axis=1).astype(F32)
    rays.tofile(str(tmp_path / "rays.f32"))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "poses.f32"), str(frames), str(n), str(tmp_path / "rays.f32"),
                        str(n_rays), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "exploration ok" in r.stdout

    ov = oracle.Volume(size, (3000.0,) * 3)
    for d, cam in fr:
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    ids, counts = explore_ref.frontiers(ov.dist, ov.weight, size)
    labels, rows, n_clusters = explore_ref.clusters(ids, size, 26, 2)
    state = explore_ref.states(ov.dist, ov.weight)
    gain, unknown, free, stop, _ = explore_ref.view_gain(state, size, ov.voxel_size(), (0.0, 0.0, 0.0), rays[:, :3], rays[:, 3:])
    half = explore_ref.view_gain(state, size, ov.voxel_size(), (0.0, 0.0, 0.0), rays[:n_rays // 2, :3], rays[:n_rays // 2, 3:])[0]
    assert len(ids) > 100 and gain > 0 and (stop == 2).any() and (stop == 1).any()
    printed = [int(v) for v in re.findall(r"\d+", r.stdout.split("exploration ok:")[1])]
    assert printed == [counts["n_unknown"], counts["n_free"], counts["n_occupied"], len(ids), int(ids[0]), int(ids[-1]), n_clusters, len(rows),
                       gain, half], r.stdout
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    assert np.array_equal(load("voxels.u32", np.uint32), ids)
    assert np.array_equal(load("labels.u32", np.uint32), labels)
    assert load("clusters.bin", explore_ref.CLUSTER_DTYPE).tobytes() == rows.tobytes()
    assert np.array_equal(load("unknown.u32", np.uint32), unknown)
    assert np.array_equal(load("free.u32", np.uint32), free)
    assert np.array_equal(load("stop.u8", np.uint8), stop)
