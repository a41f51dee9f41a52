"""Ray queries through the C++ class surface (libtsdf_host.so: TSDFVolume::cast_rays): build/test_rays (tests/cpp/test_rays.cpp) fuses
three frames on a 64^3 volume, casts the rays it is given -- without and with a range limit -- and the pixel rays of its camera
against GPURaycaster::raycast; its dumps must be the CPU reference's (tests/ray_ref.py) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import ray_ref
from tests.helpers import H, W, assert_same_floats
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_rays")
F32 = np.float32


@pytest.mark.gpu
def test_cpp_ray_queries_match_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_rays missing: run `make cpptest` (build() does)")
    n, frames = 64, 3
    fr = [synth.depth_frame(i * 9, 40, seed=0x5EEDF1E2) for i in range(frames)]
    np.concatenate([d.reshape(-1) for d, _ in fr]).astype(np.uint16).tofile(str(tmp_path / "frames.u16"))
    np.concatenate([cam.pose().astype(F32).reshape(-1) for _, cam in fr]).tofile(str(tmp_path / "poses.f32"))
    rng = np.random.RandomState(0xF1E3)
    count = 1101
    o = rng.uniform(60.0, 2940.0, (count, 3)).astype(F32)
    d = rng.normal(size=(count, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.5, 2.0, (count, 1))).astype(F32)
    o[-4:] = [[np.nan, 1500, 1500], [1500, 1500, 1500], [-500, 1500, 1500], [1500, 3000, 1500]]
    d[-4:] = [[1, 0, 0], [0, -0.0, 0], [1, 0, -0.0], [0.3, -1, 0.2]]

    ov = oracle.Volume((n,) * 3, (3000.0,) * 3)
    for depth, cam in fr:
        ov.integrate(depth, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    ref = ray_ref.cast(oracle, ov, o, d, normals=True)
    hits = ~np.isnan(ref[1])
    assert hits.sum() >= 200 and (~hits).sum() >= 200 and (~np.isnan(ref[2]).any(axis=1)).sum() >= 100
    # a limit per ray: around the hit's own parameter, so that both outcomes occur; NaN and +inf among them
    m = np.where(hits, ref[1] * rng.choice([0.5, 1.0, 2.0], count).astype(F32), F32(1000)).astype(F32)
    m[::50] = np.nan
    m[1::50] = np.inf
    lim = ray_ref.limit(*ref, m)
    assert (hits & np.isnan(lim[1])).sum() >= 50 and (~np.isnan(lim[1])).sum() >= 100

    for a, name in ((o, "origins.f32"), (d, "directions.f32"), (m, "t_max.f32")):
        a.tofile(str(tmp_path / name))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "poses.f32"), str(frames), str(n), str(tmp_path / "origins.f32"),
                        str(tmp_path / "directions.f32"), str(tmp_path / "t_max.f32"), str(count), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "ray surface ok" in r.stdout

    load = lambda name: np.fromfile(str(tmp_path / name), F32)
    assert_same_floats(load("points.f32"), ref[0], "C++ points")
    assert_same_floats(load("t.f32"), ref[1], "C++ t")
    assert_same_floats(load("normals.f32"), ref[2], "C++ normals")
    assert_same_floats(load("points_lim.f32"), lim[0], "C++ points under the limit")
    assert_same_floats(load("t_lim.f32"), lim[1], "C++ t under the limit")
    assert_same_floats(load("normals_lim.f32"), lim[2], "C++ normals under the limit")
