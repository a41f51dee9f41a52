"""Field queries through the C++ class surface (libtsdf_host.so: TSDFVolume::sample_field, extract_surface with normals, write_to_ply
with normals, GPURaycaster::raycast_gradient_normals): build/test_field (tests/cpp/test_field.cpp) fuses three frames on a 64^3
volume, samples the points it is given, extracts the surface with normals and writes a PLY; its dumps must be the CPU reference's
(tests/field_ref.py) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import field_ref
from tests.helpers import H, W, assert_same_floats
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_field")
F32 = np.float32


@pytest.mark.gpu
def test_cpp_field_queries_match_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_field missing: run `make cpptest` (build() does)")
    n, frames = 64, 3
    fr = [synth.depth_frame(i * 9, 40, seed=0x5EEDF1E2) for i in range(frames)]
    np.concatenate([d.reshape(-1) for d, _ in fr]).astype(np.uint16).tofile(str(tmp_path / "frames.u16"))
    np.concatenate([cam.pose().astype(F32).reshape(-1) for _, cam in fr]).tofile(str(tmp_path / "poses.f32"))
    rng = np.random.RandomState(0xF1E2)
    pts = rng.uniform(-150.0, 3150.0, (1500, 3)).astype(F32)           # the box enlarged by 5 %: some are outside
    pts = np.concatenate([pts, np.array([[np.nan, 1500, 1500], [1500, np.inf, 1500], [3000, 1500, 1500], [-0.0, 1500, 1500],
                                         [1500, 1500, 2999.9998], [23.4375, 1500, 1500], [1500, 46.875, 1500]], F32)])
    pts.tofile(str(tmp_path / "points.f32"))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "poses.f32"), str(frames), str(n), str(tmp_path / "points.f32"),
                        str(len(pts)), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "field surface ok" in r.stdout

    ov = oracle.Volume((n,) * 3, (3000.0,) * 3)
    for d, cam in fr:
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    geom = field_ref.geometry(ov)
    rd, rg, rw = field_ref.sample(oracle, geom, ov.dist, ov.weight, pts)
    assert (~np.isnan(rg).any(axis=1)).sum() >= 300 and np.isnan(rd).sum() >= 50 and (rw > 0).sum() >= 100
    load = lambda name: np.fromfile(str(tmp_path / name), F32)
    assert_same_floats(load("distances.f32"), rd, "C++ distances")
    assert_same_floats(load("gradients.f32"), rg, "C++ gradients")
    assert_same_floats(load("unit_gradients.f32"), field_ref.unit_rows(rg), "C++ unit gradients")
    assert_same_floats(load("weights.f32"), rw, "C++ weights")

    # the surface: the oracle's vertices, the reference's unit gradient at (every tenth of) them
    V, N = load("vertices.f32").reshape(-1, 3), load("normals.f32").reshape(-1, 3)
    assert len(V) >= 3000 and N.shape == V.shape
    assert_same_floats(V, oracle.marching_cubes(ov.dist, (n,) * 3, ov.voxel_size(), ov.offset(), nthreads=oracle.max_threads()),
                       "C++ mesh vertices")
    _, ru, _ = field_ref.sample(oracle, geom, ov.dist, ov.weight, V[::10], unit_gradient=True)
    assert (~np.isnan(ru).any(axis=1)).sum() >= 200
    assert_same_floats(N[::10], ru, "C++ mesh normals")

    # the PLY: nx ny nz after z and before the faces, one normal per vertex, values printed like the coordinates
    lines = (tmp_path / "mesh.ply").read_text().split("\n")
    end = lines.index("end_header")
    assert lines[:end] == ["ply", "format ascii 1.0", "element vertex %d" % len(V), "property float x", "property float y",
                           "property float z", "property float nx", "property float ny", "property float nz",
                           "element face %d" % (len(V) // 3), "property list uchar int vertex_indices"]
    body = lines[end + 1:end + 1 + len(V)]
    rows = np.array([[float(t) for t in line.split()] for line in body], np.float64)
    assert rows.shape == (len(V), 6)
    with np.errstate(invalid="ignore"):
        close = np.isclose(rows, np.concatenate([V, N], axis=1).astype(np.float64), rtol=1e-5, atol=0, equal_nan=True)   # six significant digits
    assert close.all()
    assert lines[end + 1 + len(V)].startswith("3 ") and len(lines[end + 1 + len(V):-1]) == len(V) // 3
