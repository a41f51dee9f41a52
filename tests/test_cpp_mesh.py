"""The indexed mesh through the C++ class surface (libtsdf_host.so: extract_surface_indexed, write_to_ply): build/test_mesh
(tests/cpp/test_mesh.cpp) fuses three colour frames on a 64^3 volume, extracts the indexed mesh with normals and colours, checks it
against extract_surface's soup and writes a PLY; its dumps must be the CPU reference's (tests/mesh_ref.py, tests/field_ref.py,
tests/colour_ref.py) bit for bit, and the PLY must index shared vertices."""
import os
import subprocess

import numpy as np
import pytest

from tests import colour_ref, field_ref, mesh_ref
from tests.helpers import H, W, assert_same_floats
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_mesh")
F32 = np.float32


@pytest.mark.gpu
def test_cpp_indexed_mesh_matches_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_mesh missing: run `make cpptest` (build() does)")
    n, frames = 64, 3
    fr = [synth.depth_frame(i * 9, 40, seed=0x5EEDF1E2) for i in range(frames)]
    rgb = [synth.colour_frame(i * 9, 40, seed=0x5EEDF1E2)[0] for i in range(frames)]
    np.concatenate([d.reshape(-1) for d, _ in fr]).astype(np.uint16).tofile(str(tmp_path / "frames.u16"))
    np.concatenate([c.reshape(-1) for c in rgb]).astype(np.uint8).tofile(str(tmp_path / "colours.u8"))
    np.concatenate([cam.pose().astype(F32).reshape(-1) for _, cam in fr]).tofile(str(tmp_path / "poses.f32"))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "colours.u8"), str(tmp_path / "poses.f32"), str(frames), str(n),
                        str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "indexed mesh ok" in r.stdout

    ov = oracle.Volume((n,) * 3, (3000.0,) * 3)
    geom = ((n, n, n), np.asarray(ov.voxel_size(), F32), np.zeros(3, F32), np.zeros(3, F32), F32(ov.truncation_distance()))
    colour = np.zeros(n ** 3, np.uint32)
    for (d, cam), c in zip(fr, rgb):
        colour, _, _ = colour_ref.integrate_colour(oracle, colour, geom, d, c, W, H, cam)
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    V, I, S, _ = mesh_ref.indexed(oracle, ov.dist, (n,) * 3, ov.voxel_size(), ov.offset())
    assert len(V) >= 500 and len(S) >= 3000
    load = lambda name, t: np.fromfile(str(tmp_path / name), t)
    gV, gT = load("vertices.f32", F32).reshape(-1, 3), load("triangles.i32", np.int32).reshape(-1, 3)
    assert_same_floats(gV, V, "C++ vertices")
    assert np.array_equal(gT, mesh_ref.triangles(I).astype(np.int32))
    # normals and colours of (every fifth of) the shared vertices
    _, ru, _ = field_ref.sample(oracle, field_ref.geometry(ov), ov.dist, ov.weight, V[::5], unit_gradient=True)
    gN, gC = load("normals.f32", F32).reshape(-1, 3), load("colours.u8", np.uint8).reshape(-1, 3)
    assert gN.shape == V.shape and gC.shape == V.shape
    assert np.isfinite(ru).all(axis=1).sum() >= 200
    assert_same_floats(gN[::5], ru, "C++ normals")
    rc = colour_ref.sample(colour, geom, V)
    assert rc.any(axis=1).sum() >= 100 and np.array_equal(gC, rc)
    # the box
    box = (3, 5, 7, 40, 41, 42)
    bV, bI, _, _ = mesh_ref.indexed(oracle, ov.dist, (n,) * 3, ov.voxel_size(), ov.offset(), box)
    assert_same_floats(load("box_vertices.f32", F32), bV, "C++ box vertices")
    assert np.array_equal(load("box_triangles.i32", np.int32).reshape(-1, 3), mesh_ref.triangles(bI).astype(np.int32))

    # the PLY: len(V) vertices with normals and colours, len(I) / 3 faces that index SHARED vertices
    lines = (tmp_path / "mesh.ply").read_text().split("\n")
    end = lines.index("end_header")
    assert "element vertex %d" % len(V) in lines[:end] and "element face %d" % (len(I) // 3) in lines[:end]
    body = lines[end + 1:end + 1 + len(V)]
    rows = np.array([[float(t) for t in line.split()] for line in body], np.float64)
    assert rows.shape == (len(V), 9)
    with np.errstate(invalid="ignore"):
        assert np.isclose(rows[:, :3], V.astype(np.float64), rtol=1e-5, atol=0, equal_nan=True).all()   # six significant digits
    assert np.array_equal(rows[:, 6:].astype(np.uint8), rc)
    faces = np.array([[int(t) for t in line.split()] for line in lines[end + 1 + len(V):] if line], np.int64)
    assert faces.shape == (len(I) // 3, 4) and (faces[:, 0] == 3).all()
    assert np.array_equal(faces[:, 1:], mesh_ref.triangles(I).astype(np.int64))
    assert faces[:, 1:].max() == len(V) - 1 and np.bincount(faces[:, 1:].reshape(-1)).max() >= 4        # vertices are shared
