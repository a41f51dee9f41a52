"""The mesh simplification through the C++ class surface (libtsdf_host.so: extract_surface_simplified, write_to_ply):
build/test_simplify (tests/cpp/test_simplify.cpp) meshes the sphere scene of tests/components_ref.py and clusters it on the device;
its dumps must be the CPU reference's (tests/mesh_ref.py, tests/simplify_ref.py) bit for bit, and the PLY must hold the simplified mesh."""
import os
import subprocess

import numpy as np
import pytest

from tests import components_ref
from tests import mesh_ref
from tests import simplify_ref as ref
from tests.helpers import assert_same_floats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_simplify")
F32 = np.float32
CELL = 20.0


@pytest.mark.gpu
def test_cpp_simplification_matches_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_simplify missing: run `make cpptest` (build() does)")
    n = components_ref.SCENE_SIZE[0]
    D = components_ref.sphere_scene()
    D.tofile(str(tmp_path / "distances.f32"))
    r = subprocess.run([BIN, str(tmp_path / "distances.f32"), str(n), str(CELL), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "simplify ok" in r.stdout

    vs = (np.float32(n * 10.0) / np.float32(n),) * 3
    load = lambda name, t: np.fromfile(str(tmp_path / name), t)
    wired = lambda I: mesh_ref.triangles(I).astype(np.int32)
    V, I, _, _ = mesh_ref.indexed(oracle, D, components_ref.SCENE_SIZE, vs, (0.0, 0.0, 0.0))
    aV, aN = load("all_vertices.f32", F32).reshape(-1, 3), load("all_normals.f32", F32).reshape(-1, 3)
    assert_same_floats(aV, V, "C++ indexed vertices")
    assert np.array_equal(load("all_triangles.i32", np.int32).reshape(-1, 3), wired(I))

    sV, sI, sN, _, _ = ref.simplify(V, I, CELL, aN)                   # (the normals are the device's own: the field's gradient)
    assert (len(sV), len(sI) // 3) == (871, 1728)
    assert_same_floats(load("vertices.f32", F32), sV, "C++ simplified vertices")
    assert np.array_equal(load("triangles.i32", np.int32).reshape(-1, 3), wired(sI))
    assert_same_floats(load("normals.f32", F32), sN, "C++ simplified normals")
    wV, wI, _, _, _ = ref.simplify(V, I, 2.0 ** -8)
    assert (len(wV), len(wI) // 3) == (4410, 8800)
    assert_same_floats(load("weld_vertices.f32", F32), wV, "C++ welded vertices")
    assert np.array_equal(load("weld_triangles.i32", np.int32).reshape(-1, 3), wired(wI))
    bV, bI, _, _ = mesh_ref.indexed(oracle, D, components_ref.SCENE_SIZE, vs, (0.0, 0.0, 0.0), (2, 2, 2, n // 2 + 8, n - 2, n - 2))
    bV, bI, _, _, _ = ref.simplify(bV, bI, CELL)
    assert len(bV) > 100
    assert_same_floats(load("box_vertices.f32", F32), bV, "C++ box vertices")
    assert np.array_equal(load("box_triangles.i32", np.int32).reshape(-1, 3), wired(bI))

    # the PLY: the simplified vertices with normals, faces that index them
    lines = (tmp_path / "simplified.ply").read_text().split("\n")
    end = lines.index("end_header")
    assert "element vertex %d" % len(sV) in lines[:end] and "element face %d" % (len(sI) // 3) in lines[:end]
    faces = np.array([[int(t) for t in line.split()] for line in lines[end + 1 + len(sV):] if line], np.int64)
    assert faces.shape == (len(sI) // 3, 4) and np.array_equal(faces[:, 1:], wired(sI).astype(np.int64))
