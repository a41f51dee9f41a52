"""The mesh components through the C++ class surface (libtsdf_host.so: extract_surface_components, write_to_ply):
build/test_components (tests/cpp/test_components.cpp) meshes the sphere scene of tests/components_ref.py and drops its small pieces
on the device; its dumps must be the CPU reference's (tests/mesh_ref.py, tests/components_ref.py) bit for bit, and the PLY must hold
the two spheres only."""
import os
import subprocess

import numpy as np
import pytest

from tests import components_ref as ref
from tests import mesh_ref
from tests.helpers import assert_same_floats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_components")
F32 = np.float32


@pytest.mark.gpu
def test_cpp_components_match_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_components missing: run `make cpptest` (build() does)")
    n = ref.SCENE_SIZE[0]
    D = ref.sphere_scene()
    D.tofile(str(tmp_path / "distances.f32"))
    r = subprocess.run([BIN, str(tmp_path / "distances.f32"), str(n), str(ref.SCENE_MIN_TRIANGLES), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "components ok" in r.stdout

    vs = (np.float32(n * 10.0) / np.float32(n),) * 3
    load = lambda name, t: np.fromfile(str(tmp_path / name), t)

    def expected(box, keep_largest):
        V, I, _, _ = mesh_ref.indexed(oracle, D, ref.SCENE_SIZE, vs, (0.0, 0.0, 0.0), box)
        L, T, info = ref.label(len(V), I)
        (kV,), kI, _ = ref.filter_mesh(L, T, info, I, [V], ref.SCENE_MIN_TRIANGLES, keep_largest)
        return kV, mesh_ref.triangles(kI).astype(np.int32), info

    kV, kT, info = expected(None, False)
    assert info["n_components"] == 5 and len(kV) > 500
    gV, gT = load("vertices.f32", F32).reshape(-1, 3), load("triangles.i32", np.int32).reshape(-1, 3)
    assert_same_floats(gV, kV, "C++ kept vertices")
    assert np.array_equal(gT, kT)
    oV, oT, _ = expected(None, True)
    assert_same_floats(load("one_vertices.f32", F32), oV, "C++ largest component's vertices")
    assert np.array_equal(load("one_triangles.i32", np.int32).reshape(-1, 3), oT) and len(oT) == info["largest_triangles"]
    bV, bT, _ = expected((2, 2, 2, n // 2 + 8, n - 2, n - 2), False)
    assert len(bV) > 0
    assert_same_floats(load("box_vertices.f32", F32), bV, "C++ box vertices")
    assert np.array_equal(load("box_triangles.i32", np.int32).reshape(-1, 3), bT)
    gN = load("normals.f32", F32).reshape(-1, 3)
    assert gN.shape == kV.shape and np.isfinite(gN).all(axis=1).sum() > len(kV) // 2

    # the PLY: the kept vertices with normals, faces that index them
    lines = (tmp_path / "kept.ply").read_text().split("\n")
    end = lines.index("end_header")
    assert "element vertex %d" % len(kV) in lines[:end] and "element face %d" % len(kT) in lines[:end]
    faces = np.array([[int(t) for t in line.split()] for line in lines[end + 1 + len(kV):] if line], np.int64)
    assert faces.shape == (len(kT), 4) and np.array_equal(faces[:, 1:], kT.astype(np.int64))
