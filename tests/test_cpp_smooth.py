"""The mesh smoothing through the C++ class surface (libtsdf_host.so: extract_surface_smoothed, write_to_ply): build/test_smooth
(tests/cpp/test_smooth.cpp) meshes the sphere scene of tests/components_ref.py and smooths it on the device, checks itself that the
class surface gives the C ABI's bytes and that bad arguments throw; its dumps must be the CPU reference's (tests/mesh_ref.py,
tests/smooth_ref.py) bit for bit, and the PLY must hold the smoothed mesh."""
import os
import subprocess

import numpy as np
import pytest

from tests import components_ref
from tests import mesh_ref
from tests import smooth_ref as ref
from tests.helpers import assert_same_floats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_smooth")
F32 = np.float32
ITERATIONS = 10


@pytest.mark.gpu
def test_cpp_smoothing_matches_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_smooth missing: run `make cpptest` (build() does)")
    n = components_ref.SCENE_SIZE[0]
    D = components_ref.sphere_scene()
    D.tofile(str(tmp_path / "distances.f32"))
    r = subprocess.run([BIN, str(tmp_path / "distances.f32"), str(n), str(ITERATIONS), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "smooth ok" in r.stdout

    vs = (np.float32(n * 10.0) / np.float32(n),) * 3
    load = lambda name, t: np.fromfile(str(tmp_path / name), t)
    wired = lambda I: mesh_ref.triangles(I).astype(np.int32)
    V, I, _, _ = mesh_ref.indexed(oracle, D, components_ref.SCENE_SIZE, vs, (0.0, 0.0, 0.0))
    assert_same_floats(load("all_vertices.f32", F32).reshape(-1, 3), V, "C++ indexed vertices")
    assert np.array_equal(load("all_triangles.i32", np.int32).reshape(-1, 3), wired(I))

    sV = ref.smooth(V, I, ITERATIONS, 0.5, -0.53)
    assert (len(sV), len(I) // 3) == (4422, 8824) and (sV.view(np.uint32) != V.view(np.uint32)).any(axis=1).sum() > 4000
    assert_same_floats(load("vertices.f32", F32), sV, "C++ smoothed vertices")
    assert np.array_equal(load("triangles.i32", np.int32).reshape(-1, 3), wired(I))
    assert_same_floats(load("normals.f32", F32), ref.vertex_normals(sV, I), "C++ face normals")
    bV, bI, _, _ = mesh_ref.indexed(oracle, D, components_ref.SCENE_SIZE, vs, (0.0, 0.0, 0.0), (0, 0, 0, 24, n, n))
    pins = ref.pinned(bV, bI)
    got = load("box_vertices.f32", F32).reshape(-1, 3)
    assert_same_floats(got, ref.smooth(bV, bI, ITERATIONS, 0.5, -0.53, ref.PIN_BOUNDARY), "C++ box vertices")
    assert pins.sum() == 108 and got[pins].tobytes() == bV[pins].tobytes()
    assert np.array_equal(load("box_triangles.i32", np.int32).reshape(-1, 3), wired(bI))

    # the PLY: the smoothed vertices with normals, faces that index them
    lines = (tmp_path / "smoothed.ply").read_text().split("\n")
    end = lines.index("end_header")
    assert "element vertex %d" % len(sV) in lines[:end] and "element face %d" % (len(I) // 3) in lines[:end]
    faces = np.array([[int(t) for t in line.split()] for line in lines[end + 1 + len(sV):] if line], np.int64)
    assert faces.shape == (len(I) // 3, 4) and np.array_equal(faces[:, 1:], wired(I).astype(np.int64))
