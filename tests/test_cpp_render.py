"""The mesh renderer through the C++ class surface (libtsdf_host.so: MeshRenderer): build/test_render (tests/cpp/test_render.cpp)
meshes the sphere scene of tests/components_ref.py with normals, renders the handle and its downloaded arrays, checks itself that both
give the same bytes, that culling a closed surface changes no pixel, that a warm handle allocates nothing and that bad arguments throw;
its dumped maps must be the CPU reference's (tests/render_ref.py) of its dumped mesh byte for byte, and the mesh the indexed reference's."""
import os
import subprocess

import numpy as np
import pytest

from tests import components_ref
from tests import mesh_ref
from tests import render_ref as ref
from tests.helpers import assert_same_floats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_render")
F32 = np.float32
W, H = 64, 48


@pytest.mark.gpu
def test_cpp_rendering_matches_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_render missing: run `make cpptest` (build() does)")
    n = components_ref.SCENE_SIZE[0]
    D = components_ref.sphere_scene()
    D.tofile(str(tmp_path / "distances.f32"))
    r = subprocess.run([BIN, str(tmp_path / "distances.f32"), str(n), str(W), str(H), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "render ok" in r.stdout

    load = lambda name, t: np.fromfile(str(tmp_path / name), t)
    vs = (np.float32(n * 10.0) / np.float32(n),) * 3
    V, I, _, _ = mesh_ref.indexed(oracle, D, components_ref.SCENE_SIZE, vs, (0.0, 0.0, 0.0))
    gV, gI, gN = load("vertices.f32", F32).reshape(-1, 3), load("indices.u32", np.uint32), load("normals.f32", F32).reshape(-1, 3)
    assert_same_floats(gV, V, "C++ indexed vertices")
    assert np.array_equal(gI, I)
    inv_pose, k = load("inv_pose.f32", F32), load("k.f32", F32)

    want = ref.render(gV, gI, W, H, inv_pose, k, 100.0, 4000.0, normals=gN)
    # (two spheres of radius 134 and 73 mm about 900 mm away at fx = 64: discs of some 9.5 and 5 pixels' radius, 360 pixels together)
    assert want["info"]["n_pixels_hit"] > 300 and want["info"]["n_dropped"] == 0
    assert ref.same_bytes(load("triangle.u32", np.uint32), want["triangle"])
    assert ref.same_bytes(load("z.f32", F32), want["z"])
    assert ref.same_bytes(load("depth.u16", np.uint16), want["depth"])
    assert ref.same_bytes(load("map_vertices.f32", F32).reshape(-1, 3), want["vertices"])
    assert ref.same_bytes(load("map_normals.f32", F32).reshape(-1, 3), want["normals"])
    counts = load("counts.u64", np.uint64)
    info = want["info"]
    assert [int(c) for c in counts] == [info["n_triangles"], info["n_live"], info["n_dropped"], info["n_large"], info["n_pixels_hit"]]
    faces = ref.render(gV, gI, W, H, inv_pose, k, 100.0, 4000.0)
    assert ref.same_bytes(load("face_normals.f32", F32).reshape(-1, 3), faces["normals"])
    small = ref.render(gV, gI, 37, 29, inv_pose, k, 100.0, 4000.0)
    assert ref.same_bytes(load("small_depth.u16", np.uint16), small["depth"])
    assert ref.same_bytes(load("small_triangle.u32", np.uint32), small["triangle"])
