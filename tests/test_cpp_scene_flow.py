"""Scene flow through the C++ class surface (libtsdf_host.so: process_frames with the reference's signature, TSDFVolume::apply_scene_flow):
build/test_scene_flow (tests/cpp/test_scene_flow.cpp) checks that process_frames leaves, through tsdf_volume_get_deformation_planes, the
nodes the C ABI call leaves; its dump must be the CPU reference's (tests/scene_flow_ref.py) bit for bit, after one frame and after two."""
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_ref, scene_flow_cases as cases, scene_flow_ref as ref
from tests.helpers import assert_same_floats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_scene_flow")
F32 = np.float32


@pytest.mark.gpu
def test_cpp_process_frames_matches_the_c_abi_and_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_scene_flow missing: run `make cpptest` (build() does)")
    size, voxel, offset = (20, 18, 15), 10.0, (-100.0, -90.0, 300.0)
    centre, radius, position = (3.0, -2.0, 372.0), 52.0, (4.0, -6.0, 20.0)
    D = cases.sphere_field(size, voxel, offset, centre, radius, 19.0)
    depth = cases.sphere_depth(position, centre, radius)
    flow = cases.random_flow(77)
    D.tofile(str(tmp_path / "dist.f32"))
    depth.tofile(str(tmp_path / "depth.u16"))
    flow.tofile(str(tmp_path / "flow.f32"))
    args = [BIN, str(tmp_path / "dist.f32")] + [str(v) for v in size] + [str(voxel)] + [str(o) for o in offset] + \
           [str(tmp_path / "depth.u16"), str(tmp_path / "flow.f32"), str(cases.WIDTH), str(cases.HEIGHT)] + [str(p) for p in position] + [str(tmp_path)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "scene flow ok" in r.stdout

    cam = np.fromfile(str(tmp_path / "camera.f32"), F32)
    pose, inv_pose, k, kinv = cam[:16], cam[16:32], cam[32:41], cam[41:50]
    vs = (F32(size[0] * voxel) / F32(size[0]),) * 3
    V, I, _, keys = mesh_ref.indexed(oracle, D, size, vs, offset)
    pix, _ = ref.correspond(oracle, V, depth, flow, cases.WIDTH, cases.HEIGHT, pose, inv_pose, k, kinv, 10.0)
    assert (pix != ref.NONE).sum() >= 100 and (pix == ref.NONE).sum() >= 100
    n = size[0] * size[1] * size[2]
    z, y, x = np.meshgrid(*[np.arange(s, dtype=F32) + F32(0.5) for s in size[::-1]], indexing="ij")
    nodes = np.zeros((n, 6), F32)
    nodes[:, 0], nodes[:, 1], nodes[:, 2] = (x * vs[0]).reshape(-1), (y * vs[1]).reshape(-1), (z * vs[2]).reshape(-1)   # (the offset at clear is 0)
    once, moved = ref.apply(nodes, keys, I, pix, flow, size)
    assert ("%d vertices, %d correspondences, %d nodes" % (len(V), (pix != ref.NONE).sum(), moved)) in r.stdout
    assert_same_floats(np.fromfile(str(tmp_path / "nodes.f32"), F32), once, "process_frames")
    twice, _ = ref.apply(once, keys, I, pix, flow, size)
    assert_same_floats(np.fromfile(str(tmp_path / "nodes_twice.f32"), F32), twice, "a second frame")
