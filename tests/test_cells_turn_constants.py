"""GPU: the cell-parallel cast with a brick's turn reading the view from the workgroup's block in LDS (cast_cells_kernel,
cell_boxes.hpp).  The pixel boxes only bound the pairs that are looked at, so every picture must stay the oracle's, bit for bit, and
the march's (TSDF_RAY_CELLS=0): the forced cell cast (TSDF_RAY_CELLS=2, read once per process: each run is a process of its own)
over a grid with partial and boundary bricks and invalid cell lanes (24 x 20 x 28, a 33 x 17 image) and over 48^3 (64 x 48), from the
six cameras of tests/test_cell_boxes.py; with three workgroups, so that every wave takes many turns and the block has to survive
them; with the bricks in parts; with the list sorted; on the voxel edge that takes the plain-division instance; and through two slabs
and the merge, for the slab instances."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import assert_same_floats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (fractions of the physical size; "near": 4.5 voxels in front of the z = 0 face, looking along it)  K = fx, fy, cx, cy, skew at 640 x 480
CAMERAS = [
    dict(name="standard", at=(0.5, 0.433, -0.2), look=(0.5, 0.467, 0.633), K=(525.0, 525.0, 320.0, 240.0, 0.0), block=1.0),
    dict(name="skew_anisotropic", at=(-0.3, 0.5, 0.3), look=(0.5, 0.467, 0.633), K=(300.0, 800.0, 320.0, 100.0, 40.0), block=1.0),
    dict(name="principal_point_off_image", at=(0.5, 0.433, -0.233), look=(0.3, 0.467, 0.633), K=(525.0, 525.0, -150.0, 240.0, 0.0), block=1.0),
    dict(name="tele", at=(0.5, 0.433, -0.833), look=(0.5, 0.467, 0.633), K=(2500.0, 2500.0, 320.0, 240.0, 0.0), block=1.0),
    dict(name="quarter_scale_pose", at=(0.467, 0.433, -0.3), look=(0.5, 0.467, 0.633), K=(525.0, 525.0, 320.0, 240.0, 0.0), block=0.25),
    dict(name="near", at=(0.5, 0.467, None), look=(1.0, 0.467, 0.2), K=(525.0, 525.0, 320.0, 240.0, 0.0), block=1.0),
]
VOLUMES = [
    dict(name="24x20x28", dims=(24, 20, 28), phys=(3000.0, 3000.0, 3000.0), offset=(-300.0, 250.0, 100.0), image=(33, 17), fast_division=True),
    dict(name="48^3", dims=(48, 48, 48), phys=(3000.0, 3000.0, 3000.0), offset=(0.0, 0.0, 0.0), image=(64, 48), fast_division=True),
    # (tests/field_cases.py: the proof of the fast division fails for a voxel edge of 0.75)
    dict(name="24x20x28, edge 0.75", dims=(24, 20, 28), phys=(18.0, 15.0, 21.0), offset=(-7.875, 3.9375, 10.5), image=(33, 17), fast_division=False),
]


def _views(vol):
    """Per camera: pose (camera -> world, column-major 4 x 4) and K (column-major 3 x 3) for the volume's image size."""
    phys, off = np.array(vol["phys"]), np.array(vol["offset"])
    vs_max = float((phys / np.array(vol["dims"])).max())
    w, h = vol["image"]
    out = []
    for cam in CAMERAS:
        at = np.array([cam["at"][0] * phys[0], cam["at"][1] * phys[1], -4.5 * vs_max if cam["at"][2] is None else cam["at"][2] * phys[2]]) + off
        z = np.array(cam["look"]) * phys + off - at
        z /= np.linalg.norm(z)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        pose = np.eye(4)
        pose[:3, :3] = cam["block"] * np.stack([x, np.cross(z, x), z], axis=1)
        pose[:3, 3] = at
        fx, fy, cx, cy, skew = cam["K"]
        k = np.array([[fx * w / 640.0, skew * w / 640.0, cx * w / 640.0], [0.0, fy * h / 480.0, cy * h / 480.0], [0.0, 0.0, 1.0]])
        out.append(dict(pose=[float(a) for a in pose.T.reshape(-1)], k=[float(a) for a in k.T.reshape(-1)]))
    return out


_PROBE = r"""
import sys, json, numpy as np
import tsdf_amd
cfg = json.loads(sys.argv[2])
class M:
    def __init__(self, pose, k, kinv): self.p, self.k_, self.ki = (np.array(a, np.float32) for a in (pose, k, kinv))
    def pose(self): return self.p
    def inverse_pose(self): return self.p      # (not used by the cast)
    def k(self): return self.k_
    def kinv(self): return self.ki
out = {}
for i, vol in enumerate(cfg):
    gv = tsdf_amd.TSDFVolume(tuple(vol["dims"]), tuple(vol["phys"]))
    gv.offset(*vol["offset"])
    assert bool(gv.info().fast_division_verified) == vol["fast_division"]
    # a sphere in the middle and a sheet that leaves the grid through four faces: mixed cells in inner, partial and boundary bricks
    nx, ny, nz = vol["dims"]
    vs, trunc = np.array(vol["phys"], np.float64) / np.array(vol["dims"]), float(gv.truncation_distance())
    x, y, z = ((np.arange(n) + 0.5) * s for n, s in zip((nx, ny, nz), vs))
    cz, cy, cx = np.meshgrid(z, y, x, indexing="ij")
    c, rad = 0.5 * np.array(vol["phys"]), 0.3 * min(vol["phys"])
    sd = np.minimum(np.sqrt((cx - c[0]) ** 2 + (cy - c[1]) ** 2 + (cz - c[2]) ** 2) - rad, 0.8 * vol["phys"][2] - cz + 0.07 * cx)
    dist = np.clip(sd, -trunc, trunc).astype(np.float32).reshape(-1)
    gv.set_distance_data(dist)
    out["D%d" % i] = dist
    for j, v in enumerate(vol["views"]):
        V, N = gv.raycast(vol["image"][0], vol["image"][1], M(v["pose"], v["k"], v["kinv"]))
        out["V%d_%d" % (i, j)], out["N%d_%d" % (i, j)], out["cells%d_%d" % (i, j)] = V, N, np.array(gv.last_raycast_cell_parallel())
np.savez(sys.argv[1], **out)
"""


def _run(script, out, arg, env):
    e = dict(os.environ, **env)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-c", script, out, arg], check=True, env=e, cwd=ROOT, timeout=300)
    return np.load(out)


@pytest.fixture(scope="module")
def scenes(oracle, tmp_path_factory):
    """The volumes with their views, the march's pictures (one process) and the oracle's: computed once, shared, read-only."""
    cfg = []
    for vol in VOLUMES:
        views = _views(vol)
        for v in views:
            v["kinv"] = [float(a) for a in oracle.mat3_inverse(np.array(v["k"], np.float32))]
        cfg.append(dict(vol, views=views))
    march = _run(_PROBE, str(tmp_path_factory.mktemp("march") / "march.npz"), json.dumps(cfg), {"TSDF_RAY_CELLS": "0"})
    ref = {}
    hits = 0
    for i, vol in enumerate(cfg):
        ov = oracle.Volume(tuple(vol["dims"]), tuple(vol["phys"]))
        ov.offset(*vol["offset"])
        ov.set_distance_data(march["D%d" % i])
        for j, v in enumerate(vol["views"]):
            Vo, No = ov.raycast(vol["image"][0], vol["image"][1], np.array(v["pose"], np.float32), np.array(v["kinv"], np.float32), nthreads=oracle.max_threads())
            Vo.setflags(write=False); No.setflags(write=False)
            ref[i, j] = (Vo, No)
            what = "%s, %s, the march" % (vol["name"], CAMERAS[j]["name"])
            assert_same_floats(march["V%d_%d" % (i, j)], Vo, what + ": vertices")
            assert_same_floats(march["N%d_%d" % (i, j)], No, what + ": normals")
            assert not bool(march["cells%d_%d" % (i, j)]), what + ": which kernels ran"
            hits += int((~np.isnan(Vo[:, 0])).sum())
    assert hits > 2000, "the views see too little surface"
    return cfg, march, ref


@pytest.mark.parametrize("env", [
    {},
    {"TSDF_RAY_CELLS_GRID": "3"},       # every wave through many bricks: the block and the rows read from it, turn after turn
    {"TSDF_RAY_CELLS_PAIRS": "64"},     # each brick in many parts
    {"TSDF_RAY_CELLS_SORT": "2"},       # the list front to back
], ids=["plain", "grid3", "pairs64", "sort2"])
def test_forced_cell_cast_is_the_march_and_the_oracle(scenes, tmp_path, env):
    cfg, march, ref = scenes
    got = _run(_PROBE, str(tmp_path / "cells.npz"), json.dumps(cfg), dict(env, TSDF_RAY_CELLS="2"))
    for i, vol in enumerate(cfg):
        assert np.array_equal(got["D%d" % i], march["D%d" % i])
        for j in range(len(vol["views"])):
            what = "%s, %s, %s" % (vol["name"], CAMERAS[j]["name"], env)
            assert bool(got["cells%d_%d" % (i, j)]), what + ": the cell-parallel cast was to run"
            for key, o in (("V", ref[i, j][0]), ("N", ref[i, j][1])):
                assert_same_floats(got["%s%d_%d" % (key, i, j)], o, what + ": %s against the oracle" % key)
                assert_same_floats(got["%s%d_%d" % (key, i, j)], march["%s%d_%d" % (key, i, j)], what + ": %s against the march" % key)


_SLAB_PROBE = r"""
import sys, json, numpy as np, torch
import tsdf_amd
from tsdf_amd import synth
n, (w, h) = 48, json.loads(sys.argv[2])
W, H = synth.WIDTH, synth.HEIGHT
whole = tsdf_amd.TSDFVolume((n, n, n), (3000, 3000, 3000))
slabs = [tsdf_amd.TSDFVolume((n, n, n), (3000, 3000, 3000), slab=s) for s in ((0, 22), (22, 48))]
for i in range(3):
    d, cam = synth.depth_frame(i, 3, seed=77)
    for v in [whole] + slabs:
        v.integrate(d, W, H, cam)
_, cam0 = synth.depth_frame(0, 3, seed=77)
k = np.array(cam0.k(), np.float64).copy()
k[0] *= w / W; k[3] *= w / W; k[6] *= w / W; k[1] *= h / H; k[4] *= h / H; k[7] *= h / H
K = k.reshape(3, 3).T
class M:
    def pose(self): return np.array(cam0.pose(), np.float32)
    def inverse_pose(self): return np.array(cam0.inverse_pose(), np.float32)
    def k(self): return k.astype(np.float32)
    def kinv(self): return np.linalg.inv(K).T.reshape(-1).astype(np.float32)
cam = M()
hits = torch.empty((len(slabs), w * h, 2), dtype=torch.float32, device="cuda")
rc = tsdf_amd.GPURaycaster(w, h)
cells = []
for i, s in enumerate(slabs):
    rc.raycast_slab_device(s, cam, hits[i].data_ptr())
    s.synchronize()
    cells.append(s.last_raycast_cell_parallel())
V, N = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda"), torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
tsdf_amd.merge_hits_normals_device(slabs[0], hits.data_ptr(), len(slabs), w, h, cam, V.data_ptr(), N.data_ptr())
torch.cuda.synchronize()
np.savez(sys.argv[1], D=whole.get_distance_data(), V=V.cpu().numpy(), N=N.cpu().numpy(), cells=np.array(cells), pose=cam.pose(), kinv=cam.kinv())
"""


def test_two_slabs_and_the_merge_through_the_forced_cell_cast(oracle, tmp_path):
    """cast_cells_kernel<SLAB = true>: each slab's records by the cell-parallel cast, merged: the whole volume's picture."""
    n, (w, h) = 48, (64, 48)
    got = _run(_SLAB_PROBE, str(tmp_path / "slabs.npz"), json.dumps([w, h]), {"TSDF_RAY_CELLS": "2"})
    assert got["cells"].all(), "the cell-parallel cast was to run on both slabs"
    ov = oracle.Volume((n, n, n), (3000, 3000, 3000))
    ov.set_distance_data(got["D"])
    Vo, No = ov.raycast(w, h, got["pose"], got["kinv"], nthreads=oracle.max_threads())
    assert (~np.isnan(Vo[:, 0])).sum() > 500
    assert_same_floats(got["V"], Vo, "merged vertices")
    assert_same_floats(got["N"], No, "merged normals")
