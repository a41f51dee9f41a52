"""GPU: the cell-parallel cast with every sample given to ONE dual cell by two exact comparisons per axis (cell_owns, cell_owner.hpp;
cast_cells_kernel no longer calls the reference's full interpolation for samples near a cell face).  Every picture must stay the
oracle's and the march's (TSDF_RAY_CELLS=0), bit for bit, NaN patterns included; the forced cell cast (TSDF_RAY_CELLS=2) and the march
each run in a process of their own (the knob is read once per process).

The shapes are the smallest at which ownership can go wrong: 16 x 12 x 20 voxels of 64 mm (a power of two: every product exact) and
33 x 29 x 31 with inexact, anisotropic edges (partial bricks on every axis); images of 48 x 40 and 13 x 9; fields whose zero crossings
and samples lie on dual-cell faces -- a plane at constant z exactly on a face (the voxels of one plane are exactly 0), the same plane
tilted by one voxel over the grid, a sphere; three cameras -- axis-aligned with its origin on the face lattice, so that the image's
middle row and column of rays run INSIDE a face (a direction component of exactly 0), yawed about y from a point on a y face (its
middle row still inside that face, x and z oblique), and a look-at camera with anisotropic intrinsics.  And two slabs that meet on the
plane's own face: each slab's records against the oracle's for the samples that slab owns, and the merge against the whole volume's cast.

So that no case passes without meeting a face, the CPU first counts, from the oracle's ray set-up (ray_direction_n, ray_box), the
table T[k + 1] = T[k] + step and the oracle's own count of samples per ray, the samples the reference evaluates within 1e-3 voxel of a
face of a mixed cell: at least 200 per case, at least 20 of them EXACTLY on a face for the lattice-aligned camera."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import assert_same_floats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

GRIDS = [
    dict(name="16x12x20", dims=(16, 12, 20), phys=(1024.0, 768.0, 1280.0)),     # 64 mm voxels
    dict(name="33x29x31", dims=(33, 29, 31), phys=(2000.0, 1900.0, 2100.0)),    # 60.6.., 65.5.., 67.7.. mm
]
FIELDS = ["plane_on_face", "plane_tilted", "sphere"]
IMAGES = [(48, 40), (13, 9)]
CAMERAS = ["lattice_aligned", "yawed_on_a_y_face", "anisotropic_look_at"]
CASES = [(g, f) for g in range(len(GRIDS)) for f in range(len(FIELDS))]
kCellPositive = 1.0e-30


def _field(oracle, grid, kind):
    nx, ny, nz = grid["dims"]
    g = oracle.Volume(grid["dims"], grid["phys"])
    vs, trunc = g.voxel_size().astype(np.float64), g.truncation_distance()
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    jz = nz // 2
    if kind == "plane_on_face":      # zero exactly at the centres of plane jz: the crossing IS the face between the cells jz - 1 and jz
        sd = (jz - iz) * vs[2]
    elif kind == "plane_tilted":     # ... and rising by one voxel from x = 0 to x = X
        sd = (jz - iz) * vs[2] + vs[2] * (ix + 0.5) / nx
    else:
        c, rad = 0.5 * np.array(grid["phys"]), 0.3 * min(grid["phys"])
        sd = np.sqrt((((ix + 0.5) * vs[0] - c[0]) ** 2 + ((iy + 0.5) * vs[1] - c[1]) ** 2 + ((iz + 0.5) * vs[2] - c[2]) ** 2)) - rad
    return np.clip(sd, -trunc, trunc).astype(F).reshape(-1)


def _views(oracle, grid):
    """Per camera and image: pose (camera -> world, column-major 4 x 4), K and its inverse (column-major 3 x 3)."""
    phys = np.array(grid["phys"])
    vs = oracle.Volume(grid["dims"], grid["phys"]).voxel_size()
    nx, ny, _ = grid["dims"]
    face_x, face_y = float((F(nx // 2 - 1) + F(0.5)) * vs[0]), float((F(ny // 2) + F(0.5)) * vs[1])   # the products the reference forms
    out = []
    for cam in CAMERAS:
        for w, h in IMAGES:
            f2 = 32.0 if w == 48 else 8.0    # powers of two and an integer principal point: the middle row's rcy is exactly 0
            if cam == "lattice_aligned":
                rot, at = np.eye(3), np.array([face_x, face_y, -0.45 * phys[2]])
                fx, fy, cx, cy = f2, f2, float(w // 2), float(h // 2)
            elif cam == "yawed_on_a_y_face":
                c, s = np.cos(0.35), np.sin(0.35)
                rot, at = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]), np.array([0.15 * phys[0], face_y, -0.4 * phys[2]])
                fx, fy, cx, cy = 1.25 * f2, f2, float(w // 2), float(h // 2)
            else:   # (300, 800, 320, 100) at 640 x 480: tests/test_parity_raycast.py, test_cell_parallel_cast_with_unusual_intrinsics
                at = np.array([-0.17, 0.5, 0.3]) * phys
                z = np.array([0.5, 0.467, 0.633]) * phys - at
                z /= np.linalg.norm(z)
                x = np.cross([0.0, 1.0, 0.0], z)
                x /= np.linalg.norm(x)
                rot = np.stack([x, np.cross(z, x), z], axis=1)
                fx, fy, cx, cy = 300.0 * w / 640.0, 800.0 * h / 480.0, 320.0 * w / 640.0, 100.0 * h / 480.0
            pose = np.eye(4)
            pose[:3, :3], pose[:3, 3] = rot, at
            k = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
            kc = [float(a) for a in k.T.reshape(-1).astype(F)]
            out.append(dict(camera=cam, image=(w, h), pose=[float(a) for a in pose.T.reshape(-1).astype(F)], k=kc,
                            kinv=[float(a) for a in oracle.mat3_inverse(np.array(kc, F))]))
    return out


def _face_samples(oracle, grid, dist, view, sample_count):
    """(samples within 1e-3 voxel of a face of a mixed cell, those exactly on one) among the samples the reference evaluates."""
    nx, ny, nz = grid["dims"]
    g = oracle.Volume(grid["dims"], grid["phys"])
    vs = g.voxel_size()
    w, h = view["image"]
    pose, kinv = np.array(view["pose"], F), np.array(view["kinv"], F)
    origin, rot = pose[12:15], pose[[0, 1, 2, 4, 5, 6, 8, 9, 10]]
    pix = np.stack(np.meshgrid(np.arange(w), np.arange(h), indexing="xy"), axis=-1).reshape(-1, 2)   # row-major pixels, (x, y)
    dirs = oracle.ray_direction_n(pix, rot, kinv)
    smin, smax = np.zeros(3, F), np.array(grid["phys"], F)
    start = np.zeros((w * h, 3), F)
    for i in range(w * h):
        ok, near_t, _ = oracle.ray_box(origin, dirs[i], smin, smax)
        assert ok or sample_count[i] == 0
        start[i] = ((F(near_t) * dirs[i]) + origin) - smin
    step = F(np.float64(F(g.truncation_distance())) * 0.05)
    table = np.zeros(4403, F)
    for k in range(1, len(table)):
        table[k] = table[k - 1] + step
    ray = np.repeat(np.arange(w * h), sample_count)
    k = np.arange(len(ray)) - np.repeat(np.cumsum(sample_count) - sample_count, sample_count)
    p = (table[k][:, None] * dirs[ray]) + start[ray]
    assert p.dtype == F
    d = dist.reshape(nz, ny, nx)
    low = d[:-1, :-1, :-1]
    for dz, dy, dx in ((0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)):
        low = np.fmin(low, d[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx])
    mixed = ~(low > kCellPositive)     # [lz, ly, lx]

    def is_mixed(l):
        ok = np.all((l >= 0) & (l <= np.array([nx, ny, nz]) - 2), axis=1)
        lc = np.clip(l, 0, np.array([nx, ny, nz]) - 2)
        return ok & mixed[lc[:, 2], lc[:, 1], lc[:, 0]]

    f = p.astype(np.float64) / vs.astype(np.float64) - 0.5
    base = np.floor(f).astype(np.int64)
    near, exact = np.zeros(len(p), bool), np.zeros(len(p), bool)
    for a in range(3):
        j = np.rint(f[:, a]).astype(np.int64)
        close = np.abs(f[:, a] - j) <= 1.0e-3
        beside = np.zeros(len(p), bool)
        for side in (j - 1, j):
            l = base.copy()
            l[:, a] = side
            beside |= is_mixed(l)
        near |= close & beside
        exact |= beside & (p[:, a] == ((j.astype(F) + F(0.5)) * vs[a]).astype(F))
    return int(near.sum()), int((near & exact).sum())


_PROBE = r"""
import sys, json, numpy as np
import tsdf_amd
cfg, fields = json.loads(sys.argv[2]), np.load(sys.argv[3])
class M:
    def __init__(self, v): self.p, self.k_, self.ki = (np.array(v[n], np.float32) for n in ("pose", "k", "kinv"))
    def pose(self): return self.p
    def inverse_pose(self): return self.p      # (not used by the cast)
    def k(self): return self.k_
    def kinv(self): return self.ki
out = {}
for gi, grid in enumerate(cfg):
    gv = tsdf_amd.TSDFVolume(tuple(grid["dims"]), tuple(grid["phys"]))
    for fi in range(grid["n_fields"]):
        gv.set_distance_data(fields["D%d_%d" % (gi, fi)])
        for j, v in enumerate(grid["views"]):
            V, N = gv.raycast(v["image"][0], v["image"][1], M(v))
            key = "%d_%d_%d" % (gi, fi, j)
            out["V" + key], out["N" + key], out["cells" + key] = V, N, np.array(gv.last_raycast_cell_parallel())
np.savez(sys.argv[1], **out)
"""


def _run(script, out, args, env):
    e = dict(os.environ, **env)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-c", script, out] + list(args), check=True, env=e, cwd=ROOT, timeout=300)
    return np.load(out)


def build_scenes(oracle):
    """The grids with their views, the fields, the oracle's pictures and the face counts per case: the CPU's part, no GPU."""
    cfg, fields, ref, counts = [], {}, {}, {}
    for gi, grid in enumerate(GRIDS):
        views = _views(oracle, grid)
        cfg.append(dict(grid, views=views, n_fields=len(FIELDS)))
        for fi, kind in enumerate(FIELDS):
            dist = _field(oracle, grid, kind)
            dist.setflags(write=False)
            fields["D%d_%d" % (gi, fi)] = dist
            ov = oracle.Volume(grid["dims"], grid["phys"])
            ov.set_distance_data(dist)
            near = exact = hits = 0
            for j, v in enumerate(views):
                w, h = v["image"]
                Vo, No, st = ov.raycast(w, h, np.array(v["pose"], F), np.array(v["kinv"], F), nthreads=oracle.max_threads(), stats=True)
                Vo.setflags(write=False); No.setflags(write=False)
                ref[gi, fi, j] = (Vo, No)
                n_, e_ = _face_samples(oracle, grid, dist, v, st["sample_count"])
                near += n_
                exact += e_ if v["camera"] == "lattice_aligned" else 0
                hits += int((~np.isnan(Vo[:, 0])).sum())
            counts[gi, fi] = dict(near=near, exact=exact, hits=hits)
    return cfg, fields, ref, counts


@pytest.fixture(scope="module")
def scenes(oracle, tmp_path_factory):
    """build_scenes, then the march's and the forced cell cast's pictures, one process each: computed once, shared, read-only."""
    cfg, fields, ref, counts = build_scenes(oracle)
    for (gi, fi), c in counts.items():
        print("%s, %s: %d samples within 1e-3 voxel of a mixed cell's face, %d exactly on one (lattice-aligned camera), %d hits"
              % (GRIDS[gi]["name"], FIELDS[fi], c["near"], c["exact"], c["hits"]))
        assert c["near"] >= 200 and c["exact"] >= 20 and c["hits"] >= 200, (GRIDS[gi]["name"], FIELDS[fi], c)
    d = tmp_path_factory.mktemp("exact_owner")
    np.savez(str(d / "fields.npz"), **fields)
    march = _run(_PROBE, str(d / "march.npz"), [json.dumps(cfg), str(d / "fields.npz")], {"TSDF_RAY_CELLS": "0"})
    cells = _run(_PROBE, str(d / "cells.npz"), [json.dumps(cfg), str(d / "fields.npz")], {"TSDF_RAY_CELLS": "2"})
    return cfg, ref, march, cells


@pytest.mark.parametrize("gi,fi", CASES, ids=["%s-%s" % (GRIDS[g]["name"], FIELDS[f]) for g, f in CASES])
def test_exact_ownership_is_the_oracle_and_the_march(scenes, gi, fi):
    cfg, ref, march, cells = scenes
    for j, v in enumerate(cfg[gi]["views"]):
        key = "%d_%d_%d" % (gi, fi, j)
        what = "%s, %s, %s, %dx%d" % (GRIDS[gi]["name"], FIELDS[fi], v["camera"], v["image"][0], v["image"][1])
        assert bool(cells["cells" + key]), what + ": the cell-parallel cast was to run"
        assert not bool(march["cells" + key]), what + ": the march was to run"
        for name, o in (("V", ref[gi, fi, j][0]), ("N", ref[gi, fi, j][1])):
            assert_same_floats(march[name + key], o, what + ": the march's %s against the oracle" % name)
            assert_same_floats(cells[name + key], o, what + ": the cell cast's %s against the oracle" % name)
            assert_same_floats(cells[name + key], march[name + key], what + ": the cell cast's %s against the march" % name)


_SLAB_PROBE = r"""
import sys, json, numpy as np, torch
import tsdf_amd
cfg, fields = json.loads(sys.argv[2]), np.load(sys.argv[3])
class M:
    def __init__(self, v): self.p, self.k_, self.ki = (np.array(v[n], np.float32) for n in ("pose", "k", "kinv"))
    def pose(self): return self.p
    def inverse_pose(self): return self.p
    def k(self): return self.k_
    def kinv(self): return self.ki
dims, phys = tuple(cfg["dims"]), tuple(cfg["phys"])
D = fields["D"].reshape(dims[2], -1)
whole = tsdf_amd.TSDFVolume(dims, phys)
whole.set_distance_data(fields["D"])
slabs = [tsdf_amd.TSDFVolume(dims, phys, slab=tuple(s)) for s in cfg["slabs"]]
out = {}
for i, s in enumerate(slabs):
    lo, hi = s.resident_planes()
    s.set_distance_data(np.ascontiguousarray(D[lo:hi]).reshape(-1))
    out["resident%d" % i], out["owned%d" % i] = np.array([lo, hi]), np.array(s.owned_planes())
for j, v in enumerate(cfg["views"]):
    w, h = v["image"]
    cam = M(v)
    rc = tsdf_amd.GPURaycaster(w, h)
    hits = torch.empty((len(slabs), w * h, 2), dtype=torch.float32, device="cuda")
    for i, s in enumerate(slabs):
        rc.raycast_slab_device(s, cam, hits[i].data_ptr())
        s.synchronize()
        out["cells%d_%d" % (j, i)] = np.array(s.last_raycast_cell_parallel())
    V, N = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda"), torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    tsdf_amd.merge_hits_normals_device(slabs[0], hits.data_ptr(), len(slabs), w, h, cam, V.data_ptr(), N.data_ptr())
    torch.cuda.synchronize()
    Vw, Nw = whole.raycast(w, h, cam)
    out["hits%d" % j], out["V%d" % j], out["N%d" % j], out["Vw%d" % j], out["Nw%d" % j] = hits.cpu().numpy().view(np.uint32), V.cpu().numpy(), N.cpu().numpy(), Vw, Nw
np.savez(sys.argv[1], **out)
"""


def test_two_slabs_that_meet_on_the_plane_s_face(oracle, tmp_path):
    """cast_cells_kernel<SLAB = true>: the tilted plane crosses the face on which the two slabs meet (cells of plane 14 are the first
    slab's, of plane 15 the second's), so samples either side of that face, and on it, belong to different ranks.  Each slab's
    records {k, t} are the oracle's for the samples that slab owns; merged they are the whole volume's forced cell cast and the oracle."""
    grid = GRIDS[1]
    nz = grid["dims"][2]
    dist = _field(oracle, grid, "plane_tilted")
    views = [v for v in _views(oracle, grid) if v["image"] == IMAGES[0]]
    cfg = dict(grid, views=views, slabs=[(0, nz // 2), (nz // 2, nz)])
    np.savez(str(tmp_path / "field.npz"), D=dist)
    got = _run(_SLAB_PROBE, str(tmp_path / "slabs.npz"), [json.dumps(cfg), str(tmp_path / "field.npz")], {"TSDF_RAY_CELLS": "2"})
    ov = oracle.Volume(grid["dims"], grid["phys"])
    ov.set_distance_data(dist)
    D = dist.reshape(nz, -1)
    for j, v in enumerate(views):
        w, h = v["image"]
        pose, kinv = np.array(v["pose"], F), np.array(v["kinv"], F)
        what = "%s, %dx%d" % (v["camera"], w, h)
        owned_hits = 0
        for i in range(2):
            assert bool(got["cells%d_%d" % (j, i)]), what + ": the cell-parallel cast was to run on slab %d" % i
            (slo, shi), (lo, hi) = got["resident%d" % i], got["owned%d" % i]
            os_ = oracle.Volume(grid["dims"], grid["phys"], z_store=(int(slo), int(shi)))
            os_.set_distance_data(D[slo:shi])
            ho = os_.raycast_slab(w, h, pose, kinv, (int(lo), int(hi)), nthreads=oracle.max_threads())
            assert np.array_equal(got["hits%d" % j][i], ho), what + ": slab %d records {k, t} differ from the oracle's" % i
            owned_hits += int((ho[:, 0] != 0xffffffff).sum())
        Vo, No = ov.raycast(w, h, pose, kinv, nthreads=oracle.max_threads())
        assert owned_hits >= (~np.isnan(Vo[:, 0])).sum() > 200
        for name, o in (("V", Vo), ("N", No)):
            assert_same_floats(got["%s%d" % (name, j)], o, what + ": merged %s against the oracle" % name)
            assert_same_floats(got["%sw%d" % (name, j)], o, what + ": the whole volume's %s against the oracle" % name)
