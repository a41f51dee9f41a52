"""Point sets and uploaded volumes shared by tests/test_field_query.py and tests/test_align.py: points of every kind a field read can
go wrong on, and two small volumes that pick one instance each of the kernels' division.  Test infrastructure only (uses oracle/)."""
import numpy as np

from tests import field_ref
from tests.helpers import sphere_tsdf

F = np.float32
SEED = 0x5EEDF1E1
N_RANDOM, N_LATTICE, N_FACE = 1200, 240, 30


class Case:
    pass


def world_for(q, offset):
    """A float32 p with p - offset == q exactly (fp32), or None: the nearest float to q + offset or one of its neighbours."""
    q, offset = F(q), F(offset)
    p = F(q + offset)
    for c in (p, np.nextafter(p, F(np.inf)), np.nextafter(p, F(-np.inf))):
        if F(c - offset) == q:
            return c
    return None


def build_points(geom, mesh, hits, n_random=N_RANDOM, n_lattice=N_LATTICE):
    """-> (points (n, 3) float32, {name: slice}).  geom = (dims, vs, offset) as field_ref.geometry gives it."""
    dims, vs, offset = geom
    rng = np.random.RandomState(SEED & 0x7FFFFFFF)
    mx = np.array(field_ref.bounds(dims, vs), F)
    parts = {}
    # uniform in the box enlarged by 10 %: some are outside
    parts["random"] = (offset + (rng.uniform(-0.05, 1.05, (n_random, 3)) * mx)).astype(F)
    parts["mesh"] = np.asarray(mesh, F).reshape(-1, 3)
    parts["hits"] = np.asarray(hits, F).reshape(-1, 3)
    # voxel centres and exact cell faces: q[a] = k * vs[a] or (k + 0.5) * vs[a] in fp32, k = 0 .. size (size itself: the upper bound)
    lattice = np.empty((n_lattice, 3), F)
    for i in range(n_lattice):
        for a in range(3):
            k = F(rng.randint(0, dims[a] + 1)) + (F(0.5) if rng.randint(2) else F(0))
            q = F(k * vs[a])
            p = world_for(q, offset[a])
            lattice[i, a] = p if p is not None else F(q + offset[a])
    parts["lattice"] = lattice
    # within one voxel of each of the six faces, well inside along the other two axes: a distance, no gradient
    face = []
    for a in range(3):
        for far in (False, True):
            q = (vs * F(1.5) + rng.uniform(0, 1, (N_FACE, 3)) * (mx - vs * F(3))).astype(F)
            t = rng.uniform(0.02, 0.98, N_FACE).astype(F) * vs[a]
            q[:, a] = (mx[a] - vs[a]) + t if far else t
            face.append((q + offset).astype(F))
    parts["faces"] = np.concatenate(face)
    # the exact upper bound per axis (invalid), NaN, both infinities, -0.0 as a coordinate
    inside = (offset + mx * F(0.5)).astype(F)
    special = []
    for a in range(3):
        p = world_for(mx[a], offset[a])
        for v in (p if p is not None else F(mx[a] + offset[a]), F(np.nan), F(np.inf), F(-np.inf), F(-0.0)):
            s = inside.copy()
            s[a] = v
            special.append(s)
    parts["special"] = np.array(special, F)
    out, where, at = [], {}, 0
    for name, p in parts.items():
        out.append(p)
        where[name] = slice(at, at + len(p))
        at += len(p)
    return np.concatenate(out).astype(F), where


# ---- both instances of the division -----------------------------------------------------------------------------------------------
# The fused scenes of both suites have one geometry each, so they run one of a kernel's two division instances.  Two small volumes that differ in the
# voxel edge alone: the proof of the fast division fails for an edge below 1 (tests/test_fuse_sweep.py) and passes for 3.  24 x 20 x 28
# voxels (non-cubic, x no multiple of 64), an offset, filled by upload: a sphere's distances and counts in a shell around it.
DIV_DIMS, DIV_EDGES, DIV_OFFSET_VOXELS = (24, 20, 28), (0.75, 3.0), (-10.5, 5.25, 14.0)
DIV_RADIUS, DIV_SHELL = 8.0, 3.0       # in voxels; the sphere's centre is voxel corner (14, 14, 14): the y = 20 face cuts the shell


def division_case(O, edge):
    """The uploaded volume of voxel edge `edge` on the CPU: geometry, arrays, points of every kind and the reference's answers, with
    what keeps a comparison against them from passing on nothing asserted on the reference alone."""
    c = Case()
    c.dims, c.phys = DIV_DIMS, tuple(n * edge for n in DIV_DIMS)
    c.offset = tuple(v * edge for v in DIV_OFFSET_VOXELS)
    ov = O.Volume(c.dims, c.phys)
    ov.offset(*c.offset)
    c.geom = field_ref.geometry(ov)
    assert all(v == F(edge) for v in c.geom[1])
    nx, ny, nz = c.dims
    cube = sphere_tsdf(O, nz, nz * edge, DIV_RADIUS * edge).reshape(nz, nz, nz)       # (z, y, x), cropped to the grid
    c.dist = np.ascontiguousarray(cube[:, :ny, :nx]).reshape(-1)
    idx = np.arange(nz, dtype=np.float64) + 0.5 - nz / 2
    r = np.sqrt(idx[:, None, None] ** 2 + idx[None, :ny, None] ** 2 + idx[None, None, :nx] ** 2)
    near = np.abs(r - DIV_RADIUS) < DIV_SHELL
    c.weight = np.where(near, 1 + (np.arange(r.size).reshape(r.shape) % 7), 0).astype(F).reshape(-1)
    rng = np.random.RandomState(int(edge * 100))
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[:, 1] = -np.abs(d[:, 1])                                                       # (the half that the y face does not cut)
    shell = (nz / 2 + d * (DIV_RADIUS + rng.uniform(-2.5, 2.5, (200, 1)))) * edge + c.geom[2]
    c.points, c.where = build_points(c.geom, shell, np.empty((0, 3), F), n_random=300, n_lattice=120)
    c.ref_d, c.ref_g, c.ref_w = field_ref.sample(O, c.geom, c.dist, c.weight, c.points)
    c.ref_u = field_ref.unit_rows(c.ref_g)
    ok, has_g = ~np.isnan(c.ref_d), ~np.isnan(c.ref_g).any(axis=1)
    assert has_g.sum() >= 50 and (ok & ~has_g).sum() >= 50
    assert (c.ref_w[ok] == 0).sum() >= 50 and (c.ref_w > 0).sum() >= 50
    assert (~ok).sum() >= 50 and np.isnan(c.points).any()
    for a in (c.dist, c.weight, c.points, c.ref_d, c.ref_g, c.ref_u, c.ref_w):
        a.setflags(write=False)
    return c


def division_volume(c, proved):
    import tsdf_amd
    """c's GPU twin; `proved`: whether this edge's fast division must have passed its proof -- which instance the kernels run."""
    vol = tsdf_amd.TSDFVolume(c.dims, c.phys)
    vol.offset(*c.offset)
    vol.set_distance_data(c.dist)
    vol.set_weight_data(c.weight)
    assert vol.info().fast_division_verified == proved
    return vol
