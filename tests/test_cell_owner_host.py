"""Which dual cell owns a sample (tsdf_amd/csrc/cell_owner.hpp), on the CPU: tsdf_selftest_cell_owner runs cell_owns -- the two exact
comparisons per axis by which cast_cells_kernel gives every sample to one cell -- beside a restatement of the reference's own choice
of the lower tap (voxel_for_point, centre_of_voxel_at and the clamps, as trilinear() inlines them), with the quotient of voxel_for_point
formed by IEEE division and by the kernels' three-instruction sequence (unverified here: a volume only uses it where it IS the IEEE
quotient, so this asks for more).

* cell_owns is true for exactly the cell the reference chooses: for that cell on all three axes, for its neighbour either side on none
  -- on every point inside the lattice of voxel centres, [0.5 vs, (size - 0.5) vs) per axis, where every lower tap is a cell of the grid;
* a point outside that lattice (the half-voxel shell, where the reference clamps: the shell workgroups' samples) is owned by no cell;
* of the two cells either side of a face exactly one owns a point constructed on or next to it.

Points: every face value (l + 0.5f) * vs and (l + 1.5f) * vs of every cell of every axis, moved by -3 .. +3 ulps, the other two
coordinates at a cell's middle and on a face of their own; and 200 000 random points per grid."""
import numpy as np
import pytest

from tsdf_amd import _capi

F = np.float32
N_RANDOM = 200000
GRIDS = {
    "24x20x28_1000mm": ((24, 20, 28), 1000.0),       # inexact voxel sizes, anisotropic
    "96^3_1000mm": ((96, 96, 96), 1000.0),
    "512^3_3000mm": ((512, 512, 512), 3000.0),       # the benchmark's: 5.859375, exact
    "500x512x300_3000mm": ((500, 512, 300), 3000.0),
}


def _grid(name):
    size, phys = GRIDS[name]
    size = np.array(size, np.uint32)
    vs = (F(phys) / size.astype(F)).astype(F)   # the volume's own division (volume.hip)
    return size, vs


def _selftest(size, vs, points, cells, fast):
    n = len(points)
    points, cells = np.ascontiguousarray(points, F), np.ascontiguousarray(cells, np.uint32)
    owns, lower = np.zeros(n, np.uint8), np.zeros((n, 3), np.int32)
    rc = _capi.lib.tsdf_selftest_cell_owner(size.ctypes.data, vs.ctypes.data, int(fast), n, points.ctypes.data, cells.ctypes.data,
                                            owns.ctypes.data, lower.ctypes.data)
    assert rc == 0
    return owns, lower


def _ulps(x, d):
    x = np.asarray(x, F).copy()
    for _ in range(abs(d)):
        x = np.nextafter(x, F(np.inf) if d > 0 else F(-np.inf))
    return x


def _face_points(size, vs, rng):
    """Per axis: {point, axis, cell index l whose LOWER face the value was built from (l = cells: the upper face of the last cell)}."""
    pts, axes, faces = [], [], []
    for a in range(3):
        n_cells = int(size[a]) - 1                      # cells l = 0 .. size - 2; face j = (j + 0.5f) * vs, j = 0 .. size - 1
        j = np.arange(n_cells + 1, dtype=np.int64)
        face = ((j.astype(F) + F(0.5)) * vs[a]).astype(F)
        also = ((np.arange(n_cells, dtype=np.int64).astype(F) + F(1.5)) * vs[a]).astype(F)   # the upper faces, as the kernel forms them
        assert np.array_equal(also, face[1:])           # consecutive cells share the product: l + 1.5f == (l + 1) + 0.5f exactly
        for d in range(-3, 4):
            v = _ulps(face, d)
            p = np.zeros((len(j), 3), F)
            p[:, a] = v
            b, c = (a + 1) % 3, (a + 2) % 3
            mb = rng.integers(0, int(size[b]) - 1, len(j))
            mc = rng.integers(0, int(size[c]) - 1, len(j))
            p[:, b] = ((mb.astype(F) + F(1.0)) * vs[b]).astype(F)      # a cell's middle
            p[:, c] = ((mc.astype(F) + F(0.5)) * vs[c]).astype(F)      # a face of its own
            pts.append(p)
            axes.append(np.full(len(j), a))
            faces.append(j)
    return np.concatenate(pts), np.concatenate(axes), np.concatenate(faces)


def _check(size, vs, points, fast):
    """The predicate against the reference's choice on every point; returns the reference's lower taps."""
    hi_cell = size.astype(np.int64) - 2
    guess = np.clip(np.floor(points.astype(np.float64) / vs.astype(np.float64) - 0.5).astype(np.int64), 0, hi_cell)
    _, lower = _selftest(size, vs, points, guess, fast)
    lower = lower.astype(np.int64)
    lo_edge = (F(0.5) * vs).astype(F)
    hi_edge = ((size.astype(F) - F(0.5)) * vs).astype(F)
    inside_axis = (points >= lo_edge) & (points < hi_edge)
    assert np.all(lower >= 0) and np.all(lower <= hi_cell + 1)
    assert np.all((lower <= hi_cell) == (points < hi_edge)), "a lower tap off the lattice of cells exactly in the upper half-voxel shell"
    for d in (-1, 0, 1):
        cells = lower + d
        ok = (cells >= 0) & (cells <= hi_cell)
        owns, lower2 = _selftest(size, vs, points, np.where(ok, cells, 0), fast)
        assert np.array_equal(lower2, lower)
        for a in range(3):
            bit = ((owns >> a) & 1).astype(bool)
            m = ok[:, a]
            # inside the lattice: the reference's cell owns, its neighbours do not; in the shell nobody owns
            want = inside_axis[:, a] & (d == 0)
            bad = m & (bit != want)
            assert not bad.any(), "axis %d, cell = lower %+d, fast = %d: %d points, first p = %r lower = %d" % (
                a, d, fast, int(bad.sum()), float(points[bad][0, a]), int(lower[bad][0, a]))
        if d == 0:
            all3 = ((owns >> 3) & 1).astype(bool)
            assert np.array_equal(all3, ok.all(axis=1) & inside_axis.all(axis=1))
    return lower


@pytest.mark.parametrize("fast", [0, 1], ids=["ieee_division", "fast_division"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_cell_owner_is_the_reference_s_cell_on_every_face(name, fast):
    size, vs = _grid(name)
    rng = np.random.default_rng(0xCE110 + len(name))
    points, axes, faces = _face_points(size, vs, rng)
    assert len(points) == 7 * int(size.astype(np.int64).sum())
    _check(size, vs, points, fast)
    # exactly one of the two cells either side of the face the point was built on owns it (along that axis)
    n = len(points)
    idx = np.arange(n)
    hi_cell = size.astype(np.int64)[axes] - 2
    below, above = faces - 1, faces            # face j lies between cells j - 1 and j
    both = (below >= 0) & (above <= hi_cell)
    cells = np.zeros((n, 3), np.int64)
    got = []
    for side in (below, above):
        cells[:] = 0
        cells[idx, axes] = np.where(both, side, 0)
        owns, _ = _selftest(size, vs, points, cells, fast)
        got.append(((owns >> axes) & 1).astype(bool))
    assert both.sum() >= 7 * (int(size.astype(np.int64).sum()) - 6)
    assert np.all((got[0] ^ got[1])[both]), "a point on a face owned by both cells or by neither"
    # on the face itself and above it the upper cell, below it the lower one: the comparison is p >= (l + 0.5f) * vs
    face_val = ((faces.astype(F) + F(0.5)) * vs[axes]).astype(F)
    assert np.array_equal(got[1][both], (points[idx, axes] >= face_val)[both])


@pytest.mark.parametrize("fast", [0, 1], ids=["ieee_division", "fast_division"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_cell_owner_is_the_reference_s_cell_on_random_points(name, fast):
    size, vs = _grid(name)
    rng = np.random.default_rng(0x0B5E55 + len(name))
    lo = (F(0.5) * vs).astype(np.float64)
    hi = ((size.astype(F) - F(0.5)) * vs).astype(np.float64)
    points = (lo + rng.random((N_RANDOM, 3)) * (hi - lo)).astype(F)
    points = np.minimum(np.maximum(points, lo.astype(F)), _ulps(hi.astype(F), -1))   # inside the lattice after rounding too
    lower = _check(size, vs, points, fast)
    assert np.all(lower <= size.astype(np.int64) - 2)
    # the draw reaches the first and the last cell of every axis
    for a in range(3):
        assert lower[:, a].min() == 0 and lower[:, a].max() == int(size[a]) - 2
