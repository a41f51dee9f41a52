"""The CPU reference of field alignment (tests/align_ref.py) on its own, no GPU: the rows by hand on a plane, the emulated order of
the sums against float64 within the bound that order implies, and the scenes of tests/test_align.py are not vacuous."""
import numpy as np
import pytest

from tests import align_ref as R
from tests import field_ref

F = np.float32


def plane_scene():
    """4 x 4 x 4 voxels of edge 1 at offset (8, -4, 16): d = x - 1.75 (x measured from the grid's origin), every weight 1.  Every
    number below is a small dyadic rational, so every fp32 operation of the rows is exact and the rows are known in closed form."""
    s = R.Scene()
    dims, vs, offset = (4, 4, 4), np.array([1, 1, 1], F), np.array([8, -4, 16], F)
    xc = (np.arange(4, dtype=F) + F(0.5)) - F(1.75)
    s.dist = np.broadcast_to(xc[None, None, :], (4, 4, 4)).astype(F).reshape(-1).copy()
    s.weight = np.ones(64, F)
    s.geom = (dims, vs, offset)
    return s


def test_rows_of_a_plane_by_hand(oracle):
    s = plane_scene()
    h, c = R.pivot(s.geom)
    assert np.array_equal(h, [2, 2, 2]) and np.array_equal(c, [10, -2, 18])
    # q = p - offset in [1, 3) on every axis has all seven samples valid; with q.x + 1 < 3.5 none of them lies in the far half voxel,
    # where the sample clamps its taps and the field stops being linear
    q = np.array([[1.0, 2.25, 1.0], [1.75, 2.5, 1.25], [2.375, 2.875, 2.75], [2.0, 2.125, 2.0], [1.25, 1.5, 1.0]], F)
    p = (q + s.geom[2]).astype(F)
    rows, inl = R.rows_at(oracle, s.geom, s.dist, s.weight, p, R.to_pivot(np.eye(4), s.geom), gate=10.0)
    assert inl.all()
    u = q - h                                      # the point about the pivot
    d = q[:, 0] - F(1.75)
    want = np.stack([np.ones(5, F), np.zeros(5, F), np.zeros(5, F), np.zeros(5, F), u[:, 2], -u[:, 1], -d], axis=1)
    assert np.array_equal(rows, want), (rows, want)
    # a quarter turn about z through the pivot and a shift: u = Rz (x - c) + (0.5, 0, 0) exactly
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = c - T[:3, :3] @ c + np.array([0.5, 0, 0])
    rows, inl = R.rows_at(oracle, s.geom, s.dist, s.weight, p, R.to_pivot(T, s.geom), gate=10.0)
    x = (p.astype(np.float64) - c)
    u = np.stack([-x[:, 1] + 0.5, x[:, 0], x[:, 2]], axis=1)
    ok = ((u + 2 >= 1) & (u + 2 < 3)).all(axis=1)
    assert ok.sum() >= 3 and np.array_equal(inl, ok)
    want = np.stack([np.ones(5), np.zeros(5), np.zeros(5), np.zeros(5), u[:, 2], -u[:, 1], -(u[:, 0] + 2 - 1.75)], axis=1)
    assert np.array_equal(rows[ok], want[ok].astype(F))
    assert np.isnan(rows[~ok]).all()
    # the gates: within a voxel of a face, a NaN, an infinity, the distance gate, an unobserved neighbour, a flat field
    edge = np.array([[0.5, 2, 2], [2, 3.0, 2], [np.nan, 2, 2], [2, np.inf, 2], [2, 2, -np.inf]], F) + s.geom[2]
    _, inl = R.rows_at(oracle, s.geom, s.dist, s.weight, edge, R.to_pivot(np.eye(4), s.geom), gate=10.0)
    assert not inl.any()
    _, inl = R.rows_at(oracle, s.geom, s.dist, s.weight, p, R.to_pivot(np.eye(4), s.geom), gate=0.5)
    assert np.array_equal(inl, np.abs(d) < 0.5) and 0 < inl.sum() < 5
    w = s.weight.copy()
    w[3 + 4 * (2 + 4 * 2)] = 0                      # voxel (3, 2, 2): the +x neighbour of q = (2, 2.125, 2)
    _, inl = R.rows_at(oracle, s.geom, s.dist, w, p, R.to_pivot(np.eye(4), s.geom), gate=10.0)
    assert not inl[3] and inl[0]
    _, inl = R.rows_at(oracle, s.geom, np.ones(64, F), s.weight, p, R.to_pivot(np.eye(4), s.geom), gate=10.0)
    assert not inl.any()
    # sums and the system: sum of d^2 in entry 27, the count in entry 28, A symmetric
    rows, inl = R.rows_at(oracle, s.geom, s.dist, s.weight, p, R.to_pivot(np.eye(4), s.geom), gate=10.0)
    total = R.sums_kernel_order(R.products(rows, inl))
    A, b, res, count = R.system(total)
    assert count == 5 and res == F((d.astype(np.float64) ** 2).sum()) and A[0, 0] == 5 and np.array_equal(A, A.T)
    assert np.array_equal(b, (rows[:, :6].astype(np.float64) * rows[:, 6:7]).sum(axis=0).astype(F))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536, 65537, 200001])
def test_the_emulated_order_lies_within_its_bound_of_float64(n):
    """Every entry passes through at most ceil(n / (256 B)) sequential additions in a thread, 6 in the shuffle tree, 3 across the
    waves and one narrowing: fewer than ceil(n / (256 B)) + 16 roundings of relative size 2^-24, each on a partial sum that is at
    most sum |row_o row_i| in magnitude (to first order).  So the bound follows from the order; it is not a measurement."""
    rng = np.random.RandomState(n)
    rows = (rng.normal(size=(n, 7)) * np.array([1, 1, 1, 800, 800, 800, 30])).astype(F)
    inl = rng.uniform(size=n) < 0.8
    P = R.products(rows, inl)
    B = R.blocks_for(n)
    assert B == min(256, -(-n // 256))
    got = R.sums_kernel_order(P).astype(np.float64)
    bound = (-(-n // (256 * B)) + 16) * 2.0 ** -24 * R.sums_abs(P)
    assert (np.abs(got - R.sums_f64(P)) <= bound).all()
    assert got[28] == inl.sum()
    # the other fp32 order of the same sums obeys its own (n-long) bound
    asc = R.sums_ascending_f32(P).astype(np.float64)
    assert (np.abs(asc - R.sums_f64(P)) <= (n + 1) * 2.0 ** -24 * R.sums_abs(P)).all()


@pytest.fixture(scope="module")
def scene(oracle):
    return R.fused_scene(oracle)


def test_the_scene_is_not_vacuous(oracle, scene):
    s = scene
    assert len(s.points) >= 1000
    _, inl = R.rows_at(oracle, s.geom, s.dist, s.weight, s.points, R.to_pivot(s.T0, s.geom), s.gate)
    print("inliers at the start pose: %d of %d" % (inl.sum(), len(inl)))
    assert inl.sum() * 2 >= len(inl)
    T, norms, counts = R.chain(oracle, s, [(s.points, 10)], s.T0, s.gate)
    print("update norms", norms, "inliers", counts, "distance to identity", R.pose_distance(T, np.eye(4)))
    assert min(counts) * 2 >= len(inl)
    assert norms[-1] < 1e-3 * norms[0]                       # the chain converges ...
    assert R.pose_distance(T, np.eye(4)) < R.pose_distance(s.T0, np.eye(4)) / 5      # ... towards the pose the mesh came from
    # the system is well posed about the pivot
    A = R.step(oracle, s, s.points, s.T0, s.gate, order="f64")[0]
    scale = np.sqrt(np.diag(A))
    assert np.linalg.cond(A / np.outer(scale, scale)) < 1e4
