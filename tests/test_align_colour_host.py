"""The CPU reference of colour alignment (tests/align_colour_ref.py) on its own, no GPU: on a textured wall the plain chain cannot
recover an in-plane shift and the colour chain does; a zero colour weight is the plain chain bit for bit; Y is exact; the intensity
and its gradient by hand on a cell whose numbers are all small dyadic rationals."""
import numpy as np
import pytest

from tests import align_colour_ref as CR
from tests import align_ref as R

F = np.float32
STAGES = 19          # 4 + 5 + 10 steps, as one stage over the full frame


@pytest.fixture(scope="module")
def wall():
    return CR.wall_scene()


def test_the_wall_scene_is_what_the_issue_asks_for(wall):
    s = wall
    assert CR.WALL_SIZE == (48, 48, 24) and CR.WALL_VOXEL == 10.0 and (CR.WALL_W, CR.WALL_H) == (80, 60)
    shift = float(np.hypot(*CR.WALL_SHIFT))
    assert shift >= CR.WALL_VOXEL and shift <= min(CR.WALL_LX, CR.WALL_LY) / 6
    assert CR.in_plane_error(s.T0) == pytest.approx(shift)
    assert len(s.points) == 80 * 60 and np.isfinite(s.points).all() and (s.points[:, 2] == F(CR.WALL_DEPTH)).all()
    # an exact plane: every distance is a whole number of millimetres, zero exactly between two planes of voxels
    assert np.array_equal(s.dist, np.rint(s.dist)) and (s.colour >> np.uint32(24) == 1).all()
    y = s.intensity
    assert y.min() >= 38 and y.max() <= 218 and y.max() - y.min() > 150          # the texture uses the range it was given


def test_the_plain_chain_slides_and_the_colour_chain_recovers(oracle, wall):
    """The plain rows of a plane that faces the camera are (0, 0, -1, u x (0, 0, -1), -d): no in-plane component, so the plain chain keeps
    (at least 3/4 of) the in-plane error whatever it does; the colour rows carry the texture's gradient, and from within a sixth of the
    shortest wavelength Gauss-Newton on them converges."""
    s = wall
    start = CR.in_plane_error(s.T0)
    plain, _, counts = R.chain(oracle, s, [(s.points, STAGES)], s.T0, s.gate)
    assert counts[-1] == len(s.points)
    rows = R.rows_at(oracle, s.geom, s.dist, s.weight, s.points, R.to_pivot(s.T0, s.geom), s.gate)[0]
    assert not rows[:, :2].any() and np.abs(rows[:, 2] + 1).max() < 1e-5      # (the distance falls along +z: the gradient points at the camera)
    ends = {}
    for order in ("f64", "ascending"):
        T, norms, counts = CR.chain(oracle, s, [(s.points, s.intensity, STAGES)], s.T0, s.gate, s.colour_gate, 0.1, order=order)
        ends[order] = CR.in_plane_error(T)
        assert counts[-1] == (len(s.points), len(s.points))
    print("wall: in-plane error %.3f mm at the start, %.3f mm after the plain chain, %.3e mm (float64 sums) / %.3e mm (ascending fp32 sums) "
          "after the colour chain" % (start, CR.in_plane_error(plain), ends["f64"], ends["ascending"]))
    assert CR.in_plane_error(plain) >= 0.75 * start
    assert max(ends.values()) <= 0.25 * start


def test_a_zero_colour_weight_is_the_plain_chain_bit_for_bit(oracle):
    """On tests/align_ref.py's fused scene with colour (the wall's plain system is singular: its reference chain never moves)."""
    s = CR.fused_colour_scene(oracle)
    T0 = s.T0
    assert np.isfinite(s.intensity).sum() * 2 >= len(s.points)
    for order in ("f64", "ascending"):
        plain = R.chain(oracle, s, [(s.points[::3], 2), (s.points, 2)], T0, s.gate, order=order)
        zero = CR.chain(oracle, s, [(s.points[::3], s.intensity[::3], 2), (s.points, s.intensity, 2)], T0, s.gate, s.colour_gate, 0.0, order=order)
        assert plain[1][0] > 1.0                                           # it moved
        assert np.array_equal(plain[0], zero[0]) and plain[1] == zero[1]
        assert plain[2] == [c[0] for c in zero[2]] and all(c[1] > 0 for c in zero[2])
    # one step in the kernel's order: the combined system at weight 0 is the geometric block's
    A0, b0, res0, count0, _, _ = R.step(oracle, s, s.points, T0, s.gate)
    A, b, res, count, rows, (inl, inl_c) = CR.step(oracle, s, s.points, s.intensity, T0, s.gate, s.colour_gate, 0.0)
    assert np.array_equal(A, A0) and np.array_equal(b, b0) and res[0] == res0 and count[0] == count0 and count[1] == inl_c.sum() > 0
    assert A.dtype == F and not (inl_c & ~inl).any()
    # ... and at a weight that is not zero it is not
    A1 = CR.step(oracle, s, s.points, s.intensity, T0, s.gate, s.colour_gate, 0.5)[0]
    assert not np.array_equal(A1, A0) and np.array_equal(A1, A1.T)


def test_y_is_exact_for_all_colours():
    """(77 r + 150 g + 29 b) <= 65280 < 2^24 and 2^-8 is a power of two: the fp32 value is the integer expression exactly."""
    for r0 in range(0, 256, 32):
        r, g, b = np.meshgrid(np.arange(r0, r0 + 32, dtype=np.uint32), np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32), indexing="ij")
        words = (r | (g << np.uint32(8)) | (b << np.uint32(16)) | np.uint32(0xAB000000)).reshape(-1)    # (n is not looked at)
        want = (77 * r.astype(np.int64) + 150 * g.astype(np.int64) + 29 * b.astype(np.int64)).reshape(-1)
        got = CR.intensity_of(words)
        assert got.dtype == F
        assert np.array_equal(got.astype(np.float64) * 256.0, want.astype(np.float64))
    assert CR.intensity_of(np.array([0x00FFFFFF, 0, 0x000000FF, 0x0000FF00, 0x00FF0000], np.uint32)).tolist() == [255.0, 0.0, 76.69921875, 149.4140625, 28.88671875]


def test_the_intensity_and_its_gradient_by_hand():
    """A 3 x 3 x 3 grid of edge 2 with grey colours that are linear in the voxel index, I = 16 i + 8 j + 4 k + 10: inside the cells the
    interpolant is that plane, every number a small dyadic rational and every fp32 operation exact."""
    dims, vs, offset = (3, 3, 3), np.array([2, 2, 2], F), np.array([5, -3, 1], F)
    k, j, i = np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij")
    grey = (16 * i + 8 * j + 4 * k + 10).astype(np.uint32).reshape(-1)
    colour = grey | (grey << np.uint32(8)) | (grey << np.uint32(16)) | np.uint32(3 << 24)
    geom = (dims, vs, offset)
    q = np.array([[1.0, 1.0, 1.0], [2.5, 3.25, 1.75], [4.5, 4.75, 3.0], [3.0, 3.0, 3.0]], F)
    c, g = CR.intensity_at(geom, colour, q)
    idx = q.astype(np.float64) / 2 - 0.5                                   # the continuous voxel index of q
    assert np.array_equal(c, (16 * idx[:, 0] + 8 * idx[:, 1] + 4 * idx[:, 2] + 10).astype(F))
    assert np.array_equal(g, np.tile(np.array([8, 4, 2], F), (4, 1)))       # 16, 8, 4 per voxel of edge 2
    # world points: q = p - offset
    c2, g2 = CR.sample_intensity(geom, colour, q + offset)
    assert np.array_equal(c2, c) and np.array_equal(g2, g)
    # the far half voxel clamps its upper tap onto the lower one: a zero difference along that axis, by definition
    c, g = CR.intensity_at(geom, colour, np.array([[5.5, 3.0, 3.0], [3.0, 3.0, 0.5]], F))
    assert g[0].tolist() == [0.0, 4.0, 2.0] and c[0] == 16 * 2 + 8 + 4 + 10
    assert g[1].tolist() == [8.0, 4.0, 2.0] and c[1] == 16 + 8 + 4 * -0.25 + 10          # the near half voxel extrapolates, as the distance does
    # not valid: outside, NaN, a tap never observed, colour off
    hole = colour.copy()
    hole[0 + 3 * (1 + 3 * 1)] &= np.uint32(0x00FFFFFF)                     # voxel (0, 1, 1): a tap of the second point's cell only
    for cc, qq in ((colour, [[6.0, 1, 1]]), (colour, [[-0.5, 1, 1]]), (colour, [[np.nan, 1, 1]]), (hole, [[2.5, 3.25, 1.75]]), (None, [[1.0, 1, 1]])):
        c, g = CR.intensity_at(geom, cc, np.array(qq, F))
        assert np.isnan(c).all() and np.isnan(g).all()
    assert np.isfinite(CR.intensity_at(geom, hole, np.array([[4.5, 4.75, 3.0]], F))[0]).all()          # a cell the hole is not in
