"""The CPU reference of the column maps (tests/columns_ref.py) against itself and against brute force, without a GPU: the counts sum to
L; a reversed map is the forward map of the volume flipped along the axis; a band's counts are the sum of the counts of its two
halves; the height lies between the two voxel centres or is the upper face; the classification equals a brute-force loop; axis 0 and
axis 2 agree on a volume and its transpose."""
import numpy as np
import pytest

from tests import columns_ref as R
from tests import explore_ref

F32 = np.float32
SIZE = (9, 6, 7)


@pytest.fixture(scope="module")
def field():
    D, Wt = explore_ref.random_state_field(SIZE, 3300, 0.7, fp32_oddities=True)
    return D, Wt


def cube(a, size):
    return np.asarray(a).reshape(size[2], size[1], size[0])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_counts_sum_to_the_band_and_bands_add_up(field, axis):
    D, Wt = field
    n = SIZE[axis]
    for band in (None, (1, n - 1), (2, 3)):
        lo, hi = R.band_of(SIZE, axis, band)
        for reversed_ in (False, True):
            rows, totals = R.project(D, Wt, SIZE, axis, band, reversed_)
            au, av = R.MAP_AXES[axis]
            assert rows.shape == (SIZE[av], SIZE[au])
            per_cell = rows["n_unknown"].astype(np.int64) + rows["n_free"] + rows["n_occupied"]
            assert (per_cell == hi - lo).all()
            assert totals["n_unknown"] + totals["n_free"] + totals["n_occupied"] == SIZE[au] * SIZE[av] * (hi - lo)
            assert ((rows["top"] >= 0) == (rows["n_occupied"] > 0)).all() and ((rows["bottom"] >= 0) == (rows["top"] >= 0)).all()
            assert (rows["bottom"] <= rows["top"]).all()
            assert (rows["headroom"][rows["top"] < 0] == 0).all()
            assert (rows["top"].astype(np.int64) + 1 + rows["headroom"] <= hi - lo).all()
    whole, _ = R.project(D, Wt, SIZE, axis)
    for cut in (1, n // 2, n - 1):
        a, _ = R.project(D, Wt, SIZE, axis, (0, cut))
        b, _ = R.project(D, Wt, SIZE, axis, (cut, n))
        for name in ("n_unknown", "n_free", "n_occupied"):
            assert np.array_equal(a[name] + b[name], whole[name]), (axis, cut, name)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_reversed_map_is_the_forward_map_of_the_flipped_volume(field, axis):
    D, Wt = field
    n = SIZE[axis]
    flip = lambda a: np.flip(cube(a, SIZE), axis=2 - axis).reshape(-1)
    for band in (None, (1, n - 2)):
        lo, hi = R.band_of(SIZE, axis, band)
        reversed_rows, _ = R.project(D, Wt, SIZE, axis, (lo, hi), True)
        forward_rows, _ = R.project(flip(D), flip(Wt), SIZE, axis, (n - hi, n - lo), False)
        assert reversed_rows.tobytes() == forward_rows.tobytes()


def test_the_height_lies_between_the_centres_or_on_the_upper_face(field):
    D, Wt = field
    seen_crossing = seen_face = 0
    for axis in (0, 1, 2):
        for reversed_ in (False, True):
            rows, _ = R.project(D, Wt, SIZE, axis, None, reversed_)
            for r in rows.reshape(-1):
                top, h = int(r["top"]), r["height"]
                if top < 0:
                    assert np.isnan(h)
                    continue
                if h == F32(top + 1):
                    seen_face += 1
                else:
                    assert F32(top + 0.5) <= h <= F32(top + 1.5) and r["headroom"] >= 1
                    seen_crossing += 1
    assert seen_crossing > 20 and seen_face > 20
    # the decreed ends of f and the fallbacks: d1 of NaN, -0.0, +0.0, +inf, d0 of -inf
    state = np.array([explore_ref.OCCUPIED, explore_ref.FREE], np.uint8)
    for d0, d1, want in ((-1.0, np.nan, 1.0), (-1.0, -0.0, 1.5), (-1.0, 0.0, 1.5), (-1.0, np.inf, 0.5), (-np.inf, 1.0, 1.0), (-1.0, 3.0, 0.75)):
        assert R.row_of(state, np.array([d0, d1], F32), None)[6] == F32(want), (d0, d1)
    assert R.row_of(state[:1], np.array([-1.0], F32), None)[5:7] == (0, F32(1.0))   # L = 1: the upper face
    # the minimum skips NaN, and a zero of either sign is stored as +0.0
    m = R.row_of(state, np.array([-1.0, 1.0], F32), np.array([np.nan, -0.0], F32))[7]
    assert m == 0 and not np.signbit(m)
    assert np.isnan(R.row_of(state, np.array([-1.0, 1.0], F32), np.array([np.nan, np.nan], F32))[7])
    assert R.row_of(state, np.array([-1.0, 1.0], F32), np.array([2.5, -3.0], F32))[7] == F32(-3.0)


def test_classify_equals_a_brute_force_loop(field):
    D, Wt = field
    rows, _ = R.project(D, Wt, SIZE, 2)
    V, U = rows.shape
    top, headroom = rows["top"].astype(np.int64), rows["headroom"].astype(np.int64)
    for max_step, min_headroom in ((0, 0), (1, 2), (2 ** 31 - 1, 0), (0, 10 ** 6)):
        got, counts = R.classify(rows, max_step, min_headroom)
        want = np.zeros((V, U), np.uint8)
        for v in range(V):
            for u in range(U):
                if top[v, u] < 0:
                    continue
                steps = [abs(top[v, u] - top[b, a]) for a, b in ((u - 1, v), (u + 1, v), (u, v - 1), (u, v + 1))
                         if 0 <= a < U and 0 <= b < V and top[b, a] >= 0]
                want[v, u] = 2 if headroom[v, u] < min_headroom or any(s > max_step for s in steps) else 1
        assert np.array_equal(got, want)
        assert counts == {"n_no_ground": int((want == 0).sum()), "n_traversable": int((want == 1).sum()), "n_blocked": int((want == 2).sum())}
        assert sum(counts.values()) == U * V
    assert (R.classify(rows, 2 ** 31 - 1, 0)[0] != R.BLOCKED).all()


def test_axis_0_and_axis_2_agree_on_a_volume_and_its_transpose(field):
    D, Wt = field
    # the transposed volume: x and z exchanged, so its columns along z are the original's along x
    T = (SIZE[2], SIZE[1], SIZE[0])
    swap = lambda a: np.ascontiguousarray(cube(a, SIZE).transpose(2, 1, 0)).reshape(-1)
    for band, reversed_ in ((None, False), ((2, 7), True)):
        along_x, totals_x = R.project(D, Wt, SIZE, 0, band, reversed_)     # cells (y, z): shape (Z, Y)
        along_z, totals_z = R.project(swap(D), swap(Wt), T, 2, band, reversed_)   # cells (x', y) = (z, y): shape (Y, Z)
        assert along_x.tobytes() == np.ascontiguousarray(along_z.T).tobytes()
        assert totals_x == totals_z


def test_height_world_is_rule_4s_expression():
    rows = np.zeros((1, 2), R.COLUMN_DTYPE)
    rows["height"] = [F32(2.25), F32(np.nan)]
    size, vs, off = (4, 5, 6), (10.0, 12.5, 9.0), (100.0, -50.0, 25.0)
    forward = R.height_world(rows, size, 2, (1, 5), False, vs, off)
    assert forward[0, 0] == F32(25.0 + (1 + 2.25) * 9.0) and np.isnan(forward[0, 1])
    assert R.height_world(rows, size, 2, (1, 5), True, vs, off)[0, 0] == F32(25.0 + (5 - 2.25) * 9.0)
