"""The CPU reference of the exploration queries (tests/explore_ref.py) against cases worked by hand (no GPU needed): what the GPU tests
compare with has to be right on its own."""
import numpy as np

from tests import explore_ref as R

F32 = np.float32


def field(size, observed=True, distance=0.5):
    n = size[0] * size[1] * size[2]
    return np.full(n, distance, F32), np.full(n, 1.0 if observed else 0.0, F32)


def vid(size, x, y, z):
    return (z * size[1] + y) * size[0] + x


def test_states_follow_the_sign_test_and_the_weight_test():
    D = np.array([0.5, -0.5, -0.0, 0.0, np.nan, -1.0, -1.0, -1.0], F32)
    W = np.array([1.0, 1.0, 1.0, 2.0, 1.0, 0.0, np.nan, -1.0], F32)
    assert R.states(D, W).tolist() == [R.FREE, R.OCCUPIED, R.FREE, R.FREE, R.FREE, R.UNKNOWN, R.UNKNOWN, R.UNKNOWN]


def test_one_unknown_centre_has_its_six_face_neighbours_as_frontiers():
    size = (3, 3, 3)
    D, W = field(size)
    W[vid(size, 1, 1, 1)] = 0.0
    ids, counts = R.frontiers(D, W, size)
    expect = sorted(vid(size, *c) for c in [(0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)])
    assert ids.tolist() == expect
    assert counts == {"n_unknown": 1, "n_free": 26, "n_occupied": 0, "n_frontiers": 6}
    # at connectivity 6 no two of them touch; at 26 they form one ring-like cluster through their shared edges
    L6, rows6, n6 = R.clusters(ids, size, 6, 1)
    assert n6 == 6 and L6.tolist() == list(range(6)) and len(rows6) == 6
    L26, rows26, n26 = R.clusters(ids, size, 26, 1)
    assert n26 == 1 and L26.tolist() == [0] * 6
    row = rows26[0]
    assert row["label"] == 0 and row["size"] == 6 and row["lo"].tolist() == [0, 0, 0] and row["hi"].tolist() == [2, 2, 2]
    assert row["sum"].tolist() == [6, 6, 6]


def test_the_grid_border_is_not_unknown_space_and_occupied_voxels_are_no_frontiers():
    size = (4, 1, 1)
    D, W = field(size)
    assert len(R.frontiers(D, W, size)[0]) == 0           # all free, nothing unknown: the border does not count
    W[3] = 0.0
    D[2] = -0.5                                            # the only neighbour of the unknown voxel is occupied
    ids, counts = R.frontiers(D, W, size)
    assert len(ids) == 0 and counts == {"n_unknown": 1, "n_free": 2, "n_occupied": 1, "n_frontiers": 0}
    D[2] = np.nan                                          # NaN is not negative: free, and a frontier
    assert R.frontiers(D, W, size)[0].tolist() == [2]


def test_two_diagonal_frontier_voxels_are_one_cluster_at_26_and_two_at_6():
    size = (5, 5, 1)
    ids = np.array([vid(size, 1, 1, 0), vid(size, 2, 2, 0)], np.uint32)
    L6, rows6, n6 = R.clusters(ids, size, 6, 1)
    assert n6 == 2 and L6.tolist() == [0, 1] and rows6["size"].tolist() == [1, 1]
    L26, rows26, n26 = R.clusters(ids, size, 26, 1)
    assert n26 == 1 and L26.tolist() == [0, 0]
    assert rows26[0]["size"] == 2 and rows26[0]["lo"].tolist() == [1, 1, 0] and rows26[0]["hi"].tolist() == [2, 2, 0]
    assert rows26[0]["sum"].tolist() == [3, 3, 0]
    # min_size drops rows, not clusters; 0 and 1 list the same
    assert len(R.clusters(ids, size, 26, 3)[1]) == 0 and R.clusters(ids, size, 26, 3)[2] == 1
    assert len(R.clusters(ids, size, 6, 0)[1]) == 2


def test_an_axis_ray_through_voxel_centres_visits_exactly_its_row():
    size, vs, off = (6, 4, 3), (10.0, 10.0, 10.0), (100.0, 0.0, -20.0)
    D, W = field(size, observed=False)
    state = R.states(D, W)
    o = (off[0] - 25.0, off[1] + 25.0, off[2] + 15.0)     # outside, on the centre line of row y = 2, z = 1
    gain, u, f, s, mask = R.view_gain(state, size, vs, off, [o], [(1.0, 0.0, 0.0)])
    assert (gain, u[0], f[0], s[0]) == (6, 6, 0, 1)
    assert sorted(mask) == [vid(size, x, 2, 1) for x in range(6)]
    # backwards from inside: the start voxel and those behind it
    gain, u, f, s, mask = R.view_gain(state, size, vs, off, [(off[0] + 35.0, off[1] + 25.0, off[2] + 15.0)], [(-2.0, 0.0, 0.0)])
    assert (gain, u[0], s[0]) == (4, 4, 1) and sorted(mask) == [vid(size, x, 2, 1) for x in range(4)]
    # t_max cuts the walk: 12 mm from x = 5 mm inside voxel 0 reaches voxel 1 only
    gain, u, f, s, mask = R.view_gain(state, size, vs, off, [(off[0] + 5.0, off[1] + 25.0, off[2] + 15.0)], [(1.0, 0.0, 0.0)], [12.0])
    assert (gain, u[0], s[0]) == (2, 2, 1)
    # free voxels count as free; an occupied one stops the ray and is not counted
    W[:] = 1.0
    D[vid(size, 4, 2, 1)] = -0.5
    gain, u, f, s, mask = R.view_gain(R.states(D, W), size, vs, off, [o], [(1.0, 0.0, 0.0)])
    assert (gain, u[0], f[0], s[0]) == (0, 0, 4, 2)


def test_a_diagonal_through_lattice_corners_takes_x_then_y_then_z():
    size, vs, off = (3, 3, 3), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    D, W = field(size, observed=False)
    gain, u, f, s, mask = R.view_gain(R.states(D, W), size, vs, off, [(0.0, 0.0, 0.0)], [(1.0, 1.0, 1.0)])
    # every boundary is a three-way tie: (0,0,0) -> x -> y -> z -> (1,1,1) -> ...
    path = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)]
    assert u[0] == 7 and s[0] == 1 and sorted(mask) == sorted(vid(size, *c) for c in path)


def test_the_decreed_skips():
    size, vs, off = (4, 4, 4), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    state = R.states(*field(size, observed=False))
    inside, along = (1.5, 1.5, 1.5), (1.0, 0.0, 0.0)
    cases = [((np.nan, 0, 0), along, None), ((np.inf, 0, 0), along, None), (inside, (np.nan, 0, 0), None), (inside, (0, -np.inf, 0), None),
             (inside, (0.0, -0.0, 0.0), None), (inside, along, np.nan), (inside, along, 0.0), (inside, along, -1.0),
             ((1.5, 9.0, 1.5), along, None),         # s_y == 0 and a_y outside [0, 4)
             ((-1.0, 1.5, 1.5), (-1.0, 0.0, 0.0), None),   # points away: t0 < t1 fails
             ((3e38, 1.5, 1.5), (-3e38, 0.0, 0.0), None)]
    for o, d, t in cases:
        gain, u, f, s, mask = R.view_gain(state, size, vs, off, [o], [d], None if t is None else [t])
        assert (gain, u[0], f[0], s[0]) == (0, 0, 0, 0), (o, d, t)
    gain, u, f, s, _ = R.view_gain(state, size, vs, off, [inside], [along], [np.inf])
    assert (gain, u[0], s[0]) == (3, 3, 1)


def test_duplicate_rays_leave_the_gain_unchanged_and_keep_mask_is_the_union():
    size, vs, off = (8, 8, 8), (2.0, 2.0, 2.0), (-8.0, -8.0, -8.0)
    rng = np.random.default_rng(11)
    D, W = R.random_state_field(size, 12, 0.3)
    state = R.states(D, W)
    o = rng.uniform(-12.0, 12.0, (20, 3)).astype(F32)
    d = rng.normal(size=(20, 3)).astype(F32)
    one = R.view_gain(state, size, vs, off, o[:1], d[:1])
    many = R.view_gain(state, size, vs, off, np.repeat(o[:1], 5, axis=0), np.repeat(d[:1], 5, axis=0))
    assert many[0] == one[0] == one[1][0] and many[1].tolist() == [one[1][0]] * 5
    a = R.view_gain(state, size, vs, off, o[:10], d[:10])
    b = R.view_gain(state, size, vs, off, o[10:], d[10:])
    kept = R.view_gain(state, size, vs, off, o[10:], d[10:], mask=a[4])
    both = R.view_gain(state, size, vs, off, o, d)
    assert kept[4] == a[4] | b[4] == both[4] and kept[0] == both[0] == len(a[4] | b[4])
    assert a[0] > 0 and b[0] > 0 and kept[0] <= a[0] + b[0]
