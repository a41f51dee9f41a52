"""The CPU reference of the reachability group (tests/reach_ref.py) against cases worked by hand from the rules of include/tsdf_amd.h,
"reachability" (no GPU needed): the costs 10 / 14 / 17, no corner cutting, both connectivities, the cap, seeds, the path order and
max_len."""
import numpy as np

from tests import reach_ref as R

U = R.UNREACHED
VS = (10.0, 10.0, 10.0)
OFF = (0.0, 0.0, 0.0)


def centre(x, y, z):
    return (10.0 * x + 5.0, 10.0 * y + 5.0, 10.0 * z + 5.0)


def field(size, blocked=(), seeds=((0, 0, 0),), connectivity=26, max_cost=0):
    X, Y, Z = size
    trav = np.ones(X * Y * Z, bool)
    for x, y, z in blocked:
        trav[(z * Y + y) * X + x] = False
    out, seed_ids = R.cost_field(trav, size, VS, OFF, [centre(*s) for s in seeds], connectivity, max_cost)
    return trav, out, seed_ids


def test_a_free_row_costs_ten_a_step():
    _, out, seeds = field((5, 1, 1))
    assert out.tolist() == [0, 10, 20, 30, 40] and seeds == [0]


def test_the_diagonal_of_a_square_and_corner_cutting():
    # ids of a 2 x 2 x 1 block: (0,0) 0, (1,0) 1, (0,1) 2, (1,1) 3
    assert field((2, 2, 1))[1].tolist() == [0, 10, 10, 14]
    assert field((2, 2, 1), blocked=[(1, 0, 0)])[1].tolist() == [0, U, 10, 20]      # round the other way: two face steps
    assert field((2, 2, 1), blocked=[(0, 1, 0)])[1].tolist() == [0, 10, U, 20]
    assert field((2, 2, 1), blocked=[(1, 0, 0), (0, 1, 0)])[1].tolist() == [0, U, U, U]   # the diagonal does not squeeze through


def test_the_corner_step_of_a_cube_needs_all_eight():
    _, out, _ = field((2, 2, 2))
    assert out.tolist() == [0, 10, 10, 14, 10, 14, 14, 17]
    for x, y, z in [(1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)]:
        _, out, _ = field((2, 2, 2), blocked=[(x, y, z)])
        # one blocked voxel of the eight forbids the corner step; the far corner is then an edge and a face step away
        assert out[7] == 24, (x, y, z, out.tolist())
        assert out[(z * 2 + y) * 2 + x] == U


def test_connectivity_six_against_twenty_six():
    assert field((2, 2, 2), connectivity=6)[1].tolist() == [0, 10, 10, 20, 10, 20, 20, 30]
    assert field((2, 2, 2), connectivity=26)[1].tolist() == [0, 10, 10, 14, 10, 14, 14, 17]
    # at 6 two blocked face neighbours do not matter to a diagonal that does not exist: the voxel is simply not reached
    assert field((2, 2, 1), blocked=[(1, 0, 0), (0, 1, 0)], connectivity=6)[1].tolist() == [0, U, U, U]


def test_max_cost_keeps_what_is_at_or_below_it():
    _, free, _ = field((5, 1, 1))
    for cap in (1, 10, 25, 30, 39, 40, 1000):
        _, out, _ = field((5, 1, 1), max_cost=cap)
        assert out.tolist() == [v if v <= cap else U for v in free.tolist()], cap
    _, out, _ = field((3, 3, 1), max_cost=14)
    assert out.reshape(3, 3).tolist() == [[0, 10, U], [10, 14, U], [U, U, U]]


def test_two_seeds_and_ignored_seeds():
    _, out, seeds = field((7, 1, 1), seeds=[(0, 0, 0), (6, 0, 0)])
    assert out.tolist() == [0, 10, 20, 30, 20, 10, 0] and seeds == [0, 6]
    # a seed in a blocked voxel, one off the grid and one that is not finite are ignored
    trav = np.ones(5, bool)
    trav[2] = False
    out, seeds = R.cost_field(trav, (5, 1, 1), VS, OFF, [centre(2, 0, 0), (-1.0, 5.0, 5.0), (np.nan, 5.0, 5.0), (50.0, 5.0, 5.0)])
    assert out.tolist() == [U] * 5 and seeds == []
    assert R.info(trav, out) == {"n_traversable": 4, "n_reached": 0, "n_seed_voxels": 0, "max_cost_reached": 0}
    out, seeds = R.cost_field(trav, (5, 1, 1), VS, OFF, [centre(2, 0, 0), centre(4, 0, 0), (49.99, 9.99, 0.0)])
    assert out.tolist() == [U, U, U, 10, 0] and seeds == [4]
    assert R.info(trav, out) == {"n_traversable": 4, "n_reached": 2, "n_seed_voxels": 1, "max_cost_reached": 10}


def test_traversable_follows_the_states_the_flag_and_the_clearance():
    d = np.array([0.5, -0.5, 0.5, np.nan, -0.0], np.float32)
    w = np.array([1.0, 1.0, 0.0, 2.0, np.nan], np.float32)      # free, occupied, unknown, free (NaN is not negative), unknown
    assert R.traversable(d, w).tolist() == [True, False, False, True, False]
    assert R.traversable(d, w, through_unknown=True).tolist() == [True, False, True, True, True]
    e = np.array([30.0, 30.0, np.nan, 10.0, 50.0], np.float32)
    assert R.traversable(d, w, True, e, 20.0).tolist() == [True, False, False, False, True]
    assert R.traversable(d, w, True, e, 0.0).tolist() == [True, False, False, True, True]   # NaN fails even a clearance of 0


def test_the_path_takes_the_first_neighbour_in_the_stated_order():
    # free 3 x 3 x 1, seed in the middle of the lower row (1, 0): the far corners are 24 away by an edge and a face step in either order
    trav, out, _ = field((3, 3, 1), seeds=[(1, 0, 0)])
    assert out.reshape(3, 3).tolist() == [[10, 0, 10], [14, 10, 14], [24, 20, 24]]
    # from (0, 2) = id 6 the candidates in order (dy = -1: dx = -1, 0, 1; ...) are (0, 1) = 14 + 10 and (1, 1) = 10 + 14: the first wins
    assert R.path(out, trav, (3, 3, 1), 26, 6) == [6, 3, 1]
    # from (2, 2) = id 8: (1, 1) comes first (dx = -1 before dx = 0)
    assert R.path(out, trav, (3, 3, 1), 26, 8) == [8, 4, 1]
    # at connectivity 6 from (0, 2): cost 30; dy = -1 comes before dx = +1
    trav, out6, _ = field((3, 3, 1), seeds=[(1, 0, 0)], connectivity=6)
    assert out6.reshape(3, 3).tolist() == [[10, 0, 10], [20, 10, 20], [30, 20, 30]]
    assert R.path(out6, trav, (3, 3, 1), 6, 6) == [6, 3, 0, 1]
    assert R.path(out6, trav, (3, 3, 1), 6, 1) == [1]          # a goal on a seed
    assert R.path(out6, trav, (3, 3, 1), 6, None) == []


def test_max_len_truncates_the_row_and_keeps_the_length():
    trav, out, _ = field((5, 1, 1))
    goals = [centre(4, 0, 0), centre(0, 0, 0), (70.0, 5.0, 5.0)]
    lengths, rows = R.paths(out, trav, (5, 1, 1), VS, OFF, 26, goals, 3)
    assert lengths.tolist() == [5, 1, 0]
    assert rows.tolist() == [[4, 3, 2], [0, U, U], [U, U, U]]
    keep = np.full((3, 5), 77, np.uint32)
    lengths, rows = R.paths(out, trav, (5, 1, 1), VS, OFF, 26, goals, 5, rows=keep)
    assert lengths.tolist() == [5, 1, 0] and rows.tolist() == [[4, 3, 2, 1, 0], [0, 77, 77, 77, 77], [77] * 5]
    assert R.lookup(out, (5, 1, 1), VS, OFF, goals + [(np.inf, 0.0, 0.0), (10.0, 0.0, 0.0)]).tolist() == [40, 0, U, U, 10]


def test_ranking_takes_the_smallest_cost_then_the_smallest_id():
    _, out, _ = field((5, 1, 1), blocked=[(3, 0, 0)], seeds=[(1, 0, 0)])
    assert out.tolist() == [10, 0, 10, U, U]
    frontier = np.array([0, 2, 4], np.uint32)
    labels = np.array([0, 0, 2], np.uint32)
    table = np.zeros(2, [("label", np.uint32)])
    table["label"] = [0, 2]
    got = R.rank(out, frontier, labels, table)
    assert got.tolist() == [(0, 10, 0, 0), (2, U, 0xFFFFFFFF, 0)]
