"""The CPU reference of the class objects (tests/objects_ref.py) against cases worked out by hand from the rules of include/tsdf_amd.h,
"class objects" (no GPU needed): the class predicate on adjacency, both connectivities, the vote and selection tests and the bridges
they cut, min_size at its edge, the vote sum, and the lookup."""
import numpy as np

from tests import objects_ref as R

F32 = np.float32


def field(size, voxels):
    """Class words of a grid that is empty but for voxels = {(x, y, z): (class, votes)}."""
    X, Y, Z = size
    w = np.zeros(X * Y * Z, np.uint32)
    for (x, y, z), (c, n) in voxels.items():
        w[(z * Y + y) * X + x] = c | (n << 16)
    return w


def row(label, size, lo, hi, s, votes, class_id):
    r = np.zeros(1, R.OBJECT_DTYPE)
    r[0] = (label, size, lo, hi, s, votes, class_id, 0)
    return r.tobytes()


def test_the_row_layout():
    D = R.OBJECT_DTYPE
    assert D.itemsize == 72 and [D.fields[n][1] for n in D.names] == [0, 4, 8, 20, 32, 56, 64, 68]


def test_face_neighbours_join_only_within_a_class():
    size = (4, 3, 2)
    for connectivity in (6, 26):
        # ids 5 and 6: (1, 1, 0) and (2, 1, 0)
        ids, L, rows, n = R.find(field(size, {(1, 1, 0): (7, 1), (2, 1, 0): (9, 1)}), size, connectivity=connectivity)
        assert ids.tolist() == [5, 6] and L.tolist() == [0, 1] and n == 2
        assert rows[0].tobytes() == row(0, 1, (1, 1, 0), (1, 1, 0), (1, 1, 0), 1, 7)
        assert rows[1].tobytes() == row(1, 1, (2, 1, 0), (2, 1, 0), (2, 1, 0), 1, 9)
        ids, L, rows, n = R.find(field(size, {(1, 1, 0): (7, 1), (2, 1, 0): (7, 3)}), size, connectivity=connectivity)
        assert L.tolist() == [0, 0] and n == 1 and rows.tobytes() == row(0, 2, (1, 1, 0), (2, 1, 0), (3, 2, 0), 4, 7)


def test_diagonal_neighbours_join_at_26_only():
    size = (3, 3, 3)
    for a, b in (((0, 0, 0), (1, 1, 0)), ((0, 0, 0), (1, 1, 1)), ((1, 0, 1), (0, 1, 2))):
        w = field(size, {a: (2, 5), b: (2, 5)})
        assert R.find(w, size, connectivity=26)[3] == 1
        ids, L, rows, n = R.find(w, size, connectivity=6)
        assert n == 2 and L.tolist() == [0, 1] and rows["size"].tolist() == [1, 1]
    # two voxels apart is no neighbour at either
    w = field(size, {(0, 0, 0): (2, 5), (2, 0, 0): (2, 5)})
    assert R.find(w, size, connectivity=26)[3] == 2


def test_a_word_without_votes_is_unlabelled_whatever_its_class_bits():
    size = (3, 1, 1)
    w = field(size, {(0, 0, 0): (4, 1), (1, 0, 0): (4, 0), (2, 0, 0): (4, 1)})
    assert w[1] == 4
    for min_votes in (0, 1):
        ids, L, rows, n = R.find(w, size, min_votes=min_votes)
        assert ids.tolist() == [0, 2] and n == 2   # the middle voxel is no bridge


def test_min_votes_and_select_remove_their_voxels_and_cut_bridges():
    # a row of five of class 3 with votes 2 2 1 2 2, and a voxel of class 5 above its middle
    size = (5, 2, 1)
    cells = {(x, 0, 0): (3, v) for x, v in enumerate((2, 2, 1, 2, 2))}
    cells[(2, 1, 0)] = (5, 9)
    w = field(size, cells)
    ids, L, rows, n = R.find(w, size)
    assert ids.tolist() == [0, 1, 2, 3, 4, 7] and L.tolist() == [0, 0, 0, 0, 0, 5] and n == 2
    assert rows[0].tobytes() == row(0, 5, (0, 0, 0), (4, 0, 0), (10, 0, 0), 9, 3)
    assert rows[1].tobytes() == row(5, 1, (2, 1, 0), (2, 1, 0), (2, 1, 0), 9, 5)
    # min_votes = 2 removes exactly the bridge: two objects of two, and the voxel above
    ids, L, rows, n = R.find(w, size, min_votes=2)
    assert ids.tolist() == [0, 1, 3, 4, 7] and L.tolist() == [0, 0, 2, 2, 4] and n == 3
    assert rows["size"].tolist() == [2, 2, 1] and rows["votes"].tolist() == [4, 4, 9] and rows["class_id"].tolist() == [3, 3, 5]
    assert R.labelled(w, 3).tolist() == [7] and R.labelled(w, 10).tolist() == []
    # a selection of class 3 alone; of class 5 alone; one too short to reach class 5; one that reaches it but says no
    assert R.labelled(w, 1, [0, 0, 0, 1]).tolist() == [0, 1, 2, 3, 4]
    assert R.labelled(w, 1, [0, 0, 0, 0, 0, 1]).tolist() == [7]
    assert R.labelled(w, 1, [1, 1, 1, 1, 1]).tolist() == [0, 1, 2, 3, 4]
    assert R.labelled(w, 1, [1, 1, 1, 1, 1, 0]).tolist() == [0, 1, 2, 3, 4]
    assert R.labelled(w, 1, [0]).tolist() == [] and R.labelled(w, 1, []).tolist() == []
    # a bridge of another class that the selection removes: 3 3 5 3 3 is three objects anyway, and two without class 5
    w2 = field((5, 1, 1), {(x, 0, 0): (c, 1) for x, c in enumerate((3, 3, 5, 3, 3))})
    assert R.find(w2, (5, 1, 1))[3] == 3
    ids, L, rows, n = R.find(w2, (5, 1, 1), select=[0, 0, 0, 1])
    assert ids.tolist() == [0, 1, 3, 4] and L.tolist() == [0, 0, 2, 2] and n == 2
    # ... and a bridge of the same class under a diagonal: select keeps it, min_votes cuts it
    w3 = field((3, 3, 1), {(0, 0, 0): (1, 2), (1, 1, 0): (1, 1), (2, 2, 0): (1, 2)})
    assert R.find(w3, (3, 3, 1), select=[0, 1])[3] == 1 and R.find(w3, (3, 3, 1), min_votes=2)[3] == 2


def test_min_size_cuts_at_its_edge():
    # objects of 1, 2 and 3 voxels of one class, a gap between them
    size = (9, 1, 1)
    w = field(size, {(x, 0, 0): (1, 1) for x in (0, 2, 3, 5, 6, 7)})
    for min_size, sizes in ((0, [1, 2, 3]), (1, [1, 2, 3]), (2, [2, 3]), (3, [3]), (4, [])):
        ids, L, rows, n = R.find(w, size, min_size=min_size)
        assert n == 3 and L.tolist() == [0, 1, 1, 3, 3, 3]
        assert rows["size"].tolist() == sizes, min_size      # size == min_size stays, size == min_size - 1 goes
        assert rows["label"].tolist() == [[0, 1, 3][[1, 2, 3].index(s)] for s in sizes]


def test_votes_are_the_plain_sum():
    size = (4, 1, 1)
    w = field(size, {(x, 0, 0): (6, v) for x, v in enumerate((65535, 65535, 1, 7))})
    rows = R.find(w, size)[2]
    assert len(rows) == 1 and int(rows[0]["votes"]) == 65535 + 65535 + 1 + 7 and rows[0]["reserved"] == 0


def test_lookup_of_listed_unlisted_and_dropped_voxels():
    # voxels of 10 x 20 x 30 mm, the grid's corner at offset + offset_at_clear = (100, 200, 300) + (5, -5, 0)
    size, vs, offset, at_clear = (6, 2, 2), (10.0, 20.0, 30.0), (100.0, 200.0, 300.0), (5.0, -5.0, 0.0)
    w = field(size, {(0, 0, 0): (1, 1), (1, 0, 0): (1, 1), (3, 0, 0): (2, 1), (5, 1, 1): (1, 1), (4, 1, 1): (1, 1), (4, 0, 1): (1, 1)})
    ids, L, rows, n = R.find(w, size, min_size=2)
    assert n == 3 and rows["size"].tolist() == [2, 3] and rows["label"].tolist() == [0, 3]   # the single voxel of class 2 is dropped
    centre = lambda x, y, z: (105.0 + (x + 0.5) * 10.0, 195.0 + (y + 0.5) * 20.0, 300.0 + (z + 0.5) * 30.0)
    points = [centre(0, 0, 0), centre(1, 0, 0), centre(5, 1, 1), centre(4, 0, 1),    # listed: rows 0, 0, 1, 1
              centre(2, 0, 0),                                                       # unlisted
              centre(3, 0, 0),                                                       # in the dropped object
              (104.9, 200.0, 310.0), centre(6, 0, 0), centre(0, 2, 0), centre(0, 0, -1),   # off the grid
              (np.nan, 200.0, 310.0), (110.0, 200.0, np.nan),                        # NaN
              (105.0, 195.0, 300.0), (164.99, 234.9, 359.9)]                         # the grid's first corner, and just inside its last
    got = R.lookup(points, ids, L, rows, size, vs, offset, at_clear)
    N = R.NONE
    assert got.tolist() == [0, 0, 1, 1, N, N, N, N, N, N, N, N, 0, 1]
    assert R.voxel_of(centre(5, 1, 1), size, vs, offset, at_clear) == (1 * 2 + 1) * 6 + 5
    # with every object listed the dropped one has a row of its own, between the two
    ids, L, rows, n = R.find(w, size, min_size=1)
    assert R.lookup(points[:6], ids, L, rows, size, vs, offset, at_clear).tolist() == [0, 0, 2, 2, N, 1]
