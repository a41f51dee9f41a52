"""The CPU reference of the indexed mesh (tests/mesh_ref.py) against itself and against the soup it is built from (no GPU): expanding
(V, I) gives the oracle's soup bit for bit, the vertices are exactly the sign-changing lattice edges, boxes that tile the grid give
the whole soup cube for cube with identical bytes on shared edges, and the host library's marching cubes emits the same soup."""
import numpy as np
import pytest

import tsdf_amd
from tests import mesh_ref

GRIDS = [(2, 2, 2), (3, 2, 5), (64, 2, 2), (65, 3, 2), (129, 7, 3), (130, 5, 4), (17, 9, 11), (40, 33, 21)]
VS, OFF = (2.0, 3.0, 1.5), (10.0, -4.0, 0.25)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def octants(size):
    """Eight boxes that tile the cubes of the grid (an octant of a 1-cube axis is empty and is left out)."""
    cuts = [(0, (s - 1) // 2, s - 1) for s in size]
    out = []
    for k in range(2):
        for j in range(2):
            for i in range(2):
                b = (cuts[0][i], cuts[1][j], cuts[2][k], cuts[0][i + 1], cuts[1][j + 1], cuts[2][k + 1])
                if all(b[a] < b[a + 3] for a in range(3)):
                    out.append(b)
    return out


@pytest.mark.parametrize("size", GRIDS)
def test_the_expansion_is_the_oracle_soup_and_the_vertices_are_the_sign_changing_edges(oracle, size):
    D = mesh_ref.random_field(size, 1000 + size[0] + size[2])
    assert (D == 0).any() and np.isnan(D).any() and np.signbit(D[D == 0]).any()
    V, I, S, keys = mesh_ref.indexed(oracle, D, size, VS, OFF)
    assert np.array_equal(bits(S), bits(oracle.marching_cubes(D, size, VS, OFF)))
    assert I.dtype == np.uint32 and len(I) == len(S) and len(I) % 3 == 0
    assert np.array_equal(bits(V[I]), bits(S))                       # NaN vertices included: their bytes are the soup's
    assert np.array_equal(keys, mesh_ref.used_edge_keys(D, size))    # one vertex per sign-changing lattice edge, in key order
    if len(I):
        assert int(I.max()) == len(V) - 1
    # every copy of an edge in the soup has the same bytes, whichever cube emitted it
    _, _, key = mesh_ref.soup(oracle, D, size, VS, OFF)
    order = np.argsort(key, kind="stable")
    same_edge = key[order][1:] == key[order][:-1]
    assert (bits(S[order][1:]) == bits(S[order][:-1]))[same_edge].all()
    # the host library's marching cubes is the same soup
    assert np.array_equal(bits(tsdf_amd.marching_cubes(D, size, VS, OFF)), bits(S))


@pytest.mark.parametrize("size", [(3, 2, 5), (65, 3, 2), (130, 5, 4), (17, 9, 11), (40, 33, 21)])
def test_octant_boxes_give_the_whole_soup_cube_for_cube(oracle, size):
    D = mesh_ref.random_field(size, 2000 + size[0])
    S, root, key = mesh_ref.soup(oracle, D, size, VS, OFF)
    whole = dict(zip(mesh_ref.indexed(oracle, D, size, VS, OFF)[3].tolist(), bits(mesh_ref.indexed(oracle, D, size, VS, OFF)[0]).tolist()))
    covered = np.zeros(len(S), bool)
    for box in octants(size):
        V, I, Sb, keys = mesh_ref.indexed(oracle, D, size, VS, OFF, box)
        inside = np.ones(len(S), bool)
        for a in range(3):
            inside &= (root[:, a] >= box[a]) & (root[:, a] < box[a + 3])
        assert not (covered & inside).any()
        covered |= inside
        assert np.array_equal(bits(V[I]), bits(S[inside]))           # the cubes of the box, in the soup's order
        assert np.array_equal(keys, mesh_ref.used_edge_keys(D, size, box))
        for k, v in zip(keys.tolist(), bits(V).tolist()):            # an edge has the same bytes in every box that holds it
            assert whole[k] == v
    assert covered.all()


def test_boxes_are_clipped_and_degenerate_grids_are_empty(oracle):
    size = (17, 9, 11)
    D = mesh_ref.random_field(size, 5)
    assert mesh_ref.clip_box(size, (10, 2, 3, 99, 99, 99)) == [10, 2, 3, 16, 8, 10]
    a = mesh_ref.indexed(oracle, D, size, VS, OFF, (10, 2, 3, 99, 99, 99))
    b = mesh_ref.indexed(oracle, D, size, VS, OFF, (10, 2, 3, 16, 8, 10))
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and len(a[0]) > 0
    assert len(mesh_ref.indexed(oracle, D, size, VS, OFF, (16, 0, 0, 20, 5, 5))[0]) == 0      # clips to nothing
    assert len(mesh_ref.indexed(oracle, np.array([1, -1], np.float32), (2, 1, 1), VS, OFF)[0]) == 0
    assert mesh_ref.triangles(np.arange(6)).tolist() == [[0, 2, 1], [3, 5, 4]]
