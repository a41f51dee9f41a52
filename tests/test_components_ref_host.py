"""The CPU reference of the mesh components (tests/components_ref.py) on its own (no GPU): it matches a ten-line union-find on every
hand-made case, obeys the tie rule, counts isolated vertices and degenerate triples as the contract says, its filter at 0 is the
identity -- and the inputs of tests/test_components.py meet the conditions those tests rely on."""
import numpy as np
import pytest

from tests import components_ref as ref
from tests import mesh_ref

CASES = ref.hand_made_cases()
MESH_GRIDS = [(3, 2, 5), (65, 3, 2), (130, 5, 4), (40, 33, 21)]
VS, OFF = (2.0, 3.0, 1.5), (10.0, -4.0, 0.25)


def mesh_seed(size):
    return 6000 + size[0] + size[2]


def union_find(n, indices):
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    tri = np.asarray(indices, np.int64).reshape(-1, 3).tolist()
    for a, b, c in tri:
        for u in (b, c):
            ra, ru = find(a), find(u)
            parent[max(ra, ru)] = min(ra, ru)
    L = [find(v) for v in range(n)]
    count = {}
    for a, _, _ in tri:
        count[L[a]] = count.get(L[a], 0) + 1
    return L, [count.get(l, 0) for l in L]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_reference_matches_a_plain_union_find(name):
    n, I = CASES[name]
    L, T, info = ref.label(n, I)
    uL, uT = union_find(n, I)
    assert L.dtype == np.uint32 and T.dtype == np.uint32
    assert L.tolist() == uL and T.tolist() == uT
    roots = sorted(set(uL))
    assert info["n_components"] == len(roots) and info["n_triangles"] == len(I) // 3
    best = max(roots, key=lambda r: (uT[r], -r))
    assert (info["largest_triangles"], info["largest_label"]) == (uT[best], best)
    assert (L <= np.arange(n)).all() and (L[L] == L).all()


def test_ties_isolated_vertices_and_degenerate_triples():
    n, I = CASES["tie"]
    L, T, info = ref.label(n, I)
    assert L.tolist() == [0, 1, 2, 3, 3, 3, 6, 6, 6] and T.tolist() == [1, 0, 0, 2, 2, 2, 2, 2, 2]
    assert info == {"n_components": 5, "n_triangles": 5, "largest_triangles": 2, "largest_label": 3}     # ties go to the smallest label
    L, T, info = ref.label(5, CASES["no triples"][1])
    assert L.tolist() == [0, 1, 2, 3, 4] and not T.any() and info["n_components"] == 5
    assert (info["largest_triangles"], info["largest_label"]) == (0, 0)
    L, T, info = ref.label(4, [1, 1, 3, 1, 1, 3, 2, 2, 2])            # (a, a, b) twice joins 1 and 3 and counts twice; (a, a, a) counts once
    assert L.tolist() == [0, 1, 2, 1] and T.tolist() == [0, 2, 1, 2]
    assert ref.label(0, [])[2] == {"n_components": 0, "n_triangles": 0, "largest_triangles": 0, "largest_label": 0xFFFFFFFF}
    n, I = CASES["pairs"]
    L, T, info = ref.label(n, I)
    assert info["n_components"] == n // 2 and (T == 1).all() and np.array_equal(L, np.arange(n) % (n // 2))
    for name in ("random 500", "random 2000", "random 8000"):        # what was planted is there
        tri = CASES[name][1].reshape(-1, 3)
        assert (tri[5] == tri[3]).all() and tri[7, 0] == tri[7, 1] and len(set(tri[13])) == 1
    shares = [ref.label(*CASES[k])[2] for k in ("random 500", "random 2000", "random 8000")]
    # (a giant component appears at about n / 6 = 833 random triples)  below: none; at 2000 it coexists with many; at 8000 it is all
    assert shares[0]["largest_triangles"] < 50 and shares[0]["n_components"] > 3000
    assert 1000 < shares[1]["largest_triangles"] < 2000 and shares[1]["n_components"] > 1000
    assert shares[2]["largest_triangles"] >= 7900 and shares[2]["n_components"] < 100


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_filter_at_zero_is_the_identity(name):
    n, I = CASES[name]
    L, T, info = ref.label(n, I)
    payload = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    (kept,), kI, keep = ref.filter_mesh(L, T, info, I, [payload], 0)
    assert keep.all() and np.array_equal(kept, payload) and np.array_equal(kI, I) and kI.dtype == np.uint32
    # ... and a threshold nothing reaches leaves nothing
    (kept,), kI, keep = ref.filter_mesh(L, T, info, I, [payload], 2 ** 40)
    assert not keep.any() and len(kept) == 0 and len(kI) == 0
    # keep_largest keeps exactly the largest component's vertices, renumbered in order
    (kept,), kI, keep = ref.filter_mesh(L, T, info, I, [payload], 0, keep_largest=True)
    assert np.array_equal(keep, L == info["largest_label"]) and len(kI) == 3 * info["largest_triangles"]
    if len(kI):
        assert np.array_equal(kept[kI], payload[I.reshape(-1, 3)[keep[I[0::3]]].reshape(-1)])


def test_the_sphere_scene_has_five_components_and_the_threshold_separates_them(oracle):
    V, I, _, _ = mesh_ref.indexed(oracle, ref.sphere_scene(), ref.SCENE_SIZE, (10.0, 10.0, 10.0))
    L, T, info = ref.label(len(V), I)
    assert info["n_components"] == 5
    sizes = sorted(T[np.unique(L)].tolist())
    assert sizes[2] < ref.SCENE_MIN_TRIANGLES < sizes[3] < sizes[4]           # three blobs, then the two spheres
    assert sizes[:3] == [8, 8, 16] and info["largest_triangles"] == sizes[4]      # an octahedron round a lone voxel, two joined


@pytest.mark.parametrize("size", MESH_GRIDS)
def test_the_random_field_meshes_have_components_of_several_sizes(oracle, size):
    V, I, _, _ = mesh_ref.indexed(oracle, mesh_ref.random_field(size, mesh_seed(size)), size, VS, OFF)
    L, T, info = ref.label(len(V), I)
    assert info["n_components"] >= 3 and len(set(T[np.unique(L)].tolist())) >= 2
