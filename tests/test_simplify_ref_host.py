"""The CPU reference of the mesh simplification (tests/simplify_ref.py) on its own (no GPU): it matches a per-vertex Python dictionary
on every hand-made case and on the random-field meshes, the hand-made cases give what the contract says in so many words, and the
meshes of tests/test_simplify.py meet the conditions those tests rely on."""
import math

import numpy as np
import pytest

from tests import components_ref
from tests import mesh_ref
from tests import simplify_ref as ref
from tests.helpers import assert_same_floats
from tests.test_components_ref_host import MESH_GRIDS, mesh_seed

CASES = ref.hand_made_cases()
F32 = np.float32
FIELD_CELL = 25.0


def naive(V, I, h, N, RGB):
    """Rules 1-6 one vertex at a time, in Python integers and floats."""
    h = F32(h)
    first, members = {}, []
    for v, p in enumerate(V):
        with np.errstate(all="ignore"):
            f = [math.floor(float(a / h)) if np.isfinite(a / h) else None for a in p]
        loose = any(not np.isfinite(a) or not abs(float(a)) < 2.0 ** 21 for a in p) or any(c is None or not abs(c) < 2 ** 20 for c in f)
        key = ("loose", v) if loose else ((f[2] + 2 ** 20) << 42) | ((f[1] + 2 ** 20) << 21) | (f[0] + 2 ** 20)
        if key not in first:
            first[key] = len(members)
            members.append([])
        members[first[key]].append(v)
    members.sort(key=lambda m: m[0])                                  # (already so: clusters appear in the order of their first member)
    new = {v: j for j, m in enumerate(members) for v in m}
    oV, oN, oC = [], [], []
    for m in members:
        n = len(m)
        if n == 1:
            oV.append(V[m[0]])
            oN.append(None if N is None else N[m[0]])
            oC.append(None if RGB is None else RGB[m[0]])
            continue
        oV.append([F32(float(sum(int(np.rint(V[v][a] * F32(1024.0))) for v in m)) / float(n) / 1024.0) for a in range(3)])
        if N is not None:
            ok = [v for v in m if all(np.isfinite(N[v]))]
            d = [float(sum(int(np.rint(N[v][a] * F32(1048576.0))) for v in ok)) for a in range(3)]
            length = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            oN.append([F32(np.nan) if length == 0.0 else F32(c / length) for c in d])
        if RGB is not None:
            oC.append([(2 * sum(int(RGB[v][a]) for v in m) + n) // (2 * n) for a in range(3)])
    tri = [[new[int(i)] for i in t] for t in np.asarray(I).reshape(-1, 3)]
    oI = [i for t in tri if len(set(t)) == 3 for i in t]
    return (np.array(oV, F32).reshape(-1, 3), np.array(oI, np.uint32), None if N is None else np.array(oN, F32).reshape(-1, 3),
            None if RGB is None else np.array(oC, np.uint8).reshape(-1, 3))


def assert_equal_meshes(got, want, what):
    assert got[0].shape == want[0].shape and got[0].dtype == F32, what
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) or not np.isfinite(want[0]).all(), what   # -0.0 is not 0.0
    assert_same_floats(got[0], want[0], what + ": vertices")
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], want[1]), what + ": indices"
    for k, name in ((2, "normals"), (3, "colours")):
        assert (got[k] is None) == (want[k] is None), what
        if got[k] is not None and k == 2:
            assert_same_floats(got[k], want[k], what + ": normals")
        elif got[k] is not None:
            assert got[k].dtype == np.uint8 and np.array_equal(got[k], want[k]), what + ": colours"


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_reference_matches_a_dictionary_on_the_hand_made_cases(name):
    V, I, h, N, C = CASES[name]
    assert_equal_meshes(ref.simplify(V, I, h, N, C)[:4], naive(V, I, h, N, C), name)


def field_mesh(oracle, size):
    return mesh_ref.indexed(oracle, mesh_ref.random_field(size, mesh_seed(size)), size, ref.FIELD_VS, ref.FIELD_OFFSET)[:2]


@pytest.mark.parametrize("size", MESH_GRIDS)
def test_the_reference_matches_a_dictionary_on_the_random_field_meshes(oracle, size):
    V, I = field_mesh(oracle, size)
    rng = np.random.default_rng(size[0])
    N, C = ref.unit(rng, len(V)), rng.integers(0, 256, (len(V), 3)).astype(np.uint8)
    N[::17] = np.nan
    assert_equal_meshes(ref.simplify(V, I, FIELD_CELL, N, C)[:4], naive(V, I, FIELD_CELL, N, C), "grid %s" % (size,))


def test_the_hand_made_cases_give_what_the_contract_says():
    bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32).tolist()
    V, I, h, N, C = CASES["one cell"]
    oV, oI, oN, oC, _ = ref.simplify(V, I, h, N, C)
    assert oV.shape == (1, 3) and len(oI) == 0 and oN.shape == (1, 3) and oC.shape == (1, 3)
    assert np.abs(oV[0] - V.astype(np.float64).mean(axis=0)).max() < 1e-3 and abs(float(np.linalg.norm(oN[0])) - 1.0) < 1e-6
    V, I, h, N, C = CASES["own cells"]                                # the identity
    oV, oI, oN, oC, cluster = ref.simplify(V, I, h, N, C)
    assert bits(oV) == bits(V) and np.array_equal(oI, I) and bits(oN) == bits(N) and np.array_equal(oC, C)
    assert np.array_equal(cluster, np.arange(len(V)))
    V, I, h, N, C = CASES["70000 in 30000"]
    oV, oI, _, _, cluster = ref.simplify(V, I, h, N, C)
    assert 25000 < len(oV) < 30000 and 0 < len(oI) < len(I) and (len(V) + 63) // 64 > 1024
    for n in (63, 64, 65, 64 * 1024 + 1):
        V, I, h, N, C = CASES["paired %d" % n]
        oV, oI, _, _, _ = ref.simplify(V, I, h, N, C)
        assert len(V) == n and len(I) == 3 * n and n // 2 <= len(oV) <= n // 2 + 3 and 0.45 * n < len(oI) // 3 < 0.55 * n
    V, I, h, N, C = CASES["interleaved"]
    oV, oI, _, _, cluster = ref.simplify(V, I, h, N, C)
    assert cluster.tolist() == [0, 1] * 5 + [2, 2] and oI.tolist() == [0, 1, 2, 2, 1, 0, 0, 1, 2, 1, 0, 2] and len(oV) == 3
    V, I, h, _, _ = CASES["cell edges"]
    loose, key = ref.cells(V, h)
    assert not loose.any()
    fx = (key & (2 ** 21 - 1)) - 2 ** 20
    k = np.arange(-5, 6)
    assert (fx[1:33:3] == fx[0:33:3]).all() and (fx[2:33:3] == fx[0:33:3] - 1).all()      # just above: the same cell; just below: the one before
    assert (fx[0:33:3] == k).all()                                                           # (k * 0.1f) / 0.1f rounds back to k
    assert (np.abs(fx[35:] - np.arange(-9, 10)) <= 1).all()
    assert fx[33] == 0 and fx[34] == 0                                                       # -0.0 and 0.0 share cell 0
    V, I, h, N, C = CASES["loose"]
    oV, oI, oN, oC, cluster = ref.simplify(V, I, h, N, C)
    loose = ref.cells(V, h)[0]
    assert loose.tolist() == [True] * 6 + [False, False, True, True, False, False, False, False, False, False, True, True]
    assert cluster[3] != cluster[4] and cluster[6] == cluster[7] and cluster[10] == cluster[11] and cluster[13] == cluster[14]
    assert cluster[12] == cluster[15] and len(oV) == 14
    assert bits(oV[cluster[3]]) == bits(V[3]) and bits(oV[cluster[5]]) == bits(V[5]) and bits(oN[cluster[16]]) == bits(N[16])
    assert oV[cluster[6]].tolist() == [2.0 ** 20 - 0.375, 0.5, 0.5] and oV[cluster[13]].tolist() == [0.375, 2.0 ** 20 - 0.625, -2.0 ** 20 + 1.375]
    V, I, h, _, _ = CASES["far out"]
    loose = ref.cells(V, h)[0]
    assert loose.tolist() == [True, False, False, True, False, False, False]
    V, I, h, N, C = CASES["singles"]
    oV, oI, oN, oC, cluster = ref.simplify(V, I, h, N, C)
    assert cluster.tolist() == [0, 1, 2, 3, 3]
    assert bits(oV[:3]) == bits(V[:3]) and bits(oN[:3]) == bits(N[:3]) and np.array_equal(oC[:3], C[:3])
    assert np.signbit(oV[0, 0]) and oV[1, 0] > 0 and oV[1, 0] < 1e-38 and np.signbit(oV[2, 2]) and np.signbit(oN[0, 0])
    assert oV[3].tolist() == [3.375, 3.625, 3.5] and oC[3].tolist() == [11, 21, 30]
    V, I, h, _, _ = CASES["triples"]
    oV, oI, _, _, cluster = ref.simplify(V, I, h)
    assert cluster.tolist() == [0, 0, 1, 2, 3, 0]
    assert oI.reshape(-1, 3).tolist() == [[0, 1, 2], [3, 2, 1], [0, 3, 2], [3, 1, 0]]      # order and winding kept
    V, I, h, N, _ = CASES["no indices"]
    oV, oI, oN, _, _ = ref.simplify(V, I, h, N)
    assert len(oV) == 4 and oI.shape == (0,) and oI.dtype == np.uint32 and oN.shape == (4, 3)
    V, I, h, _, _ = CASES["empty"]
    oV, oI, _, _, _ = ref.simplify(V, I, h)
    assert oV.shape == (0, 3) and oI.shape == (0,)
    V, I, h, N, _ = CASES["normals"]
    oN = ref.simplify(V, I, h, N)[2]
    want = np.array([0.0, 0.6, 1.8]) / math.sqrt(0.36 + 3.24)
    assert oN.shape == (3, 3) and np.abs(oN[0] - want).max() < 1e-6 and np.isnan(oN[1]).all() and np.isnan(oN[2]).all()
    V, I, h, _, C = CASES["colours"]
    oC = ref.simplify(V, I, h, None, C)[3]
    assert oC.tolist() == [[1, 1, 255], [0, 0, 1], [255, 255, 255]]   # {0, 1} -> 1, {0, 0, 1} -> 0, {255, 255} -> 255; {255, 254} -> 255


@pytest.fixture(scope="module")
def sphere_mesh(oracle):
    V, I, _, _ = mesh_ref.indexed(oracle, components_ref.sphere_scene(), components_ref.SCENE_SIZE, (10.0, 10.0, 10.0))
    return V, I


def test_the_sphere_scene_at_20_mm_keeps_less_than_a_quarter(sphere_mesh):
    V, I = sphere_mesh
    N = ref.sphere_normals(V, components_ref.SCENE_SPHERES, 10.0)
    oV, oI, oN, _, cluster = ref.simplify(V, I, 20.0, N)
    assert (len(V), len(I) // 3) == (4422, 8824)
    assert (len(oV), len(oI) // 3) == (871, 1728)                     # 0.197 and 0.196 of the source
    assert len(oV) < len(V) / 4 and len(oI) < len(I) / 4
    assert np.abs(np.linalg.norm(oN.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    oV, oI, _, _, _ = ref.simplify(V, I, 40.0)
    assert (len(oV), len(oI) // 3) == (247, 480)


def test_a_tiny_cell_only_welds(sphere_mesh):
    V, I = sphere_mesh
    h = 2.0 ** -8
    oV, oI, _, _, cluster = ref.simplify(V, I, h)
    assert (len(oV), len(oI) // 3) == (4410, 8800)
    # the clusters are exactly the sets of equal positions (+0.0 == -0.0), every output vertex is a source position, and the kept
    # triples are those with three distinct positions, in order
    _, same = np.unique(V + F32(0.0), axis=0, return_inverse=True)
    same = same.reshape(-1)
    assert len(np.unique(np.stack([same, cluster], axis=1), axis=0)) == len(np.unique(same)) == len(np.unique(cluster)) == len(oV)
    first = np.full(len(oV), len(V), np.int64)
    np.minimum.at(first, cluster, np.arange(len(V)))
    assert np.array_equal(oV, V[first])
    tri = cluster[I.astype(np.int64)].reshape(-1, 3)
    keep = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
    assert np.array_equal(oV[oI], V[I.astype(np.int64).reshape(-1, 3)[keep].reshape(-1)])


def test_the_random_field_mesh_has_every_kind_of_cluster(oracle):
    size = (40, 33, 21)
    V, I = field_mesh(oracle, size)
    oV, oI, _, _, cluster = ref.simplify(V, I, FIELD_CELL)
    count = np.bincount(cluster)
    loose = ref.cells(V, FIELD_CELL)[0]
    assert (count > 1).sum() >= 100 and (count == 1).sum() >= 1 and loose.sum() >= 1
    assert 0 < len(oI) < len(I)
    assert np.isnan(V[loose]).any(axis=1).all()                        # the loose ones are the NaN crossings


@pytest.mark.parametrize("size", MESH_GRIDS)
def test_the_random_field_meshes_carry_loose_vertices(oracle, size):
    V, I = field_mesh(oracle, size)
    assert 1 <= int(ref.cells(V, FIELD_CELL)[0].sum()) <= 4
