"""CPU reference of the mesh components (include/tsdf_amd.h, "mesh components"): scipy's connected_components on the edges of the index
triples, every component relabelled to its smallest vertex index, sizes by np.bincount, the filter in plain numpy.  Also the inputs the
tests share (hand-made index buffers, the sphere scene).  No expectations live here."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

NO_LABEL = 0xFFFFFFFF


def label(n_vertices, indices):
    """(L (n,) uint32, T (n,) uint32, info dict) of the graph whose triples are `indices`."""
    n = int(n_vertices)
    tri = np.asarray(indices, np.int64).reshape(-1, 3)
    info = {"n_components": 0, "n_triangles": len(tri), "largest_triangles": 0, "largest_label": NO_LABEL}
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32), info
    rows, cols = np.concatenate([tri[:, 0], tri[:, 0]]), np.concatenate([tri[:, 1], tri[:, 2]])
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n))
    count, comp = connected_components(graph, directed=False)
    smallest = np.full(count, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    triangles = np.bincount(comp[tri[:, 0]], minlength=count)
    L, T = smallest[comp], triangles[comp]
    most = triangles.max()
    info.update(n_components=int(count), largest_triangles=int(most), largest_label=int(smallest[triangles == most].min()))
    return L.astype(np.uint32), T.astype(np.uint32), info


def filter_mesh(L, T, info, indices, arrays, min_triangles=0, keep_largest=False):
    """(kept arrays (each (n, ...) per vertex), kept indices uint32, keep mask per vertex) of the filter."""
    keep = T.astype(np.uint64) >= np.uint64(min(int(min_triangles), 2 ** 64 - 1))
    if keep_largest:
        keep &= L == info["largest_label"]
    new = np.cumsum(keep) - 1
    tri = np.asarray(indices, np.int64).reshape(-1, 3)
    kept = tri[keep[tri[:, 0]]] if len(tri) else tri
    return [None if a is None else a[keep] for a in arrays], new[kept].reshape(-1).astype(np.uint32), keep


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def strip(n_vertices):
    k = np.arange(n_vertices - 2)
    return np.stack([k, k + 1, k + 2], axis=1)


def fan(n_triples, hub_first):
    """n_triples triples (hub, rim k, rim k + 1) round one hub: vertex 0 or the last of the n_triples + 2."""
    k = np.arange(n_triples)
    if hub_first:
        return n_triples + 2, np.stack([np.zeros_like(k), k + 1, k + 2], axis=1)
    return n_triples + 2, np.stack([np.full_like(k, n_triples + 1), k, k + 1], axis=1)


def random_triples(n_vertices, n_triples, seed):
    """Random triples with repeated, (a, a, b) and (a, a, a) triples planted."""
    rng = np.random.default_rng(seed)
    tri = rng.integers(0, n_vertices, (n_triples, 3))
    tri[5] = tri[3]
    tri[n_triples // 2] = tri[3]
    tri[7, 1] = tri[7, 0]
    tri[11, 2] = tri[11, 0]
    tri[13] = tri[13, 0]
    tri[17] = n_vertices - 1
    return tri


def pairs(n_vertices):
    i = np.arange(n_vertices // 2)
    return np.stack([i, i, i + n_vertices // 2], axis=1)


def hand_made_cases():
    """name -> (n_vertices, indices (3 n,) uint32): the smallest graphs at which a lock-free union-find can go wrong."""
    rng = np.random.default_rng(20)
    n = 64 * 40 + 3
    s = strip(n)
    hub0, hub_last = fan(4096, True), fan(4096, False)
    cases = {
        "no triples": (5, np.zeros((0, 3), np.int64)),
        "strip forwards": (n, s),                       # deep chains, hooks that always lose their root
        "strip backwards": (n, s[::-1]),
        "strip shuffled": (n, s[rng.permutation(len(s))]),
        "fan hub first": hub0,                          # every CAS contends for one word
        "fan hub last": hub_last,
        "random 500": (5000, random_triples(5000, 500, 21)),      # below, near and above the point where one component takes over
        "random 2000": (5000, random_triples(5000, 2000, 22)),
        "random 8000": (5000, random_triples(5000, 8000, 23)),
        "pairs": (5000, pairs(5000)),
        "tie": (9, np.array([[6, 7, 8], [6, 8, 7], [3, 4, 5], [5, 4, 3], [0, 0, 0]])),   # two largest of two triples each: label 3 wins
    }
    return {k: (int(v[0]), np.ascontiguousarray(v[1], np.uint32).reshape(-1)) for k, v in cases.items()}


SCENE_SIZE = (64, 64, 64)
SCENE_SPHERES = [((22.3, 24.1, 30.2), 13.4), ((47.2, 44.6, 30.7), 7.3)]          # centre and radius in voxels: they do not touch
SCENE_BLOBS = [[(5, 5, 5)], [(58, 6, 50), (59, 6, 50)], [(6, 57, 12)]]             # voxels set negative: one, two and one
SCENE_MIN_TRIANGLES = 100   # above every blob (8 or 16 triangles), below the smaller sphere (hundreds)


def sphere_scene():
    """Distances of a 64^3 volume: two spheres of different radii and three blobs of one or two voxels, far from each other."""
    X, Y, Z = SCENE_SIZE
    z, y, x = np.mgrid[0:Z, 0:Y, 0:X].astype(np.float64)
    D = np.full((Z, Y, X), 1.0)
    for (cx, cy, cz), r in SCENE_SPHERES:
        D = np.minimum(D, np.clip((np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r) / 3.0, -1.0, 1.0))
    for blob in SCENE_BLOBS:
        for bx, by, bz in blob:
            D[bz, by, bx] = -0.5
    return D.astype(np.float32).reshape(-1)
