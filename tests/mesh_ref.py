"""CPU reference of the indexed mesh (include/tsdf_amd.h, "indexed mesh"), built only from the oracle's marching cubes
(oracle.marching_cubes: the reference's triangle soup), its tables (oracle.mc_tables) and the reference's corner and edge numbering:
the cube types give every soup vertex its cube and its lattice edge, V is the soup's first vertex per sorted unique edge key, I the
inverse map.  A box filters the soup by cube.  No expectations live here."""
import numpy as np

CORNER = np.array([[0, 0, 1], [1, 0, 1], [1, 0, 0], [0, 0, 0], [0, 1, 1], [1, 1, 1], [1, 1, 0], [0, 1, 0]])   # MarkAndSweepMC.cu:80-97
EDGE = np.array([(0, 1), (2, 1), (3, 2), (3, 0), (4, 5), (6, 5), (7, 6), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)])   # :291-302
# every edge runs in the positive direction of one axis: its lower end (as an offset from the cube's root) and that axis
EDGE_LOWER = CORNER[EDGE[:, 0]]
EDGE_AXIS = np.argmax(CORNER[EDGE[:, 1]] - CORNER[EDGE[:, 0]], axis=1)
assert ((CORNER[EDGE[:, 1]] - CORNER[EDGE[:, 0]]).sum(axis=1) == 1).all() and ((CORNER[EDGE[:, 1]] - CORNER[EDGE[:, 0]]) >= 0).all()


def clip_box(size, box):
    """The box as the library clips it: ends at most size - 1 and never below the begins; None is the whole grid."""
    last = [max(int(s) - 1, 0) for s in size]
    if box is None:
        return [0, 0, 0] + last
    lo = [int(b) for b in box[:3]]
    return lo + [max(min(int(box[a + 3]), last[a]), lo[a]) for a in range(3)]


def soup(oracle, dist, size, voxel_size, offset=(0.0, 0.0, 0.0)):
    """The oracle's soup S (n, 3) float32, and per soup vertex: the root (x, y, z) of its cube (n, 3) and its lattice-edge key
    ((z Y + y) X + x) 3 + axis (n,) int64."""
    X, Y, Z = (int(v) for v in size)
    S = oracle.marching_cubes(dist, size, voxel_size, offset)
    if min(X, Y, Z) < 2:
        assert len(S) == 0
        return S, np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    table, counts = oracle.mc_tables()
    neg = (np.asarray(dist, np.float32).reshape(Z, Y, X) < 0)
    kind = np.zeros((Z - 1, Y - 1, X - 1), np.int64)
    for i, (dx, dy, dz) in enumerate(CORNER):
        kind |= neg[dz:Z - 1 + dz, dy:Y - 1 + dy, dx:X - 1 + dx].astype(np.int64) << i
    kind = kind.reshape(-1)                                   # cubes x fastest, then y, then z: the soup's order
    n = counts[kind].astype(np.int64)
    assert n.sum() == len(S)
    cube = np.repeat(np.arange(len(kind)), n)
    nth = np.arange(len(S)) - np.repeat(np.cumsum(n) - n, n)  # which entry of its cube's table row
    edge = table[kind[cube], nth].astype(np.int64)
    assert (edge >= 0).all()
    root = np.stack([cube % (X - 1), (cube // (X - 1)) % (Y - 1), cube // ((X - 1) * (Y - 1))], axis=1)
    low = root + EDGE_LOWER[edge]
    key = ((low[:, 2] * Y + low[:, 1]) * X + low[:, 0]) * 3 + EDGE_AXIS[edge]
    return S, root, key


def indexed(oracle, dist, size, voxel_size, offset=(0.0, 0.0, 0.0), box=None):
    """(V (nv, 3) float32, I (ni,) uint32, S (ni, 3) float32 the soup of the marched cubes, keys (nv,) int64)."""
    S, root, key = soup(oracle, dist, size, voxel_size, offset)
    if box is not None:
        b = clip_box(size, box)
        keep = np.ones(len(S), bool)
        for a in range(3):
            keep &= (root[:, a] >= b[a]) & (root[:, a] < b[a + 3])
        S, key = S[keep], key[keep]
    keys, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    return np.ascontiguousarray(S[first]).reshape(-1, 3), inverse.reshape(-1).astype(np.uint32), S, keys


def used_edge_keys(dist, size, box=None):
    """The keys of the lattice edges whose ends differ in d < 0 and that touch a marched cube, sorted: counted without marching."""
    X, Y, Z = (int(v) for v in size)
    if min(X, Y, Z) < 2:
        return np.zeros(0, np.int64)
    b = clip_box(size, box)
    neg = (np.asarray(dist, np.float32).reshape(Z, Y, X) < 0)
    zz, yy, xx = np.mgrid[0:Z, 0:Y, 0:X]
    pos = [xx, yy, zz]
    out = []
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[2 - axis], hi[2 - axis] = slice(0, -1), slice(1, None)
        m = neg[tuple(lo)] != neg[tuple(hi)]
        for a in range(3):   # along its axis the edge's cube range is half open, across it closed (a cube on either side)
            p = pos[a][tuple(lo)]
            m &= (p >= b[a]) & ((p < b[a + 3]) if a == axis else (p <= b[a + 3]))
        if not all(b[a] < b[a + 3] for a in range(3)):
            m &= False
        out.append(((zz[tuple(lo)][m] * Y + yy[tuple(lo)][m]) * X + xx[tuple(lo)][m]) * 3 + axis)
    return np.sort(np.concatenate(out))


def random_field(size, seed):
    """Uniform noise with half the voxels set to 1.0 and 0.0, -0.0 and NaN planted (none of the three is < 0)."""
    rng = np.random.default_rng(seed)
    n = int(size[0]) * int(size[1]) * int(size[2])
    D = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    D[rng.random(n) < 0.5] = 1.0
    at = rng.choice(n, min(n, 6), replace=False)
    D[at] = np.array([0.0, -0.0, np.nan, 0.0, -0.0, np.nan], np.float32)[:len(at)]
    return D


def triangles(I):
    """(n, 3) triangles wired as extract_surface wires them: (I[3t], I[3t+2], I[3t+1])."""
    return np.ascontiguousarray(np.asarray(I).reshape(-1, 3)[:, [0, 2, 1]])
