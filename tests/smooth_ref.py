"""CPU reference of the mesh smoothing (include/tsdf_amd.h, "mesh smoothing", rules 1-6): the live triples in plain numpy, the
neighbour sums by np.add.at on int64, every pass in float64 from the previous pass's positions, the edge multiplicities by np.unique,
the face normals by np.add.at on int64.  Also the inputs the tests share (the hand-made cases).  No expectations live here."""
import numpy as np

from tests import components_ref

F32 = np.float32
PIN_BOUNDARY, NORMALS = 1, 2
LIMIT = F32(2.0 ** 21)


def loose_vertices(V):
    """(n,) bool: a coordinate that is not finite or not below 2^21 in magnitude (rule 1)."""
    V = np.ascontiguousarray(V, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return ~(np.isfinite(V).all(axis=1) & (np.abs(V) < LIMIT).all(axis=1))


def live_triples(V, I):
    """(m, 3) int64: the triples with three different indices and no loose corner, in their order (rule 1)."""
    tri = np.asarray(I, np.int64).reshape(-1, 3)
    loose = loose_vertices(V)
    if not len(tri):
        return tri
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
    return tri[distinct & ~loose[tri].any(axis=1)]


def degrees(V, I):
    """(n,) int64: twice the live triples that name each vertex (rule 1)."""
    return 2 * np.bincount(live_triples(V, I).reshape(-1), minlength=len(np.asarray(V).reshape(-1, 3)))


def pinned(V, I):
    """(n,) bool: the ends of the edges that exactly one live triple names (rule 4)."""
    n = len(np.asarray(V).reshape(-1, 3))
    tri = live_triples(V, I)
    out = np.zeros(n, bool)
    if not len(tri):
        return out
    ends = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [0, 2]]])
    key = (ends.min(axis=1) << 32) | ends.max(axis=1)
    keys, count = np.unique(key, return_counts=True)
    once = keys[count == 1]
    out[once >> 32] = True
    out[once & 0xFFFFFFFF] = True
    return out


def one_pass(P, tri, deg, fixed, f):
    """Rules 2 and 3: every vertex from P, the previous pass's positions."""
    with np.errstate(all="ignore"):
        q = np.where(np.isfinite(P) & (np.abs(P) < LIMIT), np.rint(P * F32(1024.0)), 0).astype(np.int64)   # (a loose vertex is in no live triple)
        S = np.zeros((len(P), 3), np.int64)
        for a, b, c in ((0, 1, 2), (1, 0, 2), (2, 0, 1)):
            np.add.at(S, tri[:, a], q[tri[:, b]] + q[tri[:, c]])
        move = (deg > 0) & ~fixed
        p = P[move].astype(np.float64)
        d = (S[move].astype(np.float64) / deg[move, None].astype(np.float64)) / 1024.0
        new = (p + np.float64(F32(f)) * (d - p)).astype(F32)
        good = (np.isfinite(new) & (np.abs(new) < LIMIT)).all(axis=1)                # rule 3: all three coordinates or none
    out = P.copy()
    at = np.flatnonzero(move)[good]
    out[at] = new[good]
    return out


def smooth(V, I, iterations, lam, mu, flags=0):
    """The smoothed positions (n, 3) float32 of rules 1-5 (the indices, normals and colours of the call are the source's bytes)."""
    V = np.ascontiguousarray(V, F32).reshape(-1, 3)
    tri = live_triples(V, I)
    deg = 2 * np.bincount(tri.reshape(-1), minlength=len(V))
    fixed = pinned(V, I) if flags & PIN_BOUNDARY else np.zeros(len(V), bool)
    P = V.copy()
    for _ in range(int(iterations)):
        for f in (lam, mu):
            if F32(f) != 0:                                          # (-0.0 == 0)
                P = one_pass(P, tri, deg, fixed, f)
    return P


def vertex_normals(V, I):
    """(n, 3) float32: the area-weighted face normals of rule 6, the NaN triple where the sum has no length."""
    V = np.ascontiguousarray(V, F32).reshape(-1, 3)
    tri = live_triples(V, I)
    D = V.astype(np.float64)
    with np.errstate(all="ignore"):
        A, B, Cc = D[tri[:, 0]], D[tri[:, 2]], D[tri[:, 1]]
        e1, e2 = B - A, Cc - A
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        k = np.rint(c * 65536.0).astype(np.int64)
        S = np.zeros((len(V), 3), np.int64)
        for corner in range(3):
            np.add.at(S, tri[:, corner], k)
        d = S.astype(np.float64)
        length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        return np.where(length[:, None] == 0.0, np.nan, d / length[:, None]).astype(F32)


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def hand_made_cases():
    """name -> (V (n, 3) float32, I (3 m,) uint32, iterations, lambda, mu): the smallest meshes at which the rows, the scans, the edge
    table and the sums can go wrong, and the factor sets."""
    rng = np.random.default_rng(50)
    nan, inf = np.nan, np.inf
    taubin = (3, 0.5, -0.53)
    cases = {}
    cases["empty"] = (np.zeros((0, 3)), [], *taubin)
    cases["no triple"] = (rng.normal(size=(5, 3)), [], *taubin)
    cases["one triangle"] = ([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], [0, 1, 2], *taubin)
    quad = [[0, 0, 0], [1, 0, 0.25], [1, 1, 0], [0, 1, -0.25]]
    cases["two triangles"] = (quad, [0, 1, 2, 0, 2, 3], *taubin)
    tetra = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    faces = [0, 1, 2, 0, 3, 1, 1, 3, 2, 0, 2, 3]                      # wired (I[3t], I[3t+2], I[3t+1]) they face outwards
    cases["tetrahedron"] = (tetra * 7.3, faces, *taubin)
    cases["to the mean"] = (tetra * 7.3 + 0.1, faces, 1, 1.0, 0.0)
    cases["mu only"] = (tetra * 3.1 - 0.7, faces, 2, 0.0, -0.5)
    cases["minus zero factors"] = (tetra * 3.1, faces, 4, -0.0, 0.0)
    cases["no iterations"] = (tetra * 3.1, faces, 0, 0.5, -0.53)
    cases["guard"] = (tetra * 1000.0 + (2.0 ** 20 - 500.0), faces, 40, -1.0, -1.0)      # rule 3 must hold it
    cases["same triple twice"] = (quad, [0, 1, 2, 2, 0, 1], *taubin)                   # m == 2: nothing pinned
    cases["same triple thrice"] = (quad, [0, 1, 2, 0, 1, 2, 1, 0, 2], *taubin)         # m == 3 does not pin either
    cases["three on one edge"] = ([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0.5], [0.5, 0, 1]], [0, 1, 2, 1, 0, 3, 0, 1, 4], *taubin)
    cases["degenerate triples"] = (quad, [0, 0, 1, 2, 2, 2, 0, 1, 2, 3, 1, 3], *taubin)
    # a dead triple does not pull its other corners: 4 is NaN, 5 inf, 6 at 2^21
    V = quad + [[nan, 0, 0], [0.5, inf, 0.5], [2.0 ** 21, 0.5, 0.5], [-2.0 ** 21, 0, 0], [2, 2, 2]]
    cases["loose corners"] = (V, [0, 1, 2, 0, 2, 3, 0, 1, 4, 1, 2, 5, 2, 3, 6, 3, 0, 7, 8, 0, 2], *taubin)
    # bytes kept: -0.0 and a denormal at vertices no live triple names
    V = quad + [[-0.0, 1e-40, -1e-40], [-0.0, -0.0, -0.0], [nan, -0.0, 1e-42]]
    cases["kept bytes"] = (V, [0, 1, 2, 0, 2, 3, 4, 4, 5, 6, 0, 1], *taubin)
    # q near 2^31
    below = np.nextafter(F32(2.0 ** 21), F32(0))
    V = [[below, below, -below], [below - 1, below, -below], [below, below - 1, -below + 0.25], [below - 0.5, below - 0.5, -below + 1]]
    cases["far out"] = (V, faces, *taubin)
    for n in (65, 129, 65537):                                        # the 64-wide chunks and the scan's part boundary
        V = np.stack([np.arange(n) * 0.5, (np.arange(n) % 2) * 1.0 + rng.normal(0, 0.05, n), rng.normal(0, 0.05, n)], axis=1)
        cases["strip %d" % n] = (V, components_ref.strip(n), 2, 0.5, -0.53)
    for first in (True, False):                                       # a row longer than a wave
        n, tri = components_ref.fan(300, first)
        angle = np.arange(301) * (2 * np.pi / 300)
        rim = np.stack([np.cos(angle) * 10, np.sin(angle) * 10, rng.normal(0, 0.3, 301)], axis=1)
        hub = np.array([[0.3, -0.2, 2.0]])
        cases["fan hub %s" % ("first" if first else "last")] = (np.concatenate([hub, rim] if first else [rim, hub]), tri, *taubin)
    cases["random 1000"] = (rng.uniform(-100, 100, (1000, 3)), components_ref.random_triples(1000, 3000, 51), *taubin)   # non-manifold everywhere
    return {name: (np.ascontiguousarray(V, F32).reshape(-1, 3), np.ascontiguousarray(I, np.uint32).reshape(-1), int(it), float(lam), float(mu))
            for name, (V, I, it, lam, mu) in cases.items()}
