"""CPU reference of the mesh simplification (include/tsdf_amd.h, "mesh simplification", rules 1-6): np.unique on the cell keys, the
representatives by np.minimum.at, the sums by np.add.at on int64, the divisions in float64.  Also the inputs the tests share (the
hand-made cases, the geometry of the random-field meshes).  No expectations live here."""
import numpy as np

F32 = np.float32
FIELD_VS, FIELD_OFFSET = (10.0, 12.5, 9.0), (100.0, -50.0, 25.0)      # tests/test_mesh_indexed.volume_of's voxel size and offset


def cells(V, h):
    """(loose (n,) bool, key (n,) int64, 0 where loose) of (n, 3) float32 vertices: rule 1."""
    V = np.ascontiguousarray(V, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        f = np.floor(V / F32(h))                                      # one fp32 divide, then floor
        loose = ~(np.isfinite(V).all(axis=1) & (np.abs(f) < F32(2 ** 20)).all(axis=1) & (np.abs(V) < F32(2 ** 21)).all(axis=1))
    c = np.where(loose[:, None], 0, f).astype(np.int64) + 2 ** 20
    return loose, np.where(loose, 0, (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0])


def clusters(V, h):
    """(cluster (n,) int64: the output index of every vertex; representative (m,) int64: the smallest member of every output vertex;
    count (m,) int64; loose (n,) bool): rules 1 and 2."""
    loose, key = cells(V, h)
    n = len(loose)
    _, group = np.unique(key[~loose], return_inverse=True)
    groups = (int(group.max()) + 1) if group.size else 0
    of = np.empty(n, np.int64)
    of[~loose] = group.reshape(-1)
    of[loose] = groups + np.arange(int(loose.sum()))
    rep = np.full(groups + int(loose.sum()), n, np.int64)
    np.minimum.at(rep, of, np.arange(n))
    order = np.argsort(rep, kind="stable")
    new = np.empty(len(rep), np.int64)
    new[order] = np.arange(len(rep))
    cluster = new[of]
    return cluster, rep[order], np.bincount(cluster, minlength=len(rep)).astype(np.int64), loose


def simplify(V, I, h, N=None, RGB=None):
    """(V', I' uint32, N' or None, RGB' or None, cluster (n,) int64) of rules 1-6."""
    V = np.ascontiguousarray(V, F32).reshape(-1, 3)
    I = np.asarray(I, np.int64).reshape(-1)
    cluster, rep, count, loose = clusters(V, h)
    m, many = len(rep), count > 1
    live = ~loose                                                     # (a loose vertex is alone: its sums are never used)
    with np.errstate(all="ignore"):
        oV = V[rep].copy()
        S = np.zeros((m, 3), np.int64)
        np.add.at(S, cluster[live], np.rint(V[live] * F32(1024.0)).astype(np.int64))
        oV[many] = ((S[many].astype(np.float64) / count[many, None].astype(np.float64)) / 1024.0).astype(F32)
        oN = oC = None
        if N is not None:
            N = np.ascontiguousarray(N, F32).reshape(-1, 3)
            oN = N[rep].copy()
            use = live & np.isfinite(N).all(axis=1)
            S = np.zeros((m, 3), np.int64)
            np.add.at(S, cluster[use], np.rint(N[use] * F32(1048576.0)).astype(np.int64))
            d = S[many].astype(np.float64)
            length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
            oN[many] = np.where(length[:, None] == 0.0, np.nan, d / length[:, None]).astype(F32)
        if RGB is not None:
            RGB = np.ascontiguousarray(RGB, np.uint8).reshape(-1, 3)
            oC = RGB[rep].copy()
            S = np.zeros((m, 3), np.int64)
            np.add.at(S, cluster, RGB.astype(np.int64))
            oC[many] = ((2 * S[many] + count[many, None]) // (2 * count[many, None])).astype(np.uint8)
    tri = cluster[I].reshape(-1, 3)
    keep = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
    return oV, tri[keep].reshape(-1).astype(np.uint32), oN, oC, cluster


def duplicate_triangles(I):
    """How many triangles of I are repeats of an earlier one on the same three vertices, whatever their order."""
    tri = np.sort(np.asarray(I, np.int64).reshape(-1, 3), axis=1)
    return len(tri) - len(np.unique(tri, axis=0)) if len(tri) else 0


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def strip(n):
    k = np.arange(max(n - 2, 0))
    return np.stack([k, k + 1, k + 2], axis=1)


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(F32)


def paired(n):
    """n vertices, two per unit cell along x, and n triples (t, t + 1, t + 3) mod n: those of an even t have two corners in one cell
    and die, those of an odd t live, so the keep bits alternate."""
    rng = np.random.default_rng(40 + n % 1000)
    V = np.stack([np.arange(n) // 2 + rng.random(n), rng.random(n), rng.random(n)], axis=1).astype(F32)
    t = np.arange(n)
    return V, np.stack([t, (t + 1) % n, (t + 3) % n], axis=1), 1.0, unit(rng, n), rng.integers(0, 256, (n, 3))


def hand_made_cases():
    """name -> (V (n, 3) float32, I (3 m,) uint32, cell_size, N (n, 3) float32 or None, RGB (n, 3) uint8 or None): the smallest meshes
    at which the cell table, the scans, the order and the sums can go wrong."""
    rng = np.random.default_rng(30)
    cases = {}
    # one contended slot, one row of sums
    n = 4096
    cases["one cell"] = (rng.random((n, 3)) * 0.999, rng.integers(0, n, (500, 3)), 1.0, unit(rng, n), rng.integers(0, 256, (n, 3)))
    # the table at its highest load, and the identity
    n = 2000
    c = rng.permutation(20 ** 3)[:n]
    own = np.stack([c % 20, (c // 20) % 20, c // 400], axis=1) - 7 + rng.random((n, 3)) * 0.999
    cases["own cells"] = (own, strip(n), 1.0, unit(rng, n), rng.integers(0, 256, (n, 3)))
    # long probe walks, and a scan of more than one part (70 000 / 64 > 1024)
    n = 70000
    c = rng.integers(0, 30000, n)
    many = np.stack([c % 40, (c // 40) % 40, c // 1600], axis=1) - 11 + rng.random((n, 3)) * 0.999
    cases["70000 in 30000"] = (many, rng.integers(0, n, (n, 3)), 1.0, None, rng.integers(0, 256, (n, 3)))
    for n in (63, 64, 65, 64 * 1024 + 1):                             # ballot and scan boundaries, in vertices and in triples
        cases["paired %d" % n] = paired(n)
    # order by representative and the remapping: a b a b ..., then a cluster whose smallest member is the last vertex but one
    cell = np.array([0, 1] * 5 + [2, 2])
    V = np.stack([cell * 3 + rng.random(12), rng.random(12), rng.random(12)], axis=1)
    cases["interleaved"] = (V, [[0, 1, 10], [11, 1, 0], [2, 3, 11], [1, 2, 10], [10, 11, 0]], 1.0, unit(rng, 12), rng.integers(0, 256, (12, 3)))
    # cell edges: h = 0.1f is not exactly representable; exactly k h, either side of it, negative cells, -0.0
    h = F32(0.1)
    x = []
    for k in range(-5, 6):
        e = F32(k) * h
        x += [e, np.nextafter(e, F32(np.inf)), np.nextafter(e, F32(-np.inf))]
    x = np.array(x + [F32(-0.0), F32(0.0)] + [F32(k / 10.0) for k in range(-9, 10)], F32)    # ... and the decimals nearest k / 10
    V = np.stack([x, np.full(len(x), 0.05, F32), np.roll(x, 7)], axis=1)
    cases["cell edges"] = (V, strip(len(x)), h, None, None)
    # loose vertices: NaN, +-inf, a cell index of exactly 2^20 and those just inside, two NaN vertices of the same bytes
    nan, inf, big = np.nan, np.inf, 2.0 ** 20
    V = [[nan, 0, 0], [0.5, inf, 0.5], [0.5, 0.5, -inf], [nan, nan, nan], [nan, nan, nan], [big, 0.5, 0.5], [big - 0.5, 0.5, 0.5],
         [big - 0.25, 0.5, 0.5], [-big, 0.5, 0.5], [-big + 0.5, 0.5, 0.5], [-big + 1, 0.5, 0.5], [-big + 1.5, 0.25, 0.25], [0.5, 0.5, 0.5],
         [0.5, big - 0.5, -big + 1.5], [0.25, big - 0.75, -big + 1.25], [0.75, 0.75, 0.25], [2.0 ** 21, 0.5, 0.5], [0.5, -2.0 ** 21, 0.5]]
    cases["loose"] = (V, strip(len(V)), 1.0, unit(rng, len(V)), rng.integers(0, 256, (len(V), 3)))
    # |V| = 2^21 is loose whatever its cell; the float below is not
    below = np.nextafter(F32(2.0 ** 21), F32(0))
    V = [[2.0 ** 21, 1, 1], [below, 1, 1], [below, 2, 3], [1, -2.0 ** 21, 1], [1, -below, 1], [2, -below, 3], [1, 1, 1]]
    cases["far out"] = (V, strip(len(V)), 4.0, None, None)
    # singles keep their bytes: -0.0 and denormals, in positions, normals and colours
    V = [[-0.0, 0.5, 0.5], [1e-40, 1.5, 0.5], [-1e-40, 2.5, -0.0], [3.5, 3.5, 3.5], [3.25, 3.75, 3.5]]
    N = [[-0.0, -0.0, 1.0], [1e-40, 1.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    cases["singles"] = (V, strip(5), 1.0, N, [[0, 0, 0], [255, 255, 255], [1, 2, 3], [10, 20, 30], [11, 21, 30]])
    # triples: a source-degenerate one, two corners in one cluster, all three in one, all distinct; order and winding stay
    V = [[0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0.5, 0.25, 0.75]]
    cases["triples"] = (V, [[0, 0, 2], [0, 2, 3], [0, 1, 2], [4, 3, 2], [0, 1, 5], [5, 4, 3], [3, 3, 3], [4, 2, 1]], 1.0, None, None)
    cases["no indices"] = (V, np.zeros((0, 3), np.int64), 1.0, unit(rng, 6), None)
    cases["empty"] = (np.zeros((0, 3)), np.zeros((0, 3), np.int64), 1.0, None, None)
    # normals: a NaN member is skipped, all members NaN give NaN, exactly opposite normals give NaN
    V = [[0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [0.5, 0.5, 0.5], [1.25, 0.5, 0.5], [1.75, 0.5, 0.5], [2.25, 0.5, 0.5], [2.75, 0.5, 0.5]]
    N = [[0.0, 0.6, 0.8], [nan, 0.0, 1.0], [0.0, 0.0, 1.0], [nan, nan, nan], [0.0, inf, 0.0], [0.6, 0.0, -0.8], [-0.6, 0.0, 0.8]]
    cases["normals"] = (V, strip(7), 1.0, N, None)
    # colours: the mean rounds half up
    V = [[0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [1.25, 0.5, 0.5], [1.5, 0.5, 0.5], [1.75, 0.5, 0.5], [2.25, 0.5, 0.5], [2.75, 0.5, 0.5]]
    C = [[0, 0, 255], [1, 1, 254], [0, 0, 0], [0, 0, 1], [1, 0, 1], [255, 255, 255], [255, 255, 254]]
    cases["colours"] = (V, strip(7), 1.0, None, C)
    out = {}
    for name, (V, I, h, N, C) in cases.items():
        out[name] = (np.ascontiguousarray(V, F32).reshape(-1, 3), np.ascontiguousarray(I, np.uint32).reshape(-1), float(F32(h)),
                     None if N is None else np.ascontiguousarray(N, F32).reshape(-1, 3),
                     None if C is None else np.ascontiguousarray(C, np.uint8).reshape(-1, 3))
    return out


def sphere_normals(V, spheres, voxel):
    """The analytic unit normal at every vertex of the sphere scene: away from the centre of the sphere whose surface is nearest."""
    V = np.asarray(V, np.float64)
    centres = (np.array([c for c, _ in spheres]) + 0.5) * voxel
    radii = np.array([r for _, r in spheres]) * voxel
    away = V[:, None, :] - centres[None]
    dist = np.linalg.norm(away, axis=2)
    nearest = np.argmin(np.abs(dist - radii[None]), axis=1)
    pick = np.arange(len(V))
    return (away[pick, nearest] / dist[pick, nearest, None]).astype(F32)
