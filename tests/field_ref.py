"""CPU reference of the field queries (include/tsdf_amd.h, "field queries"): every sample S is the oracle's orc_trilinear, everything
else numpy float32 scalar operations in the order the header states.  Test infrastructure only (uses oracle/).
"""
import numpy as np

F = np.float32
NAN = F(np.nan)


def geometry(volume):
    """(dims, vs, offset) of a tsdf_amd.TSDFVolume or an oracle.Volume."""
    if hasattr(volume, "info"):
        i = volume.info()
        return tuple(int(s) for s in i.size), np.array(i.voxel_size, F), np.array(i.offset, F)
    return tuple(int(s) for s in volume.size()), np.array(volume.voxel_size(), F), np.array(volume.offset(), F)


def bounds(dims, vs):
    """size[i] * voxel_size[i], the fp32 product the ray cast forms as max_x / y / z."""
    return [F(dims[a]) * F(vs[a]) for a in range(3)]


def valid(q, mx):
    """Every component finite, >= 0 and < the bound (False for NaN and both infinities; -0.0 is valid)."""
    return all(bool(q[a] >= F(0)) and bool(q[a] < mx[a]) for a in range(3))


def unit(g):
    """The TSDF_FIELD_UNIT_GRADIENT rule on one raw gradient: g / sqrtf((gx gx + gy gy) + gz gz), the NaN triple if that is not > 0."""
    with np.errstate(all="ignore"):
        ln = F(np.sqrt(F(F(F(g[0] * g[0]) + F(g[1] * g[1])) + F(g[2] * g[2]))))
        return [F(F(c) / ln) for c in g] if bool(ln > F(0)) else [NAN, NAN, NAN]


def unit_rows(G):
    """unit() of every row of an (n, 3) array of raw gradients."""
    return np.array([unit([F(c) for c in row]) for row in np.asarray(G, F).reshape(-1, 3)], F).reshape(-1, 3)


def sample(O, geom, dist, weight, points, unit_gradient=False, gradient=True):
    """-> (distance (n,), gradient (n, 3), weight (n,)) float32 of (n, 3) float32 world points.  dist / weight: the whole grid's fp32
    arrays, x fastest.  gradient=False leaves the gradient rows NaN and saves their six samples a point."""
    dims, vs, offset = geom
    vs = [F(v) for v in vs]
    mx = bounds(dims, vs)
    dist = np.ascontiguousarray(dist, F).reshape(-1)
    weight = np.ascontiguousarray(weight, F).reshape(-1)
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(P)
    D = np.full(n, NAN, F)
    G = np.full((n, 3), NAN, F)
    Wt = np.zeros(n, F)
    S = lambda q: F(O.trilinear(np.array(q, F), dims, vs, dist))
    with np.errstate(all="ignore"):
        for i in range(n):
            q = [F(P[i, a]) - F(offset[a]) for a in range(3)]
            if not valid(q, mx):
                continue
            D[i] = S(q)
            v = [int(np.floor(q[a] / vs[a])) for a in range(3)]
            # (a valid point within rounding of the upper bound can divide to `size` itself: no such voxel, weight 0)
            if all(0 <= v[a] < dims[a] for a in range(3)):
                Wt[i] = weight[v[0] + dims[0] * (v[1] + dims[1] * v[2])]
            if not gradient:
                continue
            shifted = []
            for a in range(3):
                qp, qm = list(q), list(q)
                qp[a] = F(q[a] + vs[a])
                qm[a] = F(q[a] - vs[a])
                shifted.append((qp, qm))
            if not all(valid(qp, mx) and valid(qm, mx) for qp, qm in shifted):
                continue
            g = [F(F(S(qp) - S(qm)) / F(vs[a] + vs[a])) for a, (qp, qm) in enumerate(shifted)]
            G[i] = unit(g) if unit_gradient else g
    return D, G, Wt
