"""CPU reference of the ray queries (include/tsdf_amd.h, "ray queries"), from the oracle alone, ray by ray: a 1 x 1 image whose pose is
the identity rotation with the ray's origin as translation and whose column-major kinv is zero except its third column, which holds
the direction -- pixel (0, 0) then has exactly that direction.  Volume.raycast(1, 1) gives the point, Volume.raycast_slab(1, 1,
own=(0, Z)) the refined parameter th, oracle.ray_box near_t.  The decreed misses and the t_max rule are applied here as the header
states them; the normals are tests/field_ref.py's unit gradient at the hit points.  Test infrastructure only (uses oracle/)."""
import numpy as np

from tests import field_ref

F = np.float32
NAN = F(np.nan)
NO_HIT = 0xFFFFFFFF


def box(ov):
    """(space_min, space_max) as the ray cast forms them: offset, offset + physical size (one fp32 add per axis)."""
    offset, phys = np.array(ov.offset(), F), np.array(ov.physical_size(), F)
    return offset, (offset + phys).astype(F)


def decreed_miss(o, d):
    return (not np.isfinite(o).all()) or (not np.isfinite(d).all()) or bool((d == 0).all())


def cast(O, ov, origins, directions, t_max=None, normals=False):
    """-> (points (n, 3), t (n,), normals (n, 3) or None) float32 for (n, 3) float32 origins and directions, t_max (n,) or None."""
    o = np.ascontiguousarray(origins, F).reshape(-1, 3)
    d = np.ascontiguousarray(directions, F).reshape(-1, 3)
    n = len(o)
    assert len(d) == n
    smin, smax = box(ov)
    Z = int(ov.size()[2])
    P = np.full((n, 3), NAN, F)
    T = np.full(n, NAN, F)
    pose = np.eye(4, dtype=F).T.reshape(-1).copy()      # column-major; the identity is its own transpose
    kinv = np.zeros(9, F)
    for i in range(n):
        if decreed_miss(o[i], d[i]):
            continue
        pose[12:15] = o[i]
        kinv[6:9] = d[i]
        V, _ = ov.raycast(1, 1, pose, kinv)
        k, th_bits = ov.raycast_slab(1, 1, pose, kinv, own=(0, Z))[0]
        hit = int(k) != NO_HIT
        assert hit == (not np.isnan(V[0]).any()), "the oracle's two casts disagree on ray %d" % i
        if not hit:
            continue
        intersects, near_t, _ = O.ray_box(o[i], d[i], smin, smax)
        assert intersects
        th = np.array([th_bits], np.uint32).view(F)[0]
        P[i] = V[0]
        T[i] = F(F(near_t) + th)
    if t_max is not None:
        m = np.ascontiguousarray(t_max, F).reshape(-1)
        assert len(m) == n
        with np.errstate(invalid="ignore"):
            keep = T <= m                               # (False for a NaN t_max and for a miss)
        P[~keep] = NAN
        T[~keep] = NAN
    N = None
    if normals:
        N = np.full((n, 3), NAN, F)
        hits = np.flatnonzero(~np.isnan(T))
        if len(hits):
            geom = field_ref.geometry(ov)
            N[hits] = field_ref.sample(O, geom, ov.dist, ov.weight, P[hits], unit_gradient=True)[1]
    return P, T, N


def limit(P, T, N, t_max):
    """The t_max rule applied to an unlimited reference: the first hit counts only if t <= t_max."""
    m = np.ascontiguousarray(t_max, F).reshape(-1)
    with np.errstate(invalid="ignore"):
        keep = T <= m
    P, T = P.copy(), T.copy()
    P[~keep] = NAN
    T[~keep] = NAN
    if N is not None:
        N = N.copy()
        N[~keep] = NAN
    return P, T, N
