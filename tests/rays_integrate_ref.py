"""CPU reference of ray integration (include/tsdf_amd.h, "ray integration"), written from the header's rules 1 - 8 alone: a loop per ray
in numpy float32 scalars (float64 where the header says double), a dict voxel -> (n_v, S_v), then the apply.  A ray that repeats an
earlier one bit for bit (same geometry, ranges and flags) reuses that ray's observations: the rules are a function of the ray alone.  Test infrastructure only."""
import numpy as np

F = np.float32
D = np.float64
BAND_ONLY = 1
MAX_RAYS = 1 << 23


def geometry(volume):
    """(dims, vs, offset, trunc) of a tsdf_amd.TSDFVolume or an oracle.Volume."""
    if hasattr(volume, "info"):
        i = volume.info()
        return tuple(int(s) for s in i.size), np.array(i.voxel_size, F), np.array(i.offset, F), F(i.truncation_distance)
    return (tuple(int(s) for s in volume.size()), np.array(volume.voxel_size(), F), np.array(volume.offset(), F),
            F(volume.truncation_distance()))


def _finite(x):
    return bool(np.isfinite(x))


def walk(geom, o, p, min_range=0.0, max_range=np.inf, flags=0):
    """Rules 1 - 6 for one ray -> (cells, obs): every visited cell (x, y, z) in order, and {(x, y, z): (sdf, tsdf, q)} for the visited
    cells with an observation.  A skipped ray gives ([], {})."""
    dims, vs, offset, trunc = geom
    vs = [F(v) for v in vs]
    offset = [F(v) for v in offset]
    trunc = F(trunc)
    o = [F(v) for v in o]
    p = [F(v) for v in p]
    lo, hi = F(min_range), F(max_range)
    none = ([], {})
    with np.errstate(all="ignore"):
        # 1. ray
        if not all(_finite(v) for v in o + p):
            return none
        d = [F(p[k] - o[k]) for k in range(3)]
        r = F(np.sqrt(F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))))
        if not _finite(r) or r == F(0):
            return none
        if np.isnan(lo) or np.isnan(hi) or r < lo or r > hi:
            return none
        u = [F(d[k] / r) for k in range(3)]
        # 2. stretch
        te = F(r + trunc)
        ts = F(np.fmax(F(r - trunc), F(0))) if flags & BAND_ONLY else F(0)
        # 3. grid coordinates
        a = [F(F(o[k] - offset[k]) / vs[k]) for k in range(3)]
        s = [F(u[k] / vs[k]) for k in range(3)]
        # 4. clip
        t0, t1 = ts, te
        for k in range(3):
            if s[k] == F(0):
                if not (a[k] >= F(0) and a[k] < F(dims[k])):
                    return none
                continue
            ta = F(F(F(0) - a[k]) / s[k])
            tb = F(F(F(dims[k]) - a[k]) / s[k])
            t0 = F(np.fmax(t0, np.fmin(ta, tb)))
            t1 = F(np.fmin(t1, np.fmax(ta, tb)))
        if not t0 < t1:
            return none
        # 5. walk
        i = []
        for k in range(3):
            f = np.floor(F(a[k] + F(t0 * s[k])))
            i.append(int(min(max(f, F(0)), F(dims[k] - 1))))
        cells, obs = [], {}
        while True:
            cells.append(tuple(i))
            assert len(cells) <= sum(dims), "a ray visited more than X + Y + Z cells"
            # 6. observation
            c = [F(F(F(F(i[k]) + F(0.5)) * vs[k]) + offset[k]) for k in range(3)]
            e = [F(c[k] - o[k]) for k in range(3)]
            sdf = F(r - F(F(F(e[0] * u[0]) + F(e[1] * u[1])) + F(e[2] * u[2])))
            if not sdf < -trunc:
                tsdf = F(np.fmin(sdf, trunc)) if sdf > F(0) else sdf
                q = int(np.rint(F(F(tsdf / trunc) * F(32768.0))))
                assert -32768 <= q <= 32768
                obs[tuple(i)] = (sdf, tsdf, q)
            axis, best = -1, None
            for k in range(3):
                if s[k] == F(0):
                    continue
                tn = F(F(F(i[k] + (1 if s[k] > F(0) else 0)) - a[k]) / s[k])
                if axis < 0 or tn < best:
                    axis, best = k, tn
            if axis < 0 or best > t1:
                break
            i[axis] += 1 if s[axis] > F(0) else -1
            if i[axis] < 0 or i[axis] >= dims[axis]:
                break
        return cells, obs


_SEEN = {}   # (geometry, ranges, flags) -> {ray bytes -> its observations}


def accumulate(geom, origins, points, min_range=0.0, max_range=np.inf, flags=0):
    """Rule 7 -> {(x, y, z): [n_v, S_v]} over the whole set.  origins: (1, 3) or (n, 3)."""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    Og = np.ascontiguousarray(origins, F).reshape(-1, 3)
    n = len(P)
    assert len(Og) in (1, n) and n <= MAX_RAYS
    acc = {}
    dims, vs, offset, trunc = geom
    call = (tuple(dims), np.asarray(vs, F).tobytes(), np.asarray(offset, F).tobytes(), F(trunc).tobytes(), F(min_range).tobytes(),
            F(max_range).tobytes(), int(flags))
    seen = _SEEN.setdefault(call, {})
    for j in range(n):
        o = Og[j if len(Og) == n else 0]
        key = o.tobytes() + P[j].tobytes()
        obs = seen.get(key)
        if obs is None:
            obs = seen[key] = [(cell, v[2]) for cell, v in walk(geom, o, P[j], min_range, max_range, flags)[1].items()]
        for cell, q in obs:
            e = acc.get(cell)
            if e is None:
                acc[cell] = [1, q]
            else:
                e[0] += 1
                e[1] += q
    return acc


def apply(geom, dist, weight, acc, cap=0):
    """Rule 8 -> (distances, weights, updated mask) as new flat arrays, x fastest."""
    dims, _, _, trunc = geom
    X, Y, _ = dims
    dist = np.array(dist, F).reshape(-1)
    weight = np.array(weight, F).reshape(-1)
    updated = np.zeros(dist.size, bool)
    scale = D(F(trunc)) * (D(1.0) / D(32768.0))
    with np.errstate(all="ignore"):
        for (x, y, z), (n_v, s_v) in acc.items():
            at = (z * Y + y) * X + x
            m = F((D(s_v) / D(n_v)) * scale)
            d, w = dist[at], weight[at]
            wn = F(w + F(1))
            dist[at] = F(F(F(d * w) + m) / wn)
            weight[at] = F(cap) if cap and wn > F(cap) else wn
            updated[at] = True
    return dist, weight, updated


def integrate(geom, dist, weight, origins, points, min_range=0.0, max_range=np.inf, flags=0, cap=0):
    """One call of tsdf_integrate_rays -> (distances, weights, updated mask, acc)."""
    acc = accumulate(geom, origins, points, min_range, max_range, flags)
    d, w, upd = apply(geom, dist, weight, acc, cap)
    return d, w, upd, acc
