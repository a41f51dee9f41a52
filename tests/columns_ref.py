"""CPU reference of the column maps, written from the group comment "column maps" of include/tsdf_amd.h alone: the map's axes and a
cell's column (rules 2 - 3), its row (rule 4) column by column, the totals (rule 5) and the classification (rule 6), in numpy on the
voxel states of tests/explore_ref.py, the height in float32 scalars, every operation rounded on its own.  Slow and plain on purpose."""
import numpy as np

from tests.explore_ref import FREE, OCCUPIED, UNKNOWN, states

F32 = np.float32
COLUMN_DTYPE = np.dtype([("n_unknown", np.uint32), ("n_free", np.uint32), ("n_occupied", np.uint32), ("top", np.int32), ("bottom", np.int32),
                         ("headroom", np.uint32), ("height", np.float32), ("min_distance", np.float32)])
NO_GROUND, TRAVERSABLE, BLOCKED = 0, 1, 2
MAP_AXES = {0: (1, 2), 1: (0, 2), 2: (0, 1)}


def band_of(size, axis, band):
    """Rule 3: the resolved (lo, hi)."""
    lo, hi = (0, size[axis]) if band is None else band
    hi = size[axis] if hi == 0 else hi
    assert 0 <= lo < hi <= size[axis]
    return lo, hi


def column_ids(size, axis, u, v, lo, hi, reversed_):
    """Rules 2 - 3: the voxel ids c_0 .. c_{L-1} of cell (u, v)."""
    X, Y, _ = size
    au, av = MAP_AXES[axis]
    p = np.arange(hi - lo, dtype=np.int64)
    c = [None, None, None]
    c[au], c[av], c[axis] = u, v, (hi - 1 - p) if reversed_ else (lo + p)
    return (c[2] * Y + c[1]) * X + c[0]


def row_of(state, dist, esdf):
    """Rule 4 for one column: the states, distances and ESDF values (or None) of c_0 .. c_{L-1} in walk order."""
    L = len(state)
    occupied = np.flatnonzero(state == OCCUPIED)
    top, bottom = (int(occupied[-1]), int(occupied[0])) if len(occupied) else (-1, -1)
    headroom, height = 0, F32(np.nan)
    if top >= 0:
        p = top + 1
        while p < L and state[p] == FREE:
            headroom += 1
            p += 1
        height = F32(F32(top) + F32(1.0))
        if top + 1 < L and state[top + 1] == FREE:
            d0, d1 = F32(dist[top]), F32(dist[top + 1])
            with np.errstate(all="ignore"):
                f = F32(d0 / F32(d0 - d1))
            if f >= F32(0.0) and f <= F32(1.0):
                height = F32(F32(F32(top) + F32(0.5)) + f)
    m = F32(np.nan)
    if esdf is not None:
        seen = esdf[~np.isnan(esdf)]
        if len(seen):
            m = F32(seen.min())
            if m == 0:
                m = F32(0.0)
    return (int((state == UNKNOWN).sum()), int((state == FREE).sum()), len(occupied), top, bottom, headroom, height, m)


def project(dist, weight, size, axis, band=None, reversed_=False, esdf=None):
    """Rules 1 - 5: (rows (V, U) COLUMN_DTYPE, totals {n_unknown, n_free, n_occupied, n_ground})."""
    s = states(dist, weight)
    d = np.asarray(dist, F32).reshape(-1)
    e = None if esdf is None else np.asarray(esdf, F32).reshape(-1)
    lo, hi = band_of(size, axis, band)
    au, av = MAP_AXES[axis]
    U, V = size[au], size[av]
    rows = np.zeros((V, U), COLUMN_DTYPE)
    for v in range(V):
        for u in range(U):
            ids = column_ids(size, axis, u, v, lo, hi, reversed_)
            rows[v, u] = row_of(s[ids], d[ids], None if e is None else e[ids])
    totals = {"n_unknown": int(rows["n_unknown"].sum(dtype=np.uint64)), "n_free": int(rows["n_free"].sum(dtype=np.uint64)),
              "n_occupied": int(rows["n_occupied"].sum(dtype=np.uint64)), "n_ground": int((rows["top"] >= 0).sum())}
    return rows, totals


def classify(rows, max_step, min_headroom):
    """Rule 6: ((V, U) uint8, {n_no_ground, n_traversable, n_blocked})."""
    V, U = rows.shape
    out = np.zeros((V, U), np.uint8)
    for v in range(V):
        for u in range(U):
            top = int(rows[v, u]["top"])
            if top < 0:
                continue
            blocked = int(rows[v, u]["headroom"]) < min_headroom
            for nu, nv in ((u - 1, v), (u + 1, v), (u, v - 1), (u, v + 1)):
                if 0 <= nu < U and 0 <= nv < V:
                    t = int(rows[nv, nu]["top"])
                    if t >= 0 and abs(top - t) > max_step:
                        blocked = True
            out[v, u] = BLOCKED if blocked else TRAVERSABLE
    counts = {"n_no_ground": int((out == NO_GROUND).sum()), "n_traversable": int((out == TRAVERSABLE).sum()), "n_blocked": int((out == BLOCKED).sum())}
    return out, counts


def height_world(rows, size, axis, band, reversed_, voxel_size, offset):
    """Rule 4's world coordinate in fp32."""
    lo, hi = band_of(size, axis, band)
    off, vs = F32(offset[axis]), F32(voxel_size[axis])
    if reversed_:
        return (off + (F32(hi) - rows["height"]) * vs).astype(F32)
    return (off + (F32(lo) + rows["height"]) * vs).astype(F32)
