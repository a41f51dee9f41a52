"""CPU reference of the exploration queries, written from the group comment "exploration" of include/tsdf_amd.h alone: voxel states and
frontiers (rules 1 - 2), clusters (rule 3) and view gain (rule 4) in numpy, the ray arithmetic in float32 scalars, every operation
rounded on its own.  Slow and plain on purpose."""
import numpy as np

F32 = np.float32
UNKNOWN, FREE, OCCUPIED = 0, 1, 2
CLUSTER_DTYPE = np.dtype([("label", np.uint32), ("size", np.uint32), ("lo", np.uint32, 3), ("hi", np.uint32, 3), ("sum", np.uint64, 3)])


def states(dist, weight):
    """Rule 1: per voxel id 0 = unknown, 1 = free, 2 = occupied."""
    d = np.asarray(dist, F32).reshape(-1)
    w = np.asarray(weight, F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        observed = w > 0                      # (False for NaN)
        negative = d < 0                      # (False for NaN and both zeros)
    s = np.full(d.shape, FREE, np.uint8)
    s[~observed] = UNKNOWN
    s[observed & negative] = OCCUPIED
    return s


def frontiers(dist, weight, size):
    """Rules 1 - 2: (ascending ids of the frontier voxels (uint32), {n_unknown, n_free, n_occupied, n_frontiers})."""
    X, Y, Z = size
    s = states(dist, weight).reshape(Z, Y, X)
    unk = s == UNKNOWN
    near = np.zeros_like(unk)
    near[:, :, 1:] |= unk[:, :, :-1]
    near[:, :, :-1] |= unk[:, :, 1:]
    near[:, 1:, :] |= unk[:, :-1, :]
    near[:, :-1, :] |= unk[:, 1:, :]
    near[1:, :, :] |= unk[:-1, :, :]
    near[:-1, :, :] |= unk[1:, :, :]
    ids = np.flatnonzero(((s == FREE) & near).reshape(-1)).astype(np.uint32)
    counts = {"n_unknown": int((s == UNKNOWN).sum()), "n_free": int((s == FREE).sum()), "n_occupied": int((s == OCCUPIED).sum()),
              "n_frontiers": len(ids)}
    return ids, counts


def coordinates(ids, size):
    X, Y, _ = size
    ids = np.asarray(ids, np.int64)
    return np.stack([ids % X, (ids // X) % Y, ids // (X * Y)], axis=1)


def clusters(ids, size, connectivity, min_size):
    """Rule 3: (L (uint32 per listed voxel), rows (CLUSTER_DTYPE, size >= min_size, ascending label), n_clusters)."""
    assert connectivity in (6, 26)
    X, Y, Z = size
    n = len(ids)
    index = {int(v): i for i, v in enumerate(ids)}
    c = coordinates(ids, size)
    steps = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
             if (dx, dy, dz) != (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    labels = np.full(n, -1, np.int64)
    for seed in range(n):                      # ascending: a cluster is first met at its smallest list index
        if labels[seed] >= 0:
            continue
        labels[seed] = seed
        stack = [seed]
        while stack:
            i = stack.pop()
            x, y, z = (int(v) for v in c[i])
            for dx, dy, dz in steps:
                nx, ny, nz = x + dx, y + dy, z + dz
                if 0 <= nx < X and 0 <= ny < Y and 0 <= nz < Z:
                    j = index.get((nz * Y + ny) * X + nx)
                    if j is not None and labels[j] < 0:
                        labels[j] = seed
                        stack.append(j)
    roots = np.flatnonzero(labels == np.arange(n))
    rows = []
    for r in roots:
        member = c[labels == r]
        if len(member) >= min_size:
            rows.append((r, len(member), member.min(axis=0), member.max(axis=0), member.sum(axis=0)))
    out = np.zeros(len(rows), CLUSTER_DTYPE)
    for k, row in enumerate(rows):
        out[k] = row
    return labels.astype(np.uint32), out, len(roots)


def _finite(x):
    return bool(np.isfinite(x))


def _to_int(f):
    """The saturating conversion of rule 4d: NaN gives 0."""
    if np.isnan(f):
        return 0
    if f >= F32(2147483648.0):
        return 2147483647
    if f <= F32(-2147483648.0):
        return -2147483648
    return int(f)


def walk(state, size, voxel_size, offset, o, d, t_max):
    """Rule 4a - 4f for one ray: (unknown, free, stop, [ids of the unknown voxels visited])."""
    N = [int(v) for v in size]
    o = [F32(v) for v in o]
    d = [F32(v) for v in d]
    vs = [F32(v) for v in voxel_size]
    off = [F32(v) for v in offset]
    t_max = F32(np.inf) if t_max is None else F32(t_max)
    skipped = (0, 0, 0, [])
    with np.errstate(all="ignore"):
        if not all(_finite(v) for v in o + d):
            return skipped
        if all(v == 0 for v in d):
            return skipped
        if not (t_max > 0):
            return skipped
        a = [F32(F32(o[k] - off[k]) / vs[k]) for k in range(3)]
        s = [F32(d[k] / vs[k]) for k in range(3)]
        if not all(_finite(v) for v in a + s):
            return skipped
        t0, t1 = F32(0), t_max
        for k in range(3):
            if s[k] == 0:
                if not (a[k] >= 0 and a[k] < F32(N[k])):
                    return skipped
                continue
            ta, tb = F32(F32(F32(0) - a[k]) / s[k]), F32(F32(F32(N[k]) - a[k]) / s[k])
            t0 = max(t0, min(ta, tb))
            t1 = min(t1, max(ta, tb))
        if not (t0 < t1):
            return skipped
        i = [min(max(_to_int(np.floor(F32(a[k] + F32(t0 * s[k])))), 0), N[k] - 1) for k in range(3)]
        step = [1 if s[k] > 0 else -1 for k in range(3)]
        ahead = [1 if s[k] > 0 else 0 for k in range(3)]
        unknown = free = 0
        marked = []
        for _ in range(N[0] + N[1] + N[2]):
            vid = (i[2] * N[1] + i[1]) * N[0] + i[0]
            st = state[vid]
            if st == OCCUPIED:
                return unknown, free, 2, marked
            if st == UNKNOWN:
                unknown += 1
                marked.append(vid)
            else:
                free += 1
            axis, best = -1, F32(0)
            for k in range(3):
                if s[k] == 0:
                    continue
                tn = F32(F32(F32(i[k] + ahead[k]) - a[k]) / s[k])
                if axis < 0 or tn < best:
                    axis, best = k, tn
            if axis < 0 or best > t1:
                break
            i[axis] += step[axis]
            if i[axis] < 0 or i[axis] >= N[axis]:
                break
        return unknown, free, 1, marked


def view_gain(state, size, voxel_size, offset, origins, directions, t_max=None, mask=None):
    """Rule 4: (gain, unknown (n,) uint32, free (n,) uint32, stop (n,) uint8, mask).  `mask`: the set of marked voxel ids to add to
    (TSDF_GAIN_KEEP_MASK); None starts from the empty set."""
    o = np.asarray(origins, F32).reshape(-1, 3)
    d = np.asarray(directions, F32).reshape(-1, 3)
    n = len(o)
    mask = set() if mask is None else set(mask)
    unknown, free, stop = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for r in range(n):
        u, f, s, marked = walk(state, size, voxel_size, offset, o[r], d[r], None if t_max is None else t_max[r])
        unknown[r], free[r], stop[r] = u, f, s
        mask.update(marked)
    return len(mask), unknown, free, stop, mask


def random_state_field(size, seed, density, fp32_oddities=False):
    """(distances, weights): a share `density` of the voxels observed with whole-number weights 1 .. 3, distances of both signs with
    -0.0 and NaN planted; fp32_oddities: also NaN and fractional weights (fp32 storage only)."""
    n = size[0] * size[1] * size[2]
    rng = np.random.default_rng(seed)
    D = rng.uniform(-1.0, 1.0, n).astype(F32)
    D[rng.random(n) < 0.05] = F32(-0.0)
    D[rng.random(n) < 0.05] = F32(0.0)
    D[rng.random(n) < 0.05] = F32(np.nan)
    Wt = np.where(rng.random(n) < density, rng.integers(1, 4, n), 0).astype(F32)
    if fp32_oddities:
        Wt[rng.random(n) < 0.1] = F32(np.nan)
        Wt[rng.random(n) < 0.1] = F32(0.25)
    return D, Wt
