"""CPU reference of the reachability group, written from the group comment "reachability" of include/tsdf_amd.h alone: traversable
voxels (rule 2), admissible steps and their costs (rule 3), seeds (rule 4), the cost field by plain Dijkstra with heapq (rule 5), the
info integers (rule 6), lookup (rule 7), the path walk (rule 8) and the ranking of frontier clusters (rule 9).  The seed and lookup
arithmetic is in float32 scalars, every operation rounded on its own.  Slow and plain on purpose."""
import heapq

import numpy as np

from tests import explore_ref as E

F32 = np.float32
UNREACHED = 0xFFFFFFFF
COST = {1: 10, 2: 14, 3: 17}
THROUGH_UNKNOWN = 1
CLUSTER_DTYPE = np.dtype([("label", np.uint32), ("cost", np.uint32), ("voxel", np.uint32), ("reserved", np.uint32)])


def traversable(dist, weight, through_unknown=False, esdf=None, clearance=0.0):
    """Rule 2: a bool per voxel id."""
    s = E.states(dist, weight)
    t = s == E.FREE
    if through_unknown:
        t |= s == E.UNKNOWN
    if esdf is not None:
        with np.errstate(invalid="ignore"):
            t &= np.asarray(esdf, F32).reshape(-1) >= F32(clearance)   # (False for NaN)
    else:
        assert clearance == 0
    return t


def offsets(connectivity):
    """Rule 8's fixed neighbour order: dz outermost, then dy, then dx; (0, 0, 0) skipped; at 6 the face offsets only."""
    assert connectivity in (6, 26)
    return [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dx, dy, dz) != (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]


def admissible(trav, size, x, y, z, dx, dy, dz):
    """Rule 3: the neighbour is inside the grid and every voxel w with w_k in {u_k, v_k} is traversable."""
    X, Y, Z = size
    if not (0 <= x + dx < X and 0 <= y + dy < Y and 0 <= z + dz < Z):
        return False
    for c in {0, dz}:
        for b in {0, dy}:
            for a in {0, dx}:
                if not trav[((z + c) * Y + (y + b)) * X + (x + a)]:
                    return False
    return True


def point_voxel(p, size, voxel_size, offset):
    """Rules 4 and 7: the voxel id of a world point, None for a coordinate that is not finite or an index off the grid."""
    idx = []
    with np.errstate(all="ignore"):
        for k in range(3):
            v = F32(p[k])
            if not np.isfinite(v):
                return None
            f = np.floor(F32(F32(v - F32(offset[k])) / F32(voxel_size[k])))
            if not (f >= 0 and f < size[k]):
                return None
            idx.append(int(f))
    return (idx[2] * size[1] + idx[1]) * size[0] + idx[0]


def admissible_steps(trav, size, connectivity):
    """Rule 3 for every voxel at once: [(dx, dy, dz, cost, a bool per voxel id: the step from it is admissible)] in rule 8's order.
    The same test as admissible(), over a copy of the grid with a ring of blocked voxels round it."""
    X, Y, Z = size
    P = np.zeros((Z + 2, Y + 2, X + 2), bool)
    P[1:-1, 1:-1, 1:-1] = np.asarray(trav, bool).reshape(Z, Y, X)
    steps = []
    for dx, dy, dz in offsets(connectivity):
        ok = np.ones((Z, Y, X), bool)
        for c in {0, dz}:
            for b in {0, dy}:
                for a in {0, dx}:
                    ok &= P[1 + c:1 + c + Z, 1 + b:1 + b + Y, 1 + a:1 + a + X]
        steps.append((dx, dy, dz, COST[abs(dx) + abs(dy) + abs(dz)], ok.reshape(-1)))
    return steps


def cost_field(trav, size, voxel_size, offset, seeds, connectivity=26, max_cost=0):
    """Rules 3 - 5: (the cost per voxel id (uint32), the sorted list of seed voxel ids)."""
    X, Y, Z = size
    n = X * Y * Z
    steps = [(dx + X * (dy + Y * dz), cost, ok.tolist()) for dx, dy, dz, cost, ok in admissible_steps(trav, size, connectivity)]
    cap = max_cost if max_cost else 0xFFFFFFFE
    D = [None] * n
    heap = []
    for p in np.asarray(seeds, F32).reshape(-1, 3):
        v = point_voxel(p, size, voxel_size, offset)
        if v is not None and trav[v] and D[v] is None:
            D[v] = 0
            heap.append((0, v))
    seed_ids = sorted(v for _, v in heap)
    heapq.heapify(heap)
    while heap:
        d, v = heapq.heappop(heap)
        if d != D[v]:
            continue
        for delta, cost, ok in steps:
            if not ok[v]:
                continue
            u = v + delta       # (an admissible step stays inside the grid, so the id moves by the offset's own id)
            nd = d + cost
            if D[u] is None or nd < D[u]:
                D[u] = nd
                heapq.heappush(heap, (nd, u))
    out = np.full(n, UNREACHED, np.uint32)
    for v in range(n):
        if D[v] is not None and D[v] <= cap:
            out[v] = D[v]
    return out, seed_ids


def info(trav, out):
    """Rule 6's unique integers."""
    reached = out != UNREACHED
    return {"n_traversable": int(np.count_nonzero(trav)), "n_reached": int(reached.sum()), "n_seed_voxels": int((out == 0).sum()),
            "max_cost_reached": int(out[reached].max()) if reached.any() else 0}


def lookup(out, size, voxel_size, offset, points):
    """Rule 7."""
    res = np.full(len(points), UNREACHED, np.uint32)
    for i, p in enumerate(np.asarray(points, F32).reshape(-1, 3)):
        v = point_voxel(p, size, voxel_size, offset)
        if v is not None:
            res[i] = out[v]
    return res


def path(out, trav, size, connectivity, goal):
    """Rule 8 for one goal voxel id (None: off the grid): the list of voxel ids, goal first; empty where there is no path."""
    X, Y, Z = size
    if goal is None or out[goal] == UNREACHED:
        return []
    steps = offsets(connectivity)
    v = goal
    ids = [v]
    while out[v] != 0:
        x, y, z = v % X, (v // X) % Y, v // (X * Y)
        for dx, dy, dz in steps:
            if not admissible(trav, size, x, y, z, dx, dy, dz):
                continue
            u = ((z + dz) * Y + (y + dy)) * X + (x + dx)
            if out[u] != UNREACHED and int(out[u]) + COST[abs(dx) + abs(dy) + abs(dz)] == int(out[v]):
                v = u
                break
        else:
            raise AssertionError("a reached voxel that is no seed has no predecessor")
        ids.append(v)
        assert len(ids) <= int(out[goal]) // 10 + 1
    return ids


def paths(out, trav, size, voxel_size, offset, connectivity, goals, max_len, rows=None):
    """Rule 8: (lengths (n,) uint32, rows (n, max_len) uint32 -- what a path does not fill is left as `rows` had it (default UNREACHED))."""
    goals = np.asarray(goals, F32).reshape(-1, 3)
    n = len(goals)
    lengths = np.zeros(n, np.uint32)
    table = np.full((n, max_len), UNREACHED, np.uint32) if rows is None else np.array(rows, np.uint32).reshape(n, max_len)
    for i, p in enumerate(goals):
        ids = path(out, trav, size, connectivity, point_voxel(p, size, voxel_size, offset))
        lengths[i] = len(ids)
        k = min(len(ids), max_len)
        table[i, :k] = ids[:k]
    return lengths, table


def rank(out, frontier_ids, labels, cluster_rows):
    """Rule 9: one row per row of the cluster table, in table order."""
    res = np.zeros(len(cluster_rows), CLUSTER_DTYPE)
    for k, row in enumerate(cluster_rows):
        members = np.asarray(frontier_ids)[np.asarray(labels) == row["label"]]
        best = (UNREACHED, 0xFFFFFFFF)
        for v in members:
            if out[v] != UNREACHED:
                best = min(best, (int(out[v]), int(v)))
        res[k] = (row["label"], best[0], best[1], 0)
    return res


def centres(ids, size, voxel_size, offset):
    """The world centres of voxel ids as float32: offset + (coordinate + 0.5) * voxel_size."""
    c = E.coordinates(ids, size).astype(F32)
    return ((c + F32(0.5)) * np.asarray(voxel_size, F32) + np.asarray(offset, F32)).astype(F32)
