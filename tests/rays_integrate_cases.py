"""Seeded ray sets for ray integration (include/tsdf_amd.h, "ray integration"), shared by tests/test_integrate_rays_host.py (the CPU
reference's own properties) and tests/test_integrate_rays.py (the GPU against it).  A case is a grid and a list of calls, each
(origins (1 or n, 3), points (n, 3), min_range, max_range, flags), applied one after the other; `min_updated` / `min_multi` are the
coverage the reference alone must reach on a cleared volume (voxels updated, voxels that took more than one ray in some call).
Inputs only; the expectations come from tests/rays_integrate_ref.py."""
import functools

import numpy as np

from tests import rays_integrate_ref as ref

F = np.float32
INF = float("inf")
SEED = 0x5EED4A75
# the 37 x 34 x 45 grid of tests/field_cases.py's scenes: unequal voxel edges, an offset, X below one wave, Y no multiple of 4, Z of
# neither 4 nor 32 (the last packed weight group and the last brick are partial)
GRID = ((37, 34, 45), (3000.0, 3000.0, 3000.0), (60.0, -90.0, 120.0))
# voxel edge exactly 64 on every axis and offsets that are multiples of it: grid coordinates are exact, diagonals meet corners, ties are ties
TIE_GRID = ((40, 10, 36), (2560.0, 640.0, 2304.0), (-128.0, 64.0, 256.0))
CENTRE, RADIUS, WALL_Z = (1500.0, 1500.0, 1500.0), 500.0, 2600.0        # relative to the grid's offset
INSIDE = (600.0, 800.0, 500.0)
OUTSIDE = ((-800.0, 1500.0, 1400.0), (1500.0, -1000.0, 1700.0), (3900.0, 3600.0, -700.0))


class Case:
    def __init__(self, name, grid, calls, min_updated, min_multi):
        self.name, self.grid, self.min_updated, self.min_multi = name, grid, min_updated, min_multi
        self.calls = []
        for o, p, lo, hi, flags in calls:
            o = np.ascontiguousarray(o, F).reshape(-1, 3)
            p = np.ascontiguousarray(p, F).reshape(-1, 3)
            assert len(o) in (1, len(p))
            o.setflags(write=False)
            p.setflags(write=False)
            self.calls.append((o, p, lo, hi, flags))


def fan(n_az, n_el, el_lo=-60.0, el_hi=80.0):
    """Unit directions on a regular azimuth / elevation fan (float64)."""
    az = np.deg2rad(np.arange(n_az) * (360.0 / n_az))
    el = np.deg2rad(np.linspace(el_lo, el_hi, n_el))
    a, e = np.meshgrid(az, el)
    return np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1).reshape(-1, 3)


def aimed(dirs, origin, half_angle=30.0):
    """The directions within half_angle degrees of the one from `origin` to the sphere's centre."""
    to = np.asarray(CENTRE) - np.asarray(origin, np.float64)
    return dirs[dirs @ (to / np.linalg.norm(to)) > np.cos(np.deg2rad(half_angle))]


def scan(origin, dirs, offset):
    """The sphere-and-wall scene seen from `origin` (relative to the offset) along unit `dirs`: analytic ranges, rays without a return
    dropped.  -> (origin (3,) float32 world, points (m, 3) float32 world, ranges (m,) float64, on_sphere (m,) bool)."""
    o = np.asarray(origin, np.float64)
    oc = o - np.asarray(CENTRE)
    b = dirs @ oc
    disc = b * b - (oc @ oc - RADIUS * RADIUS)
    with np.errstate(invalid="ignore", divide="ignore"):
        t_sphere = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf)
        t_sphere = np.where(t_sphere > 0, t_sphere, np.inf)
        t_wall = np.where(dirs[:, 2] > 1e-3, (WALL_Z - o[2]) / dirs[:, 2], np.inf)
    t = np.minimum(t_sphere, t_wall)
    keep = np.isfinite(t) & (t < 6000.0)
    pts = o + dirs[keep] * t[keep, None] + np.asarray(offset, np.float64)
    return (o + np.asarray(offset, np.float64)).astype(F), pts.astype(F), t[keep], (t_sphere <= t_wall)[keep]


def _exact_world(k, vs, offset):
    """A float32 world coordinate whose grid coordinate (x - offset) / vs is exactly k in fp32 (the nearest candidate otherwise)."""
    x = F(F(F(k) * F(vs)) + F(offset))
    for c in (x, np.nextafter(x, F(np.inf)), np.nextafter(x, F(-np.inf))):
        if F(F(c - F(offset)) / F(vs)) == F(k):
            return c
    return x


def axis_rays(grid):
    """Rays along +- each axis: through voxel centres, in face planes and along edge lines (grid coordinates integral), from outside and
    from inside the box, ending inside and outside it."""
    dims, phys, offset = grid
    vs = [F(F(phys[k]) / F(dims[k])) for k in range(3)]
    O, P = [], []
    for axis in range(3):
        b, c = [k for k in range(3) if k != axis]
        for jb, jc in ((3.5, 7.5), (5.0, 9.5), (11.0, 4.0), (0.0, 0.0), (float(dims[b]), 2.5), (float(dims[b]) - 0.5, float(dims[c]) - 0.5)):
            for start, end in ((-3.0, dims[axis] * 0.6), (dims[axis] + 2.5, 4.0), (2.0, dims[axis] + 4.0), (dims[axis] - 1.5, 6.5), (-9.0, -2.0)):
                o, p = [0, 0, 0], [0, 0, 0]
                o[b] = p[b] = _exact_world(jb, vs[b], offset[b])
                o[c] = p[c] = _exact_world(jc, vs[c], offset[c])
                o[axis], p[axis] = _exact_world(start, vs[axis], offset[axis]), _exact_world(end, vs[axis], offset[axis])
                O.append(o)
                P.append(p)
    return np.array(O, F), np.array(P, F)


def tie_rays():
    """On TIE_GRID: diagonals through voxel corners and centres (all three, and pairs of, crossing times equal), both ways."""
    dims, phys, offset = TIE_GRID
    O, P = [], []
    for start in ((-1.0, -1.0, -1.0), (2.0, 1.0, 5.0), (0.5, 0.5, 0.5), (3.0, 0.5, 7.0), (6.5, 2.0, 1.5)):
        for d in ((1, 1, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, -1, 1), (-1, 1, 1), (1, 1, -1)):
            for length in (6.0, 9.5, 14.0):
                o = [offset[k] + 64.0 * start[k] for k in range(3)]
                p = [o[k] + 64.0 * length * d[k] for k in range(3)]
                O.append(o)
                P.append(p)
                O.append(p)
                P.append(o)
    return np.array(O, F), np.array(P, F)


def skip_rays(grid, rng):
    """Every decreed skip, rays that miss the box, rays from outside into it and out of it -- between rays that do update something."""
    dims, phys, offset = grid
    off = np.asarray(offset, np.float64)
    mid = off + np.asarray(phys) * 0.5
    O, P = [], []
    for bad in (np.nan, np.inf, -np.inf):
        for at in range(3):
            o, p = mid.copy(), mid + (300.0, 200.0, 100.0)
            o[at] = bad
            O.append(o)
            P.append(p)
            o, p = mid.copy(), mid + (300.0, 200.0, 100.0)
            p[at] = bad
            O.append(o)
            P.append(p)
    O.append(mid)
    P.append(mid)                                                    # r == 0
    O.append(mid)
    P.append(mid + (0.0, -0.0, 0.0))                                 # r == 0, a negative zero among the differences
    O.append((-3.0e38, 0.0, 0.0))
    P.append((3.0e38, 0.0, 0.0))                                     # d overflows: r is not finite
    O.append((1.0e20, 1.0e20, 1.0e20))
    P.append((-1.0e20, -1.0e20, 1.0e20))                             # d*d overflows
    for shift in ((-5000.0, 0.0, 0.0), (0.0, 9000.0, 0.0), (0.0, 0.0, -4000.0)):       # beside the box, parallel to a face
        O.append(mid + shift)
        P.append(mid + shift + (0.0, 700.0, 900.0) if shift[0] else mid + shift + (800.0, 0.0, 0.0))
    O.append(off - (900.0, 900.0, 900.0))
    P.append(off - (100.0, 1500.0, 200.0))                           # ends before the box, heading past its corner
    O.append(off - (2000.0, 2000.0, 2000.0))
    P.append(off - (1000.0, 1000.0, 1000.0))                         # towards the box, ends more than trunc short of it
    # from outside into the box, from inside out of it, through it
    for _ in range(60):
        a = mid + rng.uniform(-2600.0, 2600.0, 3)
        b = mid + rng.uniform(-2600.0, 2600.0, 3)
        O.append(a)
        P.append(b)
    return np.array(O, F), np.array(P, F)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.RandomState(SEED & 0x7FFFFFFF)
    offset = GRID[2]
    out = []
    o_in, p_in, _, _ = scan(INSIDE, fan(96, 48), offset)
    out.append(Case("inside", GRID, [(o_in, p_in, 0.0, INF, 0)], 15000, 8000))
    outside = [scan(o, aimed(fan(240, 120, -85.0, 85.0), o), offset) for o in OUTSIDE]
    out.append(Case("outside", GRID, [(o, p, 0.0, INF, 0) for o, p, _, _ in outside], 20000, 12000))
    per_o = np.concatenate([np.repeat(o[None], len(p), 0) for o, p, _, _ in outside])
    per_p = np.concatenate([p for _, p, _, _ in outside])
    mix = rng.permutation(len(per_p))
    out.append(Case("per_ray_origins", GRID, [(per_o[mix], per_p[mix], 0.0, INF, 0)], 20000, 15000))
    ao, ap = axis_rays(GRID)
    out.append(Case("axes", GRID, [(ao, ap, 0.0, INF, 0), (ao, ap, 0.0, INF, ref.BAND_ONLY)], 400, 400))
    to, tp = tie_rays()
    out.append(Case("ties", TIE_GRID, [(to, tp, 0.0, INF, 0)], 400, 400))
    so, sp = skip_rays(GRID, rng)
    out.append(Case("skips", GRID, [(so, sp, 0.0, INF, 0)], 1200, 10))
    # ranges at, just below and just above one ray's own r (fp32), and NaN ranges: one call each over the same 150 rays
    ro, rp = np.repeat(o_in[None], 150, 0), p_in[rng.choice(len(p_in), 150, replace=False)]
    d = (rp[0] - ro[0]).astype(F)
    r0 = F(np.sqrt(F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))))
    up, down = float(np.nextafter(r0, F(np.inf))), float(np.nextafter(r0, F(-np.inf)))
    out.append(Case("ranges", GRID, [(ro, rp, float(r0), INF, 0), (ro, rp, up, INF, 0), (ro, rp, 0.0, float(r0), 0), (ro, rp, 0.0, down, 0),
                                     (ro, rp, 900.0, 1800.0, ref.BAND_ONLY), (ro, rp, float("nan"), INF, 0), (ro, rp, 0.0, float("nan"), 0)],
                    3000, 500))
    sub = rng.choice(len(p_in), 1200, replace=False)
    out.append(Case("band_only", GRID, [(o_in, p_in[sub], 0.0, INF, ref.BAND_ONLY)], 1500, 300))
    # 70 000 identical rays and a tight fan into one voxel: a count past 2^16 in one word, and every lane on the same few words
    target = np.asarray(offset) + (1437.0, 1812.0, 2011.0)
    tight = target + rng.uniform(-12.0, 12.0, (2000, 3))
    cp = np.concatenate([np.repeat(target[None], 70000, 0), tight]).astype(F)
    out.append(Case("contention", GRID, [(o_in, cp, 0.0, INF, 0)], 30, 30))
    for c in out:
        c.calls = tuple(c.calls)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def permutation_sets():
    """2 000 rays with per-ray origins, and five permutations of them."""
    c = case("per_ray_origins")
    o, p = c.calls[0][0][:2000], c.calls[0][1][:2000]
    rng = np.random.RandomState(7)
    return [(o, p)] + [(o[perm], p[perm]) for perm in (rng.permutation(2000) for _ in range(5))]


def make_geometry(O, grid):
    """The oracle's cleared volume of a grid and its geometry for the reference."""
    dims, phys, offset = grid
    ov = O.Volume(dims, phys)
    ov.offset(*offset)
    return ov, ref.geometry(ov)


@functools.lru_cache(maxsize=None)
def accumulators(name):
    """The reference's rule-7 result of every call of a case (it does not depend on what the volume holds): computed once."""
    import oracle as O
    O.build()
    c = case(name)
    _, geom = make_geometry(O, c.grid)
    return tuple(ref.accumulate(geom, o, p, lo, hi, flags) for o, p, lo, hi, flags in c.calls)


def reference(O, c, dist=None, weight=None, cap=0):
    """Every call of case c applied in turn to (dist, weight) (default: the cleared volume) -> (distances, weights, [updated mask of
    each call])."""
    ov, geom = make_geometry(O, c.grid)
    d = ov.dist if dist is None else dist
    w = ov.weight if weight is None else weight
    masks = []
    for acc in accumulators(c.name):
        d, w, upd = ref.apply(geom, d, w, acc, cap)
        masks.append(upd)
    return d, w, masks
