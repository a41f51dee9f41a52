"""Seeded coloured ray sets for tsdf_integrate_rays_colour* (include/tsdf_amd.h, "ray integration", rules 9 - 12), shared by
tests/test_integrate_rays_colour_host.py (the CPU reference's own properties) and tests/test_integrate_rays_colour.py (the GPU
against it).  A case is a grid, optionally a truncation distance of its own, and a list of calls (origins, points, rgb, min_range,
max_range, flags) applied one after the other to start colour words whose n is drawn from {0, 1, 2, 127, 254, 255}.
Inputs only; the expectations come from tests/rays_colour_ref.py."""
import functools

import numpy as np

from tests import rays_colour_ref as cref
from tests import rays_integrate_cases as RC
from tests import rays_integrate_ref as ref

F = np.float32
INF = float("inf")
SEED = 0xC0105EED
G1 = RC.GRID
# 67 x 6 x 35 voxels of G1's size: two integrate bricks (64 x 4 x 32 voxels) on every axis, x included
G2 = ((67, 6, 35), (67 * 3000.0 / 37, 6 * 3000.0 / 34, 35 * 3000.0 / 45), (-40.0, 25.0, 310.0))
# exact 64 mm voxels, and a truncation distance of three of them: axis rays through voxel centres reach sdf == +trunc and == -trunc
G3 = RC.TIE_GRID
G3_TRUNC = 192.0
START_N = (0, 1, 2, 127, 254, 255)
UNIFORM = (201, 87, 14)
IDENTICAL = (3, 250, 129)


class Case:
    def __init__(self, name, grid, calls, trunc=None, differing=True):
        self.name, self.grid, self.trunc = name, grid, trunc
        # coverage the reference must reach (tests/test_integrate_rays_colour_host.py): a voxel with c_v >= 2 and differing colours
        # (False: a set of one colour, or of rays that do not meet in the band)
        self.differing = differing
        self.calls = []
        for o, p, c, lo, hi, flags in calls:
            o = np.ascontiguousarray(o, F).reshape(-1, 3)
            p = np.ascontiguousarray(p, F).reshape(-1, 3)
            c = np.ascontiguousarray(c, np.uint8).reshape(-1, 3)
            assert len(o) in (1, len(p)) and len(c) == len(p)
            for a in (o, p, c):
                a.setflags(write=False)
            self.calls.append((o, p, c, lo, hi, flags))
        self.calls = tuple(self.calls)


def trunc_edge_rays():
    """On G3: rays along +- each axis from voxel centre to voxel centre, so that sdf is an exact multiple of 64 in every visited cell."""
    dims, phys, offset = G3
    O, P = [], []
    for axis in range(3):
        b, c = [k for k in range(3) if k != axis]
        for jb, jc in ((3, 4), (6, 2)):
            for first, last in ((1, dims[axis] - 5), (dims[axis] - 2, 4), (2, 7)):
                o, p = [0.0] * 3, [0.0] * 3
                o[b] = p[b] = offset[b] + 64.0 * (jb + 0.5)
                o[c] = p[c] = offset[c] + 64.0 * (jc + 0.5)
                o[axis], p[axis] = offset[axis] + 64.0 * (first + 0.5), offset[axis] + 64.0 * (last + 0.5)
                O.append(o)
                P.append(p)
    return np.array(O, F), np.array(P, F)


def g2_scan(rng, n):
    """One origin beside G2's low-x face and n end points spread through the whole box."""
    dims, phys, offset = G2
    off = np.asarray(offset, np.float64)
    pts = off + rng.uniform(0.02, 0.98, (n, 3)) * np.asarray(phys)
    return (off + (-350.0, 0.5 * phys[1], 0.4 * phys[2])).astype(F), pts.astype(F)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.RandomState(SEED & 0x7FFFFFFF)
    colours = lambda n: rng.randint(0, 256, (n, 3)).astype(np.uint8)
    out = []
    # the nine sets of ray integration, a random colour per ray
    for c in RC.cases():
        # (`skips`: its 60 rays that do observe something are too few to meet in a band voxel)
        out.append(Case(c.name, c.grid, [(o, p, colours(len(p)), lo, hi, fl) for o, p, lo, hi, fl in c.calls], differing=c.name != "skips"))
    inside = RC.case("inside").calls[0]
    o_in, p_in = inside[0], inside[1]
    # a tight fan into one voxel, colours alternating 0 and 255: at an even count the voxels every ray crosses have a mean of 127.5
    target = np.asarray(G1[2]) + (1437.0, 1812.0, 2011.0)
    tight = (target + rng.uniform(-12.0, 12.0, (401, 3))).astype(F)
    alternating = np.repeat((np.arange(401) % 2 * 255).astype(np.uint8)[:, None], 3, 1)
    out.append(Case("fan_even", G1, [(o_in, tight[:400], alternating[:400], 0.0, INF, 0)]))
    out.append(Case("fan_odd", G1, [(o_in, tight, alternating, 0.0, INF, 0)]))
    # 70 000 identical rays of one colour: counts past 2^16 in every colour field, every lane on the same words
    same = np.repeat(target[None], 70000, 0).astype(F)
    out.append(Case("identical", G1, [(o_in, same, np.repeat(np.array([IDENTICAL], np.uint8), 70000, 0), 0.0, INF, 0)], differing=False))
    out.append(Case("uniform", G1, [(o_in, p_in, np.repeat(np.array([UNIFORM], np.uint8), len(p_in), 0), 0.0, INF, 0)], differing=False))
    eo, ep = trunc_edge_rays()
    out.append(Case("trunc_edges", G3, [(eo, ep, colours(len(ep)), 0.0, INF, 0)], trunc=G3_TRUNC))
    go, gp = g2_scan(rng, 700)
    out.append(Case("g2_scan", G2, [(go, gp, colours(len(gp)), 0.0, INF, 0), (go, gp[:300], colours(300), 0.0, INF, ref.BAND_ONLY)]))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


NAMES = tuple(c.name for c in cases())


def make_geometry(O, c):
    """The oracle's cleared volume of a case's grid and the geometry for the reference (with the case's own truncation distance)."""
    ov, geom = RC.make_geometry(O, c.grid)
    if c.trunc is not None:
        geom = (geom[0], geom[1], geom[2], F(c.trunc))
    return ov, geom


def start_state(geom, seed=11):
    """(distances, weights, colour words) a case starts from: the cleared field, and words with random channels whose n is drawn from
    START_N all over the grid -- so also all over the band."""
    n = int(np.prod(geom[0]))
    rng = np.random.RandomState(seed)
    words = rng.randint(0, 1 << 24, n).astype(np.uint32) | (np.array(START_N, np.uint32)[rng.randint(0, len(START_N), n)] << np.uint32(24))
    return np.full(n, geom[3], F), np.zeros(n, F), words


def permutation_sets():
    """RC.permutation_sets() with one colour per ray, permuted with its ray."""
    o, p = RC.permutation_sets()[0]
    c = np.random.RandomState(21).randint(0, 256, (len(p), 3)).astype(np.uint8)
    rng = np.random.RandomState(7)
    return [(o, p, c)] + [(o[perm], p[perm], c[perm]) for perm in (rng.permutation(len(p)) for _ in range(5))]


@functools.lru_cache(maxsize=None)
def reference(name, mutant=None, offset_at_clear=(0.0, 0.0, 0.0)):
    """Every call of a case applied in turn to its start state -> (distances, weights, colour words, [updated mask], [acc], [col]) of
    the reference: computed once, never changed."""
    import oracle as O
    O.build()
    c = case(name)
    _, geom = make_geometry(O, c)
    d, w, words = start_state(geom)
    masks, accs, cols = [], [], []
    for o, p, rgb, lo, hi, flags in c.calls:
        d, w, upd, words, acc, col = cref.integrate(geom, d, w, words, o, p, rgb, lo, hi, flags, mutant=mutant, offset_at_clear=offset_at_clear)
        masks.append(upd)
        accs.append(acc)
        cols.append(col)
    for a in (d, w, words):
        a.setflags(write=False)
    return d, w, words, masks, accs, cols
