"""Ray integration on the CPU: what the reference of tests/rays_integrate_ref.py (the header's rules 1 - 8 in numpy scalars) must itself
satisfy before the GPU is compared with it in tests/test_integrate_rays.py, and the coverage of the shared ray sets.  No GPU."""
import numpy as np
import pytest

from tests import rays_integrate_cases as RC
from tests import rays_integrate_ref as ref

F = np.float32
# a grid on which everything is representable: voxel edges 64, 32 and 128 mm, offsets that are multiples of them, truncation 200 mm
EXACT = ((16, 12, 10), np.array([64.0, 32.0, 128.0], F), np.array([-256.0, 128.0, 0.0], F), F(200.0))
# the zero crossing along the scan rays against the analytic range, sphere scene fused from the three outside origins into a cleared
# 37 x 34 x 45 volume: the largest deviation measured on the CPU reference, and the bound asserted -- half a voxel diagonal over it
CROSSING_MEASURED_MM = 94.5
HALF_DIAGONAL_MM = 0.5 * float(np.sqrt(81.08108 ** 2 + 88.23529 ** 2 + 66.666664 ** 2))


def centre(geom, cell):
    return [float(geom[2][k]) + (cell[k] + 0.5) * float(geom[1][k]) for k in range(3)]


@pytest.mark.parametrize("axis,sign", [(a, s) for a in range(3) for s in (1, -1)])
def test_an_axis_ray_through_voxel_centres_visits_exactly_its_row(axis, sign):
    dims, vs, offset, trunc = EXACT
    fixed = [5, 7, 3]
    first, last = (2, dims[axis] - 3) if sign > 0 else (dims[axis] - 3, 2)
    cell = lambda j: tuple(j if k == axis else fixed[k] for k in range(3))
    o, p = centre(EXACT, cell(first)), centre(EXACT, cell(last))
    cells, obs = ref.walk(EXACT, o, p)
    r = abs(last - first) * float(vs[axis])
    # from the origin's cell to the last cell whose near face lies within r + trunc, never leaving the row
    reach = int(np.floor(((r + float(trunc)) / float(vs[axis])) + 0.5))
    expected = [cell(first + sign * j) for j in range(min(reach, (dims[axis] - 1 - first) if sign > 0 else first) + 1)]
    assert cells == expected
    seen = 0
    for c in cells:
        sdf = r - abs(c[axis] - first) * float(vs[axis])                  # r minus the centre's distance along the ray: exact in fp32
        if sdf < -float(trunc):
            assert c not in obs
            continue
        want = min(sdf, float(trunc))
        assert obs[c][0] == F(sdf) and obs[c][1] == F(want) and obs[c][2] == int(np.rint(want / float(trunc) * 32768.0))
        seen += 1
    assert seen >= 4 and any(c not in obs for c in cells) == (reach * float(vs[axis]) - r > float(trunc))


def test_band_only_starts_at_the_band():
    dims, vs, offset, trunc = EXACT
    o, p = centre(EXACT, (1, 6, 4)), centre(EXACT, (12, 6, 4))
    full, band = ref.walk(EXACT, o, p)[0], ref.walk(EXACT, o, p, flags=ref.BAND_ONLY)[0]
    # r = 704, trunc = 200: the band starts at t = 504, grid coordinate 1.5 + 504 / 64 = 9.375: cell 9
    assert full[0] == (1, 6, 4) and band[0] == (9, 6, 4) and band == full[8:]


def test_permuting_the_rays_leaves_every_bit():
    import oracle as O
    O.build()
    sets = RC.permutation_sets()
    ov, geom = RC.make_geometry(O, RC.GRID)
    rng = np.random.RandomState(3)
    dist = rng.uniform(-1, 1, ov.dist.size).astype(F) * geom[3]
    weight = rng.randint(0, 5, ov.dist.size).astype(F)
    results = [ref.integrate(geom, dist, weight, o, p) for o, p in sets]
    assert not np.array_equal(sets[0][1], sets[1][1])
    for d, w, upd, acc in results[1:]:
        assert acc == results[0][3]
        assert np.array_equal(d.view(np.uint32), results[0][0].view(np.uint32)) and np.array_equal(w, results[0][1])
    # touched voxels gain exactly 1, the others keep their bits
    d, w, upd, _ = results[0]
    assert upd.sum() >= 10000 and (~upd).sum() >= 10000
    assert np.array_equal(w[upd], weight[upd] + 1) and np.array_equal(w[~upd], weight[~upd])
    assert np.array_equal(d[~upd].view(np.uint32), dist[~upd].view(np.uint32))
    assert (d[upd] != dist[upd]).mean() > 0.9


def test_a_weight_cap_clamps_the_stored_weight_only():
    geom = EXACT
    n = int(np.prod(EXACT[0]))
    dist, weight = np.full(n, 100.0, F), np.full(n, 4.0, F)
    o, p = centre(EXACT, (1, 6, 4)), centre(EXACT, (12, 6, 4))
    d0, w0, upd, _ = ref.integrate(geom, dist, weight, [o], [p])
    d1, w1, _, _ = ref.integrate(geom, dist, weight, [o], [p], cap=4)
    assert upd.sum() >= 10 and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    assert (w0[upd] == 5).all() and (w1[upd] == 4).all() and np.array_equal(w1[~upd], weight[~upd])


@pytest.mark.parametrize("name", [c.name for c in RC.cases()])
def test_every_case_set_keeps_its_coverage(name):
    import oracle as O
    O.build()
    c = RC.case(name)
    accs = RC.accumulators(name)
    _, _, masks = RC.reference(O, c)
    updated = np.logical_or.reduce(masks)
    multi = set()
    for acc in accs:
        multi |= {cell for cell, (n_v, _) in acc.items() if n_v > 1}
    assert int(updated.sum()) >= c.min_updated, int(updated.sum())
    assert len(multi) >= c.min_multi, len(multi)
    assert (~updated).sum() >= 1000                                        # something is left alone, too
    if name == "contention":
        assert max(n_v for n_v, _ in accs[0].values()) >= 70000            # a count past 2^16 in one word
    if name == "skips":
        # the decreed skips and the misses observe nothing on their own
        o, p = c.calls[0][0], c.calls[0][1]
        geom = RC.make_geometry(O, c.grid)[1]
        assert all(ref.walk(geom, o[i], p[i]) == ([], {}) for i in range(27))
        assert sum(1 for i in range(27, len(p)) if ref.walk(geom, o[i], p[i])[1]) >= 30
    if name == "ranges":
        # the ray the ranges are taken from is in at min_range == r and max_range == r, out one ulp beyond
        n0 = [len(acc) for acc in accs]
        o, p = c.calls[0][0][0], c.calls[0][1][0]
        geom = RC.make_geometry(O, c.grid)[1]
        seen = [bool(ref.walk(geom, o, p, lo, hi, fl)[1]) for _, _, lo, hi, fl in c.calls]
        assert seen[:4] == [True, False, True, False] and n0[5] == 0 and n0[6] == 0 and min(n0[:5]) > 0


def crossing_deviations(O):
    """Per scan ray of the `outside` case with a sign change along its walk: |interpolated zero crossing - analytic range| (mm), of the
    crossing nearest that range."""
    c = RC.case("outside")
    d, w, _ = RC.reference(O, c)
    _, geom = RC.make_geometry(O, c.grid)
    dims = geom[0]
    scans = [RC.scan(o, RC.aimed(RC.fan(240, 120, -85.0, 85.0), o), c.grid[2]) for o in RC.OUTSIDE]
    devs = []
    for (o, pts, ranges, _), call in zip(scans, c.calls):
        assert np.array_equal(pts, call[1])
        lo, hi = np.array(c.grid[2]) + 2.0 * geom[1], np.array(c.grid[2]) + np.array(c.grid[1]) - 2.0 * geom[1]
        for p, rng_mm in zip(pts[::4], ranges[::4]):
            if not ((p > lo).all() and (p < hi).all()):                  # (the surface point itself must lie in the grid, two voxels in)
                continue
            cells, _ = ref.walk(geom, o, p)
            u = (p.astype(np.float64) - o) / np.linalg.norm(p.astype(np.float64) - o)
            samples = []
            for cell in cells:
                at = (cell[2] * dims[1] + cell[1]) * dims[0] + cell[0]
                if w[at] > 0:
                    samples.append((float((np.array(centre(geom, cell)) - o) @ u), float(d[at])))
            samples.sort()
            # (a ray that grazes the sphere on its way to the wall crosses the band other rays left there: the crossing meant is its own)
            own = [abs(ta + (tb - ta) * va / (va - vb) - rng_mm) for (ta, va), (tb, vb) in zip(samples, samples[1:]) if va > 0 >= vb]
            if own:
                devs.append(min(own))
    return np.array(devs)


def test_the_fused_sphere_scene_crosses_zero_at_the_analytic_range():
    import oracle as O
    O.build()
    devs = crossing_deviations(O)
    print("zero crossing: %d rays, largest deviation %.2f mm, mean %.2f mm" % (len(devs), devs.max(), devs.mean()))
    assert len(devs) >= 350
    assert devs.max() <= CROSSING_MEASURED_MM + HALF_DIAGONAL_MM, devs.max()
