"""Colour alignment on the GPU (include/tsdf_amd.h, "colour alignment"; tsdf_amd/csrc/align.hip) against its CPU reference
(tests/align_colour_ref.py): the intensity query and both rows of every point bit for bit in both instances of the division, one step's
two blocks of sums and the combined system bit for bit, the chain on the textured wall against the float64 reference chain within the
tolerance tests/test_align.py computes, what a zero weight and outliers reduce to, what the calls leave alone, every refusal and
rgb_to_intensity."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import align_colour_ref as CR
from tests import align_ref as R
from tests import field_ref
from tests.helpers import assert_same_floats
from tsdf_amd import _capi

pytestmark = pytest.mark.gpu
F = np.float32
COUNTS = (1, 63, 64, 65, 255, 256, 257, 65536, 65537)
DIMS = (24, 20, 28)
# Three different voxel edges per volume.  One edge below 1 fails the proof of the fast division (tests/field_cases.py), and 3, 6 and 12
# share the mantissa of the 3 that passes it: the two volumes run one instance each of every kernel's division.
EDGES = {0: (0.75, 0.375, 1.5), 1: (3.0, 6.0, 12.0)}
OFFSET_VOXELS = (-10.5, 5.25, 14.0)
COLOUR_GATE = 40.0
WEIGHT = 0.37


class Case:
    pass


def surface_k(i, j):
    """The plane index (continuous) at which the case's field is zero above voxel column (i, j): a bumpy sheet without a symmetry."""
    return 12.3 - (1.5 * np.sin(0.35 * i + 0.2) * np.cos(0.3 * j) + 0.005 * (i - 12.0) * (j - 10.0))


def build_case(oracle, proved):
    """A 24 x 20 x 28 volume filled by upload: the distance (along z, mm) to surface_k, every weight 1 but 3 % zeros, random colour
    words with a tenth never observed (n = 0); its GPU twin; points of every kind; the reference's answers."""
    c = Case()
    rng = np.random.RandomState(90 + proved)
    edges = EDGES[proved]
    c.phys = tuple(n * e for n, e in zip(DIMS, edges))
    c.offset = tuple(v * e for v, e in zip(OFFSET_VOXELS, edges))
    c.vol = tsdf_amd.TSDFVolume(DIMS, c.phys)
    c.vol.offset(*c.offset)
    c.geom = field_ref.geometry(c.vol)
    dims, vs, offset = c.geom
    assert tuple(vs) == tuple(F(e) for e in edges)
    X, Y, Z = DIMS
    k, j, i = np.meshgrid(np.arange(Z) + 0.5, np.arange(Y) + 0.5, np.arange(X) + 0.5, indexing="ij")
    c.dist = ((surface_k(i, j) - k) * edges[2]).astype(F).reshape(-1)              # positive below the sheet (small z)
    c.weight = (rng.uniform(size=X * Y * Z) >= 0.03).astype(F)
    words = rng.randint(0, 1 << 24, X * Y * Z).astype(np.uint32) | (rng.randint(1, 256, X * Y * Z).astype(np.uint32) << np.uint32(24))
    words[rng.uniform(size=X * Y * Z) < 0.10] &= np.uint32(0x00FFFFFF)
    c.colour = words
    c.vol.set_distance_data(c.dist)
    c.vol.set_weight_data(c.weight)
    c.vol.enable_colour()
    c.vol.set_colour_data(c.colour)
    assert c.vol.info().fast_division_verified == proved
    c.gate = 2.0 * edges[2]
    mx = np.array(field_ref.bounds(dims, vs), F)
    c.mx = mx

    def near_surface(n, spread):
        ij = np.stack([rng.uniform(1.6, X - 1.6, n), rng.uniform(1.6, Y - 1.6, n)], axis=1)
        kk = surface_k(ij[:, 0], ij[:, 1]) + rng.uniform(-spread, spread, n)
        q = np.stack([ij[:, 0] * edges[0], ij[:, 1] * edges[1], kk * edges[2]], axis=1)
        return (q + offset).astype(F)

    parts = {"surface": near_surface(2500, 2.4), "random": (offset + rng.uniform(-0.05, 1.05, (600, 3)) * mx).astype(F)}
    face = []
    for a in range(3):                 # within one voxel of each face: the far half voxels clamp their upper taps
        for far in (False, True):
            q = (vs * F(1.5) + rng.uniform(0, 1, (40, 3)) * (mx - vs * F(3))).astype(F)
            t = rng.uniform(0.02, 0.98, 40).astype(F) * vs[a]
            q[:, a] = (mx[a] - vs[a]) + t if far else t
            face.append((q + offset).astype(F))
    parts["faces"] = np.concatenate(face)
    inside = (offset + mx * F(0.5)).astype(F)
    special = []
    for a in range(3):
        for v in (F(np.nan), F(np.inf), F(-np.inf), F(-0.0), F(3.0e38), F(offset[a] + mx[a])):
            p = inside.copy()
            p[a] = v
            special.append(p)
    parts["special"] = np.array(special, F)
    out, c.where, at = [], {}, 0
    for name, p in parts.items():
        out.append(p)
        c.where[name] = slice(at, at + len(p))
        at += len(p)
    c.points = np.concatenate(out).astype(F)
    # observed intensities: anywhere in the range the random colours' intensities have, a tenth of the points without colour
    c.intensity = rng.uniform(40, 215, len(c.points)).astype(F)
    c.intensity[rng.uniform(size=len(c.points)) < 0.1] = np.nan
    c.intensity[c.where["surface"]][5::97] = np.inf                    # (a view: an infinite intensity is no intensity either)
    c.poses = [np.eye(4), R.perturbation(0.4 * edges[0], 1.0, R.pivot(c.geom)[1], 21)]
    c.sum_points = near_surface(max(COUNTS), 1.5)
    c.sum_points[rng.uniform(size=max(COUNTS)) < 0.1] = (offset + rng.uniform(-0.05, 1.05, 3) * mx).astype(F)
    c.sum_intensity = rng.uniform(60, 195, max(COUNTS)).astype(F)
    c.sum_intensity[rng.uniform(size=max(COUNTS)) < 0.05] = np.nan
    for a in (c.dist, c.weight, c.colour, c.points, c.intensity, c.sum_points, c.sum_intensity):
        a.setflags(write=False)
    c.oracle = oracle
    c.aligner = tsdf_amd.FieldAligner()
    return c


def wall_volume(s):
    """The GPU twin of tests/align_colour_ref.py's wall scene."""
    vol = tsdf_amd.TSDFVolume(CR.WALL_SIZE, tuple(n * CR.WALL_VOXEL for n in CR.WALL_SIZE))
    vol.offset(*CR.WALL_OFFSET)
    vol.set_distance_data(s.dist)
    vol.set_weight_data(s.weight)
    vol.enable_colour()
    vol.set_colour_data(s.colour)
    geom = field_ref.geometry(vol)
    assert geom[0] == s.geom[0] and np.array_equal(geom[1], s.geom[1]) and np.array_equal(geom[2], s.geom[2])
    return vol


@pytest.fixture(scope="module", params=[0, 1], ids=["ieee-division", "fast-division"])
def case(request, oracle):
    c = build_case(oracle, request.param)
    yield c
    c.aligner.close()
    c.vol.close()


@pytest.fixture(scope="module")
def wall():
    s = CR.wall_scene()
    s.gv = wall_volume(s)
    s.aligner = tsdf_amd.FieldAligner()
    # the frame at steps 4, 2 and 1 with 4 / 5 / 10 iterations, as the tracker runs it
    s.stages = [(CR.wall_points(s.depth, st), CR.rgb_to_intensity(s.rgb, CR.WALL_W, CR.WALL_H, st).reshape(-1), it) for st, it in ((4, 4), (2, 5), (1, 10))]
    yield s
    s.aligner.close()
    s.gv.close()


def volume_state(vol):
    return (vol.get_distance_data(), vol.get_weight_data(), vol.get_colour_data()) + vol.occupancy_data() + (vol.weight_storage(), vol.occupancy())


def assert_same_state(after, before):
    assert_same_floats(after[0], before[0], "distances after the calls")
    assert_same_floats(after[1], before[1], "weights after the calls")
    assert np.array_equal(after[2], before[2]), "colours after the calls"
    for a, b, name in zip(after[3:6], before[3:6], ("fine", "cell", "reach")):
        assert np.array_equal(a, b), name
    assert after[6:] == before[6:]


def test_sample_intensity_matches_the_reference_bit_for_bit(case):
    c = case
    ref_c, ref_g = CR.sample_intensity(c.geom, c.colour, c.points)
    ok = np.isfinite(ref_c)
    print("intensity: %d of %d points valid; on the faces %d of %d" % (ok.sum(), len(ok), ok[c.where["faces"]].sum(), len(ok[c.where["faces"]])))
    assert ok.sum() >= 500 and (~ok).sum() >= 500 and ok[c.where["faces"]].sum() >= 40
    assert not ok[c.where["special"]][[0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 16, 17]].any()
    assert np.array_equal(np.isnan(ref_g).any(axis=1), ~ok)
    # a clamped tap gives a zero difference: on every far face some valid point has an exactly zero component along that axis
    for a in range(3):
        far = c.where["faces"].start + (2 * a + 1) * 40
        assert (ref_g[far:far + 40][ok[far:far + 40]][:, a] == 0).any()
    got_c, got_g = c.vol.sample_intensity(c.points)
    assert_same_floats(got_c, ref_c, "intensity")
    assert_same_floats(got_g, ref_g, "intensity gradient")
    assert_same_floats(c.vol.sample_intensity(c.points, gradient=False)[0], ref_c, "intensity alone")
    only_g = np.empty((len(c.points) + 1, 3), F)
    _capi.check(_capi.lib.tsdf_volume_sample_intensity(c.vol._h, len(c.points), c.points.ctypes.data, None, only_g.ctypes.data))
    assert_same_floats(only_g[:-1], ref_g, "gradient alone")
    assert c.vol.sample_intensity(c.points[:0])[0].shape == (0,)


def test_both_rows_match_the_reference_bit_for_bit(case):
    c = case
    for T in c.poses:
        ref, inl, inl_c = CR.rows_at(c.oracle, c.geom, c.dist, c.weight, c.colour, c.points, c.intensity, R.to_pivot(T, c.geom), c.gate, COLOUR_GATE)
        print("rows: %d geometric inliers, %d colour inliers, %d geometric inliers that are colour outliers" % (inl.sum(), inl_c.sum(), (inl & ~inl_c).sum()))
        assert inl_c.sum() >= 100 and (inl & ~inl_c).sum() >= 100 and not (inl_c & ~inl).any()
        # colour outliers of every kind among the geometric inliers: no intensity observed, a tap never seen, the colour gate
        with np.errstate(all="ignore"):
            q = ((np.c_[c.points, np.ones(len(c.points))] @ R.to_pivot(T, c.geom).T)[:, :3] + R.pivot(c.geom)[0]).astype(F)
        cq, _ = CR.intensity_at(c.geom, c.colour, q)
        assert (inl & ~np.isfinite(c.intensity)).sum() >= 20 and (inl & np.isfinite(c.intensity) & np.isnan(cq)).sum() >= 50
        assert (inl & np.isfinite(c.intensity) & np.isfinite(cq) & ~inl_c).sum() >= 20
        assert np.isnan(ref[~inl, :7]).all() and np.isfinite(ref[inl, :7]).all() and np.isnan(ref[~inl_c, 7:]).all() and np.isfinite(ref[inl_c, 7:]).all()
        A, b, res, count, rows = c.aligner.step(c.vol, c.points, T, c.gate, rows=True, intensity=c.intensity, colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
        assert rows.shape == (len(c.points), 14)
        assert_same_floats(rows, ref, "rows")
        assert count == (inl.sum(), inl_c.sum())
        # the geometric half is the plain step's
        plain = c.aligner.step(c.vol, c.points, T, c.gate, rows=True)
        assert_same_floats(rows[:, :7], plain[4], "geometric rows")


@pytest.mark.parametrize("n", COUNTS)
def test_sums_match_the_emulated_order_bit_for_bit(case, n):
    c = case
    if not hasattr(c, "sum_ref"):
        rows, inl, inl_c = CR.rows_at(c.oracle, c.geom, c.dist, c.weight, c.colour, c.sum_points, c.sum_intensity, R.to_pivot(c.poses[1], c.geom), c.gate,
                                      COLOUR_GATE)
        assert inl.sum() * 2 >= len(inl) and inl_c.sum() * 8 >= len(inl) and (inl & ~inl_c).sum() >= 3000
        c.sum_ref = (rows, inl, inl_c) + CR.blocks(rows, inl, inl_c)
    rows, inl, inl_c, Pg, Pc = c.sum_ref
    assert R.blocks_for(n) == {1: 1, 63: 1, 64: 1, 65: 1, 255: 1, 256: 1, 257: 2, 65536: 256, 65537: 256}[n]
    tg, tc = R.sums_kernel_order(Pg[:n]), R.sums_kernel_order(Pc[:n])
    T = c.poses[1]
    first = None
    # The geometric block comes out on its own at weight 0.  The call hands out the combined system only, so the colour block's 27
    # entries of A and b are read through a weight of 2^60: a power of two scales S_c exactly, and wherever |S_g| lies below a quarter
    # of an fp32 ulp of 2^60 |S_c| the combined entry is 2^60 S_c itself -- dividing it out gives S_c bit for bit.
    HUGE = 2.0 ** 60
    for w in (WEIGHT, 0.0, HUGE):
        A0, b0, _, _ = R.system(CR.combine(tg, tc, w))
        A, b, res, count = c.aligner.step(c.vol, c.sum_points[:n], T, c.gate, intensity=c.sum_intensity[:n], colour_gate=COLOUR_GATE, colour_weight=w)
        if first is None:
            first = (A, b, res, count)
            print("n = %d: inliers %s (reference %g, %g), residuals %r (reference %r, %r)" % (n, count, tg[28], tc[28], res, tg[27], tc[27]))
        assert count == (tg[28], tc[28]) == (inl[:n].sum(), inl_c[:n].sum())
        assert_same_floats(A, A0, "A at weight %g" % w)
        assert_same_floats(b, b0, "b at weight %g" % w)
        assert_same_floats(list(res), [tg[27], tc[27]], "residuals")
        assert np.array_equal(A, A.T)
        if w == HUGE:
            Ag, bg, _, _ = R.system(tg)
            Ac, bc, _, _ = R.system(tc)
            for got, sg, sc, name in ((A, Ag, Ac, "A"), (b, bg, bc, "b")):
                seen = sc != 0
                assert (np.abs(sg[seen].astype(np.float64)) < 2.0 ** -26 * HUGE * np.abs(sc[seen].astype(np.float64))).all()
                assert_same_floats((got[seen].astype(np.float64) / HUGE).astype(F), sc[seen], "the colour block's " + name)
                assert_same_floats(got[~seen], sg[~seen], "%s where the colour block is zero" % name)
            assert tc[28] == 0 or (Ac != 0).sum() >= 30
    # weight 0 is the plain step's system
    plain = c.aligner.step(c.vol, c.sum_points[:n], T, c.gate)
    assert_same_floats(plain[0], R.system(tg)[0], "the plain A")
    again = c.aligner.step(c.vol, c.sum_points[:n], T, c.gate, intensity=c.sum_intensity[:n], colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
    assert_same_floats(again[0], first[0], "A, second call")
    assert_same_floats(again[1], first[1], "b, second call")
    assert again[2:] == first[2:]
    with_rows = c.aligner.step(c.vol, c.sum_points[:n], T, c.gate, rows=True, intensity=c.sum_intensity[:n], colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
    assert_same_floats(with_rows[0], first[0], "A beside rows")
    assert_same_floats(with_rows[4], rows[:n], "rows")


def test_a_zero_weight_is_the_plain_run_bit_for_bit(case, wall):
    c = case
    near = c.points[c.where["surface"]]
    y = c.intensity[c.where["surface"]]
    stages = [(near[::3], 3), (near, 4)]
    plain = c.aligner.run(c.vol, stages, c.poses[1], c.gate)
    zero = c.aligner.run(c.vol, stages, c.poses[1], c.gate, intensity=[y[::3], y], colour_gate=COLOUR_GATE, colour_weight=0.0)
    assert plain[2] > 100 and not np.array_equal(plain[0], c.poses[1])                  # it saw the surface and moved
    assert np.array_equal(zero[0], plain[0]) and zero[1][0] == plain[1] and zero[2][0] == plain[2]
    assert zero[2][1] > 50
    moved = c.aligner.run(c.vol, stages, c.poses[1], c.gate, intensity=[y[::3], y], colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
    assert not np.array_equal(moved[0], plain[0])
    # the wall, whose plain system is singular
    s = wall
    plain = s.aligner.run(s.gv, [(p, it) for p, _, it in s.stages], s.T0, s.gate)
    zero = s.aligner.run(s.gv, [(p, it) for p, _, it in s.stages], s.T0, s.gate, intensity=[y for _, y, _ in s.stages], colour_gate=s.colour_gate,
                         colour_weight=0.0)
    assert np.array_equal(zero[0], plain[0]) and zero[1][0] == plain[1] and zero[2][0] == plain[2] == len(s.points)


def test_the_colour_chain_recovers_the_wall_and_follows_the_float64_reference(wall, oracle):
    """Tolerance: 8 x the distance between the reference chain summed in float64 and the same chain summed in fp32 in ascending point
    order -- the kernel's order is a third order of the same sums (tests/test_align.py's rule, for its reason)."""
    s = wall
    ref, norms, counts = CR.chain(oracle, s, s.stages, s.T0, s.gate, s.colour_gate, WEIGHT, order="f64")
    asc, _, _ = CR.chain(oracle, s, s.stages, s.T0, s.gate, s.colour_gate, WEIGHT, order="ascending")
    tol = 8 * R.pose_distance(ref, asc)
    points = [(p, it) for p, _, it in s.stages]
    ys = [y for _, y, _ in s.stages]
    T, res, count = s.aligner.run(s.gv, points, s.T0, s.gate, intensity=ys, colour_gate=s.colour_gate, colour_weight=WEIGHT)
    plain, _, plain_count = s.aligner.run(s.gv, points, s.T0, s.gate)
    start = CR.in_plane_error(s.T0)
    err = R.pose_distance(T, ref)
    print("wall chain: |GPU - float64 reference| = %.3e, tolerance 8 x %.3e = %.3e; in-plane error %.3f mm at the start, %.3e mm with colour "
          "(reference %.3e mm), %.3f mm without; inliers %s" % (err, tol / 8, tol, start, CR.in_plane_error(T), CR.in_plane_error(ref),
                                                                 CR.in_plane_error(plain), count))
    assert tol > 0
    assert err <= tol
    assert count == (len(s.points), len(s.points)) and plain_count == len(s.points)
    assert CR.in_plane_error(T) <= 0.25 * start
    assert CR.in_plane_error(plain) >= 0.75 * start
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-12 and np.array_equal(T[3], [0, 0, 0, 1])
    # the same bits across two runs and from a second aligner
    T2, res2, count2 = s.aligner.run(s.gv, points, s.T0, s.gate, intensity=ys, colour_gate=s.colour_gate, colour_weight=WEIGHT)
    assert np.array_equal(T2, T) and (res2, count2) == (res, count)
    other = tsdf_amd.FieldAligner()
    T3, res3, count3 = other.run(s.gv, points, s.T0, s.gate, intensity=ys, colour_gate=s.colour_gate, colour_weight=WEIGHT)
    other.close()
    assert np.array_equal(T3, T) and (res3, count3) == (res, count)
    # the convenience over a one-stage run
    one = s.aligner.run(s.gv, [(s.points, 6)], s.T0, s.gate, intensity=[s.intensity], colour_gate=s.colour_gate, colour_weight=WEIGHT)
    conv = s.gv.align_points(s.points, s.T0, iterations=6, gate=s.gate, intensity=s.intensity, colour_gate=s.colour_gate, colour_weight=WEIGHT)
    assert np.array_equal(conv[0], one[0]) and conv[1:] == one[1:]


def test_outliers_reduce_to_the_plain_system_or_leave_the_pose(case):
    c = case
    near = c.points[c.where["surface"]]
    T = c.poses[1]
    # every point a colour outlier: no intensity, or one the gate refuses
    plain = c.aligner.step(c.vol, near, T, c.gate)
    for y in (np.full(len(near), np.nan, F), np.full(len(near), 1.0e4, F)):
        A, b, res, count = c.aligner.step(c.vol, near, T, c.gate, intensity=y, colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
        assert count[0] == plain[3] > 100 and count[1] == 0 and res[1] == 0 and res[0] == plain[2]
        assert_same_floats(A, plain[0], "A of an all-outlier colour set")
        assert_same_floats(b, plain[1], "b of an all-outlier colour set")
        Tr = c.aligner.run(c.vol, [(near, 3)], T, c.gate, intensity=[y], colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
        assert np.array_equal(Tr[0], c.aligner.run(c.vol, [(near, 3)], T, c.gate)[0]) and Tr[2][1] == 0
    # every point a geometric outlier: zeros, the pose as given
    rng = np.random.RandomState(3)
    far = (np.array(c.geom[2]) + c.mx * 2 + rng.uniform(0, 50, (700, 3))).astype(F)
    far[::7] = np.nan
    y = np.full(len(far), 100.0, F)
    A, b, res, count = c.aligner.step(c.vol, far, T, c.gate, intensity=y, colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
    assert count == (0, 0) and res == (0, 0) and not A.any() and not b.any()
    Tr, res, count = c.aligner.run(c.vol, [(far, 3)], T, c.gate, intensity=[y], colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
    assert np.array_equal(Tr, T) and count == (0, 0) and res == (0, 0)
    for stages, ys in (([], []), ([(far[:0], 4)], [y[:0]]), ([(near, 0)], [c.intensity[c.where["surface"]]])):
        Tr, res, count = c.aligner.run(c.vol, stages, T, c.gate, intensity=ys, colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
        assert np.array_equal(Tr, T) and count == (0, 0)
    A, b, res, count = c.aligner.step(c.vol, far[:0], T, c.gate, intensity=y[:0], colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
    assert count == (0, 0) and not A.any()


def test_the_calls_leave_the_volume_alone(case):
    c = case
    before = volume_state(c.vol)
    near, y = c.points[c.where["surface"]], c.intensity[c.where["surface"]]
    c.vol.sample_intensity(c.points)
    c.aligner.step(c.vol, c.points, c.poses[1], c.gate, rows=True, intensity=c.intensity, colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
    c.aligner.run(c.vol, [(near[::4], 2), (near, 3)], c.poses[1], c.gate, intensity=[y[::4], y], colour_gate=COLOUR_GATE, colour_weight=WEIGHT)
    c.vol.align_points(near, c.poses[1], iterations=2, gate=c.gate, intensity=y)
    assert_same_state(volume_state(c.vol), before)


def test_refusals(case):
    c = case
    lib = _capi.lib
    slab = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3, slab=(0, 8))
    grey = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3)              # no colour enabled
    guard = np.full(36 + 6 + 4, 7.0, F)
    T = np.ascontiguousarray(np.eye(4).T.reshape(-1))
    stage = (_capi.AlignColourStage * 9)()
    dp = C.c_void_p()
    _capi.check(lib.tsdf_device_alloc(4096, C.byref(dp)))
    for st in stage:
        st.device_points, st.device_intensity, st.n, st.iterations = dp.value, dp.value, 4, 1
    res, inl = np.full(2, 7.0, F), np.full(2, 7.0, F)
    h, v = c.aligner._h, c.vol._h
    ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x

    def step(a=h, vol=v, points=dp, ys=dp, pose=T, gate=50.0, cg=30.0, cw=0.5, A=guard[:36], b=guard[36:42], ri=guard[42:]):
        return lib.tsdf_aligner_step_colour(a, vol, 4, points, ys, ptr(pose), gate, cg, cw, ptr(A), ptr(b), ptr(ri), None)

    def run(a=h, vol=v, n=1, stages=stage, pose=T, gate=50.0, cg=30.0, cw=0.5):
        return lib.tsdf_aligner_run_colour(a, vol, n, stages, gate, cg, cw, ptr(pose), res.ctypes.data, inl.ctypes.data)

    def sample(vol=v, points=dp, out_c=dp, out_g=None):
        return lib.tsdf_volume_sample_intensity_device(vol, 4, points, out_c, out_g, None)

    bad = T.copy()
    try:
        _capi.check(lib.tsdf_device_upload(dp, np.zeros(1024, F).ctypes.data, 4096))
        assert step() == _capi.TSDF_OK and run() == _capi.TSDF_OK and run(n=8) == _capi.TSDF_OK and sample() == _capi.TSDF_OK
        assert step(cw=0.0) == _capi.TSDF_OK
        guard[:], res[:], inl[:] = 7.0, 7.0, 7.0
        refused = []
        # everything tsdf_aligner_* refuses
        refused += [step(a=None), step(vol=None), step(points=None), step(pose=None), step(A=None), step(b=None), step(ri=None)]
        refused += [run(a=None), run(vol=None), run(pose=None), run(stages=None), run(n=9)]
        refused += [step(vol=slab._h), run(vol=slab._h), sample(vol=slab._h)]
        for i, value in ((0, np.nan), (6, np.inf), (13, -np.inf)):
            bad[:] = T
            bad[i] = value
            refused += [step(pose=bad), run(pose=bad)]
        for gate in (0.0, -1.0, float("nan")):
            refused += [step(gate=gate), run(gate=gate)]
        null_points = (_capi.AlignColourStage * 1)()
        null_points[0].device_intensity, null_points[0].n, null_points[0].iterations = dp.value, 4, 1
        refused += [run(stages=null_points)]
        # what the colour term adds
        refused += [step(vol=grey._h), run(vol=grey._h), sample(vol=grey._h)]
        refused += [step(ys=None)]
        null_ys = (_capi.AlignColourStage * 1)()
        null_ys[0].device_points, null_ys[0].n, null_ys[0].iterations = dp.value, 4, 1
        refused += [run(stages=null_ys)]
        for cg in (0.0, -3.0, float("nan")):
            refused += [step(cg=cg), run(cg=cg)]
        for cw in (-0.5, float("nan"), float("inf"), -float("inf")):
            refused += [step(cw=cw), run(cw=cw)]
        refused += [sample(vol=None), sample(points=None), sample(out_c=None, out_g=None)]
        refused += [lib.tsdf_volume_sample_intensity(v, 4, None, guard.ctypes.data, None), lib.tsdf_volume_sample_intensity(v, 4, guard.ctypes.data, None, None)]
        r2i = lambda rgb=dp, out=dp, step=1, w=4: lib.tsdf_rgb_to_intensity_device(w, 4, rgb, step, out, None)
        refused += [r2i(step=0), r2i(rgb=None), r2i(out=None), r2i(w=0), r2i(w=70000)]
        assert all(rc == _capi.TSDF_ERR_INVALID for rc in refused), refused
        assert (guard == 7.0).all() and (res == 7.0).all() and (inl == 7.0).all(), "a refused call wrote a result"
        assert np.array_equal(T, np.eye(4).reshape(-1))
        assert _capi.last_error()
        # the Python surface raises
        pts, ys = np.zeros((4, 3), F), np.zeros(4, F)
        with pytest.raises(ValueError):
            c.aligner.run(grey, [(pts, 1)], intensity=[ys])
        with pytest.raises(ValueError):
            c.aligner.run(c.vol, [(pts, 1)], intensity=[ys], colour_weight=-1.0)
        with pytest.raises(ValueError):
            c.aligner.step(c.vol, pts, intensity=ys, colour_gate=0.0)
        with pytest.raises(ValueError):
            c.aligner.step(c.vol, pts, intensity=ys[:3])
        with pytest.raises(ValueError):
            c.vol.align_points(pts, intensity=ys, colour_weight=float("inf"))
        with pytest.raises(ValueError):
            grey.sample_intensity(pts)
        with pytest.raises(ValueError):
            tsdf_amd.rgb_to_intensity(np.zeros(48, np.uint8), 4, 4, step=0)
    finally:
        lib.tsdf_device_free(dp)
        slab.close()
        grey.close()


@pytest.mark.parametrize("step", [1, 2, 4])
def test_rgb_to_intensity_matches_the_reference(step):
    w, h = 37, 29
    rng = np.random.RandomState(12)
    rgb = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    rgb[0, 0], rgb[h - 1, w - 1], rgb[h - 1, 0] = (0, 0, 0), (255, 255, 255), (255, 0, 255)
    got = tsdf_amd.rgb_to_intensity(rgb, w, h, step=step)
    ref = CR.rgb_to_intensity(rgb, w, h, step)
    assert got.shape == ref.shape == (-(-h // step), -(-w // step))
    assert_same_floats(got, ref, "intensities at step %d" % step)
    assert got[0, 0] == 0 and (step != 4 or got[-1, -1] == 255)              # (36 and 28 are multiples of 4, 2 and 1)
    # it pairs up with depth_to_points at the same step
    depth = np.full(w * h, 1000, np.uint16)
    assert tsdf_amd.depth_to_points(depth, w, h, np.eye(3, dtype=F).reshape(-1), step=step).shape[:2] == got.shape
