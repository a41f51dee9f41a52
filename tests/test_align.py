"""Field alignment on the GPU (include/tsdf_amd.h, "field alignment"; tsdf_amd/csrc/align.hip) against its CPU reference
(tests/align_ref.py): the per-point rows and one step's sums bit for bit, the chain against the float64 reference chain within a
tolerance the test computes from two orders of the same sums, what the calls leave alone, every refusal, and depth_to_points.

The grid is that of tests/test_field_query.py: 37 x 34 x 45 voxels with three different edges and an offset, three fused frames."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import align_ref as R
from tests import field_ref
from tests.field_cases import DIV_EDGES, division_case, division_volume
from tests.helpers import assert_same_floats
from tsdf_amd import _capi

pytestmark = pytest.mark.gpu
F = np.float32
COUNTS = (1, 255, 256, 257, 65536, 65537)


def make_volume(s, storage=None):
    vol = tsdf_amd.TSDFVolume(R.SIZE, R.PHYS)
    vol.offset(*R.OFFSET)
    for d, cam in s.frames:
        vol.integrate(d, R.W, R.H, cam)
    if storage:
        vol.set_weight_storage(storage)
    return vol


def row_points(s):
    """Every kind of point the rows can go wrong on."""
    dims, vs, offset = s.geom
    rng = np.random.RandomState(R.SEED & 0x7FFFFFFF)
    mx = np.array(field_ref.bounds(dims, vs), F)
    parts = {}
    parts["random"] = (offset + (rng.uniform(-0.05, 1.05, (1500, 3)) * mx)).astype(F)
    parts["mesh"] = s.mesh[::2]                                 # front and back face: the back face's neighbourhood is partly unobserved
    jitter = rng.uniform(-1, 1, (len(s.mesh), 3)) * s.gate * 1.2
    parts["band"] = (s.mesh + jitter).astype(F)[1::2]           # around the surface, on both sides of the gate
    face = []
    for a in range(3):
        for far in (False, True):
            q = (vs * F(1.5) + rng.uniform(0, 1, (30, 3)) * (mx - vs * F(3))).astype(F)
            t = rng.uniform(0.02, 0.98, 30).astype(F) * vs[a]
            q[:, a] = (mx[a] - vs[a]) + t if far else t
            face.append((q + offset).astype(F))
    parts["faces"] = np.concatenate(face)
    inside = (offset + mx * F(0.5)).astype(F)
    special = []
    for a in range(3):
        for v in (F(np.nan), F(np.inf), F(-np.inf), F(-0.0), F(3.0e38)):
            p = inside.copy()
            p[a] = v
            special.append(p)
    parts["special"] = np.array(special, F)
    out, where, at = [], {}, 0
    for name, p in parts.items():
        out.append(p)
        where[name] = slice(at, at + len(p))
        at += len(p)
    return np.concatenate(out).astype(F), where


def sum_points(s):
    """65 537 points: the observed surface's vertices, repeated with a jitter inside the gate, and a tenth anywhere in the box."""
    rng = np.random.RandomState(77)
    n = max(COUNTS)
    base = s.points[rng.randint(0, len(s.points), n)]
    p = (base + rng.uniform(-1, 1, (n, 3)) * s.gate * 0.6).astype(F)
    dims, vs, offset = s.geom
    mx = np.array(field_ref.bounds(dims, vs), F)
    anywhere = rng.uniform(size=n) < 0.1
    p[anywhere] = (offset + rng.uniform(-0.05, 1.05, (int(anywhere.sum()), 3)) * mx).astype(F)
    return p


@pytest.fixture(scope="module")
def scene(oracle):
    """The reference's scene, its GPU twin and the reference's answers -- computed once, never changed."""
    s = R.fused_scene(oracle)
    s.gv = make_volume(s)
    assert s.gv.weight_storage() == (8, False)
    assert_same_floats(s.gv.get_distance_data(), s.dist, "fused distances")
    assert_same_floats(s.gv.get_weight_data(), s.weight, "fused weights")
    assert_same_floats(s.gv.extract_surface(), s.mesh, "mesh")
    s.aligner = tsdf_amd.FieldAligner()
    s.row_points, s.where = row_points(s)
    s.poses = [np.eye(4), np.array(s.T0)]
    s.ref_rows = [R.rows_at(oracle, s.geom, s.dist, s.weight, s.row_points, R.to_pivot(T, s.geom), s.gate) for T in s.poses]
    s.sum_points = sum_points(s)
    s.sum_rows, s.sum_inl = R.rows_at(oracle, s.geom, s.dist, s.weight, s.sum_points, R.to_pivot(s.T0, s.geom), s.gate)
    s.sum_products = R.products(s.sum_rows, s.sum_inl)
    for a in (s.row_points, s.sum_points, s.sum_rows, s.sum_inl, s.sum_products):
        a.setflags(write=False)
    yield s
    s.aligner.close()
    s.gv.close()


def test_the_parity_is_not_vacuous(scene, oracle):
    s = scene
    for i, (rows, inl) in enumerate(s.ref_rows):
        assert inl[s.where["random"]].sum() >= 50 and (~inl[s.where["random"]]).sum() >= 500
        assert inl[s.where["mesh"]].sum() >= 500 and (~inl[s.where["mesh"]]).sum() >= 500     # observed front, half-observed back face
        assert inl[s.where["band"]].sum() >= 300 and (~inl[s.where["band"]]).sum() >= 300
        assert not inl[s.where["special"]][[0, 1, 2, 4, 5, 6, 7, 9, 10, 11, 12, 14]].any()
        if i == 0:      # (at the identity the face points stay within a voxel of their face: a distance, no gradient)
            assert not inl[s.where["faces"]].any()
        assert np.isnan(rows[~inl]).all() and np.isfinite(rows[inl]).all()
    # partly unobserved neighbourhoods: valid everywhere, a finite distance inside the gate, and still outliers by a weight alone
    d, g, w = field_ref.sample(oracle, s.geom, s.dist, s.weight, s.row_points[s.where["mesh"]][:400])
    own = ~s.ref_rows[0][1][s.where["mesh"]][:400] & (w > 0) & np.isfinite(g).all(axis=1) & (np.abs(d) < F(s.gate))
    assert own.sum() >= 20
    assert s.sum_inl.sum() * 2 >= len(s.sum_inl) and (~s.sum_inl).sum() >= 3000


def test_rows_match_the_reference_bit_for_bit(scene):
    s = scene
    for T, (ref, inl) in zip(s.poses, s.ref_rows):
        A, b, res, count, rows = s.aligner.step(s.gv, s.row_points, T, s.gate, rows=True)
        assert_same_floats(rows, ref, "rows")
        assert count == inl.sum()


@pytest.mark.parametrize("edge, proved", zip(DIV_EDGES, (0, 1)))
def test_both_instances_of_the_division_give_the_reference_rows(oracle, edge, proved):
    """The scene above has one geometry, so one of the kernel's two division instances; tests/test_field_query.py's two uploaded
    volumes pick one each.  Their query points, through a pose 0.4 voxels and 1.5 degrees off, gate one voxel."""
    c = division_case(oracle, edge)
    T = R.perturbation(0.4 * edge, 1.5, R.pivot(c.geom)[1], 21)
    gate = 1.0 * edge           # (inside the truncation of 1.9 voxels: the gate decides, not the clamp)
    ref, inl = R.rows_at(oracle, c.geom, c.dist, c.weight, c.points, R.to_pivot(T, c.geom), gate)
    assert inl.sum() >= 50 and (~inl).sum() >= 50
    # outliers that pass the seven validity tests and leave later: at the weights (inliers once every voxel counts as observed), and
    # -- every weight > 0 -- at the gate (inliers once it is infinite)
    Tc = R.to_pivot(T, c.geom)
    _, seen = R.rows_at(oracle, c.geom, c.dist, c.weight, c.points, Tc, np.inf)
    _, anywhere = R.rows_at(oracle, c.geom, c.dist, np.ones_like(c.weight), c.points, Tc, np.inf)
    assert (anywhere & ~seen).sum() >= 50 and (seen & ~inl).sum() >= 50
    vol = division_volume(c, proved)
    aligner = tsdf_amd.FieldAligner()
    A, b, res, count, rows = aligner.step(vol, c.points, T, gate, rows=True)
    assert_same_floats(rows, ref, "rows")
    assert count == inl.sum()
    aligner.close()
    vol.close()


def test_every_weight_storage_gives_the_same_rows(scene, oracle):
    s = scene
    T, (ref, inl) = s.poses[1], s.ref_rows[1]
    first = s.aligner.step(s.gv, s.row_points, T, s.gate)
    vol = make_volume(s)
    for step, want in ((16, 16), (32, 32)):
        vol.set_weight_storage(step)
        before = vol.weight_storage()
        assert before[0] == want
        A, b, res, count, rows = s.aligner.step(vol, s.row_points, T, s.gate, rows=True)
        assert vol.weight_storage() == before, "the step changed the storage"
        assert_same_floats(rows, ref, "rows at %d bits" % want)
        assert_same_floats(A, first[0], "A at %d bits" % want)
        assert_same_floats(b, first[1], "b at %d bits" % want)
        assert (res, count) == first[2:4]
    vol.close()
    # uploaded distances and weights that are no counts: fractions count as observed, zero and NaN do not
    vol = tsdf_amd.TSDFVolume(R.SIZE, R.PHYS)
    vol.offset(*R.OFFSET)
    rng = np.random.RandomState(5)
    weights = np.array(s.weight)
    seen = np.flatnonzero(weights > 0)
    weights[seen[::3]] = rng.uniform(0.01, 0.9, len(seen[::3])).astype(F)
    weights[seen[1::17]] = F(np.nan)
    weights[seen[2::19]] = F(0)
    dist = (np.array(s.dist) * F(0.75)).astype(F)
    vol.set_distance_data(dist)
    vol.set_weight_data(weights)
    ref2, inl2 = R.rows_at(oracle, s.geom, dist, weights, s.row_points, R.to_pivot(T, s.geom), s.gate)
    assert inl2.sum() >= 300 and (inl & ~inl2).sum() >= 100
    rows = s.aligner.step(vol, s.row_points, T, s.gate, rows=True)[4]
    assert_same_floats(rows, ref2, "rows over uploaded fractional weights")
    vol.close()


@pytest.mark.parametrize("n", COUNTS)
def test_sums_match_the_emulated_order_bit_for_bit(scene, n):
    s = scene
    assert R.blocks_for(n) == {1: 1, 255: 1, 256: 1, 257: 2, 65536: 256, 65537: 256}[n]
    A0, b0, res0, count0 = R.system(R.sums_kernel_order(s.sum_products[:n]))
    A, b, res, count = s.aligner.step(s.gv, s.sum_points[:n], s.T0, s.gate)
    print("n = %d: inliers %g (reference %g), residual %r (reference %r)" % (n, count, count0, res, res0))
    assert count == count0 == s.sum_inl[:n].sum()
    assert_same_floats(A, A0, "A")
    assert_same_floats(b, b0, "b")
    assert_same_floats([res], [res0], "residual")
    assert np.array_equal(A, A.T)
    again = s.aligner.step(s.gv, s.sum_points[:n], s.T0, s.gate)
    assert_same_floats(again[0], A, "A, second call")
    assert_same_floats(again[1], b, "b, second call")
    assert again[2:] == (res, count)
    # with the rows asked for: the same sums
    with_rows = s.aligner.step(s.gv, s.sum_points[:n], s.T0, s.gate, rows=True)
    assert_same_floats(with_rows[0], A, "A beside rows")
    assert_same_floats(with_rows[4], s.sum_rows[:n], "rows")


def test_an_all_outlier_set_gives_zeros_and_leaves_the_pose(scene):
    s = scene
    rng = np.random.RandomState(3)
    far = (np.array(R.OFFSET) + np.array(R.PHYS) * 2 + rng.uniform(0, 500, (700, 3))).astype(F)
    far[::7] = np.nan
    A, b, res, count = s.aligner.step(s.gv, far, s.T0, s.gate)
    assert count == 0 and res == 0 and not A.any() and not b.any()
    T, res, count = s.aligner.run(s.gv, [(far, 3)], s.T0, s.gate)
    assert count == 0 and res == 0
    assert np.array_equal(T, s.T0)
    # no points, no iterations, no stages: nothing to do, the pose as given
    for stages in ([], [(far[:0], 4)], [(s.points, 0)]):
        T, res, count = s.aligner.run(s.gv, stages, s.T0, s.gate)
        assert np.array_equal(T, s.T0) and count == 0
    A, b, res, count = s.aligner.step(s.gv, far[:0], s.T0, s.gate)
    assert count == 0 and not A.any()


def test_the_chain_follows_the_float64_reference(scene, oracle):
    """Start 15 mm / 1.5 degrees off.  Tolerance: 8 x the distance between the reference chain summed in float64 and the same chain
    summed in fp32 in ascending point order -- the kernel's order is a third order of the same sums."""
    s = scene
    stages = [(s.points, 10)]
    ref, norms, counts = R.chain(oracle, s, stages, s.T0, s.gate, order="f64")
    asc, _, _ = R.chain(oracle, s, stages, s.T0, s.gate, order="ascending")
    tol = 8 * R.pose_distance(ref, asc)
    T, res, count = s.aligner.run(s.gv, stages, s.T0, s.gate)
    err = R.pose_distance(T, ref)
    print("chain: |GPU - float64 reference| = %.3e, tolerance 8 x %.3e = %.3e, inliers %g of %d, start error %.3f -> %.3e"
          % (err, tol / 8, tol, count, len(s.points), R.pose_distance(s.T0, np.eye(4)), R.pose_distance(T, np.eye(4))))
    assert tol > 0
    assert err <= tol
    assert count * 2 >= len(s.points)
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(T[:3, :3]) - 1) < 1e-12
    assert np.array_equal(T[3], [0, 0, 0, 1])
    # the same bits across two runs in one process
    T2, res2, count2 = s.aligner.run(s.gv, stages, s.T0, s.gate)
    assert np.array_equal(T2, T) and (res2, count2) == (res, count)
    other = tsdf_amd.FieldAligner()
    T3, res3, count3 = other.run(s.gv, stages, s.T0, s.gate)
    other.close()
    assert np.array_equal(T3, T) and (res3, count3) == (res, count)
    # a two-stage run is two one-stage runs chained by hand (different point sets: different grids in one chain)
    coarse = s.points[::4]
    two = s.aligner.run(s.gv, [(coarse, 4), (s.points, 6)], s.T0, s.gate)
    mid = s.aligner.run(s.gv, [(coarse, 4)], s.T0, s.gate)
    end = s.aligner.run(s.gv, [(s.points, 6)], mid[0], s.gate)
    # (by hand the pose passes through the host's shift to the world frame and back, in double: 1e-9 mm, not bits)
    assert np.abs(two[0] - end[0]).max() < 1e-9 and two[2] == end[2]
    # the convenience over a one-stage run
    T4, res4, count4 = s.gv.align_points(s.points, s.T0, iterations=10)
    assert np.array_equal(T4, T) and (res4, count4) == (res, count)


def test_the_calls_leave_the_volume_alone(scene, oracle):
    s = scene
    from tests.test_field_query import CAST_H, CAST_W, cast_camera
    cam = cast_camera(oracle, s.frames[1][1])
    caster = tsdf_amd.GPURaycaster(CAST_W, CAST_H)
    v0, n0 = caster.raycast(s.gv, cam)
    before = (s.gv.get_distance_data(), s.gv.get_weight_data()) + s.gv.occupancy_data() + (s.gv.weight_storage(), s.gv.occupancy())
    s.aligner.step(s.gv, s.row_points, s.T0, s.gate, rows=True)
    s.aligner.run(s.gv, [(s.points[::4], 2), (s.points, 3)], s.T0, s.gate)
    after = (s.gv.get_distance_data(), s.gv.get_weight_data()) + s.gv.occupancy_data() + (s.gv.weight_storage(), s.gv.occupancy())
    assert_same_floats(after[0], before[0], "distances after the calls")
    assert_same_floats(after[1], before[1], "weights after the calls")
    for a, b, name in zip(after[2:5], before[2:5], ("fine", "cell", "reach")):
        assert np.array_equal(a, b), name
    assert after[5:] == before[5:]
    v1, n1 = caster.raycast(s.gv, cam)
    assert_same_floats(v1, v0, "vertices after the calls")
    assert_same_floats(n1, n0, "normals after the calls")


def test_refusals(scene):
    s = scene
    lib = _capi.lib
    slab = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3, slab=(0, 8))
    pts = np.zeros((4, 3), F)
    guard = np.full(36 + 6 + 2, 7.0, F)
    T = np.ascontiguousarray(np.eye(4).T.reshape(-1))
    stage = (_capi.AlignStage * 9)()
    dp = C.c_void_p()
    _capi.check(lib.tsdf_device_alloc(4096, C.byref(dp)))
    for st in stage:
        st.device_points, st.n, st.iterations = dp.value, 4, 1
    res, inl = C.c_float(7.0), C.c_float(7.0)
    h, v = s.aligner._h, s.gv._h

    def step(a=h, vol=v, points=dp, pose=T, gate=50.0, A=guard[:36], b=guard[36:42], ri=guard[42:]):
        ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
        return lib.tsdf_aligner_step(a, vol, 4, points, ptr(pose), gate, ptr(A), ptr(b), ptr(ri), None)

    def run(a=h, vol=v, n=1, stages=stage, pose=T, gate=50.0):
        return lib.tsdf_aligner_run(a, vol, n, stages, gate, pose.ctypes.data if pose is not None else None, C.byref(res), C.byref(inl))

    bad = T.copy()
    try:
        assert step() == _capi.TSDF_OK
        guard[:] = 7.0
        refused = []
        refused += [step(a=None), step(vol=None), step(points=None), step(pose=None), step(A=None), step(b=None), step(ri=None)]
        refused += [run(a=None), run(vol=None), run(pose=None), run(stages=None), lib.tsdf_aligner_create(None)]
        refused += [step(vol=slab._h), run(vol=slab._h)]
        for i, value in ((0, np.nan), (6, np.inf), (13, -np.inf)):
            bad[:] = T
            bad[i] = value
            refused += [step(pose=bad), run(pose=bad)]
            assert np.array_equal(bad[np.arange(16) != i], T[np.arange(16) != i])
        for gate in (0.0, -1.0, float("nan")):
            refused += [step(gate=gate), run(gate=gate)]
        refused += [run(n=9)]
        null_stage = (_capi.AlignStage * 1)()
        null_stage[0].n, null_stage[0].iterations = 4, 1
        refused += [run(stages=null_stage)]
        depth = np.zeros(16, np.uint16)
        kinv = np.eye(3, dtype=F).reshape(-1)
        d2p = lambda d=dp, k=kinv.ctypes.data, out=dp, step=1: lib.tsdf_depth_to_points_device(4, 4, d, k, step, 1e9, out, None)
        refused += [d2p(step=0), d2p(d=None), d2p(k=None), d2p(out=None)]
        assert all(rc == _capi.TSDF_ERR_INVALID for rc in refused), refused
        assert (guard == 7.0).all() and res.value == 7.0 and inl.value == 7.0, "a refused call wrote a result"
        assert np.array_equal(T, np.eye(4).reshape(-1))
        assert _capi.last_error()
        # a non-finite bottom row is not looked at; 8 stages are allowed
        bad[:] = T
        bad[3] = np.nan
        assert step(pose=bad) == _capi.TSDF_OK and run(n=8) == _capi.TSDF_OK
        # the Python surface raises
        with pytest.raises(ValueError):
            s.aligner.run(slab, [(pts, 1)])
        with pytest.raises(ValueError):
            s.gv.align_points(pts, gate=0.0)
        with pytest.raises(ValueError):
            s.aligner.run(s.gv, [(pts, 1)] * 9)
        with pytest.raises(ValueError):
            tsdf_amd.depth_to_points(depth, 4, 4, kinv, step=0)
        # a second device: refused as soon as the volume lives elsewhere
        import torch
        if torch.cuda.device_count() > 1:
            n = C.c_int()
            _capi.check(lib.tsdf_get_device(C.byref(n)))
            _capi.check(lib.tsdf_set_device(1 - n.value if n.value < 2 else 0))
            try:
                elsewhere = tsdf_amd.FieldAligner()
                assert step(a=elsewhere._h) == _capi.TSDF_ERR_INVALID and run(a=elsewhere._h) == _capi.TSDF_ERR_INVALID
                elsewhere.close()
            finally:
                _capi.check(lib.tsdf_set_device(n.value))
    finally:
        lib.tsdf_device_free(dp)
        slab.close()


@pytest.mark.parametrize("step", [1, 2, 4])
def test_depth_to_points_matches_the_oracle(oracle, step):
    w, h = 37, 29
    rng = np.random.RandomState(11)
    depth = rng.randint(400, 6000, (h, w)).astype(np.uint16)
    depth[rng.uniform(size=(h, w)) < 0.15] = 0
    depth[0, 0], depth[h - 1, w - 1], depth[4, 8], depth[8, 4] = 0, 65535, 4000, 4001
    cutoff = 4000.0
    k, kinv = oracle.camera_k(591.1 / 16, 590.1 / 16, 331.0 / 16, 234.6 / 16)
    got = tsdf_amd.depth_to_points(depth, w, h, kinv, step=step, depth_cutoff=cutoff)
    ys, xs = np.arange(0, h, step), np.arange(0, w, step)
    assert got.shape == (-(-h // step), -(-w // step), 3) == (len(ys), len(xs), 3)
    px = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)          # (x, y) pairs, row-major over the output
    d = depth[px[:, 1], px[:, 0]]
    ref = oracle.pixel_to_camera_n(px, d.astype(F), kinv)
    gone = (d == 0) | (d > cutoff)
    ref[gone] = np.nan
    assert gone.sum() >= 10 and (~gone).sum() >= 30
    assert_same_floats(got, ref, "points at step %d" % step)
    assert np.isnan(got.reshape(-1, 3)[gone]).all()
    if step == 4:
        assert not np.isnan(got[1, 2]).any() and np.isnan(got[2, 1]).all()       # depth == cutoff stays, cutoff + 1 goes
        # no cutoff: only the zeros go
        every = tsdf_amd.depth_to_points(depth, w, h, kinv, step=step)
        assert np.array_equal(np.isnan(every[..., 0]).reshape(-1), d == 0)
