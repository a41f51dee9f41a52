"""Field queries on the GPU (include/tsdf_amd.h, "field queries"; tsdf_amd/csrc/field.hip) against their CPU reference
(tests/field_ref.py: the oracle's trilinear sample for every S, numpy float32 for the rest), bit for bit.

The grid is the smallest on which the kernel can go wrong: 37 x 34 x 45 voxels (odd X; Z a multiple of neither 4 nor 2, so the last
z-packed weight group is partial in both packed storages), 2900 x 3100 x 3300 mm (three different voxel edges), offset
(-150, 40, 275) set before the first integrate, three fused frames."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import field_ref
from tests.field_cases import DIV_EDGES, N_RANDOM, SEED, build_points, division_case, division_volume
from tests.helpers import H, W, Cam, assert_same_floats, sphere_tsdf
from tsdf_amd import _capi, synth

F = np.float32
SIZE, PHYS, OFFSET = (37, 34, 45), (2900.0, 3100.0, 3300.0), (-150.0, 40.0, 275.0)
FRAMES, PERIOD = (0, 9, 18), 40
CAST_W, CAST_H = 80, 60
GUARD = 0x7FC0BEEF


def frames():
    return [synth.depth_frame(i, PERIOD, seed=SEED) for i in FRAMES]


def cast_camera(O, cam):
    """The frame's pose with the default intrinsics scaled to an 80 x 60 image."""
    k, kinv = O.camera_k(591.1 / 8, 590.1 / 8, 331.0 / 8, 234.6 / 8)
    return Cam(cam.pose(), cam.inverse_pose(), k, kinv)


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(oracle):
    """The fused volume, its oracle twin, the points and the reference's answers -- computed once, never changed."""
    s = Scene()
    s.gv = tsdf_amd.TSDFVolume(SIZE, PHYS)
    s.ov = oracle.Volume(SIZE, PHYS)
    s.gv.offset(*OFFSET)
    s.ov.offset(*OFFSET)
    fr = frames()
    for d, cam in fr:
        s.gv.integrate(d, W, H, cam)
        s.ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    assert s.gv.weight_storage() == (8, False)
    assert_same_floats(s.gv.get_distance_data(), s.ov.dist, "fused distances")
    assert_same_floats(s.gv.get_weight_data(), s.ov.weight, "fused weights")
    s.cam = cast_camera(oracle, fr[1][1])
    s.mesh = s.gv.extract_surface()
    s.cast_v, _ = tsdf_amd.GPURaycaster(CAST_W, CAST_H).raycast(s.gv, s.cam)
    hits = s.cast_v[~np.isnan(s.cast_v[:, 0])]
    s.geom = field_ref.geometry(s.gv)
    s.points, s.where = build_points(s.geom, s.mesh, hits)
    s.ref_d, s.ref_g, s.ref_w = field_ref.sample(oracle, s.geom, s.ov.dist, s.ov.weight, s.points)
    s.ref_u = field_ref.unit_rows(s.ref_g)
    for a in (s.points, s.ref_d, s.ref_g, s.ref_u, s.ref_w, s.ov.dist, s.ov.weight):
        a.setflags(write=False)
    yield s
    s.gv.close()


def bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def device_query(vol, points, want_d=True, want_g=True, want_w=True, unit=False):
    """sample_field_device with all three output buffers filled with a guard word and only the wanted ones handed over:
    -> (distance, gradient, weight) as downloaded, guards and all."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(p)
    outs = [np.full(n, GUARD, np.uint32), np.full(3 * n, GUARD, np.uint32), np.full(n, GUARD, np.uint32)]
    ptrs = [C.c_void_p() for _ in range(4)]
    try:
        for ptr, a in zip(ptrs, [p] + outs):
            _capi.check(_capi.lib.tsdf_device_alloc(a.nbytes, C.byref(ptr)))
            _capi.check(_capi.lib.tsdf_device_upload(ptr, a.ctypes.data, a.nbytes))
        vol.sample_field_device(n, ptrs[0].value, ptrs[1].value if want_d else None, ptrs[2].value if want_g else None,
                                ptrs[3].value if want_w else None, unit_gradient=unit)
        vol.synchronize()
        for ptr, a in zip(ptrs[1:], outs):
            _capi.check(_capi.lib.tsdf_device_download(a.ctypes.data, ptr, a.nbytes))
    finally:
        for ptr in ptrs:
            if ptr.value:
                _capi.lib.tsdf_device_free(ptr)
    return outs[0].view(F), outs[1].view(F).reshape(-1, 3), outs[2].view(F)


@pytest.mark.gpu
def test_the_parity_is_not_vacuous(scene):
    """The reference alone, on these inputs: enough points with a gradient, every kind of point present."""
    s = scene
    has_g = ~np.isnan(s.ref_g).any(axis=1)
    assert has_g[s.where["random"]].sum() * 4 >= N_RANDOM
    assert has_g[s.where["mesh"]].sum() >= 100
    assert has_g[s.where["hits"]].sum() >= 100
    assert np.isnan(s.ref_d[s.where["random"]]).sum() >= 50            # some random points are outside
    face_d, face_g = s.ref_d[s.where["faces"]], s.ref_g[s.where["faces"]]
    assert not np.isnan(face_d).any() and np.isnan(face_g).all()       # near a face: a distance, no gradient
    assert np.isnan(s.ref_d[s.where["special"]]).sum() >= 12           # the bound where it could be hit exactly, NaN, +-inf
    assert (s.ref_w > 0).sum() >= 500 and (s.ref_w[~np.isnan(s.ref_d)] == 0).sum() >= 100   # observed and unobserved voxels
    q = s.points[s.where["lattice"]] - s.geom[2]
    k = q / s.geom[1]
    assert (k == np.round(k)).sum() >= 50 and (k * 2 == np.round(k * 2)).sum() >= 150       # exact faces and centres were reached


@pytest.mark.gpu
def test_distance_gradient_and_weight_match_the_reference_bit_for_bit(scene):
    s = scene
    d, g, w = s.gv.sample_field(s.points)
    assert_same_floats(d, s.ref_d, "distance")
    assert_same_floats(g, s.ref_g, "gradient")
    assert_same_floats(w, s.ref_w, "weight")
    d2, u, w2 = s.gv.sample_field(s.points, unit_gradient=True)
    assert_same_floats(u, s.ref_u, "unit gradient")
    assert_same_floats(d2, s.ref_d, "distance (unit call)")
    assert_same_floats(w2, s.ref_w, "weight (unit call)")
    lens = np.linalg.norm(u[~np.isnan(u).any(axis=1)].astype(np.float64), axis=1)
    assert len(lens) >= 100 and np.abs(lens - 1.0).max() < 1e-6
    # no points: empty arrays, nothing launched
    e = s.gv.sample_field(np.empty((0, 3), F))
    assert [len(a) for a in e] == [0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("edge, proved", zip(DIV_EDGES, (0, 1)))
def test_both_instances_of_the_division_match_the_reference(oracle, edge, proved):
    c = division_case(oracle, edge)
    vol = division_volume(c, proved)
    d, g, w = vol.sample_field(c.points)
    assert_same_floats(d, c.ref_d, "distance")
    assert_same_floats(g, c.ref_g, "gradient")
    assert_same_floats(w, c.ref_w, "weight")
    _, u, _ = vol.sample_field(c.points, weight=False, unit_gradient=True)
    assert_same_floats(u, c.ref_u, "unit gradient")
    # the instances of one output each
    for i, (ref, name) in enumerate(((c.ref_d, "distance"), (c.ref_u, "unit gradient"), (c.ref_w, "weight"))):
        assert_same_floats(device_query(vol, c.points, *(j == i for j in range(3)), unit=True)[i], ref, "%s alone" % name)
    vol.close()


@pytest.mark.gpu
def test_every_weight_storage_gives_the_same_answers(scene, oracle):
    s = scene
    vol = tsdf_amd.TSDFVolume(SIZE, PHYS)
    vol.offset(*OFFSET)
    for d, cam in frames():
        vol.integrate(d, W, H, cam)
    for step, want in ((None, 8), (16, 16), (32, 32)):
        if step:
            vol.set_weight_storage(step)
        before = vol.weight_storage()
        assert before[0] == want
        d, g, w = vol.sample_field(s.points)
        assert vol.weight_storage() == before, "the query changed the storage"
        assert_same_floats(d, s.ref_d, "distance at %d bits" % want)
        assert_same_floats(g, s.ref_g, "gradient at %d bits" % want)
        assert_same_floats(w, s.ref_w, "weight at %d bits" % want)
    vol.close()
    # uploaded weights that are no counts come back as stored
    vol = tsdf_amd.TSDFVolume(SIZE, PHYS)
    vol.offset(*OFFSET)
    vol.set_distance_data(s.ov.dist)
    weights = s.ov.weight.copy()
    voxels = [(3, 5, 7), (36, 33, 44), (20, 0, 43)]
    for (x, y, z), value in zip(voxels, (0.5, 300.25, np.nan)):
        weights[x + SIZE[0] * (y + SIZE[1] * z)] = value
    vol.set_weight_data(weights)
    before = vol.weight_storage()
    dims, vs, offset = s.geom
    centres = np.array([[F(F(F(c) + F(0.5)) * vs[a]) + offset[a] for a, c in enumerate(v)] for v in voxels], F)
    pts = np.concatenate([centres, s.points[:400]])
    rd, _, rw = field_ref.sample(oracle, s.geom, s.ov.dist, weights, pts, gradient=False)
    d, _, w = vol.sample_field(pts, gradient=False)
    assert vol.weight_storage() == before
    assert_same_floats(w, rw, "uploaded weights")
    assert_same_floats(d, rd, "distance beside uploaded weights")
    assert w[0] == F(0.5) and w[1] == F(300.25) and np.isnan(w[2])
    vol.close()


@pytest.mark.gpu
def test_output_subsets_equal_the_full_call_and_write_nothing_else(scene):
    s = scene
    d, g, w = device_query(s.gv, s.points)
    assert_same_floats(d, s.ref_d, "device distance")
    assert_same_floats(g, s.ref_g, "device gradient")
    assert_same_floats(w, s.ref_w, "device weight")
    for unit in (False, True):
        for want in ((True, False, False), (False, True, False), (False, False, True)):
            got = device_query(s.gv, s.points, *want, unit=unit)
            for asked, out, full, name in zip(want, got, (d, s.ref_u if unit else g, w), ("distance", "gradient", "weight")):
                if asked:
                    assert_same_floats(out, full, "%s alone" % name)
                else:
                    assert (bits(out) == GUARD).all(), "%s was written though not asked for" % name


@pytest.mark.gpu
def test_queries_leave_the_volume_alone(scene):
    s = scene
    caster = tsdf_amd.GPURaycaster(CAST_W, CAST_H)
    v0, n0 = caster.raycast(s.gv, s.cam)
    before = (s.gv.get_distance_data(), s.gv.get_weight_data()) + s.gv.occupancy_data() + (s.gv.weight_storage(),)
    s.gv.sample_field(s.points)
    s.gv.sample_field(s.points, gradient=False, weight=False)
    device_query(s.gv, s.points, unit=True)
    caster.raycast_gradient_normals(s.gv, s.cam)
    after = (s.gv.get_distance_data(), s.gv.get_weight_data()) + s.gv.occupancy_data() + (s.gv.weight_storage(),)
    assert_same_floats(after[0], before[0], "distances after the queries")
    assert_same_floats(after[1], before[1], "weights after the queries")
    for a, b, name in zip(after[2:5], before[2:5], ("fine", "cell", "reach")):
        assert np.array_equal(a, b), name
    assert after[5] == before[5]
    v1, n1 = caster.raycast(s.gv, s.cam)
    assert_same_floats(v1, v0, "vertices after the queries")
    assert_same_floats(n1, n0, "normals after the queries")


@pytest.mark.gpu
def test_raycast_gradient_normals(scene):
    s = scene
    caster = tsdf_amd.GPURaycaster(CAST_W, CAST_H)
    v, n = caster.raycast_gradient_normals(s.gv, s.cam)
    assert_same_floats(v, s.cast_v, "vertices of the gradient-normal cast")
    _, u, _ = s.gv.sample_field(v, weight=False, unit_gradient=True)
    assert_same_floats(n, u, "gradient normals")
    miss = np.isnan(v[:, 0])
    assert miss.sum() >= 100 and (~miss).sum() >= 100
    assert np.isnan(n[miss]).all()
    # where the cross-product normals of a hit are NaN (silhouettes, beside misses) the field still has an answer
    _, cross = caster.raycast(s.gv, s.cam)
    filled = ~miss & np.isnan(cross).any(axis=1) & ~np.isnan(n).any(axis=1)
    assert filled.sum() >= 10


@pytest.mark.gpu
def test_sphere_gradients_are_radial(oracle):
    """An analytic field: a sphere's distance clamped to +-trunc on a 48^3 grid (no offset).  The unit gradient at every mesh vertex
    against the radial direction, and -- because this volume has no offset -- the points whose q can be given exactly."""
    n, phys, radius = 48, 3000.0, 900.0
    dist = sphere_tsdf(oracle, n, phys, radius)
    vol = tsdf_amd.TSDFVolume((n,) * 3, (phys,) * 3)
    vol.set_distance_data(dist)
    geom = field_ref.geometry(vol)
    weight = np.zeros(n ** 3, F)
    mesh = vol.extract_surface()
    assert len(mesh) >= 1000
    mesh = mesh[::7]                       # (every seventh vertex: a reference of seven samples a point on the CPU)
    _, ref_u, _ = field_ref.sample(oracle, geom, dist, weight, mesh, unit_gradient=True)
    _, u, _ = vol.sample_field(mesh, weight=False, unit_gradient=True)
    assert_same_floats(u, ref_u, "sphere unit gradients")

    def min_cosine(g):
        ok = ~np.isnan(g).any(axis=1)
        assert ok.sum() >= 500
        r = mesh[ok].astype(np.float64) - phys / 2
        r /= np.linalg.norm(r, axis=1)[:, None]
        return float((g[ok].astype(np.float64) * r).sum(axis=1).min())

    # the reference's minimum on this shape, computed on the CPU: 0.9999994509 over the 3331 vertices (radius 900 mm = 14.4 voxels)
    ref_min = min_cosine(ref_u)
    assert ref_min > 0.9
    assert min_cosine(u) >= ref_min - 1e-6
    # exact q: -0.0, the exact bound, exact faces and centres, the last float below the bound
    vs, mx = geom[1], np.array(field_ref.bounds(geom[0], geom[1]), F)
    mid = F(phys / 2)
    special = []
    for a in range(3):
        for v in (F(-0.0), F(0.0), mx[a], np.nextafter(mx[a], F(0)), F(F(17) * vs[a]), F(F(17.5) * vs[a]), vs[a], F(mx[a] - vs[a]),
                  np.nextafter(vs[a], F(0)), np.nextafter(F(mx[a] - vs[a]), F(np.inf))):
            p = np.array([mid, mid, mid], F)
            p[a] = v
            special.append(p)
    special = np.array(special, F)
    rd, rg, rw = field_ref.sample(oracle, geom, dist, weight, special)
    d, g, w = vol.sample_field(special)
    assert_same_floats(d, rd, "special distances")
    assert_same_floats(g, rg, "special gradients")
    assert_same_floats(w, rw, "special weights")
    assert np.isnan(rd).sum() == 3 and (~np.isnan(rg).any(axis=1)).sum() >= 9
    vol.close()


@pytest.mark.gpu
def test_refusals():
    lib = _capi.lib
    out = np.zeros(16, F)
    pts = np.zeros(9, F)
    slab = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3, slab=(0, 8))
    whole = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3)

    def refused(rc):
        assert rc == _capi.TSDF_ERR_INVALID
        assert len(_capi.last_error()) > 0

    refused(lib.tsdf_volume_sample_field(slab._h, 3, pts.ctypes.data, out.ctypes.data, None, None, 0))
    refused(lib.tsdf_volume_sample_field_device(slab._h, 0, None, None, None, None, 0, None))
    refused(lib.tsdf_volume_sample_field(whole._h, 3, pts.ctypes.data, None, None, None, 0))
    refused(lib.tsdf_volume_sample_field_device(whole._h, 3, None, None, None, None, 0, None))
    refused(lib.tsdf_volume_sample_field(whole._h, 3, None, out.ctypes.data, None, None, 0))
    dv = C.c_void_p()
    _capi.check(lib.tsdf_device_alloc(64, C.byref(dv)))
    try:
        refused(lib.tsdf_volume_sample_field_device(whole._h, 3, None, dv, None, None, 0, None))
        assert lib.tsdf_volume_sample_field_device(whole._h, 0, None, dv, None, None, 0, None) == _capi.TSDF_OK
    finally:
        lib.tsdf_device_free(dv)
    assert lib.tsdf_volume_sample_field(whole._h, 0, None, out.ctypes.data, None, None, 0) == _capi.TSDF_OK
    with pytest.raises(ValueError):
        slab.sample_field(pts.reshape(-1, 3))
    slab.close()
    whole.close()
