"""Ray queries on the GPU (include/tsdf_amd.h, "ray queries"; tsdf_amd/csrc/raycast_rays.hpp) against their CPU reference
(tests/ray_ref.py: the oracle's 1 x 1 image cast per ray, tests/field_ref.py for the normals), bit for bit, on the ray sets of
tests/ray_cases.py: the grid of tests/test_field_query.py, 37 x 34 x 45 voxels with three voxel edges, an offset and three fused
frames."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import ray_cases, ray_ref
from tests.helpers import H, W, assert_same_floats, sphere_tsdf
from tsdf_amd import _capi, api

F = np.float32
GUARD = 0x7FC0BEEF
SETS = ("pixels", "shuffled", "inside", "outside", "edges", "scaled", "decreed", "limited")


def fused_volume(frames):
    vol = tsdf_amd.TSDFVolume(ray_cases.SIZE, ray_cases.PHYS)
    vol.offset(*ray_cases.OFFSET)
    for d, cam in frames:
        vol.integrate(d, W, H, cam)
    return vol


@pytest.fixture(scope="module")
def scene(oracle):
    s = ray_cases.scene(oracle)
    gv = fused_volume(s.frames)
    assert_same_floats(gv.get_distance_data(), s.ov.dist, "fused distances")
    yield s, gv
    gv.close()


def bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def device_cast(vol, o, d, m=None, want_p=True, want_t=True, want_n=True):
    """cast_rays_device with all three output buffers filled with a guard word and only the wanted ones handed over:
    -> (points, t, normals) as downloaded, guards and all."""
    o = np.ascontiguousarray(o, F).reshape(-1, 3)
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    n = len(o)
    ins = [o, d] + ([np.ascontiguousarray(m, F)] if m is not None else [])
    outs = [np.full(3 * n, GUARD, np.uint32), np.full(n, GUARD, np.uint32), np.full(3 * n, GUARD, np.uint32)]
    ptrs = [C.c_void_p() for _ in ins + outs]
    try:
        for ptr, a in zip(ptrs, ins + outs):
            _capi.check(_capi.lib.tsdf_device_alloc(a.nbytes, C.byref(ptr)))
            _capi.check(_capi.lib.tsdf_device_upload(ptr, a.ctypes.data, a.nbytes))
        op = ptrs[len(ins):]
        vol.cast_rays_device(n, ptrs[0].value, ptrs[1].value, ptrs[2].value if m is not None else None,
                             op[0].value if want_p else None, op[1].value if want_t else None, op[2].value if want_n else None)
        vol.synchronize()
        for ptr, a in zip(op, outs):
            _capi.check(_capi.lib.tsdf_device_download(a.ctypes.data, ptr, a.nbytes))
    finally:
        for ptr in ptrs:
            if ptr.value:
                _capi.lib.tsdf_device_free(ptr)
    return outs[0].view(F).reshape(-1, 3), outs[1].view(F), outs[2].view(F).reshape(-1, 3)


def assert_cast(got, ref, what):
    for g, r, name in zip(got, ref, ("points", "t", "normals")):
        assert_same_floats(g, r, "%s: %s" % (what, name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_points_t_and_normals_match_the_reference_bit_for_bit(scene, name):
    s, gv = scene
    o, d, m = s.sets[name]
    assert_cast(gv.cast_rays(o, d, t_max=m, normals=True), s.ref[name], name)
    p, t = gv.cast_rays(o, d, t_max=m)                         # the instance without the gradient
    assert_cast((p, t), s.ref[name][:2], name + " without normals")


@pytest.mark.gpu
def test_pixel_rays_give_the_image_casts_vertex_map(scene):
    s, gv = scene
    o, d, _ = s.sets["pixels"]
    V, _ = tsdf_amd.GPURaycaster(ray_cases.CAST_W, ray_cases.CAST_H).raycast(gv, s.cam)
    p, _ = gv.cast_rays(o, d)
    assert_same_floats(p, V, "ray query against GPURaycaster.raycast")


@pytest.mark.gpu
def test_output_subsets_and_both_entry_points(scene):
    s, gv = scene
    o, d, m = s.sets["limited"]
    ref = s.ref["limited"]
    full = device_cast(gv, o, d, m)
    assert_cast(full, ref, "device entry point")
    assert_cast(gv.cast_rays(o, d, t_max=m, normals=True), full, "host against device entry point")
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        got = device_cast(gv, o, d, m, *want)
        for asked, out, r, name in zip(want, got, ref, ("points", "t", "normals")):
            if asked:
                assert_same_floats(out, r, "%s of %r" % (name, want))
            else:
                assert (bits(out) == GUARD).all(), "%s was written though not asked for" % name
    # no range limit handed over
    o3, d3, _ = s.sets["inside"]
    assert_cast(device_cast(gv, o3, d3), s.ref["inside"], "device entry point without t_max")


@pytest.mark.gpu
def test_no_rays_and_refusals(scene):
    s, gv = scene
    lib = _capi.lib
    p, t, n = gv.cast_rays(np.empty((0, 3), F), np.empty((0, 3), F), normals=True)
    assert p.shape == (0, 3) and t.shape == (0,) and n.shape == (0, 3)
    buf = np.zeros(12, F)
    q = buf.ctypes.data

    def refused(rc):
        assert rc == _capi.TSDF_ERR_INVALID
        assert len(_capi.last_error()) > 0

    refused(lib.tsdf_volume_cast_rays(gv._h, 3, q, q, None, None, None, None))
    refused(lib.tsdf_volume_cast_rays_device(gv._h, 3, q, q, None, None, None, None))
    refused(lib.tsdf_volume_cast_rays(gv._h, 0, None, None, None, None, None, None))
    refused(lib.tsdf_volume_cast_rays(gv._h, 1, None, q, None, q, None, None))
    refused(lib.tsdf_volume_cast_rays(gv._h, 1, q, None, None, q, None, None))
    refused(lib.tsdf_volume_cast_rays_device(gv._h, 1 << 62, q, q, None, q, None, None))
    refused(lib.tsdf_volume_cast_rays_device(gv._h, (1 << 64) - 1, q, q, None, q, None, None))      # (n + 255 would wrap)
    refused(lib.tsdf_volume_cast_rays_device(gv._h, 0x7FFFFFFF * 256 + 1, q, q, None, q, None, None))
    assert lib.tsdf_volume_cast_rays(gv._h, 0, None, None, None, q, None, None) == _capi.TSDF_OK
    assert lib.tsdf_volume_cast_rays_device(gv._h, 0, None, None, None, None, q, None) == _capi.TSDF_OK
    slab = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3, slab=(0, 8))
    refused(lib.tsdf_volume_cast_rays(slab._h, 1, q, q, None, q, None, None))
    refused(lib.tsdf_volume_cast_rays_device(slab._h, 0, None, None, None, q, None, None))
    with pytest.raises(ValueError):
        slab.cast_rays(buf[:3], buf[3:6])
    slab.close()


@pytest.mark.gpu
def test_a_cleared_volume_gives_all_misses(scene):
    s, _ = scene
    vol = tsdf_amd.TSDFVolume(ray_cases.SIZE, ray_cases.PHYS)
    vol.offset(*ray_cases.OFFSET)
    o, d, _ = s.sets["inside"]
    p, t, n = vol.cast_rays(o, d, normals=True)
    assert np.isnan(p).all() and np.isnan(t).all() and np.isnan(n).all()
    # ... and again after fused frames are cleared away
    depth, cam = s.frames[0]
    vol.integrate(depth, W, H, cam)
    assert (~np.isnan(vol.cast_rays(o, d)[1])).sum() >= 100
    vol.clear()
    assert np.isnan(vol.cast_rays(o, d)[1]).all()
    vol.close()


@pytest.mark.gpu
def test_an_uploaded_sphere_and_a_later_upload_are_seen(oracle):
    """set_distance_data hands the occupancy over as dirty: the query rebuilds it, and rebuilds it again for the next upload."""
    n, phys = 48, 3000.0
    vol = tsdf_amd.TSDFVolume((n,) * 3, (phys,) * 3)
    ov = oracle.Volume((n,) * 3, (phys,) * 3)
    rng = np.random.RandomState(0x5AFE)
    d = rng.normal(size=(333, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)
    o = (phys / 2 - d.astype(np.float64) * 1400.0).astype(F)          # on a sphere around the centre, looking at it and past it
    d[::3] = (d[::3] + rng.normal(scale=0.4, size=d[::3].shape)).astype(F)
    for radius in (900.0, 500.0):
        dist = sphere_tsdf(oracle, n, phys, radius)
        vol.set_distance_data(dist)
        ov.set_distance_data(dist)
        ref = ray_ref.cast(oracle, ov, o, d, normals=True)
        hits = ~np.isnan(ref[1])
        assert hits.sum() >= 100 and (~hits).sum() >= 20
        assert_cast(vol.cast_rays(o, d, normals=True), ref, "sphere of %g mm" % radius)
        # the hit points lie on the sphere to within a fraction of a voxel
        r = np.linalg.norm(ref[0][hits].astype(np.float64) - phys / 2, axis=1)
        assert np.abs(r - radius).max() < 0.5 * phys / n
    vol.close()


@pytest.mark.gpu
def test_query_integrate_query_sees_the_new_field(scene, oracle):
    s, _ = scene
    vol = fused_volume(s.frames[:2])
    ov = oracle.Volume(ray_cases.SIZE, ray_cases.PHYS)
    ov.offset(*ray_cases.OFFSET)
    for depth, cam in s.frames[:2]:
        ov.integrate(depth, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    o, d, _ = s.sets["inside"]
    o, d = o[:499], d[:499]
    before = ray_ref.cast(oracle, ov, o, d, normals=True)
    assert_cast(vol.cast_rays(o, d, normals=True), before, "two frames")
    depth, cam = s.frames[2]
    vol.integrate(depth, W, H, cam)
    after = tuple(a[:499] for a in s.ref["inside"])
    assert (bits(before[0]) != bits(after[0])).any()
    assert_cast(vol.cast_rays(o, d, normals=True), after, "three frames")
    vol.close()


@pytest.mark.gpu
def test_a_query_writes_nothing_of_the_volume_and_leaves_the_image_cast_alone(scene):
    s, _ = scene
    vol = fused_volume(s.frames)
    caster = tsdf_amd.GPURaycaster(ray_cases.CAST_W, ray_cases.CAST_H)
    v0, n0 = caster.raycast(vol, s.cam)
    kind0 = vol.last_raycast_cell_parallel()
    before = (vol.get_distance_data(), vol.get_weight_data(), vol.weight_storage())
    for name in ("pixels", "inside", "limited"):
        o, d, m = s.sets[name]
        vol.cast_rays(o, d, t_max=m, normals=True)
    assert vol.last_raycast_cell_parallel() == kind0
    after = (vol.get_distance_data(), vol.get_weight_data(), vol.weight_storage())
    assert_same_floats(after[0], before[0], "distances after the queries")
    assert_same_floats(after[1], before[1], "weights after the queries")
    assert after[2] == before[2]
    v1, n1 = caster.raycast(vol, s.cam)
    assert vol.last_raycast_cell_parallel() == kind0
    assert_same_floats(v1, v0, "vertices after the queries")
    assert_same_floats(n1, n0, "normals after the queries")
    # the same around a bulk upload, where the image cast counts the flagged bricks before it chooses its kernels
    twin = tsdf_amd.TSDFVolume(ray_cases.SIZE, ray_cases.PHYS)
    twin.offset(*ray_cases.OFFSET)
    for v, query in ((vol, True), (twin, False)):
        v.set_distance_data(s.ov.dist)
        if query:
            o, d, _ = s.sets["inside"]
            assert_same_floats(v.cast_rays(o, d)[0], s.ref["inside"][0], "query after an upload")
    va, _ = caster.raycast(vol, s.cam)
    vb, _ = caster.raycast(twin, s.cam)
    assert vol.last_raycast_cell_parallel() == twin.last_raycast_cell_parallel()
    assert_same_floats(va, vb, "image cast after upload + query against upload alone")
    assert_same_floats(va, v0, "image cast after the upload")
    vol.close()
    twin.close()


@pytest.mark.gpu
def test_normalise_and_visible(scene, oracle):
    s, gv = scene
    o, d, _ = s.sets["outside"]
    u = api.unit_directions(d)
    ref = ray_ref.cast(oracle, s.ov, o, u, normals=True)
    assert (~np.isnan(ref[1])).sum() >= 200
    assert_cast(gv.cast_rays(o, d, normals=True, normalise=True), ref, "normalise=True")
    # visible(a, b): a = the origins, b = points before, at and behind the first surface, and some decreed misses
    hit = np.flatnonzero(~np.isnan(ref[1]))[:150]
    miss = np.flatnonzero(np.isnan(ref[1]))[:50]
    a = np.concatenate([o[hit], o[hit], o[miss], o[:3]])
    scale = np.concatenate([ref[1][hit] * F(0.5), ref[1][hit] * F(1.5), np.full(len(miss), 4000, F)])
    b = np.concatenate([(a[:len(scale)] + u[np.concatenate([hit, hit, miss])] * scale[:, None]).astype(F),
                        np.array([o[0], [np.nan, 0, 0], [np.inf, 0, 0]], F)])
    diff = b - a
    expected = np.isnan(ray_ref.cast(oracle, s.ov, a, api.unit_directions(diff), t_max=api.direction_lengths(diff))[1])
    got = gv.visible(a, b)
    assert got.dtype == np.bool_ and (got == expected).all()
    assert expected[:len(hit)].sum() >= 100 and (~expected[len(hit):2 * len(hit)]).sum() >= 100 and expected[-3:].all()
