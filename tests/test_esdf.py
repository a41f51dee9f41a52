"""GPU: the distance field (tsdf_volume_compute_esdf; include/tsdf_amd.h, "distance field") against the CPU reference
tests/esdf_ref.py, bit for bit: random fields with unobserved voxels and planted zeros and NaNs on odd grids, every cap and both flag
settings, a fused volume in all three weight storages, a cleared volume, a reused handle, the refusals, the scratch bound, that a
computation leaves the volume alone, and that sampling is the field queries' own kernel on the ESDF array.
Grids are the smallest at which the passes can go wrong: rows shorter than, equal to and longer than a wave (the x pass stages a row
per wave in LDS, 64 lanes wide), more than one workgroup on every axis (blocks are 64 x 4 lanes, one plane each), odd sizes."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import esdf_ref
from tests.helpers import H, W, assert_same_floats
from tsdf_amd import _capi, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
# The y and z kernels have no tile of their own along the scanned axis -- a lane walks its column outwards through global memory -- so
# the last two grids make those columns much longer than anything else here (a wave, a block's four rows, the 64-voxel LDS pitch):
# 300 and 260 steps with few sites, so that the scans really run that far.
GRIDS = [(2, 2, 2), (3, 2, 5), (64, 2, 2), (65, 3, 2), (129, 7, 3), (40, 33, 21), (8, 300, 5), (5, 4, 260)]
OFFSET = (100.0, -50.0, 25.0)
VS = np.array([10.0, 12.5, 9.0], F32)
CAPS = [np.inf, 3.5 * 10.0, 4.5, 10.0]      # none, 3.5 voxels, less than one voxel (of every axis), exactly vs[0]


def volume_of(size, D=None, Wt=None):
    """Anisotropic voxels (10 x 12.5 x 9 mm), as tests/test_mesh_indexed.py::volume_of makes them."""
    gv = tsdf_amd.TSDFVolume(size, (size[0] * 10.0, size[1] * 12.5, size[2] * 9.0))
    gv.offset(*OFFSET)
    assert np.array_equal(gv.voxel_size(), VS)
    if D is not None:
        gv.set_distance_data(D)
        gv.set_weight_data(Wt)
    return gv


def state(gv):
    return gv.get_distance_data(), gv.get_weight_data(), gv.weight_storage()


def assert_state(gv, before, what):
    d, w, s = state(gv)
    assert_same_floats(d, before[0], what + ": distances")
    assert_same_floats(w, before[1], what + ": weights")
    assert s == before[2], what


@pytest.mark.parametrize("size", GRIDS)
@pytest.mark.parametrize("density", ["dense", "sparse"])
def test_random_fields_equal_the_reference_bit_for_bit(size, density):
    n = size[0] * size[1] * size[2]
    # dense: a site almost everywhere, a NaN weight planted (fp32 weights); sparse: a handful of negative voxels, so scans run the
    # length of the grid, and whole-number weights (packed counts)
    share = 0.5 if density == "dense" else min(0.5, 6.0 / n)
    D, Wt = esdf_ref.random_field(size, 5001 + size[0] + 7 * size[2], share, nan_weight=density == "dense")
    gv = volume_of(size, D, Wt)
    before = state(gv)
    site = esdf_ref.sites(D, Wt, size)
    q = esdf_ref.squared(site, size, VS)
    assert site.sum() >= 2                       # (by the CPU reference; the seeds are chosen so)
    handle = tsdf_amd.ESDF()
    for cap in CAPS:
        for fill in (False, True):
            ref = esdf_ref.finish(q, D, Wt, cap, fill)
            got = gv.compute_esdf(cap, fill, into=handle)
            assert got is handle
            assert_same_floats(got.distances, ref, "grid %s %s cap %s fill %s" % (size, density, cap, fill))
            i = got.info
            assert tuple(i.size) == tuple(size) and i.flags == (1 if fill else 0) and i.n_sites == int(site.sum()) == got.n_sites
            assert np.array_equal(np.array(i.voxel_size, F32), VS) and tuple(i.offset) == OFFSET
            assert F32(i.max_distance) == F32(cap)
    assert handle.scratch_bytes <= 4 * n + 65536
    assert_state(gv, before, "grid %s after the computations" % (size,))
    gv.close()


@pytest.fixture(scope="module")
def fused():
    """Eight synthetic frames on 64^3: (frames, distances, weights) of the device's own integration."""
    n = 64
    frames = [synth.depth_frame(i * 5, 40, seed=0x5EEDE5DF) for i in range(8)]
    gv = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    for d, cam in frames:
        gv.integrate(d, W, H, cam)
    D, Wt = gv.get_distance_data(), gv.get_weight_data()
    vs = gv.voxel_size()
    gv.close()
    site = esdf_ref.sites(D, Wt, (n,) * 3)
    return frames, D, Wt, vs, site, esdf_ref.squared(site, (n,) * 3, vs)


def fused_volume(frames):
    gv = tsdf_amd.TSDFVolume((64,) * 3, (3000.0,) * 3)
    for d, cam in frames:
        gv.integrate(d, W, H, cam)
    return gv


def test_a_fused_volume_in_all_three_weight_storages(fused):
    frames, D, Wt, vs, site, q = fused
    assert site.sum() > 1000 and (Wt == 0).sum() > 1000
    results = {}
    for bits in (8, 16, 32):
        gv = fused_volume(frames)
        assert gv.weight_storage() == (8, False)
        if bits != 8:
            gv.set_weight_storage(bits)
        for cap in (np.inf, 200.0):
            for fill in (False, True):
                e = gv.compute_esdf(cap, fill)
                assert gv.weight_storage() == (bits, False)
                assert e.n_sites == int(site.sum()) > 0
                results[(bits, cap, fill)] = e.distances
                assert_same_floats(results[(bits, cap, fill)], esdf_ref.finish(q, D, Wt, cap, fill), "%d-bit weights, cap %s" % (bits, cap))
                assert_same_floats(results[(bits, cap, fill)], results[(8, cap, fill)], "%d-bit against 8-bit weights" % bits)
        assert_same_floats(gv.get_weight_data(), Wt, "weights after")
        gv.close()


def test_a_computation_leaves_the_volume_alone(fused):
    frames = fused[0]
    gv = fused_volume(frames)
    cam = frames[3][1]
    before = state(gv)
    v0, n0 = gv.raycast(W, H, cam)
    s0 = gv.extract_surface()
    assert (~np.isnan(v0[:, 0])).sum() > 1000 and len(s0) > 1000
    gv.compute_esdf(150.0).distances
    assert_state(gv, before, "after the computation")
    v1, n1 = gv.raycast(W, H, cam)
    assert_same_floats(v1, v0, "ray-cast vertices")
    assert_same_floats(n1, n0, "ray-cast normals")
    assert_same_floats(gv.extract_surface(), s0, "the soup")
    # ... also when the cast's state is fresh and the computation comes between an integration and the next cast
    gv.integrate(frames[0][0], W, H, frames[0][1])
    twin = fused_volume(frames)
    twin.integrate(frames[0][0], W, H, frames[0][1])
    gv.compute_esdf().distances
    for a, b, what in zip(gv.raycast(W, H, cam), twin.raycast(W, H, cam), ("vertices", "normals")):
        assert_same_floats(a, b, "ray cast beside a twin without a distance field: " + what)
    gv.close()
    twin.close()


def test_a_cleared_volume_has_no_sites():
    size = (33, 5, 6)
    gv = volume_of(size)
    gv.clear()
    n = size[0] * size[1] * size[2]
    e = gv.compute_esdf()
    assert e.n_sites == 0 and np.isnan(e.distances).all()
    assert np.isposinf(gv.compute_esdf(fill_unknown=True).distances).all()
    assert (gv.compute_esdf(40.0, fill_unknown=True).distances == F32(40.0)).all()
    # observed, no crossing: +inf without a cap, the cap with one, the sign of the voxel
    gv.set_weight_data(np.ones(n, F32))
    gv.set_distance_data(np.full(n, -0.25, F32))
    assert np.isneginf(gv.compute_esdf().distances).all()
    assert (gv.compute_esdf(7.0).distances == F32(-7.0)).all()
    gv.close()


def test_a_handle_is_reused_across_grids_and_two_computations_give_the_same_bytes():
    handle = tsdf_amd.ESDF()
    assert handle.device_buffer() == 0
    for k, size in enumerate([(40, 33, 21), (3, 2, 5), (129, 7, 3), (40, 33, 21)]):
        D, Wt = esdf_ref.random_field(size, 6000 + k, 0.02)
        gv = volume_of(size, D, Wt)
        ref, n_sites = esdf_ref.esdf(D, Wt, size, VS, 60.0)
        first = gv.compute_esdf(60.0, into=handle).distances
        assert_same_floats(first, ref, "reused handle, grid %s" % (size,))
        again = gv.compute_esdf(60.0, into=handle).distances
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32)) and handle.n_sites == n_sites
        # the device array is the download
        n = size[0] * size[1] * size[2]
        host = np.empty(n, F32)
        p = handle.device_buffer()
        assert p
        _capi.check(_capi.lib.tsdf_device_download(host.ctypes.data, C.c_void_p(p), host.nbytes))
        assert np.array_equal(host.view(np.uint32), first.view(np.uint32))
        assert handle.scratch_bytes <= 4 * 40 * 33 * 21 + 65536     # (arrays only grow: the largest grid so far)
        gv.close()


def sample_points(size, rng):
    """World points: inside, on voxel faces and grid faces, outside, NaN."""
    phys = np.array([size[0] * 10.0, size[1] * 12.5, size[2] * 9.0])
    inside = rng.uniform(0.0, 1.0, (600, 3)) * phys
    faces = np.floor(rng.uniform(0.0, 1.0, (200, 3)) * np.array(size)) * VS.astype(np.float64)       # whole voxels: cell faces
    faces[::3, 0] += 0.5 * 10.0                                                                      # ... and voxel centres
    edge = rng.uniform(0.0, 1.0, (120, 3)) * phys
    edge[:40, 0], edge[40:80, 1], edge[80:, 2] = 0.0, phys[1], phys[2] - 1e-3                        # on and next to the grid's faces
    outside = rng.uniform(-0.5, 1.5, (200, 3)) * phys
    p = np.concatenate([inside, faces, edge, outside]) + np.array(OFFSET)
    p = p.astype(F32)
    p[5], p[17, 1], p[29, 2] = np.nan, np.nan, np.inf
    return np.ascontiguousarray(p)


@pytest.mark.parametrize("fill", [False, True])
def test_sampling_is_the_field_query_on_the_esdf_array(fill):
    size = (40, 33, 21)
    D, Wt = esdf_ref.random_field(size, 6100, 0.01, unobserved_share=0.02)
    gv = volume_of(size, D, Wt)
    e = gv.compute_esdf(180.0, fill)
    field = e.distances
    assert np.isnan(field).any() != fill
    twin = volume_of(size)
    twin.set_distance_data(field)
    P = sample_points(size, np.random.default_rng(61))
    td, tg, _ = twin.sample_field(P, gradient=True, weight=False)
    _, tu, _ = twin.sample_field(P, gradient=True, weight=False, unit_gradient=True)
    assert np.isfinite(td).sum() > 300 and np.isfinite(tg).all(axis=1).sum() > 200 and np.isnan(td).sum() > 100
    if not fill:
        assert (np.isnan(td[:600])).sum() > 20                      # inside the grid, next to an unknown voxel: NaN taps propagate
    gv.close()                                                      # sampling needs no volume
    d, g = e.sample(P, gradient=True)
    assert_same_floats(d, td, "distance")
    assert_same_floats(g, tg, "raw gradient")
    d2, u = e.sample(P, gradient=True, unit=True)
    assert_same_floats(d2, td, "distance beside the unit gradient")
    assert_same_floats(u, tu, "unit gradient")
    assert_same_floats(e.sample(P), td, "distance alone")
    assert e.sample(np.empty((0, 3), F32)).shape == (0,)
    # the device entry point, gradient only, on the null stream
    lib = _capi.lib
    dp, dg = C.c_void_p(), C.c_void_p()
    _capi.check(lib.tsdf_device_alloc(P.nbytes, C.byref(dp)))
    _capi.check(lib.tsdf_device_alloc(P.nbytes, C.byref(dg)))
    try:
        _capi.check(lib.tsdf_device_upload(dp, P.ctypes.data, P.nbytes))
        e.sample_device(len(P), dp.value, None, dg.value, unit=True)
        _capi.check(lib.tsdf_stream_synchronize(None))
        out = np.empty_like(P)
        _capi.check(lib.tsdf_device_download(out.ctypes.data, dg, out.nbytes))
        assert_same_floats(out, tu, "unit gradient through the device entry point")
        with pytest.raises(ValueError, match="no output"):
            e.sample_device(len(P), dp.value, None, None)
        with pytest.raises(ValueError, match="null points"):
            e.sample_device(len(P), None, dg.value, None)
        e.sample_device(0, None, dg.value, None)                     # n == 0 launches nothing
    finally:
        lib.tsdf_device_free(dp)
        lib.tsdf_device_free(dg)
    twin.close()


def test_refusals():
    lib, invalid = _capi.lib, _capi.TSDF_ERR_INVALID
    size = (8, 6, 5)
    D, Wt = esdf_ref.random_field(size, 6200)
    gv = volume_of(size, D, Wt)
    before = state(gv)
    handle = tsdf_amd.ESDF()
    # a handle that has never been computed
    with pytest.raises(ValueError, match="never been computed"):
        handle.sample(np.zeros((1, 3), F32))
    one = np.zeros(1, F32)
    assert lib.tsdf_esdf_download(handle._h, one.ctypes.data) == invalid and "never been computed" in _capi.last_error()
    assert handle.device_buffer() == 0 and handle.n_sites == 0
    # null arguments
    assert lib.tsdf_volume_compute_esdf(None, 1.0, 0, handle._h) == invalid
    assert lib.tsdf_volume_compute_esdf(gv._h, 1.0, 0, None) == invalid
    assert lib.tsdf_esdf_get_info(handle._h, None) == invalid and lib.tsdf_esdf_buffer(handle._h, None) == invalid
    assert lib.tsdf_esdf_download(handle._h, None) == invalid and lib.tsdf_esdf_scratch_bytes(handle._h, None) == invalid
    # max_distance that is not > 0
    for bad in (0.0, -0.0, -5.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="max_distance"):
            gv.compute_esdf(bad, into=handle)
    # unknown flags
    assert lib.tsdf_volume_compute_esdf(gv._h, 1.0, 2, handle._h) == invalid and "unknown flags" in _capi.last_error()
    assert lib.tsdf_volume_compute_esdf(gv._h, 1.0, 0x80000001, handle._h) == invalid
    # a Z-slab, a materialised deformation-node array, an axis longer than 4096
    slab = tsdf_amd.TSDFVolume((16, 16, 16), (160.0,) * 3, slab=(0, 8))
    with pytest.raises(ValueError, match="Z-slab"):
        slab.compute_esdf(into=handle)
    nodes = tsdf_amd.TSDFVolume((16, 16, 16), (160.0,) * 3)
    nodes.deformation()
    with pytest.raises(ValueError, match="has a materialised deformation-node array: voxel centres must be the implicit grid"):
        nodes.compute_esdf(into=handle)
    for size_long in ((4097, 2, 2), (2, 4097, 2), (2, 2, 4097)):
        long_axis = tsdf_amd.TSDFVolume(size_long, tuple(10.0 * s for s in size_long))
        with pytest.raises(ValueError, match="longer than 4096"):
            long_axis.compute_esdf(into=handle)
        long_axis.close()
    # nothing was computed, nothing was written
    assert handle.device_buffer() == 0
    assert_state(gv, before, "after the refusals")
    # and the handle still works
    assert_same_floats(gv.compute_esdf(25.0, into=handle).distances, esdf_ref.esdf(D, Wt, size, VS, 25.0)[0], "after the refusals")
    for v in (slab, nodes, gv):
        v.close()
    handle.close()
    handle.close()


def test_the_longest_axis_allowed():
    """4096 voxels along x: one wave stages the whole row (16 KiB of LDS), and (float)(j * j) is still exact."""
    size = (4096, 2, 1)
    D = np.full(4096 * 2, 0.5, F32)
    D[4095] = -0.5                   # one crossing at the far end of row 0: row 0 scans 4094 steps, row 1 has no site of its own
    Wt = np.ones(4096 * 2, F32)
    gv = volume_of(size, D, Wt)
    ref, n_sites = esdf_ref.esdf(D, Wt, size, VS)
    e = gv.compute_esdf()
    assert n_sites == 3 and e.n_sites == 3          # both ends of the x crossing and the end of the y crossing below 4095
    assert_same_floats(e.distances, ref, "4096 x 2 x 1")
    assert abs(ref[0]) == F32(40940.0)
    gv.close()
