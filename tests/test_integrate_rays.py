"""Ray integration on the GPU (include/tsdf_amd.h, "ray integration"; tsdf_amd/csrc/integrate_rays.hip) against its CPU reference
(tests/rays_integrate_ref.py, written from the header's rules), bit for bit in distances and weights: every ray set of
tests/rays_integrate_cases.py through both entry points, with one origin and with one per ray, in all three weight storages, under a
weight cap, between two depth frames and call after call (which shows the scratch is zero again)."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import ray_ref
from tests import rays_integrate_cases as RC
from tests import rays_integrate_ref as ref
from tests.helpers import H, W, Cam, assert_same_floats
from tsdf_amd import _capi, synth
from tsdf_amd.api import _DeviceArray, unit_directions

F = np.float32
NAMES = [c.name for c in RC.cases()]
SEED, PERIOD = 0x5EEDF05E, 40
GUARD_WORD, GUARD_FLOATS = 0x7FC0BEEF7FC0BEEF, 64
CAST_W, CAST_H = 80, 60


def gpu_volume(grid, bits=8):
    dims, phys, offset = grid
    v = tsdf_amd.TSDFVolume(dims, phys)
    v.offset(*offset)
    if bits != 8:
        v.set_weight_storage(bits)
    return v


def assert_state(vol, dist, weight, what):
    assert_same_floats(vol.get_distance_data(), dist, what + ": distances")
    assert_same_floats(vol.get_weight_data(), weight, what + ": weights")


def call_host(vol, o, p, lo, hi, flags):
    return vol.integrate_rays(o[0] if len(o) == 1 else o, p, band_only=bool(flags & ref.BAND_ONLY), min_range=lo, max_range=hi)


def call_device(vol, o, p, lo, hi, flags, count=True):
    """Through tsdf_integrate_rays_device, the rays between guard regions on the device; -> updated voxels (None without count)."""
    guard = np.full(GUARD_FLOATS, np.nan, F)
    guard.view(np.uint32)[:] = 0x7FC0BEEF
    host = np.concatenate([guard, o.reshape(-1), guard, p.reshape(-1), guard]).astype(F)
    at_o, at_p = GUARD_FLOATS, 2 * GUARD_FLOATS + o.size
    box = (C.c_uint64 * 3)(GUARD_WORD, GUARD_WORD, GUARD_WORD)
    with _DeviceArray(host) as dev:
        base = dev.ptr.value
        out = C.cast(C.byref(box, 8), C.POINTER(C.c_uint64)) if count else None
        _capi.check(_capi.lib.tsdf_integrate_rays_device(vol._h, len(p), C.c_void_p(base + 4 * at_o), len(o), C.c_void_p(base + 4 * at_p),
                                                         lo, hi, flags, out))
        vol.synchronize()
        back = np.empty_like(host)
        _capi.check(_capi.lib.tsdf_device_download(back.ctypes.data, dev.ptr, host.nbytes))
    assert np.array_equal(back.view(np.uint32), host.view(np.uint32)), "the rays or the guard regions around them were written"
    assert box[0] == GUARD_WORD and box[2] == GUARD_WORD
    return int(box[1]) if count else None


def run(vol, c, entry=call_host, expand=False):
    """Every call of the case; -> the updated-voxel counts."""
    counts = []
    for o, p, lo, hi, flags in c.calls:
        if expand and len(o) == 1:
            o = np.ascontiguousarray(np.repeat(o, len(p), 0))
        counts.append(entry(vol, o, p, lo, hi, flags))
    return counts


@pytest.fixture(scope="module")
def refs(oracle):
    """name -> (distances, weights, updated masks) of the case applied to a cleared volume: computed once, never changed."""
    out = {}
    for c in RC.cases():
        d, w, masks = RC.reference(oracle, c)
        for a in (d, w):
            a.setflags(write=False)
        out[c.name] = (d, w, masks)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("bits", (8, 16, 32))
@pytest.mark.parametrize("name", NAMES)
def test_bit_parity_in_every_weight_storage(refs, name, bits):
    c = RC.case(name)
    d, w, masks = refs[name]
    vol = gpu_volume(c.grid, bits)
    counts = run(vol, c)                                                   # several calls in a row: the scratch is zero again each time
    assert counts == [int(m.sum()) for m in masks]
    assert_state(vol, d, w, "%s, %d-bit weights" % (name, bits))
    assert vol.weight_storage() == (bits, False)
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_the_device_entry_point_and_its_guards(refs, name):
    c = RC.case(name)
    d, w, masks = refs[name]
    vol = gpu_volume(c.grid)
    assert run(vol, c, call_device) == [int(m.sum()) for m in masks]
    assert_state(vol, d, w, name + ", device pointers")
    vol.close()
    # updated_voxels == NULL: asynchronous, the same bits
    vol = gpu_volume(c.grid)
    run(vol, c, lambda *a: call_device(*a, count=False))
    assert_state(vol, d, w, name + ", device pointers, no count")
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_one_origin_per_ray_gives_the_bits_of_one_origin(refs, name):
    c = RC.case(name)
    d, w, masks = refs[name]
    vol = gpu_volume(c.grid)
    assert run(vol, c, expand=True) == [int(m.sum()) for m in masks]
    assert_state(vol, d, w, name + ", n origins")
    vol.close()


def depth_frame(i):
    return synth.depth_frame(i, PERIOD, seed=SEED)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_between_two_depth_frames_and_under_a_weight_cap(oracle, name):
    """A depth frame, the rays, a depth frame -- then the rays alone on counts of 4 and more under a cap of 4, which bites."""
    c = RC.case(name)
    dims, phys, offset = c.grid
    ov, geom = RC.make_geometry(oracle, c.grid)
    (d0, cam0), (d1, cam1) = depth_frame(3), depth_frame(12)
    integrate = lambda frame, cam: ov.integrate(frame, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    integrate(d0, cam0)
    first_d, first_w = ov.dist.copy(), ov.weight.copy()
    assert (first_w > 0).sum() >= 1000
    rd, rw, masks = RC.reference(oracle, c, first_d, first_w)
    if name != "ties":                                                     # (that grid's rays pass where this frame saw nothing)
        assert (np.logical_or.reduce(masks) & (first_w > 0)).sum() >= 20   # blends, not only first observations
    ov.set_distance_data(rd)
    ov.set_weight_data(rw)
    integrate(d1, cam1)
    vol = gpu_volume(c.grid)
    vol.integrate(d0, W, H, cam0)
    run(vol, c)
    assert_state(vol, rd, rw, name + ", after a depth frame")
    vol.integrate(d1, W, H, cam1)
    assert_state(vol, ov.dist, ov.weight, name + ", then another depth frame")
    vol.close()
    # the cap
    high = np.where(first_w > 0, first_w * F(4), F(4)).astype(F)
    cd, cw, _ = RC.reference(oracle, c, first_d, high, cap=4)
    pd, pw, _ = RC.reference(oracle, c, first_d, high)
    assert (pw > 4).sum() >= 20 and cw.max() == 4
    vol = gpu_volume(c.grid)
    vol.set_distance_data(first_d)
    vol.set_weight_data(high)
    vol.set_weight_cap(4)
    run(vol, c)
    assert_state(vol, cd, cw, name + ", weight cap 4")
    assert vol.weight_storage() == (8, False)
    vol.close()


@pytest.mark.gpu
def test_counts_near_255_widen_the_storage_first(oracle, refs):
    c = RC.case("inside")
    ov, geom = RC.make_geometry(oracle, c.grid)
    weights = np.full(ov.weight.size, 255.0, F)
    rd, rw, masks = RC.reference(oracle, c, ov.dist, weights)
    assert rw.max() == 256
    vol = gpu_volume(c.grid)
    vol.set_weight_data(weights)
    assert vol.weight_storage() == (8, False)
    run(vol, c)
    assert vol.weight_storage() == (16, False)
    assert_state(vol, rd, rw, "widened")
    vol.close()


@pytest.mark.gpu
def test_five_permutations_give_identical_bits(oracle):
    sets = RC.permutation_sets()
    _, geom = RC.make_geometry(oracle, RC.GRID)
    ov, _ = RC.make_geometry(oracle, RC.GRID)
    rd, rw, upd, _ = ref.integrate(geom, ov.dist, ov.weight, *sets[0])
    for i, (o, p) in enumerate(sets):
        vol = gpu_volume(RC.GRID)
        assert vol.integrate_rays(o, p) == int(upd.sum())
        assert_state(vol, rd, rw, "permutation %d" % i)
        vol.close()


@pytest.mark.gpu
def test_release_the_scratch_then_call_again(oracle, refs):
    c = RC.case("outside")
    d, w, masks = refs["outside"]
    vol = gpu_volume(c.grid)
    vol.release_ray_scratch()                                              # nothing to release yet
    for i, (o, p, lo, hi, flags) in enumerate(c.calls):
        assert call_host(vol, o, p, lo, hi, flags) == int(masks[i].sum())
        vol.release_ray_scratch()
    assert_state(vol, d, w, "released between the calls")
    vol.close()


@pytest.mark.gpu
def test_colours_are_left_alone(refs):
    c = RC.case("inside")
    vol = gpu_volume(c.grid)
    vol.enable_colour(True)
    colours = np.random.RandomState(5).randint(0, 2 ** 32, vol.resident_voxels(), dtype=np.uint64).astype(np.uint32)
    vol.set_colour_data(colours)
    run(vol, c)
    assert np.array_equal(np.asarray(vol.get_colour_data()).reshape(-1), colours)
    assert_state(vol, refs["inside"][0], refs["inside"][1], "with colour enabled")
    vol.close()


@pytest.mark.gpu
def test_an_image_cast_after_the_call_sees_the_new_field(oracle, refs):
    """The occupancy hand-over: the flags the first cast built are for the distances before the rays."""
    c = RC.case("outside")
    d, w, _ = refs["outside"]
    _, cam = depth_frame(9)
    k, kinv = oracle.camera_k(591.1 / 8, 590.1 / 8, 331.0 / 8, 234.6 / 8)
    cam = Cam(cam.pose(), cam.inverse_pose(), k, kinv)
    caster = tsdf_amd.GPURaycaster(CAST_W, CAST_H)
    vol = gpu_volume(c.grid)
    before, _ = caster.raycast(vol, cam)
    assert np.isnan(before).all()                                          # a cleared volume: nothing to hit
    run(vol, c)
    v, n = caster.raycast(vol, cam)
    ov, _ = RC.make_geometry(oracle, c.grid)
    ov.set_distance_data(d)
    ov.set_weight_data(w)
    ovv, ovn = ov.raycast(CAST_W, CAST_H, cam.pose(), cam.kinv(), nthreads=oracle.max_threads())
    assert_same_floats(v, ovv, "vertices after the rays")
    assert_same_floats(n, ovn, "normals after the rays")
    assert (~np.isnan(ovv[:, 0])).sum() >= 200
    vol.close()


@pytest.mark.gpu
def test_end_to_end_fuse_by_rays_then_cast_the_scan_rays(oracle, refs):
    c = RC.case("outside")
    d, w, _ = refs["outside"]
    vol = gpu_volume(c.grid)
    run(vol, c)
    ov, _ = RC.make_geometry(oracle, c.grid)
    ov.set_distance_data(d)
    ov.set_weight_data(w)
    origins = np.concatenate([np.repeat(o, len(p), 0)[::5] for o, p, _, _, _ in c.calls])
    points = np.concatenate([p[::5] for _, p, _, _, _ in c.calls])
    dirs = unit_directions(points - origins)
    _, rt, _ = ray_ref.cast(oracle, ov, origins, dirs)
    gp, gt = vol.cast_rays(origins, dirs)
    hit = ~np.isnan(rt)
    assert hit.sum() >= 200 and np.isfinite(gt[hit]).all() and np.isfinite(gp[hit]).all()
    assert_same_floats(gt, rt, "t along the scan rays")
    # and the surface is where the scanner saw it: within two voxels of the measured range
    measured = np.sqrt(((points - origins).astype(np.float64) ** 2).sum(axis=1))
    assert np.median(np.abs(gt[hit] - measured[hit])) < 90.0
    vol.close()


@pytest.mark.gpu
def test_refusals_change_nothing(refs):
    lib = _capi.lib
    c = RC.case("inside")
    o, p = c.calls[0][0], c.calls[0][1]
    vol = gpu_volume(c.grid)
    run(vol, c)
    slab = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3, slab=(0, 8))
    nodes = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3)
    nodes.deformation()                                                    # materialises the node array
    before = (vol.get_distance_data(), vol.get_weight_data(), vol.weight_storage())

    def refused(v, n, op, n_origins, pp, flags=0):
        for fn in (lib.tsdf_integrate_rays, lib.tsdf_integrate_rays_device):
            count = C.c_uint64(GUARD_WORD)
            rc = fn(v._h if v else None, n, op, n_origins, pp, 0.0, float("inf"), flags, C.byref(count))
            assert rc == _capi.TSDF_ERR_INVALID
            assert len(_capi.last_error()) > 0
            assert count.value == GUARD_WORD, "updated_voxels was written by a refused call"

    op, pp = C.c_void_p(o.ctypes.data), C.c_void_p(p.ctypes.data)
    n = len(p)
    refused(None, n, op, 1, pp)
    refused(vol, n, None, 1, pp)
    refused(vol, n, op, 1, None)
    refused(vol, n, op, 2, pp)
    refused(vol, n, op, 0, pp)
    refused(vol, n, op, n + 1, pp)
    refused(vol, (1 << 23) + 1, op, 1, pp)
    refused(vol, n, op, 1, pp, flags=2)
    refused(vol, n, op, 1, pp, flags=ref.BAND_ONLY | 4)
    refused(slab, n, op, 1, pp)
    refused(nodes, n, op, 1, pp)
    with pytest.raises(ValueError):
        vol.integrate_rays(np.zeros((2, 3), F), p)
    with pytest.raises(ValueError):
        vol.integrate_rays(np.zeros(4, F), p)
    # n == 0 succeeds and changes nothing
    assert vol.integrate_rays(o[0], np.empty((0, 3), F)) == 0
    after = (vol.get_distance_data(), vol.get_weight_data(), vol.weight_storage())
    assert_same_floats(after[0], before[0], "distances after the refusals")
    assert_same_floats(after[1], before[1], "weights after the refusals")
    assert after[2] == before[2]
    assert_state(vol, refs["inside"][0], refs["inside"][1], "after the refusals")
    for v in (vol, slab, nodes):
        v.close()
