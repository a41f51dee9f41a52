"""Volume fusion on the GPU (include/tsdf_amd.h, "volume fusion"; tsdf_amd/csrc/fuse.hip) against its CPU reference
(tests/fuse_ref.py: the oracle's trilinear sample for every S, numpy float32 for the rest), bit for bit in distances and weights.

The grids are the smallest on which the kernel can go wrong.  The destination is 72 x 21 x 22 voxels (X above one wave and no multiple
of 64, Y no multiple of 4, Z a multiple of neither 4 nor 32: the last packed weight group and the last brick are partial) over
2900 x 3100 x 3300 mm at offset (-150, 40, 275), two fused frames.  The source is 37 x 34 x 45 voxels over 3000^3 mm at another offset,
truncation distance 300 mm (above the destination's 235.7, so the clamp bites), three fused frames.  The transform turns by 20 degrees
about the axis (1, 2, 3) and shifts so that part of the destination lies outside the source."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import fuse_ref
from tests.helpers import H, W, Cam, assert_same_floats
from tsdf_amd import _capi, synth

F = np.float32
DST = ((72, 21, 22), (2900.0, 3100.0, 3300.0), (-150.0, 40.0, 275.0), None, (0, 9))
SRC = ((37, 34, 45), (3000.0, 3000.0, 3000.0), (60.0, -90.0, 120.0), 300.0, (3, 12, 21))
# the identity fuse: the destination's grid and the source's frames, at offset 0 -- with an offset, (centre + offset) - offset is not the
# centre in every voxel, and the sample is then not the voxel's own value to the last bit
TWIN = (DST[0], DST[1], (0.0, 0.0, 0.0), None, (3, 12, 21))
SEED, PERIOD = 0x5EEDF05E, 40
AXIS, DEGREES, SHIFT = (1.0, 2.0, 3.0), 20.0, (500.0, -653.0, -650.0)
CAST_W, CAST_H = 80, 60
GUARD = 0x7FC0BEEF7FC0BEEF


def frame(i):
    return synth.depth_frame(i, PERIOD, seed=SEED)


def set_truncation(vol, trunc):
    """A new truncation distance, then clear(): every distance is the new +trunc."""
    i = vol.info()
    zero = np.zeros(3, F)
    _capi.check(_capi.lib.tsdf_volume_set_header(vol._h, np.array(i.offset, F).ctypes.data_as(C.POINTER(C.c_float)), float(trunc),
                                                 float(i.max_weight), zero.ctypes.data_as(C.POINTER(C.c_float)),
                                                 zero.ctypes.data_as(C.POINTER(C.c_float))))
    vol.clear()


def gpu_volume(spec, fill=True):
    size, phys, offset, trunc, frames = spec
    v = tsdf_amd.TSDFVolume(size, phys)
    v.offset(*offset)
    if trunc:
        set_truncation(v, trunc)
    for i in frames if fill else ():
        d, cam = frame(i)
        v.integrate(d, W, H, cam)
    return v


def oracle_volume(O, spec, fill=True):
    size, phys, offset, trunc, frames = spec
    v = O.Volume(size, phys)
    v.offset(*offset)
    if trunc:
        v.g.trunc = trunc
        v.clear()
    for i in frames if fill else ():
        d, cam = frame(i)
        v.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=O.max_threads())
    return v


def reference(O, dv, sv, m, dist=None, weight=None, src_weight=None, cap=0):
    return fuse_ref.fuse(O, fuse_ref.geometry(dv), dv.g.trunc, dv.dist if dist is None else dist, dv.weight if weight is None else weight,
                         fuse_ref.geometry(sv), sv.dist, sv.weight if src_weight is None else src_weight, m, cap=cap)


def state(vol):
    return vol.get_distance_data(), vol.get_weight_data(), vol.weight_storage()


def assert_state(vol, dist, weight, what):
    assert_same_floats(vol.get_distance_data(), dist, what + ": distances")
    assert_same_floats(vol.get_weight_data(), weight, what + ": weights")


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(oracle):
    """The oracle's twins of the two volumes and the reference's answer for the common transform -- computed once, never changed."""
    s = Scene()
    s.dv, s.sv = oracle_volume(oracle, DST), oracle_volume(oracle, SRC)
    s.m = fuse_ref.rotation(AXIS, DEGREES, SHIFT)
    s.ref_d, s.ref_w, s.updated = reference(oracle, s.dv, s.sv, s.m)
    for a in (s.dv.dist, s.dv.weight, s.sv.dist, s.sv.weight, s.m, s.ref_d, s.ref_w, s.updated):
        a.setflags(write=False)
    return s


@pytest.mark.gpu
def test_the_parity_is_not_vacuous(scene):
    """The reference alone, on these inputs."""
    s = scene
    share = s.updated.mean()
    assert 0.05 <= share <= 0.95, share
    assert s.dv.g.trunc != s.sv.g.trunc and 235.0 < s.dv.g.trunc < 236.0
    assert (np.abs(s.ref_d[s.updated]) <= F(s.dv.g.trunc)).all()
    assert (np.abs(s.sv.dist) > F(s.dv.g.trunc)).sum() >= 1000           # the clamp has something to do
    assert (s.dv.weight[s.updated] > 0).sum() >= 500 and (s.dv.weight[s.updated] == 0).sum() >= 500   # blends and first observations
    # the last partial weight group (planes 20, 21) and the lanes beyond the first wave (x >= 64) are updated too
    grid = s.updated.reshape(22, 21, 72)
    assert grid[20:].sum() >= 50 and grid[:, :, 64:].sum() >= 50 and grid[:, 20].sum() >= 50


@pytest.mark.gpu
@pytest.mark.parametrize("src_bits", (8, 16, 32))
@pytest.mark.parametrize("dst_bits", (8, 16, 32))
def test_bit_parity_in_every_pair_of_weight_storages(scene, dst_bits, src_bits):
    s = scene
    dst, src = gpu_volume(DST), gpu_volume(SRC)
    assert_state(dst, s.dv.dist, s.dv.weight, "destination before")
    assert_state(src, s.sv.dist, s.sv.weight, "source before")
    for vol, bits in ((dst, dst_bits), (src, src_bits)):
        assert vol.weight_storage() == (8, False)
        if bits != 8:
            vol.set_weight_storage(bits)
    n = dst.fuse(src, s.m)
    assert n == int(s.updated.sum())
    assert_state(dst, s.ref_d, s.ref_w, "fused %d <- %d bits" % (dst_bits, src_bits))
    assert dst.weight_storage() == (dst_bits, False)                    # (2 + 3 frames: nothing to widen)
    assert_state(src, s.sv.dist, s.sv.weight, "source after")
    assert src.weight_storage() == (src_bits, False)
    dst.close()
    src.close()


@pytest.mark.gpu
def test_the_asynchronous_call_and_the_default_identity(scene, oracle):
    s = scene
    dst, src = gpu_volume(DST), gpu_volume(SRC)
    _capi.check(_capi.lib.tsdf_volume_fuse(dst._h, src._h, s.m.ctypes.data_as(C.POINTER(C.c_float)), None))
    dst.synchronize()
    assert_state(dst, s.ref_d, s.ref_w, "fused_voxels == NULL")
    # a second fuse on top, with the default transform: the reference from the first result
    d2, w2, upd2 = reference(oracle, s.dv, s.sv, None, dist=s.ref_d, weight=s.ref_w)
    assert dst.fuse(src) == int(upd2.sum()) > 0
    assert_state(dst, d2, w2, "second fuse, identity")
    dst.close()
    src.close()


@pytest.mark.gpu
def test_counts_near_250_widen_the_storage_before_the_fuse(scene, oracle):
    s = scene
    weights = np.where(s.dv.weight > 0, s.dv.weight + F(252), F(0)).astype(F)     # up to 254; the source adds up to 3
    dst, src = gpu_volume(DST), gpu_volume(SRC)
    dst.set_weight_data(weights)
    assert dst.weight_storage() == (8, False)
    rd, rw, upd = reference(oracle, s.dv, s.sv, s.m, weight=weights)
    assert rw.max() > 255 and (rw[upd] > 255).sum() >= 10                # an 8-bit count would have wrapped
    assert dst.fuse(src, s.m) == int(upd.sum())
    assert dst.weight_storage() == (16, False)
    assert_state(dst, rd, rw, "widened")
    dst.close()
    src.close()


@pytest.mark.gpu
def test_fractional_source_weights_put_the_destination_into_fp32(scene, oracle):
    s = scene
    weights = np.where(s.sv.weight > 0, s.sv.weight + F(0.25), F(0)).astype(F)
    dst, src = gpu_volume(DST), gpu_volume(SRC)
    src.set_weight_data(weights)
    assert src.weight_storage() == (32, False) and dst.weight_storage() == (8, False)
    rd, rw, upd = reference(oracle, s.dv, s.sv, s.m, src_weight=weights)
    assert (rw[upd] != np.round(rw[upd])).all()
    assert dst.fuse(src, s.m) == int(upd.sum()) == int(s.updated.sum())
    assert dst.weight_storage() == (32, False)
    assert_state(dst, rd, rw, "fractional source weights")
    dst.close()
    src.close()


@pytest.mark.gpu
def test_weight_cap_stores_the_minimum_and_divides_by_the_sum(scene, oracle):
    s = scene
    weights = (s.dv.weight * F(2)).astype(F)                               # 0, 2, 4: with up to 3 from the source the cap of 5 bites
    dst, src = gpu_volume(DST), gpu_volume(SRC)
    dst.set_weight_data(weights)
    dst.set_weight_cap(5)
    rd, rw, upd = reference(oracle, s.dv, s.sv, s.m, weight=weights, cap=5)
    plain_d, plain_w, _ = reference(oracle, s.dv, s.sv, s.m, weight=weights)
    assert (plain_w[upd] > 5).sum() >= 100 and rw.max() == 5 and np.array_equal(rd.view(np.uint32), plain_d.view(np.uint32))
    assert dst.fuse(src, s.m) == int(upd.sum())
    assert dst.weight_storage() == (8, False)
    assert_state(dst, rd, rw, "capped")
    dst.close()
    src.close()


@pytest.mark.gpu
def test_identity_fuse_onto_a_cleared_volume(oracle):
    sv, dv = oracle_volume(oracle, TWIN), oracle_volume(oracle, TWIN, fill=False)
    rd, rw, upd = reference(oracle, dv, sv, None)
    assert 0.05 <= upd.mean() <= 0.95
    # every updated voxel holds the source's distance bits and weight: (trunc * 0 + s ws) / ws with s the source's own value
    assert np.array_equal(rd[upd].view(np.uint32), sv.dist[upd].view(np.uint32)) and np.array_equal(rw[upd], sv.weight[upd])
    assert (rd[~upd] == F(dv.g.trunc)).all() and (rw[~upd] == 0).all()
    assert ((sv.weight > 0) & ~upd).sum() >= 100                         # observed voxels with an unobserved tap stay cleared
    src, dst = gpu_volume(TWIN), gpu_volume(TWIN, fill=False)
    src.set_weight_storage(16)
    assert dst.fuse(src) == int(upd.sum())
    assert_state(dst, rd, rw, "identity")
    assert_state(src, sv.dist, sv.weight, "source after the identity fuse")
    assert src.weight_storage() == (16, False)
    dst.close()
    src.close()


@pytest.mark.gpu
def test_ray_cast_after_a_fuse_equals_the_cast_of_the_same_distances(scene, oracle):
    """The occupancy hand-over: the flags the first cast built are for the distances before the fuse."""
    s = scene
    _, cam = frame(9)
    k, kinv = oracle.camera_k(591.1 / 8, 590.1 / 8, 331.0 / 8, 234.6 / 8)
    cam = Cam(cam.pose(), cam.inverse_pose(), k, kinv)
    caster = tsdf_amd.GPURaycaster(CAST_W, CAST_H)
    dst, src = gpu_volume(DST), gpu_volume(SRC)
    before_v, _ = caster.raycast(dst, cam)
    dst.fuse(src, s.m)
    v, n = caster.raycast(dst, cam)
    fresh = gpu_volume(DST, fill=False)
    fresh.set_distance_data(s.ref_d)
    fv, fn = caster.raycast(fresh, cam)
    assert_same_floats(v, fv, "vertices after the fuse")
    assert_same_floats(n, fn, "normals after the fuse")
    hit = ~np.isnan(fv[:, 0])
    assert hit.sum() >= 500
    assert (before_v.view(np.uint32) != fv.view(np.uint32)).any()         # the fuse changed what the camera sees
    for vol in (dst, src, fresh):
        vol.close()


@pytest.mark.gpu
def test_integrate_after_a_fuse(scene, oracle):
    s = scene
    dst, src = gpu_volume(DST), gpu_volume(SRC)
    dst.fuse(src, s.m)
    d, cam = frame(18)
    dst.integrate(d, W, H, cam)
    ov = oracle_volume(oracle, DST, fill=False)
    ov.set_distance_data(s.ref_d)
    ov.set_weight_data(s.ref_w)
    ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    assert_state(dst, ov.dist, ov.weight, "fuse, then integrate")
    assert ov.weight.max() == 6
    dst.close()
    src.close()


@pytest.mark.gpu
def test_disjoint_volumes(scene):
    s = scene
    dst, src = gpu_volume(DST), gpu_volume(SRC)
    before = state(dst)
    assert dst.fuse(src, fuse_ref.rotation(AXIS, DEGREES, (10000.0, 0.0, 0.0))) == 0
    after = state(dst)
    assert_same_floats(after[0], before[0], "distances")
    assert_same_floats(after[1], before[1], "weights")
    assert after[2] == before[2]
    dst.close()
    src.close()


@pytest.mark.gpu
def test_refusals(scene):
    """(Volumes on different devices are refused too; that needs two GPUs and is not run here.)"""
    s = scene
    lib = _capi.lib
    dst, src = gpu_volume(DST), gpu_volume(SRC)
    slab = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3, slab=(0, 8))
    nodes = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3)
    nodes.deformation()                                                   # materialises the node array
    before = state(dst)
    mp = lambda m: np.ascontiguousarray(m, F).ctypes.data_as(C.POINTER(C.c_float))
    eye = np.eye(4, dtype=F).reshape(-1)

    def refused(d, sr, m):
        count = C.c_uint64(GUARD)
        rc = lib.tsdf_volume_fuse(d._h if d else None, sr._h if sr else None, mp(m) if m is not None else None, C.byref(count))
        assert rc == _capi.TSDF_ERR_INVALID
        assert len(_capi.last_error()) > 0
        assert count.value == GUARD, "fused_voxels was written by a refused call"

    refused(None, src, eye)
    refused(dst, None, eye)
    refused(dst, src, None)
    refused(dst, dst, eye)
    refused(dst, slab, eye)
    refused(slab, src, eye)
    refused(dst, nodes, eye)
    refused(nodes, src, eye)
    for at in (0, 6, 9, 14):                                              # rows 0 - 2 of columns 0 - 3
        for bad in (np.nan, np.inf, -np.inf):
            m = s.m.copy()
            m[at] = bad
            refused(dst, src, m)
    with pytest.raises(ValueError):
        dst.fuse(dst)
    after = state(dst)
    assert_same_floats(after[0], before[0], "distances after the refusals")
    assert_same_floats(after[1], before[1], "weights after the refusals")
    assert after[2] == before[2]
    # the bottom row is not used: a NaN there changes nothing
    m = s.m.copy()
    m[[3, 7, 11, 15]] = np.nan
    assert dst.fuse(src, m) == int(s.updated.sum())
    assert_state(dst, s.ref_d, s.ref_w, "NaN in the unused row")
    for vol in (dst, src, slab, nodes):
        vol.close()
