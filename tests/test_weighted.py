"""Weighted integration on the GPU (include/tsdf_amd.h, "weighted integration"): tsdf_integrate_weighted* against
the CPU reference (tests/weighted_ref.py: the oracle's frame set on the masked image, the header's blend in numpy fp32), the weight
models against their numpy restatement, and the tracker's weighted mode against the same calls made by hand.

Every comparison is bit for bit.  Grid as in tests/test_weight_cap.py: a partial last brick layer, 80 rows, x past one wave.
"""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import colour_ref, deintegrate_ref
from tests import weighted_ref as R
from tests.helpers import H, W, Cam, assert_same_floats, camera_at
from tsdf_amd import synth

pytestmark = pytest.mark.gpu
SIZE, PHYS = (96, 80, 72), (3000.0, 2500.0, 2250.0)
SMALL, SMALL_PHYS = (40, 12, 20), (1200.0, 360.0, 600.0)
SEED = 0x5EED0C02
PERIOD = 200
SPECIALS = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf], np.float32)


def frames(n, seed=SEED):
    return [synth.depth_frame(i, PERIOD, seed=seed) for i in range(n)]


def uniform(rng, lo, hi, n=W * H):
    return rng.uniform(lo, hi, n).astype(np.float32)


def same(gv, ov, what):
    assert_same_floats(gv.get_weight_data(), ov.weight, what + ": weights")
    assert_same_floats(gv.get_distance_data(), ov.dist, what + ": distances")


def plain_step(oracle, ov, d, cam, width=W, height=H):
    ov.integrate(d, width, height, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())


def stripes(i, n=W * H):
    """Every third run of 7 pixels, shifted by the frame number: where the special weights are planted."""
    return (np.arange(n) // 7) % 3 == i % 3


def with_specials(p, i):
    s = stripes(i, p.size)
    p = p.copy()
    p[s] = SPECIALS[np.arange(int(s.sum())) % SPECIALS.size]
    return p, s


# ---- 1: the unit property ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("start", [8, 16, 32, "pinned"])
def test_unit_weights_are_the_plain_integrate(start):
    gv, tv = tsdf_amd.TSDFVolume(SIZE, PHYS), tsdf_amd.TSDFVolume(SIZE, PHYS)
    fresh = gv.weight_storage()
    tv.set_weight_storage(32)
    if start == "pinned":
        assert gv.weight_data() and gv.weight_storage() == (32, True)
    elif start != 8:
        gv.set_weight_storage(start)
    ones = np.ones(W * H, np.float32)
    for v in (gv, tv):
        v.set_counting(True)
    for i, (d, cam) in enumerate(frames(4)):
        gv.integrate_weighted(d, ones, W, H, cam)
        tv.integrate(d, W, H, cam)
        assert gv.last_updated_voxels() == tv.last_updated_voxels() > 1000, "frame %d" % i
        assert gv.last_distance_stores() == tv.last_distance_stores(), "frame %d" % i
        assert gv.weight_storage() == (32, start == "pinned"), "frame %d" % i
    assert_same_floats(gv.get_weight_data(), tv.get_weight_data(), "unit weights: weights")
    assert_same_floats(gv.get_distance_data(), tv.get_distance_data(), "unit weights: distances")
    assert gv.get_weight_data().max() == 4.0
    for a, b, what in zip(gv.occupancy_data(), tv.occupancy_data(), ("fine", "cell", "reach")):
        assert np.array_equal(a, b), "occupancy %s differs from the plain integrate's" % what
    gv.clear()
    assert gv.weight_storage() == ((32, True) if start == "pinned" else fresh)


# ---- 2: random weights -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counting", [True, False])
def test_random_weights_equal_the_reference(oracle, counting):
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    gv.set_counting(counting)
    rng = np.random.RandomState(11)
    for i, (d, cam) in enumerate(frames(5)):
        p = uniform(rng, 1.0 / 64.0, 64.0)
        keep_d, keep_p = d.copy(), p.copy()
        gv.integrate_weighted(d, p, W, H, cam)
        updated, stores = R.integrate(oracle, ov, d, p, cam)
        assert np.array_equal(d, keep_d) and np.array_equal(p, keep_p)
        same(gv, ov, "random weights, frame %d" % i)
        if counting:
            assert gv.last_updated_voxels() == updated > 1000, "frame %d" % i
            assert gv.last_distance_stores() == stores, "frame %d" % i
    assert gv.weight_storage() == (32, False)
    w = ov.weight[ov.weight > 0]
    assert w.size > 1000 and np.any(w != np.round(w))                 # (weights that are no counts)


# ---- 3: special weights ------------------------------------------------------------------------------------------------------

def test_special_weights_are_pixels_without_depth(oracle):
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    gv.set_counting(True)
    rng = np.random.RandomState(12)
    for i, (d, cam) in enumerate(frames(3)):
        p, s = with_specials(uniform(rng, 1.0 / 64.0, 64.0), i)
        gv.integrate_weighted(d, p, W, H, cam)
        zeroed = np.where(s, 0, d).astype(np.uint16)
        updated, stores = R.integrate(oracle, ov, zeroed, np.where(s, np.float32(1.0), p), cam)
        same(gv, ov, "specials, frame %d" % i)
        assert gv.last_updated_voxels() == updated > 1000 and gv.last_distance_stores() == stores
    assert np.isfinite(gv.get_weight_data()).all()
    # a frame whose every weight is invalid changes nothing
    d, cam = frames(4)[3]
    gv.integrate_weighted(d, SPECIALS[np.arange(W * H) % SPECIALS.size], W, H, cam)
    same(gv, ov, "a frame of invalid weights")
    assert gv.last_updated_voxels() == 0 and gv.last_distance_stores() == 0


# ---- 4: the cap --------------------------------------------------------------------------------------------------------------

def test_weighted_frames_under_a_cap(oracle):
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    gv.set_weight_cap(3)
    rng = np.random.RandomState(13)
    for i, (d, cam) in enumerate(frames(6)):
        p = uniform(rng, 0.25, 2.5)
        gv.integrate_weighted(d, p, W, H, cam)
        R.integrate(oracle, ov, d, p, cam, cap=3)
        same(gv, ov, "cap 3, frame %d" % i)
    got = gv.get_weight_data()
    assert got.max() == 3.0 and (got == 3.0).sum() > 1000 and np.any((got > 0) & (got < 3.0))


# ---- 5: general cameras and explicit nodes -------------------------------------------------------------------------------------

def small_frames(n):
    cam = camera_at((600.0, 180.0, -1700.0))
    return [(synth.depth_frame(i, PERIOD, seed=SEED)[0], cam) for i in range(n)]


def test_weighted_frames_with_a_general_camera(oracle):
    """Skewed K: integrate_weighted_kernel<false, *, false>."""
    gv, ov = tsdf_amd.TSDFVolume(SMALL, SMALL_PHYS), oracle.Volume(SMALL, SMALL_PHYS)
    rng = np.random.RandomState(14)
    for i, (d, cam) in enumerate(small_frames(3)):
        k = np.array(cam.k(), np.float32).copy()
        k[3] = 0.02                           # column-major: K[0][1], a skew term -- not the standard shape
        kinv = np.linalg.inv(k.reshape(3, 3).T.astype(np.float64)).T.astype(np.float32).reshape(-1)
        cam = Cam(cam.pose(), cam.inverse_pose(), k, kinv)
        p = uniform(rng, 1.0 / 64.0, 64.0)
        gv.set_counting(i % 2 == 0)
        gv.integrate_weighted(d, p, W, H, cam)
        assert R.integrate(oracle, ov, d, p, cam)[0] > 100
        same(gv, ov, "skewed intrinsics, frame %d" % i)
    assert (ov.dist < np.float32(ov.truncation_distance())).sum() > 100    # (the surface passes through the grid)


def test_weighted_frames_with_explicit_deformation_nodes(oracle):
    """set_deformation of the regular grid plus a perturbation: integrate_weighted_kernel<true, *, false>."""
    gv, ov = tsdf_amd.TSDFVolume(SMALL, SMALL_PHYS), oracle.Volume(SMALL, SMALL_PHYS)
    vs = ov.voxel_size()
    zz, yy, xx = np.meshgrid(np.arange(SMALL[2]), np.arange(SMALL[1]), np.arange(SMALL[0]), indexing="ij")
    tr = np.stack([(xx + 0.5) * vs[0], (yy + 0.5) * vs[1], (zz + 0.5) * vs[2]], -1).astype(np.float32)
    tr += np.random.RandomState(3).uniform(-10, 10, tr.shape).astype(np.float32)
    ov.translation = np.ascontiguousarray(tr.reshape(-1))
    gv.set_deformation(np.concatenate([tr.reshape(-1, 3), np.zeros((tr.size // 3, 3), np.float32)], axis=1))
    rng = np.random.RandomState(15)
    for i, (d, cam) in enumerate(small_frames(3)):
        p, _ = with_specials(uniform(rng, 1.0 / 64.0, 64.0), i)
        gv.set_counting(i % 2 == 0)
        gv.integrate_weighted(d, p, W, H, cam)
        assert R.integrate(oracle, ov, d, p, cam)[0] > 100
        same(gv, ov, "explicit nodes, frame %d" % i)
    assert gv.weight_storage()[0] == 32


# ---- 6: a brick without a depth tile -------------------------------------------------------------------------------------------

def test_a_close_camera_takes_the_global_gathers(oracle):
    """The camera stands 300 mm in front of the grid and sees a wall 500 mm inside it: the pixel box of the bricks it looks through
    exceeds the 8192-pixel tile, so depth and weight are both gathered from global memory."""
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    cam = camera_at((1500.0, 1250.0, -300.0))
    d = synth.wall_depth(800)
    rng = np.random.RandomState(16)
    p, _ = with_specials(uniform(rng, 1.0 / 64.0, 64.0), 0)
    in_set, _, pidx = R.frame(oracle, ov, d, p, cam)
    # the pixels the updated voxels of one integrate brick (64 x 4 x 32 voxels) use span more than a tile: so does the brick's box
    idx = np.nonzero(in_set)[0]
    x, y, z = idx % SIZE[0], (idx // SIZE[0]) % SIZE[1], idx // (SIZE[0] * SIZE[1])
    brick = (x // 64) + 2 * ((y // 4) + 20 * (z // 32))
    worst = 0
    for b in np.unique(brick):
        px = pidx[idx[brick == b]]
        worst = max(worst, int((px % W).max() - (px % W).min() + 1) * int((px // W).max() - (px // W).min() + 1))
    assert worst > 8192, "no updated voxel lies in a brick whose pixel box exceeds the tile (largest: %d pixels)" % worst
    for i in range(2):
        gv.integrate_weighted(d, p, W, H, cam)
        assert R.integrate(oracle, ov, d, p, cam)[0] > 1000
        same(gv, ov, "close camera, frame %d" % i)


# ---- 7: slabs ----------------------------------------------------------------------------------------------------------------

def test_two_weighted_slabs_are_the_whole_volume():
    size, phys = (64, 48, 70), (2000.0, 1500.0, 2187.5)
    whole = tsdf_amd.TSDFVolume(size, phys)
    rng = np.random.RandomState(17)
    fr = [(d, cam, with_specials(uniform(rng, 1.0 / 64.0, 64.0), i)[0]) for i, (d, cam) in enumerate(frames(4, seed=0x5EED0C03))]
    for d, cam, p in fr:
        whole.integrate_weighted(d, p, W, H, cam)
    wd, ww = whole.get_distance_data().reshape(size[2], -1), whole.get_weight_data().reshape(size[2], -1)
    assert (ww > 0).sum() > 1000
    parts_d, parts_w = [], []
    for lo, hi in ((0, 37), (37, 70)):
        s = tsdf_amd.TSDFVolume(size, phys, slab=(lo, hi))
        for d, cam, p in fr:
            s.integrate_weighted(d, p, W, H, cam)
        a = s.info().z_store_begin
        n_planes = s.info().z_store_end - a
        parts_d.append(s.get_distance_data().reshape(n_planes, -1)[lo - a:hi - a])
        parts_w.append(s.get_weight_data().reshape(n_planes, -1)[lo - a:hi - a])
    assert_same_floats(np.concatenate(parts_d), wd, "slabs, concatenated: distances")
    assert_same_floats(np.concatenate(parts_w), ww, "slabs, concatenated: weights")


# ---- 8: colour ---------------------------------------------------------------------------------------------------------------

def test_colour_words_are_those_of_the_masked_image(oracle):
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    gv.enable_colour()
    geom = colour_ref.geometry(gv)
    colour = np.zeros(gv.resident_voxels(), np.uint32)
    rng = np.random.RandomState(18)
    for i in range(3):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        rgb, _ = synth.colour_frame(i, PERIOD, seed=SEED)
        p, _ = with_specials(uniform(rng, 1.0 / 64.0, 64.0), i)
        gv.integrate_weighted(d, p, W, H, cam, rgb=rgb)
        R.integrate(oracle, ov, d, p, cam)
        colour, _, coloured = colour_ref.integrate_colour(oracle, colour, geom, R.masked_depth(d, p), rgb, W, H, cam)
        assert coloured.sum() > 1000
    same(gv, ov, "weighted colour frames")
    got = gv.get_colour_data()
    bad = np.nonzero(got != colour)[0]
    assert bad.size == 0, "%d colour words differ, first at %d: %08x vs %08x" % (bad.size, bad[0], got[bad[0]], colour[bad[0]])
    assert int((got >> 24).max()) == 3                                  # colour counts are counts: not weighted


# ---- 9: a mixed sequence -------------------------------------------------------------------------------------------------------

def test_plain_weighted_plain_and_a_removal(oracle):
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    fr = frames(3)
    rng = np.random.RandomState(19)
    gv.integrate(fr[0][0], W, H, fr[0][1])
    plain_step(oracle, ov, *fr[0])
    assert gv.weight_storage() == tsdf_amd.TSDFVolume(SIZE, PHYS).weight_storage()      # (still the starting mode: 8-bit counts)
    same(gv, ov, "plain integrate")
    p, _ = with_specials(uniform(rng, 1.0 / 64.0, 64.0), 1)
    gv.integrate_weighted(fr[1][0], p, W, H, fr[1][1])
    R.integrate(oracle, ov, fr[1][0], p, fr[1][1])
    assert gv.weight_storage() == (32, False)
    same(gv, ov, "then a weighted frame (the counts survive the widening)")
    assert (ov.weight == 1.0).sum() > 100                                # voxels only the first frame saw keep their count
    gv.integrate(fr[2][0], W, H, fr[2][1])
    plain_step(oracle, ov, *fr[2])
    same(gv, ov, "then a plain integrate on fp32 weights")
    gv.deintegrate(fr[0][0], W, H, fr[0][1])
    deintegrate_ref.oracle_remove(oracle, ov, *fr[0])
    same(gv, ov, "then the first frame taken out")
    assert gv.weight_storage() == (32, False)


# ---- 10: occupancy -------------------------------------------------------------------------------------------------------------

def test_raycast_after_weighted_frames_equals_the_cast_after_a_rebuild():
    gv = tsdf_amd.TSDFVolume(SIZE, PHYS)
    rng = np.random.RandomState(20)
    fr = frames(3)
    for i, (d, cam) in enumerate(fr):
        gv.integrate_weighted(d, with_specials(uniform(rng, 1.0 / 64.0, 64.0), i)[0], W, H, cam)
    cam = fr[-1][1]
    V, N = gv.raycast(W, H, cam)
    before = gv.occupancy_data()
    rebuilt = gv.occupancy_data(force_rebuild=True)
    for a, b, what in zip(before[:2], rebuilt[:2], ("fine", "cell")):
        assert np.all(a >= b), "occupancy %s: a flag the distances need is missing" % what
    assert rebuilt[0].sum() > 100
    V2, N2 = gv.raycast(W, H, cam)
    assert (~np.isnan(V2[:, 0])).sum() > 1000
    assert_same_floats(V, V2, "vertices")
    assert_same_floats(N, N2, "normals")


# ---- 11: the models ------------------------------------------------------------------------------------------------------------

def model_frame(width, height):
    d, cam = synth.depth_frame(0, PERIOD, seed=SEED)
    y0, x0 = min(100, H - height), min(200, W - width)
    d = d.reshape(H, W)[y0:y0 + height, x0:x0 + width].copy()
    d[height // 3:height // 3 + 3, width // 4:width // 2] = 0          # dropouts
    d[height - 2, 1] = 0
    d[::5, ::7] += 40                                                   # relief, so that the normals differ
    return np.ascontiguousarray(d.reshape(-1)), np.array(cam.kinv(), np.float32)


@pytest.mark.parametrize("width,height", [(640, 480), (37, 23)])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_depth_weights_equal_the_numpy_reference(width, height, flags):
    import torch
    d, kinv = model_frame(width, height)
    z_ref = 2400.0
    want = R.depth_weights(d, width, height, kinv, flags, z_ref)
    dd = torch.from_numpy(d.view(np.int16).copy()).cuda()
    out = torch.full((height * width,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tsdf_amd.depth_weights_device(width, height, dd.data_ptr(), kinv, flags, z_ref, out.data_ptr())
    torch.cuda.synchronize()
    assert_same_floats(out.cpu().numpy(), want, "depth_weights_device, flags %d" % flags)
    assert np.array_equal(dd.cpu().numpy().view(np.uint16), d), "the caller's depth image was written"
    assert_same_floats(tsdf_amd.depth_weights(d, width, height, kinv, flags, z_ref), want, "depth_weights (host), flags %d" % flags)
    assert (want > 0).sum() > width * height // 4 and (want == 0).sum() > 0
    if flags == 3:
        assert np.unique(want).size > 50


# ---- 12: the tracker -------------------------------------------------------------------------------------------------------------

def test_the_tracker_integrates_with_the_models_weights():
    import torch
    from tsdf_amd.tracking import FrameToModelTracker
    n, phys = (128,) * 3, (3000.0,) * 3
    flags, z_ref = tsdf_amd.WEIGHTS_INVERSE_SQUARE | tsdf_amd.WEIGHTS_COSINE, 2400.0
    gv, tv = tsdf_amd.TSDFVolume(n, phys), tsdf_amd.TSDFVolume(n, phys)
    trk = FrameToModelTracker(gv, W, H, weighting=(flags, z_ref))
    assert trk.weighting() == (flags, z_ref) and trk.window() == 0
    weights = torch.empty(W * H, dtype=torch.float32, device="cuda")
    for i in range(6):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED, noise=False)
        trk.process(d, initial_pose=cam.pose().astype(np.float64).reshape(4, 4).T if i == 0 else None)
        _, filtered = trk.last_icp_inputs()
        used = Cam(trk.camera.pose(), trk.camera.inverse_pose(), trk.camera.k(), trk.camera.kinv())
        fd = torch.from_numpy(filtered.view(np.int16).copy()).cuda()
        torch.cuda.synchronize()
        tsdf_amd.depth_weights_device(W, H, fd.data_ptr(), used.kinv(), flags, z_ref, weights.data_ptr())
        torch.cuda.synchronize()
        tv.integrate_weighted_device(fd.data_ptr(), weights.data_ptr(), W, H, used)
        tv.synchronize()
    trk.synchronize()
    assert gv.weight_storage() == (32, False)
    got = gv.get_weight_data()
    assert (got > 0).sum() > 10000 and np.any((got > 0) & (got != np.round(got)))
    assert_same_floats(got, tv.get_weight_data(), "tracker vs the calls by hand: weights")
    assert_same_floats(gv.get_distance_data(), tv.get_distance_data(), "tracker vs the calls by hand: distances")
    # weighting and a window exclude each other, in either order
    with pytest.raises(ValueError, match="weighting"):
        trk.set_window(3)
    assert trk.window() == 0
    trk.set_weighting(0)
    assert trk.weighting() == (0, 0.0)
    trk.set_window(3)
    with pytest.raises(ValueError, match="window"):
        trk.set_weighting(flags, z_ref)
    assert trk.weighting() == (0, 0.0)
    for bad_flags, bad_z in ((4, 1.0), (1, 0.0), (1, float("nan")), (3, float("inf"))):
        trk.set_window(0)
        with pytest.raises(ValueError, match="tsdf_tracker_set_weighting"):
            trk.set_weighting(bad_flags, bad_z)
    trk.close()


# ---- 13: refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals():
    import torch
    from tsdf_amd import _capi
    lib = _capi.lib
    gv = tsdf_amd.TSDFVolume(SMALL, SMALL_PHYS)
    d, cam = frames(1)[0]
    before_w, before_d = gv.get_weight_data(), gv.get_distance_data()
    dd = torch.from_numpy(d.view(np.int16).copy()).cuda()
    pp = torch.ones(W * H, dtype=torch.float32, device="cuda")
    rgb = torch.zeros(W * H * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="tsdf_integrate_weighted: null argument"):
        gv.integrate_weighted_device(dd.data_ptr(), 0, W, H, cam)
    with pytest.raises(ValueError, match="tsdf_integrate_weighted: null argument"):
        gv.integrate_weighted_device(0, pp.data_ptr(), W, H, cam)
    with pytest.raises(ValueError, match="empty depth map"):
        gv.integrate_weighted_device(dd.data_ptr(), pp.data_ptr(), 0, H, cam)
    with pytest.raises(ValueError):
        gv.integrate_weighted(d, None, W, H, cam)
    with pytest.raises(ValueError):
        gv.integrate_weighted(d, np.ones(5, np.float32), W, H, cam)
    fp = C.POINTER(C.c_float)
    m = [np.array(a, np.float32) for a in (cam.pose(), cam.inverse_pose(), cam.k(), cam.kinv())]
    ptr = lambda a: a.ctypes.data_as(fp)
    assert lib.tsdf_integrate_weighted(gv._h, d.ctypes.data, None, None, W, H, ptr(m[0]), ptr(m[1]), ptr(m[2]), ptr(m[3])) == _capi.TSDF_ERR_INVALID
    assert lib.tsdf_integrate_weighted(gv._h, d.ctypes.data, np.ones(W * H, np.float32).ctypes.data, None, W, H, ptr(m[0]), None, ptr(m[2]),
                                       ptr(m[3])) == _capi.TSDF_ERR_INVALID
    # colour on a volume without colour, device and host
    with pytest.raises(ValueError, match="colour is not enabled"):
        gv.integrate_weighted_device(dd.data_ptr(), pp.data_ptr(), W, H, cam, rgb_ptr=rgb.data_ptr())
    with pytest.raises(ValueError, match="colour is not enabled"):
        gv.integrate_weighted(d, np.ones(W * H, np.float32), W, H, cam, rgb=np.zeros(W * H * 3, np.uint8))
    assert gv.weight_storage() == tsdf_amd.TSDFVolume(SMALL, SMALL_PHYS).weight_storage()   # a refused call does not widen
    assert_same_floats(gv.get_weight_data(), before_w, "refused calls: weights")
    assert_same_floats(gv.get_distance_data(), before_d, "refused calls: distances")
    # the models
    out = torch.empty(W * H, dtype=torch.float32, device="cuda")
    kinv = cam.kinv()
    for kw, word in [(dict(flags=4), "unknown flag bits"), (dict(flags=7), "unknown flag bits"), (dict(flags=1, z_ref=0.0), "z_ref"),
                     (dict(flags=1, z_ref=-1.0), "z_ref"), (dict(flags=3, z_ref=float("nan")), "z_ref"), (dict(flags=1, z_ref=float("inf")), "z_ref"),
                     (dict(depth=0), "null argument"), (dict(out=0), "null argument"), (dict(width=0), "bad image size"),
                     (dict(width=65536), "bad image size")]:
        a = dict(width=W, height=H, depth=dd.data_ptr(), flags=0, z_ref=1000.0, out=out.data_ptr())
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            tsdf_amd.depth_weights_device(a["width"], a["height"], a["depth"], kinv, a["flags"], a["z_ref"], a["out"])
    with pytest.raises(ValueError, match="unknown flag bits"):
        tsdf_amd.depth_weights(d, W, H, kinv, flags=8)
    tsdf_amd.depth_weights_device(W, H, dd.data_ptr(), kinv, 2, 0.0, out.data_ptr())      # z_ref is only read with the inverse-square flag
    torch.cuda.synchronize()
