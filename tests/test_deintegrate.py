"""De-integration (include/tsdf_amd.h, "de-integration"): tsdf_deintegrate takes a fused frame back out.

Reference (tests/deintegrate_ref.py): the frame's voxel set and tsdf values from one oracle integrate of the cleared grid, then the
header's formula in numpy fp32.  Every comparison is bit for bit.  Grid as in tests/test_weight_cap.py: a partial last brick layer, 80
rows, x past one wave.
"""
import numpy as np
import pytest

import tsdf_amd
from tests.deintegrate_ref import frame_set, oracle_remove
from tests.helpers import H, W, Cam, assert_same_floats, camera_at
from tests.test_fuzz_parity import random_camera, random_case, random_depth
from tsdf_amd import synth

pytestmark = pytest.mark.gpu
SIZE, PHYS = (96, 80, 72), (3000.0, 2500.0, 2250.0)
SEED, PERIOD = 0x5EED0B02, 200


def frames(n, seed=SEED):
    return [synth.depth_frame(i, PERIOD, seed=seed) for i in range(n)]


def same(gv, ov, what):
    assert_same_floats(gv.get_weight_data(), ov.weight, what + ": weights")
    assert_same_floats(gv.get_distance_data(), ov.dist, what + ": distances")


def both_integrate(oracle, gv, ov, d, cam, w=W, h=H):
    gv.integrate(d, w, h, cam)
    ov.integrate(d, w, h, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())


def both_remove(oracle, gv, ov, d, cam, w=W, h=H, counted=False):
    gv.deintegrate(d, w, h, cam)
    updated, stores = oracle_remove(oracle, ov, d, cam, w, h)
    if counted:
        assert (gv.last_updated_voxels(), gv.last_distance_stores()) == (updated, stores)
    return updated


def cleared(gv):
    w, d = gv.get_weight_data(), gv.get_distance_data()
    assert not w.view(np.uint32).any(), "%d weights are not +0" % np.count_nonzero(w.view(np.uint32))
    t = np.float32(gv.truncation_distance()).view(np.uint32)
    assert (d.view(np.uint32) == t).all(), "%d distances are not +trunc" % np.count_nonzero(d.view(np.uint32) != t)


# ---- 1: every storage, one removal then all of them, counters ---------------------------------------------------------------

@pytest.mark.parametrize("storage", ["8", "16", "32", "pinned"])
def test_removal_equals_the_reference_in_every_storage(oracle, storage):
    """8 / 16: integrate_packed_remove_kernel<*, 8 / 16>; 32 and pinned: integrate_remove_kernel<false, *, true>.  Counting on: the
    COUNT instances, counters against the reference's; the same stream with counting off runs in the cases below."""
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    if storage == "pinned":
        assert gv.weight_data() and gv.weight_storage() == (32, True)
    elif storage != "8":
        gv.set_weight_storage(int(storage))
    mode = gv.weight_storage()
    gv.set_counting(True)
    fr = frames(6)
    for d, cam in fr:
        both_integrate(oracle, gv, ov, d, cam)
    assert both_remove(oracle, gv, ov, *fr[2], counted=True) > 1000
    same(gv, ov, "%s: frame 2 of 6 removed" % storage)
    assert ov.weight.max() == 5.0
    for i in (5, 0, 3):
        both_remove(oracle, gv, ov, *fr[i], counted=True)
        same(gv, ov, "%s: then frame %d" % (storage, i))
    both_integrate(oracle, gv, ov, *fr[2])                       # re-integration at another place in the order
    same(gv, ov, "%s: frame 2 integrated again" % storage)
    for i in (1, 2, 4):
        both_remove(oracle, gv, ov, *fr[i], counted=True)
    same(gv, ov, "%s: all removed" % storage)
    cleared(gv)
    assert gv.weight_storage() == mode                           # neither widened nor narrowed


def test_removal_without_counting(oracle):
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    fr = frames(4)
    for d, cam in fr:
        both_integrate(oracle, gv, ov, d, cam)
    both_remove(oracle, gv, ov, *fr[0])
    same(gv, ov, "8-bit, no counting")
    gv.set_weight_storage(32)
    both_remove(oracle, gv, ov, *fr[3])
    same(gv, ov, "fp32, no counting")


# ---- 2: uploaded weights ----------------------------------------------------------------------------------------------------

def test_uploaded_weights_of_every_kind(oracle):
    """Non-integer, exactly 1, in (1, 2), below 1, 0 and NaN, with distances that no integrate produced; the frame was never
    integrated: !(w >= 1) stays untouched, the others follow the formula (1.0 -> the cleared state, 1.5 -> 0.5)."""
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    n = gv.resident_voxels()
    w = np.array([2.5, 1.0, 1.5, 0.5, 0.0, np.nan, 7.0], np.float32)[np.arange(n) % 7]
    D = (np.random.RandomState(1).uniform(-1, 1, n) * gv.truncation_distance()).astype(np.float32)
    for v in (gv, ov):
        v.set_weight_data(w)
        v.set_distance_data(D)
    assert gv.weight_storage() == (32, False)
    gv.set_counting(True)
    d, cam = frames(1)[0]
    in_set, _ = frame_set(oracle, ov, d, cam)
    both_remove(oracle, gv, ov, d, cam, counted=True)
    same(gv, ov, "uploaded fp32 weights")
    got_w, got_d = gv.get_weight_data(), gv.get_distance_data()
    for r, after in ((0, 1.5), (1, 0.0), (2, 0.5), (6, 6.0)):
        sel = in_set[r::7]
        assert sel.sum() > 100 and (got_w[r::7][sel] == np.float32(after)).all()
    assert (got_d[1::7][in_set[1::7]] == np.float32(gv.truncation_distance())).all()
    for r in (3, 4, 5):
        assert_same_floats(got_w[r::7], w[r::7], "weights that are not >= 1")
        assert_same_floats(got_d[r::7], D[r::7], "their distances")


@pytest.mark.parametrize("bits,top", [(8, 255), (16, 65535)])
def test_a_count_goes_down_in_its_own_field(oracle, bits, top):
    """Planes 4g .. 4g + 3 (2g, 2g + 1) of one (x, y) share a dword: top, 0, 1, top - 1 plane after plane puts 255 -> 254 beside a field
    at 0 (left alone, nothing borrowed) and one that goes 1 -> 0; then one integrate takes 254 back to 255."""
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    n = gv.resident_voxels()
    w0 = np.array([top, 0, 1, top - 1], np.float32)[(np.arange(n) // (n // SIZE[2])) % 4]
    D = (np.random.RandomState(2).uniform(-1, 1, n) * gv.truncation_distance()).astype(np.float32)
    for v in (gv, ov):
        v.set_weight_data(w0)
        v.set_distance_data(D)
    assert gv.weight_storage() == (bits, False)
    d, cam = frames(1)[0]
    in_set, _ = frame_set(oracle, ov, d, cam)
    both_remove(oracle, gv, ov, d, cam)
    same(gv, ov, "%d-bit fields" % bits)
    assert_same_floats(gv.get_weight_data(), np.where(in_set & (w0 >= 1), w0 - 1, w0), "each plane its own count")
    assert gv.weight_storage() == (bits, False)
    both_remove(oracle, gv, ov, d, cam)                          # the fields at top - 1 .. and those now at 0 stay
    same(gv, ov, "%d-bit fields, removed twice" % bits)
    both_integrate(oracle, gv, ov, d, cam)
    same(gv, ov, "%d-bit fields, integrated again" % bits)
    assert gv.weight_storage()[0] in (bits, 16 if bits == 8 else 32)


# ---- 3: grids, images, offsets, cameras ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(12))
def test_random_grids_images_offsets_and_cameras(oracle, seed):
    """tests/test_fuzz_parity.py's generator: grids of 5-72 voxels a side, images of 1-200 x 1-160 pixels, offsets moved and then
    cleared, cameras inside, beside and far from the grid.  Three frames in, one out, compare; the rest out, cleared."""
    rng = np.random.default_rng(0xDE1 + seed)
    dims, phys, width, height, offset = random_case(rng)
    gv, ov = tsdf_amd.TSDFVolume(dims, phys), oracle.Volume(dims, phys)
    if offset is not None:
        gv.offset(*offset); gv.clear()
        ov.offset(*offset); ov.clear()
        if seed % 2:                                             # moved again after clear(): the nodes keep the offset of the clear
            gv.offset(offset[0] + 33.0, offset[1] - 21.0, offset[2] + 5.0)
            ov.offset(offset[0] + 33.0, offset[1] - 21.0, offset[2] + 5.0)
    fr = []
    for _ in range(3):
        cam, dist = random_camera(rng, dims, phys, offset, width, height)
        fr.append((random_depth(rng, width, height, max(dist, 50.0)), cam))
        both_integrate(oracle, gv, ov, fr[-1][0], cam, width, height)
    what = "seed %d dims %s image %dx%d" % (seed, dims, width, height)
    both_remove(oracle, gv, ov, *fr[1], width, height)
    same(gv, ov, what + ", frame 1 removed")
    V, N = gv.raycast(width, height, fr[2][1])
    Vo, No = ov.raycast(width, height, fr[2][1].pose(), fr[2][1].kinv(), nthreads=oracle.max_threads())
    assert_same_floats(V, Vo, what + " vertices")
    assert_same_floats(N, No, what + " normals")
    for i in (2, 0):
        both_remove(oracle, gv, ov, *fr[i], width, height)
    same(gv, ov, what + ", all removed")
    cleared(gv)


def general_cameras(cam):
    """Skewed, K(2,2) != 1 and projective versions of `cam` (column-major matrices)."""
    out = []
    for kind in ("skew", "k22", "projective"):
        k = np.array(cam.k(), np.float32).copy()
        ip = np.array(cam.inverse_pose(), np.float32).copy()
        if kind == "skew":
            k[3] = 0.02                                          # K[0][1]
        elif kind == "k22":
            k[8] = 1.25
        else:
            ip[3], ip[15] = 1.0e-5, 1.05                         # last row of the inverse pose: (1e-5, 0, 0, 1.05)
        kinv = np.linalg.inv(k.reshape(3, 3).T.astype(np.float64)).T.astype(np.float32).reshape(-1)
        out.append((kind, Cam(cam.pose(), ip, k, kinv)))
    return out


def test_general_cameras(oracle):
    """integrate_remove_kernel<false, *, false>."""
    d, cam = frames(1)[0]
    d2, cam2 = frames(8)[7]
    for kind, gcam in general_cameras(cam):
        gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
        both_integrate(oracle, gv, ov, d2, cam2)
        both_integrate(oracle, gv, ov, d, gcam)
        both_integrate(oracle, gv, ov, d2, gcam)
        assert gv.weight_storage() == (32, False)
        assert both_remove(oracle, gv, ov, d, gcam) > 1000, kind
        same(gv, ov, kind + ": one removed")
        both_remove(oracle, gv, ov, d2, cam2)
        both_remove(oracle, gv, ov, d2, gcam)
        same(gv, ov, kind + ": all removed")
        cleared(gv)


def test_a_general_camera_on_packed_counts_takes_the_fp32_layout(oracle):
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    fr = frames(3)
    for d, cam in fr:
        both_integrate(oracle, gv, ov, d, cam)
    assert gv.weight_storage() == (8, False)
    kind, gcam = general_cameras(fr[0][1])[0]
    both_remove(oracle, gv, ov, fr[0][0], gcam)                 # (a frame that was not integrated at this camera)
    same(gv, ov, "skewed removal from 8-bit counts")
    assert gv.weight_storage() == (32, False)


def test_explicit_deformation_nodes(oracle):
    """integrate_remove_kernel<true, *, false>."""
    size, phys = (40, 36, 33), (1200.0, 1080.0, 990.0)
    gv, ov = tsdf_amd.TSDFVolume(size, phys), oracle.Volume(size, phys)
    vs = ov.voxel_size()
    zz, yy, xx = np.meshgrid(np.arange(size[2]), np.arange(size[1]), np.arange(size[0]), indexing="ij")
    tr = np.stack([(xx + 0.5) * vs[0], (yy + 0.5) * vs[1], (zz + 0.5) * vs[2]], -1).astype(np.float32)
    tr += np.random.RandomState(3).uniform(-10, 10, tr.shape).astype(np.float32)
    ov.translation = np.ascontiguousarray(tr.reshape(-1))
    gv.set_deformation(np.concatenate([tr.reshape(-1, 3), np.zeros((tr.size // 3, 3), np.float32)], axis=1))
    cam = camera_at((600, 540, -900))
    fr = [(synth.depth_frame(i, PERIOD, seed=SEED)[0], cam) for i in range(4)]
    for d, c in fr:
        both_integrate(oracle, gv, ov, d, c)
    assert both_remove(oracle, gv, ov, *fr[1]) > 1000
    same(gv, ov, "explicit nodes: one removed")
    for i in (0, 3, 2):
        both_remove(oracle, gv, ov, *fr[i])
    same(gv, ov, "explicit nodes: all removed")
    cleared(gv)


@pytest.mark.parametrize("parts", [2, 3, 8])
def test_slabs_take_out_their_own_planes(oracle, parts):
    from tsdf_amd import multi
    size, phys = (64, 48, 70), (2000.0, 1500.0, 2187.5)
    whole, ov = tsdf_amd.TSDFVolume(size, phys), oracle.Volume(size, phys)
    fr = frames(4, seed=0x5EED0B03)
    for d, cam in fr:
        both_integrate(oracle, whole, ov, d, cam)
    both_remove(oracle, whole, ov, *fr[1])
    same(whole, ov, "whole volume")
    wd, ww = whole.get_distance_data().reshape(size[2], -1), whole.get_weight_data().reshape(size[2], -1)
    for r in range(parts):
        lo, hi = multi.slab_range(size[2], parts, r)
        s = tsdf_amd.TSDFVolume(size, phys, slab=(lo, hi))
        for d, cam in fr:
            s.integrate(d, W, H, cam)
        s.deintegrate(fr[1][0], W, H, fr[1][1])
        a = s.info().z_store_begin
        n_planes = s.info().z_store_end - a
        assert_same_floats(s.get_distance_data().reshape(n_planes, -1)[lo - a:hi - a], wd[lo:hi], "slab %d of %d: distances" % (r, parts))
        assert_same_floats(s.get_weight_data().reshape(n_planes, -1)[lo - a:hi - a], ww[lo:hi], "slab %d of %d: weights" % (r, parts))
        for i in (0, 2, 3):
            s.deintegrate(fr[i][0], W, H, fr[i][1])
        cleared(s)


# ---- 4: colour, cap ---------------------------------------------------------------------------------------------------------

def test_colour_words_are_not_touched(oracle):
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    gv.enable_colour()
    fr = frames(3)
    for i, (d, cam) in enumerate(fr):
        rgb, _ = synth.colour_frame(i, PERIOD, seed=SEED)
        gv.integrate_colour(d, rgb, W, H, cam)
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    before = gv.get_colour_data().copy()
    assert before.any()
    both_remove(oracle, gv, ov, *fr[0])
    same(gv, ov, "colour volume")
    assert np.array_equal(gv.get_colour_data(), before)


def test_a_capped_volume_is_refused(oracle):
    gv = tsdf_amd.TSDFVolume(SIZE, PHYS)
    d, cam = frames(1)[0]
    gv.integrate(d, W, H, cam)
    gv.set_weight_cap(15)
    w0, d0 = gv.get_weight_data(), gv.get_distance_data()
    with pytest.raises(ValueError, match="weight cap"):
        gv.deintegrate(d, W, H, cam)
    assert_same_floats(gv.get_weight_data(), w0, "refused: weights")
    assert_same_floats(gv.get_distance_data(), d0, "refused: distances")
    gv.set_weight_cap(0)
    gv.deintegrate(d, W, H, cam)
    cleared(gv)


# ---- 5: full removal at size, packed kernels ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,count", [(128, 12), (512, 6)])
def test_removing_every_frame_gives_the_cleared_volume_back(n, count):
    import torch
    gv = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    fr = frames(count)
    bufs = [torch.from_numpy(d.view(np.int16).copy()).cuda() for d, _ in fr]
    torch.cuda.synchronize()
    for (d, cam), b in zip(fr, bufs):
        gv.integrate_device(b.data_ptr(), W, H, cam)
    gv.synchronize()
    assert gv.get_weight_data().max() == float(count) and gv.weight_storage() == (8, False)
    for i in np.random.RandomState(n).permutation(count):
        gv.deintegrate_device(bufs[i].data_ptr(), W, H, fr[i][1])
    gv.synchronize()
    cleared(gv)
    assert gv.weight_storage() == (8, False)


# ---- 6: the picture after removals ----------------------------------------------------------------------------------------------

def test_raycast_after_removals(oracle):
    """The occupancy flags stay a superset of what the distances need: the picture is the oracle's of the reference arrays, and the one
    the volume gives after a forced rebuild of its flags."""
    size, phys = (128,) * 3, (3000.0,) * 3
    gv, ov = tsdf_amd.TSDFVolume(size, phys), oracle.Volume(size, phys)
    fr = frames(10)
    for i, (d, cam) in enumerate(fr):
        both_integrate(oracle, gv, ov, d, cam)
        if i % 3 == 0:                                           # (a cast between integrates moves the flag refresh schedule)
            gv.raycast(W, H, cam)
    for i in (0, 1, 2, 9, 5):
        both_remove(oracle, gv, ov, *fr[i])
        cam = fr[i][1]
        V, N = gv.raycast(W, H, cam)
        Vo, No = ov.raycast(W, H, cam.pose(), cam.kinv(), nthreads=oracle.max_threads())
        assert (~np.isnan(Vo[:, 0])).sum() > 1000
        assert_same_floats(V, Vo, "after removing frame %d: vertices" % i)
        assert_same_floats(N, No, "after removing frame %d: normals" % i)
    same(gv, ov, "five of ten removed")
    lazy = gv.occupancy_data()
    rebuilt = gv.occupancy_data(force_rebuild=True)
    for a, b, what in zip(lazy, rebuilt, ("fine", "cell")):
        assert np.all(a >= b), "occupancy %s: a flag the distances need is missing" % what
    assert np.all(lazy[2] <= rebuilt[2]), "occupancy reach: a clear block larger than the distances allow"   # (0 = set, l = clear block size class)
    V2, N2 = gv.raycast(W, H, fr[5][1])
    assert_same_floats(V2, V, "after the forced rebuild: vertices")
    assert_same_floats(N2, N, "after the forced rebuild: normals")
