"""The weight cap (include/tsdf_amd.h, "weight cap"): integrate stores min(weight + 1, cap) and divides by
weight + 1 as ever.

Reference (tests/weight_cap_ref.py): one oracle integrate, then a clamp of the oracle's weight array.  Every comparison is bit for
bit.  Grid as in tests/test_weight_storage.py: a partial last brick layer, 80 rows, x past one wave.
"""
import numpy as np
import pytest

import tsdf_amd
from tests import colour_ref
from tests.helpers import H, W, Cam, assert_same_floats, camera_at
from tests.weight_cap_ref import oracle_step
from tsdf_amd import synth

pytestmark = pytest.mark.gpu
SIZE, PHYS = (96, 80, 72), (3000.0, 2500.0, 2250.0)
SEED = 0x5EED0A01
PERIOD = 200          # a slow orbit: consecutive frames see nearly the same voxels, so counts grow by one a frame
# frames per cap, so that the UNCLAMPED oracle reaches cap + 4 somewhere (asserted in the test; checked on the CPU beforehand)
N_FRAMES = {1: 6, 2: 8, 15: 24, 255: 8}


def frames(n, seed=SEED):
    return [synth.depth_frame(i, PERIOD, seed=seed) for i in range(n)]


def start_weights(cap, n):
    """cap 255: counts of 253 with every 7th at 3 (tests/test_weight_storage.py); the small caps start from a cleared volume."""
    if cap != 255:
        return None
    w = np.full(n, 253.0, np.float32)
    w[::7] = 3.0
    return w


def same(gv, ov, what):
    assert_same_floats(gv.get_weight_data(), ov.weight, what + ": weights")
    assert_same_floats(gv.get_distance_data(), ov.dist, what + ": distances")


def plain_step(oracle, ov, d, cam):
    ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())


def run_stream(oracle, gv, ov, free, cap, fr, what, per_frame=True):
    """gv (capped) against ov (clamped oracle) frame by frame; `free` is the oracle without the clamp, which must pass cap + 4."""
    for i, (d, cam) in enumerate(fr):
        gv.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, cap)
        plain_step(oracle, free, d, cam)
        if per_frame or i + 1 == len(fr):
            same(gv, ov, "%s, cap %d, frame %d" % (what, cap, i))
    assert free.weight[free.weight < 1e5].max() >= cap + 4, "the cap never binds: the stream is too short"


def trio(oracle, size=SIZE, phys=PHYS):
    return tsdf_amd.TSDFVolume(size, phys), oracle.Volume(size, phys), oracle.Volume(size, phys)


# ---- 1: parity per frame, every storage and kernel --------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("cap", [1, 2, 15, 255])
def test_capped_stream_equals_the_clamped_oracle_in_every_storage(oracle, cap, bits):
    """8 bits: integrate_packed_capped_kernel<*, 8>; forced 16: <*, 16>; forced 32: integrate_capped_kernel<false, *, true>."""
    gv, ov, free = trio(oracle)
    w = start_weights(cap, gv.resident_voxels())
    if w is not None:
        for v in (gv, ov, free):
            v.set_weight_data(w)
    if bits != 8:
        gv.set_weight_storage(bits)
    gv.set_weight_cap(cap)
    assert gv.weight_cap() == cap
    run_stream(oracle, gv, ov, free, cap, frames(N_FRAMES[cap]), "%d-bit" % bits)
    assert gv.weight_storage() == (bits, False)
    assert gv.get_weight_data().max() == float(cap)


def test_capped_stream_on_pinned_fp32_weights(oracle):
    gv, ov, free = trio(oracle)
    assert gv.weight_data() and gv.weight_storage() == (32, True)
    gv.set_weight_cap(15)
    run_stream(oracle, gv, ov, free, 15, frames(N_FRAMES[15]), "pinned fp32", per_frame=False)
    assert gv.weight_storage() == (32, True)


def test_capped_stream_with_a_general_camera(oracle):
    """Skewed K: integrate_capped_kernel<false, *, false>."""
    gv, ov, free = trio(oracle)
    gv.set_weight_cap(15)
    fr = []
    for d, cam in frames(N_FRAMES[15]):
        k = np.array(cam.k(), np.float32).copy()
        k[3] = 0.02                           # column-major: K[0][1], a skew term -- not the standard shape
        kinv = np.linalg.inv(k.reshape(3, 3).T.astype(np.float64)).T.astype(np.float32).reshape(-1)
        fr.append((d, Cam(cam.pose(), cam.inverse_pose(), k, kinv)))
    run_stream(oracle, gv, ov, free, 15, fr, "skewed intrinsics", per_frame=False)
    assert gv.weight_storage() == (32, False)


def test_capped_stream_with_explicit_deformation_nodes(oracle):
    """set_deformation of the regular grid plus a perturbation: integrate_capped_kernel<true, *, false>."""
    size, phys = (40, 36, 33), (1200.0, 1080.0, 990.0)
    gv, ov, free = trio(oracle, size, phys)
    vs = ov.voxel_size()
    zz, yy, xx = np.meshgrid(np.arange(size[2]), np.arange(size[1]), np.arange(size[0]), indexing="ij")
    tr = np.stack([(xx + 0.5) * vs[0], (yy + 0.5) * vs[1], (zz + 0.5) * vs[2]], -1).astype(np.float32)
    tr += np.random.RandomState(3).uniform(-10, 10, tr.shape).astype(np.float32)
    ov.translation = free.translation = np.ascontiguousarray(tr.reshape(-1))
    gv.set_deformation(np.concatenate([tr.reshape(-1, 3), np.zeros((tr.size // 3, 3), np.float32)], axis=1))
    gv.set_weight_cap(2)
    cam = camera_at((600, 540, -900))
    fr = [(synth.depth_frame(i, PERIOD, seed=SEED)[0], cam) for i in range(N_FRAMES[2])]
    run_stream(oracle, gv, ov, free, 2, fr, "explicit nodes")
    assert gv.weight_storage()[0] == 32


def test_capped_stream_on_weights_that_are_not_counts(oracle):
    """2.5, 14.75 and 1e6 in fp32, cap 15: the comparison form -- 2.5 -> 3.5 ... -> 14.5 -> 15, 14.75 -> 15, 1e6 -> 15 where updated."""
    gv, ov, free = trio(oracle)
    n = gv.resident_voxels()
    w = np.array([2.5, 14.75, 1e6], np.float32)[np.arange(n) % 3]
    for v in (gv, ov, free):
        v.set_weight_data(w)
    assert gv.weight_storage() == (32, False)
    gv.set_weight_cap(15)
    run_stream(oracle, gv, ov, free, 15, frames(N_FRAMES[15]), "fractions", per_frame=False)
    got = gv.get_weight_data()
    assert set(np.unique(got[1::3])) == {np.float32(14.75), np.float32(15.0)}
    assert set(np.unique(got[2::3])) == {np.float32(1e6), np.float32(15.0)}


# ---- 2: storage -----------------------------------------------------------------------------------------------------------

def test_a_cap_of_at_most_255_keeps_the_bytes(oracle):
    gv, ov, free = trio(oracle)
    twin = tsdf_amd.TSDFVolume(SIZE, PHYS)
    w = start_weights(255, gv.resident_voxels())
    for v in (gv, ov, free, twin):
        v.set_weight_data(w)
    gv.set_weight_cap(255)
    fr = frames(6)
    for i, (d, cam) in enumerate(fr):
        gv.integrate(d, W, H, cam)
        twin.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, 255)
        assert gv.weight_storage() == (8, False), "frame %d" % i
    same(gv, ov, "253 + 6 under cap 255")
    assert gv.get_weight_data().max() == 255.0
    assert twin.weight_storage() == (16, False) and twin.get_weight_data().max() > 255.0


def test_a_cap_above_255_widens_to_16_bits_and_stops_there(oracle):
    gv, ov, free = trio(oracle)
    n = gv.resident_voxels()
    w = start_weights(255, n)
    for v in (gv, ov):
        v.set_weight_data(w)
    gv.set_weight_cap(300)
    fr = frames(4)
    for d, cam in [fr[0]] * 52:                              # (one pose: every voxel in view is updated 52 times)
        gv.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, 300)
    assert gv.weight_storage() == (16, False)
    same(gv, ov, "253 + 52 under cap 300")
    assert gv.get_weight_data().max() == 300.0
    # cap 65535 from 65534 in 16 bits: stays 16
    w = np.full(n, 65534.0, np.float32)
    w[::5] = 300.0
    gv.set_weight_data(w); ov.set_weight_data(w)
    gv.set_weight_cap(65535)
    for d, cam in fr[:4]:
        gv.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, 65535)
        assert gv.weight_storage() == (16, False)
    same(gv, ov, "65534 + 4 under cap 65535")
    assert gv.get_weight_data().max() == 65535.0


# ---- 3: no carry between the fields of a packed word -----------------------------------------------------------------------

@pytest.mark.parametrize("bits,top", [(8, 255), (16, 65535)])
def test_a_saturated_field_does_not_carry_into_its_neighbour(oracle, bits, top):
    """Planes 4g .. 4g + 3 (2g, 2g + 1) of one (x, y) share a dword: top, 0, 1, top - 1 plane after plane puts a saturated count
    beside an empty one in every word."""
    gv, ov, free = trio(oracle)
    n = gv.resident_voxels()
    per = n // SIZE[2]
    w0 = np.array([top, 0, 1, top - 1], np.float32)[(np.arange(n) // per) % 4]
    for v in (gv, ov, free):
        v.set_weight_data(w0)
    assert gv.weight_storage()[0] == bits
    gv.set_weight_cap(top)
    for d, cam in frames(2):
        gv.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, top)
        plain_step(oracle, free, d, cam)
    assert gv.weight_storage()[0] == bits
    same(gv, ov, "%d-bit fields" % bits)
    n_updates = free.weight - w0                       # (exact: integers below 2^24)
    assert n_updates.max() == 2.0
    assert_same_floats(gv.get_weight_data(), np.minimum(w0 + n_updates, np.float32(top)), "each plane its own min(w + updates, cap)")


# ---- 4: weights above the cap ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 32])
def test_a_weight_above_the_cap_blends_as_it_is_and_comes_out_as_the_cap(oracle, bits):
    gv, ov, free = trio(oracle)
    w = np.full(gv.resident_voxels(), 40.0, np.float32)
    gv.set_weight_data(w); free.set_weight_data(w)
    if bits != 8:
        gv.set_weight_storage(bits)
    gv.set_weight_cap(15)
    d, cam = frames(1)[0]
    gv.integrate(d, W, H, cam)
    plain_step(oracle, free, d, cam)
    updated = free.weight == 41.0
    assert 1000 < updated.sum() < updated.size
    assert_same_floats(gv.get_weight_data(), np.where(updated, np.float32(15.0), np.float32(40.0)), "15 where updated, 40 elsewhere")
    assert_same_floats(gv.get_distance_data(), free.dist, "the blend used the prior weight 40")


# ---- 5: switching ---------------------------------------------------------------------------------------------------------

def test_the_cap_can_be_switched_between_any_two_integrates(oracle):
    gv, ov, _ = trio(oracle)
    fr = frames(33)
    gv.set_weight_cap(15)
    for d, cam in fr[:20]:
        gv.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, 15)
    same(gv, ov, "20 frames under cap 15")
    assert ov.weight.max() == 15.0
    gv.set_weight_cap(0)
    assert gv.weight_cap() == 0
    for d, cam in fr[20:30]:
        gv.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, 0)
    same(gv, ov, "10 more without a cap")
    assert ov.weight.max() == 25.0
    gv.set_weight_cap(4)
    for d, cam in fr[30:]:
        gv.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, 4)
    same(gv, ov, "3 more under cap 4")
    got = gv.get_weight_data()
    assert (got == 4.0).sum() > 1000 and got.max() > 4.0     # (fallen to 4 where updated; voxels out of view keep theirs)
    gv.clear(); ov.clear()
    assert gv.weight_cap() == 4                              # clear() keeps the cap
    for d, cam in fr[:6]:
        gv.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, 4)
    same(gv, ov, "after clear()")
    assert gv.get_weight_data().max() == 4.0
    with pytest.raises(ValueError, match="65535"):
        gv.set_weight_cap(65536)
    assert gv.weight_cap() == 4


# ---- 6: colour ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 32])
def test_colour_integrate_with_a_cap(oracle, bits):
    """8: integrate_packed_colour_capped_kernel; 32: integrate_capped_kernel and the separate colour pass.  Distances and weights
    are the capped plain integrate's, colour words the uncapped reference's."""
    gv, tv = tsdf_amd.TSDFVolume(SIZE, PHYS), tsdf_amd.TSDFVolume(SIZE, PHYS)
    ov = oracle.Volume(SIZE, PHYS)
    gv.enable_colour()
    for v in (gv, tv):
        if bits != 8:
            v.set_weight_storage(bits)
        v.set_weight_cap(15)
    geom = colour_ref.geometry(gv)
    colour = np.zeros(gv.resident_voxels(), np.uint32)
    for i in range(N_FRAMES[15]):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        rgb, _ = synth.colour_frame(i, PERIOD, seed=SEED)
        gv.integrate_colour(d, rgb, W, H, cam)
        tv.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, 15)
        colour, _, _ = colour_ref.integrate_colour(oracle, colour, geom, d, rgb, W, H, cam)
    assert gv.weight_storage()[0] == bits
    assert ov.weight.max() == 15.0
    same(gv, ov, "integrate_colour under cap 15 vs the clamped oracle")
    assert_same_floats(gv.get_weight_data(), tv.get_weight_data(), "vs the capped plain integrate: weights")
    assert_same_floats(gv.get_distance_data(), tv.get_distance_data(), "vs the capped plain integrate: distances")
    got = gv.get_colour_data()
    bad = np.nonzero(got != colour)[0]
    assert bad.size == 0, "%d colour words differ, first at %d: %08x vs %08x" % (bad.size, bad[0], got[bad[0]], colour[bad[0]])
    assert int((got >> 24).max()) > 15                       # (the colour count has its own saturation, at 255)


# ---- 7: counting ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 32])
def test_updated_voxels_are_counted_capped_or_not(oracle, bits):
    gv, tv = tsdf_amd.TSDFVolume(SIZE, PHYS), tsdf_amd.TSDFVolume(SIZE, PHYS)
    ov = oracle.Volume(SIZE, PHYS)
    for v in (gv, tv):
        if bits != 8:
            v.set_weight_storage(bits)
        v.set_counting(True)
    gv.set_weight_cap(2)
    for i, (d, cam) in enumerate(frames(8)):
        gv.integrate(d, W, H, cam)
        tv.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, 2)
        assert gv.last_updated_voxels() == tv.last_updated_voxels() > 1000, "frame %d" % i
        assert gv.last_distance_stores() <= gv.last_updated_voxels()
    same(gv, ov, "counting kernels under cap 2")
    assert gv.get_weight_data().max() == 2.0


# ---- 8: ray cast after saturation ------------------------------------------------------------------------------------------

def test_raycast_of_a_saturated_volume(oracle):
    """After the stream of case 1 under cap 15 (whole bricks then store no weight, many no distance either) the picture is the clamped
    oracle's: the occupancy flags and `touched` marks are right."""
    gv, ov, free = trio(oracle)
    gv.set_weight_cap(15)
    fr = frames(N_FRAMES[15] + 8)
    run_stream(oracle, gv, ov, free, 15, fr, "stream", per_frame=False)
    for cam in (fr[-1][1], fr[0][1]):
        V, N = gv.raycast(W, H, cam)
        Vo, No = ov.raycast(W, H, cam.pose(), cam.kinv(), nthreads=oracle.max_threads())
        assert (~np.isnan(Vo[:, 0])).sum() > 1000
        assert_same_floats(V, Vo, "vertices")
        assert_same_floats(N, No, "normals")
    for a, b, what in zip(gv.occupancy_data(), gv.occupancy_data(force_rebuild=True), ("fine", "cell", "reach")):
        assert np.all(a >= b), "occupancy %s: a flag the distances need is missing" % what


# ---- 9: the per-frame drivers ---------------------------------------------------------------------------------------------

def test_pipeline_step_honours_the_cap(oracle):
    import torch
    from tsdf_amd.pipeline import FusionPipeline
    gv, tv = tsdf_amd.TSDFVolume(SIZE, PHYS), tsdf_amd.TSDFVolume(SIZE, PHYS)
    ov = oracle.Volume(SIZE, PHYS)
    for v in (gv, tv):
        v.set_weight_cap(15)
    fr = frames(24)
    pipe = FusionPipeline(gv, tsdf_amd.BilateralFilter(30.0, 4.5), tsdf_amd.GPURaycaster(W, H), W, H, overlap=True)
    bufs = [torch.from_numpy(d.view(np.int16).copy()).cuda() for d, _ in fr]
    vert = torch.empty((H * W, 3), dtype=torch.float32, device="cuda")
    norm = torch.empty_like(vert)
    filt = tsdf_amd.BilateralFilter(30.0, 4.5)
    for i, (d, cam) in enumerate(fr):
        nxt = bufs[i + 1].data_ptr() if i + 1 < len(fr) else None
        pipe.step(bufs[i].data_ptr(), cam, vert.data_ptr(), norm.data_ptr(), nxt, fr[i + 1][1] if nxt else None)
        f = d.copy()
        filt.filter(f, W, H)
        fd = torch.from_numpy(f.view(np.int16)).cuda()
        tv.integrate_device(fd.data_ptr(), W, H, cam)
        tv.synchronize()
        oracle_step(oracle, ov, f, cam, 15)
    pipe.synchronize()
    assert ov.weight.max() == 15.0
    assert_same_floats(gv.get_weight_data(), tv.get_weight_data(), "pipeline vs sequential integrate_device: weights")
    assert_same_floats(gv.get_distance_data(), tv.get_distance_data(), "pipeline vs sequential integrate_device: distances")
    same(gv, ov, "pipeline vs the clamped oracle")
    Vt, _ = tv.raycast(W, H, fr[-1][1])
    assert_same_floats(vert.cpu().numpy(), Vt, "last vertex map")
    assert gv.weight_storage() == (8, False)
    pipe.close()


def test_the_tracker_integrates_with_the_cap():
    from tsdf_amd.tracking import FrameToModelTracker
    gv = tsdf_amd.TSDFVolume((128,) * 3, (3000.0,) * 3)
    gv.set_weight_cap(3)
    trk = FrameToModelTracker(gv, W, H)
    for i in range(8):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED, noise=False)
        trk.process(d, initial_pose=cam.pose().astype(np.float64).reshape(4, 4).T if i == 0 else None)
    trk.close()
    assert gv.get_weight_data().max() == 3.0


def test_two_capped_slabs_are_the_capped_volume(oracle):
    size, phys = (64, 48, 70), (2000.0, 1500.0, 2187.5)
    whole, ov = tsdf_amd.TSDFVolume(size, phys), oracle.Volume(size, phys)
    whole.set_weight_cap(2)
    fr = frames(6, seed=0x5EED0A02)
    for d, cam in fr:
        whole.integrate(d, W, H, cam)
        oracle_step(oracle, ov, d, cam, 2)
    same(whole, ov, "whole volume")
    assert ov.weight.max() == 2.0
    wd, ww = whole.get_distance_data().reshape(size[2], -1), whole.get_weight_data().reshape(size[2], -1)
    parts_d, parts_w = [], []
    for lo, hi in ((0, 37), (37, 70)):
        s = tsdf_amd.TSDFVolume(size, phys, slab=(lo, hi))
        s.set_weight_cap(2)
        for d, cam in fr:
            s.integrate(d, W, H, cam)
        a = s.info().z_store_begin
        n_planes = s.info().z_store_end - a
        parts_d.append(s.get_distance_data().reshape(n_planes, -1)[lo - a:hi - a])
        parts_w.append(s.get_weight_data().reshape(n_planes, -1)[lo - a:hi - a])
    assert_same_floats(np.concatenate(parts_d), wd, "slabs, concatenated: distances")
    assert_same_floats(np.concatenate(parts_w), ww, "slabs, concatenated: weights")


# ---- 10: what the feature is for ---------------------------------------------------------------------------------------------

def test_a_capped_volume_follows_a_wall_that_moves(oracle):
    """128^3 / 3000 mm, a fixed camera on the -z side looking along +z.  200 frames of a wall, then 64 of a wall 500 mm nearer.  A voxel
    s behind the new wall (0 < s <= trunc) holds trunc r^m - s (1 - r^m), r = 15 / 16, after m new frames under cap 15: at m = 64,
    r^m < 0.017, negative for every s > 0.017 trunc -- the zero crossing is at the near wall.  Uncapped it holds
    (200 trunc - 64 s) / 264 > 0: no crossing there, the ray goes on to the far wall.  A crossing found between two samples lies
    within two voxel sizes of the wall along z.  The camera stands 4 m in front of the grid, so that the whole grid lies inside its
    frustum: every ray that meets the grid runs through voxels the frames updated (with the camera nearer, the rays of the image's
    corner pixels interpolate with voxels outside the frustum and find no crossing at the near wall; the CPU oracle shows the same).
    Checked on the clamped CPU oracle beforehand: the crossings lie within 1.7 mm of the walls, the bound is 46.9 mm."""
    n, phys = 128, 3000.0
    gv, tv = tsdf_amd.TSDFVolume((n,) * 3, (phys,) * 3), tsdf_amd.TSDFVolume((n,) * 3, (phys,) * 3)
    ov = oracle.Volume((n,) * 3, (phys,) * 3)
    gv.set_weight_cap(15)
    cam_z = -4000.0
    cam = camera_at((1500.0, 1500.0, cam_z))
    far, near = 5800, 5300                                   # depth in mm: world z = 1800 and 1300
    for depth_mm, count in ((far, 200), (near, 64)):
        d = synth.wall_depth(depth_mm)
        for _ in range(count):
            gv.integrate(d, W, H, cam)
            tv.integrate(d, W, H, cam)
            oracle_step(oracle, ov, d, cam, 15)
    assert gv.weight_storage() == (8, False) and tv.weight_storage() == (16, False)
    same(gv, ov, "264 frames under cap 15")
    vs = phys / n
    Vg, Ng = gv.raycast(W, H, cam)
    Vt, _ = tv.raycast(W, H, cam)
    Vo, No = ov.raycast(W, H, cam.pose(), cam.kinv(), nthreads=oracle.max_threads())
    assert_same_floats(Vg, Vo, "the capped picture")
    assert_same_floats(Ng, No, "the capped picture's normals")
    for V, wall_z, what in ((Vg, near + cam_z, "capped: the near wall"), (Vt, far + cam_z, "uncapped: the far wall")):
        hit = ~np.isnan(V[:, 0])
        assert hit.sum() > 10000, what
        off = np.abs(V[hit, 2] - wall_z)
        print("%s: %d hits, |z - wall| max %.3f mm (bound %.3f)" % (what, hit.sum(), off.max(), 2 * vs))
        assert off.max() <= 2 * vs, what
