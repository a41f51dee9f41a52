"""Windowed tracking (include/tsdf_amd.h, tsdf_tracker_set_window): with a window of n frames every integrate past
the n-th takes the oldest kept frame back out, so the volume holds exactly the last n frames.

The replay (tests/deintegrate_ref.py over the oracle) is given the filtered frames and the poses the tracker used, in the tracker's
order of operations: equal bit for bit.  A volume given only the last n frames saw other operations per voxel: equal weights, distances
within the header's per-operation bound."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests.deintegrate_ref import frame_set, remove
from tests.helpers import H, W, Cam, assert_same_floats
from tsdf_amd import synth
from tsdf_amd._capi import check, lib
from tsdf_amd.pipeline import _matrices
from tsdf_amd.tracking import FrameToModelTracker

pytestmark = pytest.mark.gpu
SIZE, PHYS = (128,) * 3, (3000.0,) * 3
SEED, PERIOD = 0x5EED0B04, 200
U = 2.0 ** -24


def start_pose(cam):
    return cam.pose().astype(np.float64).reshape(4, 4).T


def track(gv, m, window):
    """m synthetic frames through a tracker; returns the (filtered frame, camera) pairs it integrated."""
    trk = FrameToModelTracker(gv, W, H, window=window)
    assert trk.window() == window
    used = []
    for i in range(m):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED, noise=False)
        trk.process(d, initial_pose=start_pose(cam) if i == 0 else None)
        c = trk.camera
        used.append((trk.last_icp_inputs()[1].copy(), Cam(c.pose().copy(), c.inverse_pose().copy(), c.k().copy(), c.kinv().copy())))
    trk.close()
    return used


def test_a_window_of_n_frames_holds_exactly_the_last_n(oracle):
    n, m = 3, 8
    gv, ov = tsdf_amd.TSDFVolume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    used = track(gv, m, n)
    seen = np.zeros(ov.weight.size, np.float64)                 # integrates per voxel
    for i, (f, cam) in enumerate(used):
        ov.integrate(f, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
        seen += frame_set(oracle, ov, f, cam)[0]
        if i >= n:
            remove(ov, *frame_set(oracle, ov, *used[i - n]))
    assert ov.weight.max() == float(n)
    assert_same_floats(gv.get_weight_data(), ov.weight, "window %d over %d frames vs the replay: weights" % (n, m))
    assert_same_floats(gv.get_distance_data(), ov.dist, "window %d over %d frames vs the replay: distances" % (n, m))
    assert gv.weight_storage() == (8, False)
    # against a volume that was only ever given the last n frames: in the sum D * w every operation errs by at most 3 c u T at count
    # c <= n + 1 (header); a voxel seen a times had a integrates and a - w removals here and w integrates there: 2 a operations
    tv = tsdf_amd.TSDFVolume(SIZE, PHYS)
    for f, cam in used[m - n:]:
        tv.integrate(f, W, H, cam)
    w = tv.get_weight_data()
    assert_same_floats(gv.get_weight_data(), w, "vs the last %d frames: weights" % n)
    T = gv.truncation_distance()
    dev = np.abs(gv.get_distance_data().astype(np.float64) - tv.get_distance_data().astype(np.float64))
    bound = np.where(w > 0, 3 * (n + 1) * U * T * 2 * seen / np.maximum(w, 1), 0.0)
    print("vs the last %d frames: max deviation %.2f * 2^-23 * trunc, %d voxels removed from" % (n, dev.max() / T * 2 ** 23, int((seen > w).sum())))
    assert (seen > w).sum() > 1000 and np.all(dev <= bound)


def test_window_0_is_the_tracker_as_it_was():
    a, b = tsdf_amd.TSDFVolume(SIZE, PHYS), tsdf_amd.TSDFVolume(SIZE, PHYS)
    trk = FrameToModelTracker(a, W, H)
    assert trk.window() == 0
    trk.set_window(2); trk.set_window(0)                        # (switched off again before the first frame)
    plain = FrameToModelTracker(b, W, H)
    for i in range(5):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED, noise=False)
        pa = trk.process(d, initial_pose=start_pose(cam) if i == 0 else None)
        pb = plain.process(d, initial_pose=start_pose(cam) if i == 0 else None)
        assert np.array_equal(pa, pb)
    trk.close(); plain.close()
    assert_same_floats(a.get_weight_data(), b.get_weight_data(), "weights")
    assert_same_floats(a.get_distance_data(), b.get_distance_data(), "distances")
    assert a.get_weight_data().max() == 5.0


def test_colour_tracking_with_a_window_leaves_the_colours_as_without_one():
    """The same frames at the same (ground-truth) poses through tsdf_tracker_filter + tsdf_tracker_integrate_colour: the windowed
    volume's colour words are the unwindowed one's, its weights the last n frames'."""
    import torch
    vols = []
    for window in (2, 0):
        gv = tsdf_amd.TSDFVolume(SIZE, PHYS)
        gv.enable_colour()
        trk = FrameToModelTracker(gv, W, H, window=window)
        for i in range(5):
            d, cam = synth.depth_frame(i, PERIOD, seed=SEED, noise=False)
            rgb, _ = synth.colour_frame(i, PERIOD, seed=SEED)
            dd = torch.from_numpy(d.view(np.int16).copy()).cuda()
            cc = torch.from_numpy(np.ascontiguousarray(rgb, np.uint8).reshape(-1)).cuda()
            torch.cuda.synchronize()
            check(lib.tsdf_tracker_filter(trk._h, C.c_void_p(dd.data_ptr())))
            m = _matrices(cam)
            check(lib.tsdf_tracker_integrate_colour(trk._h, C.byref(m), C.c_void_p(cc.data_ptr())))
            trk.synchronize()
        trk.close()
        vols.append(gv)
    assert np.array_equal(vols[0].get_colour_data(), vols[1].get_colour_data()) and vols[0].get_colour_data().any()
    assert vols[0].get_weight_data().max() == 2.0 and vols[1].get_weight_data().max() == 5.0


def test_the_refusals():
    import torch
    gv = tsdf_amd.TSDFVolume((64,) * 3, PHYS)
    gv.set_weight_cap(15)
    with pytest.raises(ValueError, match="weight cap"):
        FrameToModelTracker(gv, W, H, window=3)
    gv.set_weight_cap(0)
    trk = FrameToModelTracker(gv, W, H, window=3)
    d, _ = synth.depth_frame(0, PERIOD, seed=SEED, noise=False)
    dd = torch.from_numpy(d.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    check(lib.tsdf_tracker_filter(trk._h, C.c_void_p(dd.data_ptr())))
    with pytest.raises(ValueError, match="between frames"):
        trk.set_window(5)
    assert trk.window() == 3
    with pytest.raises(MemoryError, match="ring"):
        m = _matrices(trk.camera)
        check(lib.tsdf_tracker_integrate(trk._h, C.byref(m)))
        trk.synchronize()
        trk.set_window(0xFFFFFFFF)                               # (2.6 PB)
    assert trk.window() == 0
    trk.close()
