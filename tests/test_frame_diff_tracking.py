"""GPU: dynamic rejection in the tracked loop (include/tsdf_amd.h, tsdf_tracker_set_dynamic_rejection) on a 64^3 volume and 64 x 48
frames at ground-truth cameras.

Off: the tracker's volume is the one the plain calls build.  On: after every frame the volume equals, bit for bit, a twin volume that
integrates the frame masked by the CPU reference (tests/frame_diff_ref.py on the twin's own model image) through the plain
tsdf_integrate_device; with a window the twin also takes the masked frames back out.

Condition on the scene, not a measurement of the code: on the frames without a disc the reference masks at most 1 % of the pixels with
f > 0.  With PARAMS below the reference masks 0 of them on every disc-free frame of the sequence (observed share 0.0 %: 64^3 voxels of
47 mm against a tolerance of 250 mm and blobs of at least 12 pixels).  tests/test_frame_diff_scene_host.py checks the same on the CPU,
with the oracle's filter, ray cast and integrate in place of the device's; here it is asserted on the device's own model image."""
import ctypes as C

import numpy as np
import pytest

from tests import frame_diff_ref as R

pytestmark = pytest.mark.gpu
SIZE, PHYS = (64,) * 3, (3000.0,) * 3
W, H = 64, 48
FRAMES, FIRST_DISC, PERIOD, SEED = 8, 3, 40, 0x5EEDD1FF
PARAMS = dict(tolerance=250, quadratic=0, connectivity=8, depth_step=100, min_pixels=12, dilate=2)
REF = dict(tolerance_mm=250, quadratic=0, connectivity=8, depth_step=100, min_pixels=12, dilate_px=2)


def small_camera():
    """The default depth camera's view on a 64 x 48 image: its intrinsics divided by ten."""
    import tsdf_amd
    return tsdf_amd.Camera(59.11, 59.01, 33.1, 23.46)


def frames():
    from tsdf_amd import synth
    out = []
    for i in range(FRAMES):
        cam = small_camera()
        if i >= FIRST_DISC:
            d, cam, disc = synth.moving_disc_frame(i, PERIOD, SEED, W, H, camera=cam, disc_depth=900, radius=7)
        else:
            d, cam = synth.depth_frame(i, PERIOD, SEED, W, H, camera=cam)
            disc = np.zeros(W * H, bool)
        out.append((d, cam, disc))
    return out


def same_volume(a, b, what):
    assert np.array_equal(a.get_weight_data().view(np.uint32), b.get_weight_data().view(np.uint32)), what + ": weights"
    assert np.array_equal(a.get_distance_data().view(np.uint32), b.get_distance_data().view(np.uint32)), what + ": distances"


def drive(trk, depth, cam):
    """One frame through tsdf_tracker_filter + tsdf_tracker_integrate at the given camera; returns the filtered frame."""
    import torch
    from tsdf_amd._capi import check, lib
    from tsdf_amd.pipeline import _matrices
    dd = torch.from_numpy(depth.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    check(lib.tsdf_tracker_filter(trk._h, C.c_void_p(dd.data_ptr())))
    m = _matrices(cam)
    check(lib.tsdf_tracker_integrate(trk._h, C.byref(m)))
    trk.synchronize()
    return trk.last_icp_inputs()[1].reshape(H, W)


def model_image(volume, cam):
    """tsdf_raycast_depth_device of the volume at the camera, downloaded."""
    import torch
    import tsdf_amd
    out = torch.zeros(W * H, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    tsdf_amd.GPURaycaster(W, H).render_to_depth_device(volume, cam, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16).reshape(H, W)


def integrate_plain(volume, frame, cam, remove=False):
    import torch
    dd = torch.from_numpy(np.ascontiguousarray(frame, np.uint16).reshape(-1).view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    (volume.deintegrate_device if remove else volume.integrate_device)(dd.data_ptr(), W, H, cam)
    torch.cuda.synchronize()
    volume.get_weight_data()   # (a blocking read: the volume's stream is done with dd)


def test_rejection_off_is_the_tracker_as_it_was():
    import tsdf_amd
    from tsdf_amd.tracking import FrameToModelTracker
    a, b = tsdf_amd.TSDFVolume(SIZE, PHYS), tsdf_amd.TSDFVolume(SIZE, PHYS)
    trk = FrameToModelTracker(a, W, H, camera=small_camera())
    assert trk.dynamic_rejection() is None
    trk.set_dynamic_rejection(**PARAMS)
    assert trk.dynamic_rejection() == PARAMS
    trk.set_dynamic_rejection(False)                       # (switched off again before the first frame)
    assert trk.dynamic_rejection() is None
    with pytest.raises(ValueError, match="dynamic rejection is off"):
        trk.last_rejection()
    for d, cam, _ in frames():
        filtered = drive(trk, d, cam)
        integrate_plain(b, filtered, cam)
    trk.close()
    same_volume(a, b, "rejection off")
    assert a.get_weight_data().max() == float(FRAMES)


@pytest.mark.parametrize("window", [0, 3])
def test_rejection_on_fuses_the_reference_masked_frames(window):
    import tsdf_amd
    from tsdf_amd.tracking import FrameToModelTracker
    a, twin = tsdf_amd.TSDFVolume(SIZE, PHYS), tsdf_amd.TSDFVolume(SIZE, PHYS)
    trk = FrameToModelTracker(a, W, H, camera=small_camera(), window=window, reject_dynamic=PARAMS)
    with pytest.raises(ValueError, match="no frame has been integrated"):
        trk.last_rejection()
    kept = []
    for i, (d, cam, disc) in enumerate(frames()):
        model = model_image(twin, cam)
        filtered = drive(trk, d, cam)
        want = R.run(filtered, model, **REF)
        counts, n_blobs, mask = trk.last_rejection()
        assert np.array_equal(counts, want["counts"]), i
        assert n_blobs == len(want["blobs"]) and np.array_equal(mask, want["mask"]), i
        integrate_plain(twin, want["frame_out"], cam)
        kept.append((want["frame_out"], cam))
        if window and i >= window:
            integrate_plain(twin, *kept[i - window], remove=True)
        same_volume(a, twin, "frame %d, window %d" % (i, window))
        seen = filtered > 0
        if i == 0:
            assert not want["mask"].any() and want["counts"][R.NEARER] == 0 and np.array_equal(want["frame_out"], filtered)
        if i < FIRST_DISC:
            # the condition on the scene: at most 1 % of the measured pixels masked where nothing moves
            assert want["mask"][seen].sum() <= 0.01 * seen.sum(), (i, int(want["mask"][seen].sum()), int(seen.sum()))
        elif window == 0:
            on_model = disc.reshape(H, W) & (model > 0) & seen
            assert on_model.sum() > 50 and want["mask"][on_model].all(), i
        # (With a window the frames that saw the wall behind the disc leave the volume and the model goes empty there, NO_MODEL: the few
        # disc pixels left over a model form blobs below min_pixels, which the rules do not mask.  With a window the volume is checked.)
    trk.close()
    assert a.get_weight_data().max() == float(window if window else FRAMES)


def test_the_refusals_of_the_setter():
    import tsdf_amd
    from tsdf_amd.tracking import FrameToModelTracker
    trk = FrameToModelTracker(tsdf_amd.TSDFVolume(SIZE, PHYS), W, H, camera=small_camera())
    with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
        trk.set_dynamic_rejection(connectivity=6)
    with pytest.raises(ValueError, match="above 32"):
        trk.set_dynamic_rejection(dilate=33)
    with pytest.raises(ValueError, match="unknown parameters"):
        trk.set_dynamic_rejection(tolerence=3)
    assert trk.dynamic_rejection() is None
    trk.close()
