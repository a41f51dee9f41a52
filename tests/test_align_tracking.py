"""The tracked loop with field alignment in place of the model ray cast and ICP (FrameToModelTracker(method="field"),
tsdf_tracker_align_field): eight noisy synthetic frames at 128^3, judged against what method="icp" reaches on the same frames in the
same test.  The two minimise different costs (squared field distance against point-to-plane distance to a rendered model), so the
field tracker may end up to twice as far from the truth as ICP, no further.  The trajectory error is the largest distance between a
tracked camera position and the true one (mm)."""
import numpy as np
import pytest

import tsdf_amd
from tsdf_amd import synth
from tsdf_amd.tracking import FrameToModelTracker

pytestmark = pytest.mark.gpu
W, H = synth.WIDTH, synth.HEIGHT
N, FRAMES, STREAM, SEED = 128, 8, 200, 0x5EED0005


def rotation_angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0)))


def track(data, **kwargs):
    vol = tsdf_amd.TSDFVolume((N, N, N), (3000.0,) * 3)
    tracker = FrameToModelTracker(vol, W, H, **kwargs)
    poses, inliers = [], []
    for i, (depth, cam) in enumerate(data):
        truth = cam.pose().astype(np.float64).reshape(4, 4).T
        poses.append(tracker.process(depth, initial_pose=truth if i == 0 else None))
        inliers.append(tracker.last_inliers)
    tracker.close()
    vol.close()
    return np.stack(poses), inliers


def errors(poses, data):
    truth = [cam.pose().astype(np.float64).reshape(4, 4).T for _, cam in data]
    return (max(float(np.linalg.norm(p[:3, 3] - t[:3, 3])) for p, t in zip(poses, truth)),
            max(rotation_angle(p[:3, :3], t[:3, :3]) for p, t in zip(poses, truth)))


def test_field_tracking_is_no_worse_than_twice_icp():
    data = [synth.depth_frame(i, STREAM, seed=SEED) for i in range(FRAMES)]
    moved = float(np.linalg.norm(data[-1][1].pose().reshape(4, 4).T[:3, 3] - data[0][1].pose().reshape(4, 4).T[:3, 3]))
    assert moved > 20.0                                   # the camera really moved (mm)
    default, _ = track(data)
    icp, _ = track(data, method="icp")
    assert np.array_equal(default, icp), "method='icp' is not the tracker built without the argument"
    field, inliers = track(data, method="field")
    icp_t, icp_r = errors(icp, data)
    field_t, field_r = errors(field, data)
    print("trajectory error over %d frames (camera moved %.1f mm): icp %.3f mm / %.5f rad, field %.3f mm / %.5f rad; field inliers %s"
          % (FRAMES, moved, icp_t, icp_r, field_t, field_r, [int(i) for i in inliers[1:]]))
    assert all(i > 0.2 * W * H for i in inliers[1:])      # it saw the surface, frame after frame
    assert not np.array_equal(field, icp)
    for p in field:
        assert np.allclose(p[:3, :3] @ p[:3, :3].T, np.eye(3), atol=1e-5)
    assert field_t <= 2.0 * icp_t, (field_t, icp_t)


def test_a_tracker_refuses_an_unknown_method():
    vol = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3)
    with pytest.raises(ValueError):
        FrameToModelTracker(vol, W, H, method="both")
    vol.close()
