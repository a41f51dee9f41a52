"""The tracked loop with the colour term (FrameToModelTracker(method="field", colour_weight=W), tsdf_tracker_align_field_colour).

A camera translating along the textured wall of tests/align_colour_ref.py: nothing in the distance field holds the pose in the wall's
plane, so the plain field tracker stays where it was and drifts by the whole motion; with the colour term it follows.  And on the orbit
sequence of tests/test_align_tracking.py, where the geometry does constrain the pose, the colour term must not make things worse than
the spread between two orders of the same sums."""
import numpy as np
import pytest

import tsdf_amd
from tests import align_colour_ref as CR
from tests import align_ref as R
from tests.test_align_colour import assert_same_state, volume_state, wall_volume
from tests.test_align_tracking import FRAMES, N, SEED, STREAM, H, W, errors
from tsdf_amd import synth
from tsdf_amd.tracking import FrameToModelTracker

pytestmark = pytest.mark.gpu
WALL_FRAMES, WALL_MOVE = 6, (7.0, -5.0)          # mm a frame along the wall: 8.6 mm, well inside a sixth of the shortest wavelength


def wall_camera():
    return tsdf_amd.Camera(CR.WALL_F, CR.WALL_F, (CR.WALL_W - 1) / 2.0, (CR.WALL_H - 1) / 2.0)


def track_wall(colour_weight):
    s = CR.wall_scene()
    vol = wall_volume(s)
    tracker = FrameToModelTracker(vol, CR.WALL_W, CR.WALL_H, camera=wall_camera(), method="field", colour_weight=colour_weight,
                                  colour_gate=CR.WALL_COLOUR_GATE)
    poses, inliers = [], []
    for i in range(WALL_FRAMES):
        depth, rgb = CR.wall_frame((i * WALL_MOVE[0], i * WALL_MOVE[1]))
        poses.append(tracker.process(depth, initial_pose=np.eye(4) if i == 0 else None, rgb=rgb))
        inliers.append((tracker.last_inliers, tracker.last_colour_inliers))
    tracker.close()
    vol.close()
    return np.stack(poses), inliers


def test_the_colour_term_follows_a_camera_along_a_wall():
    moved = float(np.hypot(*WALL_MOVE)) * (WALL_FRAMES - 1)
    truth = np.array([WALL_MOVE[0], WALL_MOVE[1]]) * (WALL_FRAMES - 1)
    with_colour, inliers = track_wall(tsdf_amd.api.COLOUR_WEIGHT)
    without, plain_inliers = track_wall(0.0)
    drift = float(np.linalg.norm(with_colour[-1][:2, 3] - truth))
    plain_drift = float(np.linalg.norm(without[-1][:2, 3] - truth))
    print("wall, %d frames, camera moved %.1f mm in-plane: drift %.3f mm with colour (inliers %s), %.3f mm without"
          % (WALL_FRAMES, moved, drift, [(int(a), int(b)) for a, b in inliers[1:]], plain_drift))
    assert all(a > 0.5 * CR.WALL_W * CR.WALL_H and b > 0.5 * CR.WALL_W * CR.WALL_H for a, b in inliers[1:])
    assert all(a > 0.5 * CR.WALL_W * CR.WALL_H and b == 0 for a, b in plain_inliers[1:])
    assert drift <= 0.25 * moved
    assert plain_drift >= 0.75 * moved


def orbit(colour_weight):
    vol = tsdf_amd.TSDFVolume((N, N, N), (3000.0,) * 3)
    vol.enable_colour()
    tracker = FrameToModelTracker(vol, W, H, method="field", colour_weight=colour_weight)
    poses = []
    for i in range(FRAMES):
        depth, cam = synth.depth_frame(i, STREAM, seed=SEED)
        rgb, _ = synth.colour_frame(i, STREAM, seed=SEED)
        truth = cam.pose().astype(np.float64).reshape(4, 4).T
        poses.append(tracker.process(depth, initial_pose=truth if i == 0 else None, rgb=rgb))
    tracker.close()
    vol.close()
    return np.stack(poses)


def test_the_colour_term_does_not_hurt_where_the_geometry_holds(oracle):
    """The orbit of tests/test_align_tracking.py: with colour at the default weight the track ends no farther from the truth than
    without, plus the spread between two orders of summation: 8 x the distance between the colour reference chains of
    tests/align_colour_ref.py's fused scene summed in float64 and in ascending fp32, at that weight, computed here.

    Measured on an MI355X, end error in mm: 0.783433 without colour; 0.781443 / 0.779948 / 0.789413 / 0.823257 at weights 0.001 / 0.01 /
    0.1 / 1 (spreads 2.6e-04 / 2.7e-05 / 4.0e-05 / 4.0e-05).  Weights of 0.1 and more pull this noisy-depth track off by more than the
    bound allows, which is why the default is 0.01."""
    data = [synth.depth_frame(i, STREAM, seed=SEED) for i in range(FRAMES)]
    w = tsdf_amd.api.COLOUR_WEIGHT
    s = CR.fused_colour_scene(oracle)
    stages = [(s.points, s.intensity, 10)]
    spread = R.pose_distance(CR.chain(oracle, s, stages, s.T0, s.gate, tsdf_amd.api.COLOUR_GATE, w, order="f64")[0],
                             CR.chain(oracle, s, stages, s.T0, s.gate, tsdf_amd.api.COLOUR_GATE, w, order="ascending")[0])
    plain = orbit(0.0)
    colour = orbit(w)
    plain_end = float(np.linalg.norm(plain[-1][:3, 3] - data[-1][1].pose().reshape(4, 4).T[:3, 3]))
    colour_end = float(np.linalg.norm(colour[-1][:3, 3] - data[-1][1].pose().reshape(4, 4).T[:3, 3]))
    print("orbit, %d frames: end error %.6f mm without colour, %.6f mm with (weight %g); allowance 8 x %.3e = %.3e mm; trajectory errors %s / %s"
          % (FRAMES, plain_end, colour_end, w, spread, 8 * spread, errors(plain, data), errors(colour, data)))
    assert not np.array_equal(plain, colour)
    assert spread > 0
    assert colour_end <= plain_end + 8 * spread


def test_a_tracker_refuses_a_colour_weight_it_cannot_use():
    vol = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3)
    for kwargs in (dict(method="icp", colour_weight=0.1), dict(method="field", colour_weight=-1.0), dict(method="field", colour_weight=float("nan")),
                   dict(method="field", colour_weight=float("inf"))):
        with pytest.raises(ValueError):
            FrameToModelTracker(vol, 640, 480, **kwargs)
    vol.close()


def test_the_tracker_entry_point_refuses_what_it_cannot_do():
    import ctypes as C

    import torch
    from tsdf_amd import _capi
    lib = _capi.lib
    s = CR.wall_scene()
    grey = tsdf_amd.TSDFVolume(CR.WALL_SIZE, tuple(n * CR.WALL_VOXEL for n in CR.WALL_SIZE))      # no colour enabled
    grey.offset(*CR.WALL_OFFSET)
    vol = wall_volume(s)
    kinv = np.ascontiguousarray(wall_camera().kinv(), np.float32).reshape(-1)
    rgb = torch.from_numpy(np.ascontiguousarray(s.rgb).reshape(-1)).cuda()
    torch.cuda.synchronize()
    T = np.ascontiguousarray(np.eye(4).reshape(-1))
    out = np.full(4, 7.0, np.float32)
    trackers = {id(v): FrameToModelTracker(v, CR.WALL_W, CR.WALL_H, camera=wall_camera(), method="field") for v in (grey, vol)}

    def align(v, rgb_ptr=rgb.data_ptr(), cg=30.0, cw=0.5, pose=T):
        return lib.tsdf_tracker_align_field_colour(trackers[id(v)]._h, kinv.ctypes.data, C.c_void_p(rgb_ptr) if rgb_ptr else None, cg, cw,
                                                   pose.ctypes.data if pose is not None else None, out.ctypes.data, out[2:].ctypes.data)

    assert align(vol) == _capi.TSDF_ERR_INVALID                                  # nothing filtered, nothing integrated yet
    depth = torch.from_numpy(np.ascontiguousarray(s.depth).view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    for v in (grey, vol):
        trackers[id(v)].process(s.depth, initial_pose=np.eye(4))
        assert align(v) == _capi.TSDF_ERR_INVALID                                # the integrate took the filtered frame
        _capi.check(lib.tsdf_tracker_filter(trackers[id(v)]._h, C.c_void_p(depth.data_ptr())))      # the next frame, filtered and waiting
    assert (out == 7.0).all()
    before = volume_state(vol)
    assert align(vol, pose=T.copy()) == _capi.TSDF_OK and (out != 7.0).all() and out[2] == out[3] == len(s.points)
    assert_same_state(volume_state(vol), before)                                 # the call reads the volume and writes nothing of it
    out[:] = 7.0
    refused = [align(grey), align(vol, rgb_ptr=None), align(vol, pose=None)]
    refused += [align(vol, cg=cg) for cg in (0.0, -1.0, float("nan"))] + [align(vol, cw=cw) for cw in (-0.5, float("nan"), float("inf"))]
    assert all(rc == _capi.TSDF_ERR_INVALID for rc in refused), refused
    assert "tsdf_tracker_align_field_colour" in _capi.last_error()
    assert (out == 7.0).all() and np.array_equal(T, np.eye(4).reshape(-1)), "a refused call wrote a result"
    for v in (grey, vol):
        trackers[id(v)].synchronize()
        trackers[id(v)].close()
        v.close()
