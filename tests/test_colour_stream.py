"""Colour fusion frame after frame: tsdf_pipeline_step_colour, tsdf_tracker_integrate_colour and kinfu_stream --colour (include/tsdf_amd.h,
"colour fusion"), and integrate_packed_colour_kernel, the colour update made inside the packed integrate kernel.

Every coloured run is held to a per-call twin -- bilateral filter, integrate_colour_device of the filtered frame, raycast_colour_device,
frame by frame -- and, where it can be recomputed on the CPU, to tests/colour_ref.py on the filtered frames (the anchor, in case the twin
shares a bug).  A coloured run must leave distances, weights, pictures and counters exactly as the plain run does."""
import json
import os
import subprocess

import numpy as np
import pytest

import tsdf_amd
from tests import colour_ref
from tests.helpers import H, W, assert_same_floats, camera_at
from tests.test_colour_parity import noise_rgb, set_trunc, voxel_sdf
from tsdf_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "kinfu_stream")
PHYS = (3000.0,) * 3


def _frames(count, width=W, height=H, inside=False, seed=0x5EED00C1, stream=40):
    out = []
    for i in range(count):
        depth, cam = synth.depth_frame(i, stream, seed, width, height, inside=inside)
        rgb, _ = synth.colour_frame(i, stream, seed, width, height, inside=inside)
        out.append((depth, rgb.reshape(-1), cam))
    return out


def _upload(frames):
    import torch
    depth = torch.from_numpy(np.stack([d for d, _, _ in frames]).view(np.int16)).cuda()
    rgb = torch.from_numpy(np.stack([c for _, c, _ in frames])).cuda()
    return depth, rgb


def _volume(n, colour=True, wbits=None, counting=False, pin_fp32=False, trunc=None, phys=PHYS, start_words=None):
    v = tsdf_amd.TSDFVolume((n, n, n), phys)
    if colour:
        v.enable_colour()
        if start_words is not None:
            v.set_colour_data(start_words)
    if trunc is not None:
        set_trunc(v, trunc)
    if wbits is not None:
        v.set_weight_storage(wbits)
    if pin_fp32:
        assert v.weight_data()           # (the device pointer: the weights are fp32 from now on)
    if counting:
        v.set_counting(True)
    return v


def _run_pipeline(frames, n, colour=True, overlap=True, ahead=True, width=W, height=H, **vol_kw):
    """-> (per-frame [(V, N, C or None)], distances, weights, colour words or None, per-frame counters)"""
    import torch
    from tsdf_amd.pipeline import FusionPipeline
    vol = _volume(n, colour=colour, **vol_kw)
    pipe = FusionPipeline(vol, tsdf_amd.BilateralFilter(30.0, 4.5), tsdf_amd.GPURaycaster(width, height), width, height, overlap=overlap)
    depth, rgb = _upload(frames)
    vert = torch.empty((width * height, 3), dtype=torch.float32, device="cuda")
    norm = torch.empty_like(vert)
    cols = torch.empty((width * height, 3), dtype=torch.uint8, device="cuda")
    pictures, counters = [], []
    for i, (_, _, cam) in enumerate(frames):
        j = i + 1 if i + 1 < len(frames) else None
        nxt = depth[j].data_ptr() if (ahead and j is not None) else None
        ncam = frames[j][2] if (ahead and j is not None) else None
        if colour:
            pipe.step_colour(depth[i].data_ptr(), rgb[i].data_ptr(), cam, vert.data_ptr(), norm.data_ptr(), cols.data_ptr(), nxt, ncam)
        else:
            pipe.step(depth[i].data_ptr(), cam, vert.data_ptr(), norm.data_ptr(), nxt, ncam)
        pipe.synchronize()
        pictures.append((vert.cpu().numpy().copy(), norm.cpu().numpy().copy(), cols.cpu().numpy().copy() if colour else None))
        if vol_kw.get("counting"):
            counters.append((vol.last_updated_voxels(), vol.last_distance_stores()))
    pipe.synchronize()
    out = (pictures, vol.get_distance_data(), vol.get_weight_data(), vol.get_colour_data() if colour else None, counters)
    pipe.close()
    vol.close()
    return out


def _filter(depth_dev, width, height):
    """The pipeline's bilateral filter on a device frame -> (device result, host copy)."""
    import torch
    out = torch.empty_like(depth_dev)
    tsdf_amd.BilateralFilter(30.0, 4.5).filter_device(depth_dev.data_ptr(), out.data_ptr(), width, height)
    torch.cuda.synchronize()
    return out, out.cpu().numpy().view(np.uint16).copy()


def _run_twin(frames, n, width=W, height=H, **vol_kw):
    """The per-call twin: filter -> integrate_colour_device(filtered, rgb) -> raycast_colour_device, frame by frame.
    -> (pictures, distances, weights, colour words, host filtered frames)"""
    import torch
    vol = _volume(n, **vol_kw)
    caster = tsdf_amd.GPURaycaster(width, height)
    depth, rgb = _upload(frames)
    vert = torch.empty((width * height, 3), dtype=torch.float32, device="cuda")
    norm = torch.empty_like(vert)
    cols = torch.empty((width * height, 3), dtype=torch.uint8, device="cuda")
    pictures, filtered = [], []
    for i, (_, _, cam) in enumerate(frames):
        f_dev, f_host = _filter(depth[i], width, height)
        filtered.append(f_host)
        vol.integrate_colour_device(f_dev.data_ptr(), rgb[i].data_ptr(), width, height, cam)
        vol.synchronize()
        caster.raycast_colour_device(vol, cam, vert.data_ptr(), norm.data_ptr(), cols.data_ptr())
        vol.synchronize()
        torch.cuda.synchronize()
        pictures.append((vert.cpu().numpy().copy(), norm.cpu().numpy().copy(), cols.cpu().numpy().copy()))
    out = (pictures, vol.get_distance_data(), vol.get_weight_data(), vol.get_colour_data(), filtered)
    vol.close()
    return out


def _reference_words(oracle, n, frames, filtered, width=W, height=H, trunc=None, phys=PHYS, start_words=None, masks=None):
    """colour_ref over the filtered frames from the same start words; masks (a list) receives each frame's coloured mask."""
    geom_vol = _volume(n, colour=False, trunc=trunc, phys=phys)
    geom = colour_ref.geometry(geom_vol)
    geom_vol.close()
    words = np.zeros(n * n * n, np.uint32) if start_words is None else np.array(start_words, np.uint32)
    coloured = 0
    for (_, rgb, cam), f in zip(frames, filtered):
        words, _, col = colour_ref.integrate_colour(oracle, words, geom, f, rgb, width, height, cam)
        coloured += int(col.sum())
        if masks is not None:
            masks.append(col)
    assert coloured > 1000, "the reference coloured almost nothing: the case is vacuous"
    return words


def _same_words(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d colour words differ, first at %d: %08x vs %08x" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _same_run(got, twin, what):
    pictures, dist, weight, words = got[:4]
    assert_same_floats(dist, twin[1], what + ": distances")
    assert_same_floats(weight, twin[2], what + ": weights")
    _same_words(words, twin[3], what)
    for i, ((v, nn, c), (vt, nt, ct)) in enumerate(zip(pictures, twin[0])):
        assert_same_floats(v, vt, "%s: vertices of frame %d" % (what, i))
        assert_same_floats(nn, nt, "%s: normals of frame %d" % (what, i))
        assert np.array_equal(c, ct), "%s: colours of frame %d" % (what, i)


# ---- 1 + 2: the pipeline equals the per-call twin, and colour changes nothing else -----------------------------------------------
@pytest.mark.parametrize("n", [128, 256])
def test_pipeline_step_colour_equals_the_per_call_twin(oracle, n):
    frames = _frames(12)
    twin = _run_twin(frames, n)
    assert (twin[3] >> 24).any() and twin[0][-1][2].any(), "nothing coloured"
    if n == 128:
        _same_words(twin[3], _reference_words(oracle, n, frames, twin[4]), "twin vs colour_ref")
    for overlap in (True, False):
        for ahead in (True, False):
            got = _run_pipeline(frames, n, overlap=overlap, ahead=ahead)
            _same_run(got, twin, "%d^3, overlap %s, culling ahead %s" % (n, overlap, ahead))


def test_colour_changes_nothing_else():
    frames = _frames(10)
    col = _run_pipeline(frames, 128, colour=True, counting=True)
    plain = _run_pipeline(frames, 128, colour=False, counting=True)
    assert_same_floats(col[1], plain[1], "distances")
    assert_same_floats(col[2], plain[2], "weights")
    for i, ((v, nn, _), (vp, np_, _)) in enumerate(zip(col[0], plain[0])):
        assert_same_floats(v, vp, "vertices of frame %d" % i)
        assert_same_floats(nn, np_, "normals of frame %d" % i)
    assert col[4] == plain[4] and col[4][-1][0] > 0, (col[4], plain[4])


# ---- 3: every fused variant against colour_ref -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["wbits16_count", "camera_inside", "odd_width", "integer_trunc"])
def test_fused_variants_against_the_reference(oracle, case):
    n, width, kw, inside = 128, W, {}, False
    if case == "wbits16_count":
        kw = dict(wbits=16, counting=True)
    elif case == "camera_inside":
        inside = True
    elif case == "odd_width":
        width = W - 1
    elif case == "integer_trunc":
        kw = dict(trunc=47.0)
    frames = _frames(6, width=width, inside=inside)
    got = _run_pipeline(frames, n, width=width, **kw)
    twin = _run_twin(frames, n, width=width, **{k: v for k, v in kw.items() if k != "counting"})
    _same_run(got, twin, case)
    masks = []
    _same_words(got[3], _reference_words(oracle, n, frames, twin[4], width=width, trunc=kw.get("trunc"), masks=masks), case + " vs colour_ref")
    if inside:
        # the case is only worth its name if voxels of bricks that straddle the camera plane were coloured: brick_cull_kernel
        # gives such a brick no pixel box, so its walk looks its depths up in depth_pad, not in an LDS tile
        probe = _volume(n, colour=False)
        dims, vs, off, off0, _ = colour_ref.geometry(probe)
        probe.close()
        centres = colour_ref.voxel_centres(dims, vs, off, off0)
        x, y, z = (np.arange(n ** 3) % n), (np.arange(n ** 3) // n) % n, np.arange(n ** 3) // (n * n)
        brick = (x // 64) + (n // 64) * ((y // 4) + (n // 4) * (z // 32))   # 64 x 4 x 32 bricks (integrate_grid.hpp)
        straddling = 0
        for (_, _, cam), col in zip(frames, masks):
            behind = np.zeros(brick.max() + 1, bool)
            behind[brick[oracle.world_to_camera_n(centres, cam.inverse_pose())[:, 2] <= 0]] = True
            straddling += int((col & behind[brick]).sum())
        assert straddling > 0, "no coloured voxel in a brick that straddles the camera plane"


def test_band_edges_at_an_exact_truncation_distance(oracle):
    """trunc = 60 mm, voxel centres 20 i + 10 mm, the camera on the -z side looking along +z: after the bilateral filter the depths
    are still integers, so the sdf is an exact multiple of 1 mm and voxels sit exactly on +trunc (coloured: free space starts above
    it), exactly on -trunc and just outside both.  The pipeline's words against colour_ref on the filtered frames."""
    n, phys, trunc = 40, (800.0,) * 3, 60.0
    rng = np.random.default_rng(60)
    cam = camera_at((400.0, 400.0, -834.0))            # camera z: voxel z = 20 k + 844
    frames = [((20 * rng.integers(50, 80, size=W * H) + 4 + rng.choice([-1, 0, 0, 0, 1], size=W * H)).astype(np.uint16),
               noise_rgb(rng, W * H).reshape(-1), cam) for _ in range(3)]
    kw = dict(trunc=trunc, phys=phys)
    got = _run_pipeline(frames, n, **kw)
    twin = _run_twin(frames, n, **kw)
    _same_run(got, twin, "band edges")
    probe = _volume(n, colour=False, **kw)
    for f in twin[4]:
        sdf, _ = voxel_sdf(oracle, probe, f, W, H, cam)
        for name, g in {"+trunc": sdf == trunc, "-trunc": sdf == -trunc, "just above": (sdf > trunc) & (sdf <= trunc + 2),
                        "just below": (sdf < -trunc) & (sdf >= -trunc - 2)}.items():
            assert g.any(), "no voxel %s in a filtered frame" % name
    probe.close()
    _same_words(got[3], _reference_words(oracle, n, frames, twin[4], **kw), "band edges vs colour_ref")


def test_counts_saturate_in_the_pipeline(oracle):
    """Start words with n in 240..255 on every voxel: over 12 coloured steps the counts reach 255 and must stay there."""
    n = 128
    rng = np.random.default_rng(255)
    start = (rng.integers(0, 2 ** 24, size=n ** 3, dtype=np.uint64).astype(np.uint32) |
             (rng.integers(240, 256, size=n ** 3).astype(np.uint32) << np.uint32(24)))
    frames = _frames(12)
    got = _run_pipeline(frames, n, start_words=start)
    twin = _run_twin(frames, n, start_words=start)
    _same_run(got, twin, "saturating counts")
    masks = []
    want = _reference_words(oracle, n, frames, twin[4], start_words=start, masks=masks)
    _same_words(got[3], want, "saturating counts vs colour_ref")
    once = np.flatnonzero(masks[0])
    assert (start[once] >> np.uint32(24) == 255).any(), "no coloured voxel started saturated"


# ---- 4: the fallback inside the pipeline (fp32 weights: integrate_kernel + the colour pass on the same brick list) -------------
def test_fallback_colour_pass_inside_the_pipeline(oracle):
    frames = _frames(12)
    twin = _run_twin(frames, 128, pin_fp32=True)
    for overlap, ahead in ((True, True), (True, False), (False, True)):
        got = _run_pipeline(frames, 128, overlap=overlap, ahead=ahead, pin_fp32=True)
        _same_run(got, twin, "fp32 weights, overlap %s, culling ahead %s" % (overlap, ahead))
    _same_words(twin[3], _reference_words(oracle, 128, frames, twin[4]), "fp32 twin vs colour_ref")


# ---- 5: the tracker --------------------------------------------------------------------------------------------------------
def test_tracker_integrate_colour():
    import torch
    from tsdf_amd.tracking import FrameToModelTracker
    n, F = 128, 8
    frames = _frames(F, seed=0x5EED0005, stream=200)
    truth = frames[0][2].pose().astype(np.float64).reshape(4, 4).T

    def run(colour):
        vol = _volume(n, colour=colour)
        trk = FrameToModelTracker(vol, W, H)
        poses, filtered = [], []
        for i, (d, c, _) in enumerate(frames):
            poses.append(trk.process(d, initial_pose=truth if i == 0 else None, rgb=c if colour else None))
            if i > 0:
                filtered.append(trk.last_icp_inputs()[1])
        trk.synchronize()
        out = (poses, vol.get_distance_data(), vol.get_colour_data() if colour else None, filtered)
        trk.close()
        vol.close()
        return out

    col, plain = run(True), run(False)
    for i, (a, b) in enumerate(zip(col[0], plain[0])):
        assert np.array_equal(a, b), "pose of frame %d" % i
    assert_same_floats(col[1], plain[1], "tracked distances")
    # the twin: the same filtered frames at the poses the tracker returned
    depth, rgb = _upload(frames)
    twin = _volume(n)
    for i, pose in enumerate(col[0]):
        f_dev, f_host = _filter(depth[i], W, H)
        if i > 0:
            assert np.array_equal(f_host, col[3][i - 1]), "filtered frame %d" % i
        cam = tsdf_amd.Camera.default_depth_camera()
        cam.set_pose_rows(pose)
        twin.integrate_colour_device(f_dev.data_ptr(), rgb[i].data_ptr(), W, H, cam)
        twin.synchronize()
    _same_words(col[2], twin.get_colour_data(), "tracker vs twin")
    assert (col[2] >> 24).any()
    assert_same_floats(twin.get_distance_data(), col[1], "twin distances")
    twin.close()
    torch.cuda.synchronize()


# ---- 6: kinfu_stream --colour ------------------------------------------------------------------------------------------------
def _kinfu(d, out, *extra):
    out.mkdir()
    r = subprocess.run([BIN, "-d", str(d), "-n", "128", "-k", "5", "-w", "2", "--dump", str(out)] + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_kinfu_stream_colour(tmp_path):
    import torch
    from tsdf_amd.pipeline import FusionPipeline
    F, seed, stream = 5, 0x5EED0003, 40
    d = tmp_path / "tum"
    synth.write_tum_directory(str(d), F, seed=seed, stream_frames=stream, colour=True)
    plain = _kinfu(d, tmp_path / "plain")
    col = _kinfu(d, tmp_path / "colour", "--colour")
    assert "colour" not in plain and col["colour"] is True
    for k in ("last_frame_vertex_bits", "last_frame_normal_bits", "last_frame_hits"):
        assert col[k] == plain[k], k
    for f in ("vertices.f32", "normals.f32", "distances.f32", "weights.f32"):
        assert_same_floats(np.fromfile(str(tmp_path / "colour" / f), np.float32), np.fromfile(str(tmp_path / "plain" / f), np.float32), f)
    words = np.fromfile(str(tmp_path / "colour" / "colour.u32"), np.uint32)
    colours = np.fromfile(str(tmp_path / "colour" / "colours.u8"), np.uint8)
    assert col["last_frame_colour_bits"] == int(colours.astype(np.int64).sum()) > 0

    # FusionPipeline.step_colour on the same frames and steps
    loaded, _ = tsdf_amd.load_tum_directory(str(d))
    rgbs = [synth.colour_frame(i, stream, seed)[0].reshape(-1) for i in range(F)]
    vol = _volume(128)
    pipe = FusionPipeline(vol, tsdf_amd.BilateralFilter(30.0, 4.5), tsdf_amd.GPURaycaster(W, H), W, H)
    depth = torch.from_numpy(np.stack([f for f, _ in loaded]).view(np.int16)).cuda()
    rgb = torch.from_numpy(np.stack(rgbs)).cuda()
    vert = torch.empty((H * W, 3), dtype=torch.float32, device="cuda")
    norm = torch.empty_like(vert)
    cols = torch.empty((H * W, 3), dtype=torch.uint8, device="cuda")
    for i in range(7):
        a, b = i % F, (i + 1) % F
        pipe.step_colour(depth[a].data_ptr(), rgb[a].data_ptr(), loaded[a][1], vert.data_ptr(), norm.data_ptr(), cols.data_ptr(),
                         depth[b].data_ptr(), loaded[b][1])
    pipe.synchronize()
    _same_words(words, vol.get_colour_data(), "kinfu_stream --colour vs FusionPipeline.step_colour")
    assert np.array_equal(colours, cols.cpu().numpy().reshape(-1))
    pipe.close()
    vol.close()

    # --track: the same poses and distances as the plain tracked run; the colour words of a twin at the dumped poses
    tp = _kinfu(d, tmp_path / "track", "--track")
    tc = _kinfu(d, tmp_path / "track_colour", "--track", "--colour")
    assert tc["colour"] is True and "colour" not in tp
    for f in ("poses.f32", "distances.f32"):
        assert_same_floats(np.fromfile(str(tmp_path / "track_colour" / f), np.float32), np.fromfile(str(tmp_path / "track" / f), np.float32), f)
    poses = np.fromfile(str(tmp_path / "track_colour" / "poses.f32"), np.float32).reshape(-1, 16)
    twin = _volume(128)
    for i, p in enumerate(poses):
        f_dev, _ = _filter(depth[i], W, H)
        cam = tsdf_amd.Camera.default_depth_camera()
        cam.set_pose_rows(p.reshape(4, 4).T.astype(np.float64))
        twin.integrate_colour_device(f_dev.data_ptr(), rgb[i].data_ptr(), W, H, cam)
        twin.synchronize()
    _same_words(np.fromfile(str(tmp_path / "track_colour" / "colour.u32"), np.uint32), twin.get_colour_data(), "kinfu_stream --track --colour vs twin")
    twin.close()


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from tsdf_amd.pipeline import FusionPipeline
    from tsdf_amd.tracking import FrameToModelTracker
    frames = _frames(1)
    depth, rgb = _upload(frames)
    vert = torch.empty((H * W, 3), dtype=torch.float32, device="cuda")
    cam = frames[0][2]

    plain = _volume(64, colour=False)
    pipe = FusionPipeline(plain, tsdf_amd.BilateralFilter(30.0, 4.5), tsdf_amd.GPURaycaster(W, H), W, H)
    with pytest.raises(ValueError, match="colour is not enabled"):
        pipe.step_colour(depth[0].data_ptr(), rgb[0].data_ptr(), cam, vert.data_ptr())
    pipe.close()
    trk = FrameToModelTracker(plain, W, H)
    with pytest.raises(ValueError, match="colour is not enabled"):
        trk.process(frames[0][0], rgb=frames[0][1])
    trk.close()
    plain.close()

    vol = _volume(64)
    pipe = FusionPipeline(vol, tsdf_amd.BilateralFilter(30.0, 4.5), tsdf_amd.GPURaycaster(W, H), W, H)
    with pytest.raises(ValueError, match="null rgb frame"):
        pipe.step_colour(depth[0].data_ptr(), 0, cam, vert.data_ptr())
    pipe.close()
    trk = FrameToModelTracker(vol, W, H)
    trk.process(frames[0][0], rgb=frames[0][1])                 # (a coloured frame is accepted)
    with pytest.raises(ValueError, match="null rgb frame"):
        trk.process_device(depth[0].data_ptr(), rgb_ptr=0)
    trk.close()
    vol.close()

    # a sharded pipeline: one rank's Z-slab with a loop-back exchange
    from tsdf_amd import _capi
    import ctypes as C
    slab = tsdf_amd.TSDFVolume((64, 64, 64), PHYS, slab=(0, 32))
    x = C.c_void_p()
    assert _capi.lib.tsdf_slab_exchange_create_loopback(0, 2, C.byref(x)) == 0
    p = C.c_void_p()
    bil = tsdf_amd.BilateralFilter(30.0, 4.5)
    assert _capi.lib.tsdf_pipeline_create(slab._h, bil._h, W, H, 0, x, C.byref(p)) == 0
    from tsdf_amd.pipeline import _matrices
    m = _matrices(cam)
    rc = _capi.lib.tsdf_pipeline_step_colour(p, C.c_void_p(depth[0].data_ptr()), C.c_void_p(rgb[0].data_ptr()), C.byref(m),
                                             C.c_void_p(vert.data_ptr()), None, None, None, None)
    assert rc != 0 and b"sharded" in _capi.lib.tsdf_last_error()
    _capi.lib.tsdf_pipeline_destroy(p)
    _capi.lib.tsdf_slab_exchange_destroy(x)
    slab.close()
