"""Colour fusion off the GPU: the C ABI's new entry points, the coloured PLY writer, the synthetic colour frames, the TUM loader's
colour frames and the CPU colour reference the GPU tests (tests/test_colour_fusion.py) compare against."""
import ctypes
import os
import re

import numpy as np

from tests import colour_ref
from tests.helpers import H, W
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLOUR_ABI = ("tsdf_volume_enable_colour", "tsdf_volume_colour_enabled", "tsdf_volume_colours", "tsdf_volume_get_colour_data",
              "tsdf_volume_set_colour_data", "tsdf_integrate_colour", "tsdf_integrate_colour_device",
              "tsdf_volume_sample_colours_device", "tsdf_raycast_colour", "tsdf_raycast_colour_device")
HOST_ENTRIES = ("tsdf_host_tum_next_rgb", "tsdf_host_write_ply_coloured")


def test_the_colour_entry_points_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsdf_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tsdf_[a-z0-9_]+)\s*\(", text))
    hip = ctypes.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    host = ctypes.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_host.so"))
    for name in COLOUR_ABI:
        assert name in declared, name
        assert hasattr(hip, name), name
    for name in HOST_ENTRIES:
        assert hasattr(host, name), name


MESH_V = np.array([[0, 0, 0], [1.5, 0, 0], [0, 2.25, 0], [1.5, 2.25, -0.5]], np.float32)
MESH_T = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
MESH_C = np.array([[255, 0, 0], [0, 128, 0], [0, 0, 7], [10, 20, 30]], np.uint8)


def test_coloured_ply_bytes(tmp_path):
    from tsdf_amd import _capi
    path = str(tmp_path / "c.ply")
    assert _capi.host.tsdf_host_write_ply_coloured(path.encode(), MESH_V.ctypes.data, 4, MESH_T.ctypes.data, 2, MESH_C.ctypes.data) == 0
    expected = ("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 2\n"
                "property list uchar int vertex_indices\nend_header\n"
                "0 0 0 255 0 0\n1.5 0 0 0 128 0\n0 2.25 0 0 0 7\n1.5 2.25 -0.5 10 20 30\n3 0 1 2\n3 1 3 2\n")
    assert open(path, "rb").read() == expected.encode()
    # the three-argument writer is unchanged on the same mesh
    plain = str(tmp_path / "p.ply")
    _capi.host.tsdf_host_write_ply(plain.encode(), MESH_V.ctypes.data, 4, MESH_T.ctypes.data, 2)
    assert open(plain, "rb").read() == ("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                                        "element face 2\nproperty list uchar int vertex_indices\nend_header\n"
                                        "0 0 0\n1.5 0 0\n0 2.25 0\n1.5 2.25 -0.5\n3 0 1 2\n3 1 3 2\n").encode()
    # null arrays are refused, not dereferenced
    assert _capi.host.tsdf_host_write_ply_coloured(path.encode(), None, 4, MESH_T.ctypes.data, 2, MESH_C.ctypes.data) == -1


def test_colour_frames_are_deterministic_and_leave_depth_alone(tmp_path):
    a, cam_a = synth.colour_frame(5, 40, seed=0x5EED0003)
    b, _ = synth.colour_frame(5, 40, seed=0x5EED0003)
    assert a.dtype == np.uint8 and a.shape == (W * H, 3)
    assert np.array_equal(a, b)
    d, cam_d = synth.depth_frame(5, 40, seed=0x5EED0003)
    assert np.array_equal(cam_a.pose(), cam_d.pose())
    # registered: a pixel with depth has the colour of an object, a pixel the trace misses is black
    z = synth.trace_depth(cam_d).reshape(-1)
    assert np.all((a[:, 2] != 0) == np.isfinite(z))
    assert set(np.unique(a[:, 2])) <= {0, synth.WALL_B, synth.SPHERE_B, synth.BOX_B}
    # the depth directory is byte-identical with and without colour; colour adds rgb/
    plain, col = tmp_path / "plain", tmp_path / "col"
    fa = synth.write_tum_directory(str(plain), 3, 0x5EED0003, stream_frames=40)
    fb = synth.write_tum_directory(str(col), 3, 0x5EED0003, stream_frames=40, colour=True)
    for (da, pa), (db, pb) in zip(fa, fb):
        assert np.array_equal(da, db) and np.array_equal(pa, pb)
    assert not (plain / "rgb").exists()
    assert (plain / "ground_truth.txt").read_bytes() == (col / "ground_truth.txt").read_bytes()
    for f in sorted(os.listdir(plain / "depth")):
        assert (plain / "depth" / f).read_bytes() == (col / "depth" / f).read_bytes()
    assert sorted(os.listdir(col / "rgb")) == sorted(os.listdir(col / "depth"))


def test_tum_loader_hands_out_the_colour_frames(tmp_path):
    from tsdf_amd import _capi
    d = tmp_path / "tum"
    frames = synth.write_tum_directory(str(d), 3, 0x5EED0003, stream_frames=40, colour=True)
    os.remove(d / "rgb" / sorted(os.listdir(d / "rgb"))[1])        # the second record's colour frame is missing
    h = _capi.host.tsdf_host_tum_open(str(d).encode())
    assert h
    try:
        depth = np.empty(W * H, np.uint16)
        rgb = np.empty(W * H * 3, np.uint8)
        size = (ctypes.c_uint * 2)()
        pose = np.empty(16, np.float32)
        results = []
        for i in range(4):
            rgb[:] = 0
            rc = _capi.host.tsdf_host_tum_next_rgb(h, depth.ctypes.data, depth.size, size, _capi_fp(pose), rgb.ctypes.data, rgb.size)
            results.append(rc)
            if rc == 1:
                assert (size[0], size[1]) == (W, H)
                cam = synth.camera_for_frame(i, 40)
                assert np.array_equal(rgb.reshape(-1, 3), synth.trace_colour(cam)), "frame %d" % i
                assert np.array_equal(depth, frames[i][0])
        assert results == [1, -1, 1, 0]
    finally:
        _capi.host.tsdf_host_tum_close(h)


def _capi_fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def test_cpu_colour_reference_updates_the_oracles_voxels(oracle):
    """The reference's update set (tests/colour_ref.py) is exactly the set of voxels whose oracle weight rose, frame by frame."""
    n = 64
    ov = oracle.Volume((n,) * 3, (3000.0,) * 3)
    geom = ((n,) * 3, ov.voxel_size(), ov.offset(), np.array(ov.g.offset_at_clear, np.float32), np.float32(ov.truncation_distance()))
    colour = np.zeros(n ** 3, np.uint32)
    for i in range(3):
        d, cam = synth.depth_frame(i * 7, 40, seed=0x5EED0003)
        rgb, _ = synth.colour_frame(i * 7, 40, seed=0x5EED0003)
        before = ov.weight.copy()
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
        colour, updated, coloured = colour_ref.integrate_colour(oracle, colour, geom, d, rgb, W, H, cam)
        rose = ov.weight > before
        assert rose.sum() > 1000
        assert np.array_equal(updated, rose), "frame %d" % i
        assert coloured.sum() > 0 and not np.any(coloured & ~updated)
    assert np.all((colour >> 24) <= 3) and np.any((colour >> 24) == 3)


def test_cpu_colour_blend_and_sample_by_hand():
    """The integer blend and the sampling rule on a few hand-made words."""
    colour = np.array([0, (100 << 0) | (50 << 8) | (7 << 16) | (1 << 24), 0xFD141E0A], np.uint32)   # last: n = 253
    coloured = np.array([True, True, True])
    rgb = np.array([[10, 20, 30], [201, 0, 8], [255, 255, 255]], np.uint8)
    out = colour_ref.blend(colour, coloured, np.array([0, 1, 2]), rgb)
    assert out[0] == 10 | (20 << 8) | (30 << 16) | (1 << 24)
    # n = 1: (100 + 201 + 1) // 2, (50 + 0 + 1) // 2, (7 + 8 + 1) // 2
    assert out[1] == 151 | (25 << 8) | (8 << 16) | (2 << 24)
    # n = 253 -> 254: (r_old * 253 + 255 + 127) // 254
    assert out[2] >> 24 == 254 and out[2] & 0xFF == (0x0A * 253 + 255 + 127) // 254
    geom = ((2, 2, 2), np.float32([10, 10, 10]), np.float32([0, 0, 0]), np.float32([0, 0, 0]), np.float32(1))
    words = np.zeros(8, np.uint32)
    words[1] = 1 | (2 << 8) | (3 << 16) | (5 << 24)
    words[2] = 9 | (9 << 8)                           # n = 0: unobserved
    pts = np.array([[15, 5, 5], [5, 15, 5], [np.nan, 1, 1], [-0.01, 5, 5], [19.99, 0, 0], [20, 0, 0]], np.float32)
    got = colour_ref.sample(words, geom, pts)
    assert got.tolist() == [[1, 2, 3], [0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 2, 3], [0, 0, 0]]

