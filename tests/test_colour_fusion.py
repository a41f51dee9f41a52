"""Colour fusion on the GPU (include/tsdf_amd.h, "colour fusion"; tsdf_amd/csrc/colour.hip).

  * colour integrate leaves distances, weights and occupancy exactly as plain integrate does (twin volume + the CPU oracle), in
    every weight storage;
  * the colour words are bit-equal to the CPU reference (tests/colour_ref.py: numpy over the oracle's pinned transforms) --
    a stream, dropouts, off-axis intrinsics (the kernels' general-camera path), saturation of the observation count;
  * sampling, the coloured ray cast (both casts) and the coloured surface are the sampling rule applied to their vertices;
  * physically: fused colour seen from a new pose is the analytic texture;
  * the .tsdf round trip and the C++ class surface (build/test_colour), clear(), and the refusals.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import tsdf_amd
from tests import colour_ref
from tests.helpers import H, W, Cam, assert_same_floats, camera_at
from tsdf_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0003            # bench.py's stream


def stream(n_frames, period=200):
    """(depth, rgb, camera) of the first frames of bench.py's trajectory, with their colour frames."""
    out = []
    for i in range(n_frames):
        d, cam = synth.depth_frame(i, period, seed=SEED)
        rgb, _ = synth.colour_frame(i, period, seed=SEED)
        out.append((d, rgb, cam))
    return out


def coloured_volume(n):
    gv = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    gv.enable_colour()
    return gv


def noise_rgb(seed, n=W * H):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 3), dtype=np.uint8)


@pytest.mark.parametrize("mode", [8, 16, 32])
@pytest.mark.parametrize("n", [128, 256])
def test_colour_integrate_leaves_the_distance_update_alone(oracle, n, mode):
    """24 frames: distances, weights and occupancy flags of integrate_colour are the twin's (plain integrate) and the oracle's."""
    gv, tv = coloured_volume(n), tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    ov = oracle.Volume((n,) * 3, (3000.0,) * 3)
    if mode == 16:
        w = np.zeros(gv.resident_voxels(), np.float32)
        w[0] = 300.0                                        # (the grid's corner voxel: behind the camera of every frame here)
        for v in (gv, tv, ov):
            v.set_weight_data(w)
    elif mode == 32:
        assert gv.weight_data() and tv.weight_data()
    assert gv.weight_storage()[0] == tv.weight_storage()[0] == mode
    for d, rgb, cam in stream(24):
        gv.integrate_colour(d, rgb, W, H, cam)
        tv.integrate(d, W, H, cam)
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    assert gv.weight_storage()[0] == mode
    for got, twin, ref, what in ((gv.get_distance_data(), tv.get_distance_data(), ov.dist, "distances"),
                                 (gv.get_weight_data(), tv.get_weight_data(), ov.weight, "weights")):
        assert_same_floats(got, twin, "%d^3 %d-bit: %s vs twin" % (n, mode, what))
        assert_same_floats(got, ref, "%d^3 %d-bit: %s vs oracle" % (n, mode, what))
    for a, b, what in zip(gv.occupancy_data(), tv.occupancy_data(), ("fine", "cell", "reach")):
        assert np.array_equal(a, b), "%d^3 %d-bit: occupancy %s" % (n, mode, what)
    assert int((gv.get_colour_data() >> 24).astype(bool).sum()) > 10000


def run_reference(oracle, gv, colour, frames):
    geom = colour_ref.geometry(gv)
    for d, rgb, cam in frames:
        colour, _, _ = colour_ref.integrate_colour(oracle, colour, geom, d, rgb, W, H, cam)
    return colour


def check_colour(oracle, gv, frames, start=None):
    n = gv.resident_voxels()
    start = np.zeros(n, np.uint32) if start is None else start
    for d, rgb, cam in frames:
        gv.integrate_colour(d, rgb, W, H, cam)
    got = gv.get_colour_data()
    want = run_reference(oracle, gv, start, frames)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%d colour words differ, first at %d: %08x vs %08x" % (bad.size, bad[0], got[bad[0]], want[bad[0]])
    return got


def test_colour_words_equal_the_cpu_reference_over_a_stream(oracle):
    got = check_colour(oracle, coloured_volume(128), stream(16))
    assert int(((got >> 24) == 16).sum()) > 1000


def test_colour_words_with_dropouts(oracle):
    cam = camera_at((1500, 1500, -1000))
    got = check_colour(oracle, coloured_volume(128), [(synth.config1_depth(), noise_rgb(1), cam), (synth.config1_depth(2), noise_rgb(2), cam)])
    assert int((got >> 24).astype(bool).sum()) > 10000


def test_colour_words_with_off_axis_intrinsics(oracle):
    """A skewed, off-centre K: the general-camera instantiations of integrate and of the colour kernel."""
    base = camera_at((1400, 1550, -900), look_at=(1500, 1500, 1500))
    k = np.array([[560.0, 3.0, 300.5], [0.0, 575.0, 251.25], [0.0, 0.0, 1.0]], np.float32)
    kinv = np.linalg.inv(k.astype(np.float64)).astype(np.float32)
    cam = Cam(base.pose(), base.inverse_pose(), k.T.reshape(-1), kinv.T.reshape(-1))
    frames = [(synth.config1_depth(3), noise_rgb(3), cam), (synth.wall_depth(2300), noise_rgb(4), cam)]
    got = check_colour(oracle, coloured_volume(128), frames)
    assert int((got >> 24).astype(bool).sum()) > 10000


def test_observation_count_saturates(oracle):
    gv = coloured_volume(128)
    start = (np.uint32(253) << np.uint32(24)) | np.uint32(0x405060)
    start = np.full(gv.resident_voxels(), start, np.uint32)
    gv.set_colour_data(start)
    got = check_colour(oracle, gv, stream(3), start=start)
    assert int(((got >> 24) == 255).sum()) > 1000
    assert (got >> 24).min() == 253


def test_sample_colours_equals_numpy(oracle):
    gv = coloured_volume(64)
    rng = np.random.default_rng(7)
    words = rng.integers(0, 2 ** 32, size=gv.resident_voxels(), dtype=np.uint64).astype(np.uint32)
    words[rng.random(words.size) < 0.2] &= np.uint32(0x00FFFFFF)     # n = 0: unobserved
    gv.set_colour_data(words)
    vs = float(gv.voxel_size()[0])
    pts = rng.uniform(-100.0, 3100.0, size=(100000, 3)).astype(np.float32)
    special = np.array([[np.nan, 5, 5], [5, np.nan, 5], [5, 5, np.nan], [-1e-3, 10, 10], [3000.0, 10, 10], [0, 0, 0],
                        [vs, vs, vs], [2999.99, 2999.99, 2999.99], [1e30, 0, 0], [-1e30, 0, 0], [np.inf, 1, 1]], np.float32)
    pts = np.concatenate([pts, special])
    got = gv.sample_colours(pts)
    want = colour_ref.sample(words, colour_ref.geometry(gv), pts)
    assert np.array_equal(got, want)
    assert np.all(got[-11:-8] == 0) and np.all(got[-3:] == 0)
    # the same after an offset: the rule reads offset and offset_at_clear
    gv.offset(11.5, -7.25, 3.0)
    assert np.array_equal(gv.sample_colours(pts), colour_ref.sample(words, colour_ref.geometry(gv), pts))


_CAST_PROBE = r"""
import sys
import numpy as np
import tsdf_amd
from tsdf_amd import synth
n = int(sys.argv[2])
gv = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
gv.enable_colour()
for i in range(12):
    d, cam = synth.depth_frame(i, 200, seed=0x5EED0003)
    rgb, _ = synth.colour_frame(i, 200, seed=0x5EED0003)
    gv.integrate_colour(d, rgb, synth.WIDTH, synth.HEIGHT, cam)
cam = synth.camera_for_frame(57, 200)
r = tsdf_amd.GPURaycaster(synth.WIDTH, synth.HEIGHT)
V, N = r.raycast(gv, cam)
Vc, Nc, rgb = r.raycast_colour(gv, cam)
np.savez(sys.argv[1], V=V, N=N, Vc=Vc, Nc=Nc, rgb=rgb, S=gv.sample_colours(Vc), cells=np.array(gv.last_raycast_cell_parallel()))
"""


@pytest.mark.parametrize("cells", ["0", "2"])
def test_coloured_ray_cast_is_the_cast_plus_sampling(tmp_path, cells):
    """Vertices and normals are raycast()'s bits; rgb is sample_colours(vertices), misses (0, 0, 0) -- the march (TSDF_RAY_CELLS=0)
    and the cell-parallel cast (=2), each in a process of its own."""
    out = str(tmp_path / "cast.npz")
    e = dict(os.environ, TSDF_RAY_CELLS=cells)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-c", _CAST_PROBE, out, "128"], check=True, env=e, cwd=ROOT, timeout=600)
    got = np.load(out)
    assert bool(got["cells"]) == (cells == "2")
    assert_same_floats(got["Vc"], got["V"], "vertices")
    assert_same_floats(got["Nc"], got["N"], "normals")
    assert np.array_equal(got["rgb"], got["S"])
    miss = np.isnan(got["V"][:, 0])
    assert miss.any() and (~miss).sum() > 50000
    assert np.all(got["rgb"][miss] == 0)
    assert (got["rgb"][~miss].any(axis=1)).mean() > 0.95


def test_coloured_surface_is_the_surface_plus_sampling():
    gv = coloured_volume(128)
    for d, rgb, cam in stream(8):
        gv.integrate_colour(d, rgb, W, H, cam)
    V, C = gv.extract_coloured_surface()
    assert_same_floats(V, gv.extract_surface(), "vertices")
    assert np.array_equal(C, gv.sample_colours(V))
    assert len(V) > 10000 and C.any(axis=1).mean() > 0.9


def test_fused_colour_matches_the_analytic_texture():
    """40 frames of the synthetic stream at 256^3 with colour_frame, then a coloured ray cast from a pose not in the stream: on hit
    pixels whose voxel has been observed, |fused - analytic| per channel has median <= 2 and 99th percentile <= 8 (estimates from
    trunc ~ 1.9 voxels and a texture slope of 0.085 per mm)."""
    n, F = 256, 40
    gv = coloured_volume(n)
    for i in range(F):
        d, cam = synth.depth_frame(i, F, seed=SEED)
        rgb, _ = synth.colour_frame(i, F, seed=SEED)
        gv.integrate_colour(d, rgb, W, H, cam)
    cam = synth.camera_for_frame(0.5, F)                 # halfway between the stream's first two poses
    V, _, rgb = tsdf_amd.GPURaycaster(W, H).raycast_colour(gv, cam)
    hit = ~np.isnan(V[:, 0]) & rgb.any(axis=1)
    assert hit.sum() > 100000
    # the analytic colour at the ray cast's hit: the texture at the vertex, with the blue of the object the exact trace hits there
    _, obj, _, _ = synth._trace(cam, W, H)
    truth = synth.texture(V[hit], obj.reshape(-1)[hit])
    known = obj.reshape(-1)[hit] != 0
    err = np.abs(rgb[hit][known].astype(np.int32) - truth[known].astype(np.int32))
    med, p99 = np.median(err, axis=0), np.percentile(err, 99, axis=0)
    print("colour error per channel: median %s, 99th percentile %s, max %s" % (med, p99, err.max(axis=0)))
    assert np.all(med <= 2), med
    assert np.all(p99 <= 8), p99


def test_clear_zeroes_colour_and_refusals_explain_themselves():
    gv = coloured_volume(64)
    d, rgb, cam = stream(1)[0]
    gv.integrate_colour(d, rgb, W, H, cam)
    assert gv.get_colour_data().any()
    gv.clear()
    assert gv.colour_enabled() and not gv.get_colour_data().any()
    # a slab refuses colour
    slab = tsdf_amd.TSDFVolume((64,) * 3, (3000.0,) * 3, slab=(0, 32))
    with pytest.raises(ValueError, match="slab"):
        slab.enable_colour()
    # colour calls on a volume without colour
    plain = tsdf_amd.TSDFVolume((64,) * 3, (3000.0,) * 3)
    for call in (lambda: plain.integrate_colour(d, rgb, W, H, cam), lambda: plain.sample_colours(np.zeros((4, 3), np.float32)),
                 lambda: plain.get_colour_data(), lambda: tsdf_amd.GPURaycaster(W, H).raycast_colour(plain, cam)):
        with pytest.raises(ValueError, match="not enabled"):
            call()
    # explicit deformation nodes
    gv.deformation()
    with pytest.raises(ValueError, match="deformation"):
        gv.integrate_colour(d, rgb, W, H, cam)
    # disabling frees, enabling again starts from zero
    gv2 = coloured_volume(64)
    gv2.integrate_colour(d, rgb, W, H, cam)
    gv2.enable_colour(False)
    assert not gv2.colour_enabled()
    gv2.enable_colour()
    assert not gv2.get_colour_data().any()


def test_class_surface_and_tsdf_round_trip(tmp_path):
    """build/test_colour: the C++ classes integrate with rgb, extract a coloured surface, write a coloured PLY, ray cast with colour
    and round-trip the .tsdf colour block; every result is the Python path's."""
    n, frames = 128, stream(6)
    d = np.stack([f[0] for f in frames])
    c = np.stack([f[1] for f in frames])
    p = np.stack([f[2].pose() for f in frames]).astype(np.float32)
    d.tofile(tmp_path / "d.u16"); c.tofile(tmp_path / "c.u8"); p.tofile(tmp_path / "p.f32")
    r = subprocess.run([os.path.join(ROOT, "build", "test_colour"), str(tmp_path / "d.u16"), str(tmp_path / "c.u8"), str(tmp_path / "p.f32"),
                        str(len(frames)), str(n), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    gv = coloured_volume(n)
    for dd, rgb, cam in frames:
        gv.integrate_colour(dd, rgb, W, H, cam)
    colour = gv.get_colour_data()
    assert np.array_equal(np.fromfile(tmp_path / "colour.u32", np.uint32), colour)
    # PLY: counts, positions and colours
    with open(tmp_path / "mesh.ply") as f:
        lines = f.read().splitlines()
    end = lines.index("end_header")
    assert lines[:end + 1][3:9] == ["property float x", "property float y", "property float z", "property uchar red",
                                    "property uchar green", "property uchar blue"]
    nv, nf = int(lines[2].split()[-1]), int(lines[9].split()[-1])
    V, C = gv.extract_coloured_surface()
    assert nv == len(V) and nf == len(V) // 3
    rows = [l.split() for l in lines[end + 1:end + 1 + nv]]
    assert all(len(row) == 6 for row in rows)
    assert np.array_equal(np.array([row[3:] for row in rows], np.int64), C.astype(np.int64))
    assert np.allclose(np.array([row[:3] for row in rows], np.float64), V, rtol=1e-5, atol=1e-3)
    # ray cast from the last pose
    Vc, _, rgb = tsdf_amd.GPURaycaster(W, H).raycast_colour(gv, frames[-1][2])
    assert_same_floats(np.fromfile(tmp_path / "ray_vertices.f32", np.float32).reshape(-1, 3), Vc, "ray vertices")
    assert np.array_equal(np.fromfile(tmp_path / "ray_rgb.u8", np.uint8).reshape(-1, 3), rgb)
    # .tsdf: r, g, b round-trip; n = min(max((int)weight, 1), 255) where the colour is not black, else 0
    loaded = np.fromfile(tmp_path / "loaded.u32", np.uint32)
    w = gv.get_weight_data()
    rgb24 = colour & np.uint32(0xFFFFFF)
    n_rule = np.where(rgb24 != 0, np.clip(w.astype(np.int64), 1, 255), 0).astype(np.uint32)
    assert np.array_equal(loaded, rgb24 | (n_rule << np.uint32(24)))
    # a volume without colour writes a zero colour block: 68-byte header, N distances, N weights, then 3 N colour bytes
    N = n ** 3
    raw = np.fromfile(tmp_path / "plain.tsdf", np.uint8, count=68 + 8 * N + 3 * N)
    assert not raw[68 + 8 * N:].any()
