"""Colour fusion against its CPU reference where kernels go wrong (include/tsdf_amd.h, "colour fusion"; tsdf_amd/csrc/colour.hip).

test_colour_fusion.py checks colour on cubic 3000 mm grids seen from outside at 640x480.  band_pass_kernel (tsdf_amd/csrc/band_pass.hpp) has a brick walk,
camera split, rounding, frustum test, depth read and band test of its own, so here it meets the corners the distance path is held to
(test_fuzz_parity.py, test_parity_integrate.py): random grids, images and cameras, appended planes, odd widths and unaligned
pointers, cameras inside the grid, voxels with sdf exactly +-trunc, every observation count, the weight storage transitions and the
colour lifecycle.  Every case that integrates checks

  * the colour words against tests/colour_ref.py (numpy over the oracle's transforms), word for word, from the same start words;
  * distances and weights against a plain twin (integrate on an identical volume) and the oracle; occupancy against the twin;
  * sample_colours of random, off-grid, NaN and cell-face points against colour_ref.sample;
  * where it casts or meshes: the coloured cast / surface is the plain one plus sampling.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import tsdf_amd
from tests import colour_ref
from tests.helpers import H, W, Cam, assert_same_floats, camera_at
from tests.test_fuzz_parity import random_camera, random_depth
from tsdf_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SEEN = {"scenes": 0, "coloured": 0, "general": 0, "saturated": 0}


class Fusion:
    """A colour volume, its plain twin, the oracle and the reference colour words, driven in lockstep."""

    def __init__(self, oracle, dims, phys, colour=True):
        self.O = oracle
        self.gv = tsdf_amd.TSDFVolume(dims, phys)
        self.tv = tsdf_amd.TSDFVolume(dims, phys)
        self.ov = oracle.Volume(dims, phys)
        if colour:
            self.gv.enable_colour()
        self.words = np.zeros(self.gv.resident_voxels(), np.uint32) if colour else None
        self.coloured = np.zeros(self.gv.resident_voxels(), bool)

    def volumes(self):
        return (self.gv, self.tv, self.ov)

    def offset(self, o):
        for v in self.volumes():
            v.offset(*o)

    def clear(self):
        for v in self.volumes():
            v.clear()
        if self.words is not None:
            self.words[:] = 0

    def set_words(self, words):
        self.gv.set_colour_data(words)
        self.words = np.array(words, np.uint32)

    def integrate(self, depth, rgb, width, height, cam):
        if self.words is None:
            self.gv.integrate(depth, width, height, cam)
        else:
            self.gv.integrate_colour(depth, rgb, width, height, cam)
            self.words, _, col = colour_ref.integrate_colour(self.O, self.words, colour_ref.geometry(self.gv), depth, rgb, width, height, cam)
            self.coloured |= col
        self.tv.integrate(depth, width, height, cam)
        self.ov.integrate(depth, width, height, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=self.O.max_threads())

    def check(self, what):
        if self.words is not None:
            got = self.gv.get_colour_data()
            bad = np.flatnonzero(got != self.words)
            assert bad.size == 0, "%s: %d colour words differ, first at %d: %08x vs %08x" % (what, bad.size, bad[0], got[bad[0]], self.words[bad[0]])
        gw, gd = self.gv.get_weight_data(), self.gv.get_distance_data()
        assert_same_floats(gw, self.tv.get_weight_data(), what + ": weights vs twin")
        assert_same_floats(gd, self.tv.get_distance_data(), what + ": distances vs twin")
        assert_same_floats(gw, self.ov.weight, what + ": weights vs oracle")
        assert_same_floats(gd, self.ov.dist, what + ": distances vs oracle")
        for a, b, name in zip(self.gv.occupancy_data(), self.tv.occupancy_data(), ("fine", "cell", "reach")):
            assert np.array_equal(a, b), "%s: occupancy %s vs twin" % (what, name)

    def check_sampling(self, rng, what, n=20000):
        geom = colour_ref.geometry(self.gv)
        dims, vs, off, off0, _ = geom
        lo = (off0 + off).astype(np.float64)
        ext = np.array(dims) * vs.astype(np.float64)
        pts = rng.uniform(lo - 0.2 * ext, lo + 1.2 * ext, size=(n, 3)).astype(np.float32)
        # on cell faces: the float a face's index gives back through the rule's own subtraction, and its neighbours
        i = rng.integers(0, np.array(dims) + 1, size=(n // 4, 3)).astype(np.float32)
        face = ((i * vs) + off0) + off
        face = np.concatenate([face, np.nextafter(face, np.float32(np.inf)), np.nextafter(face, np.float32(-np.inf))])
        mixed = pts[:len(face)].copy()
        axis = rng.integers(0, 3, size=len(face))
        mixed[np.arange(len(face)), axis] = face[np.arange(len(face)), axis]
        special = np.tile((lo + 0.5 * ext).astype(np.float32), (7, 1))     # the grid's centre with NaN, inf or huge coordinates
        special[[0, 1, 2, 3], [0, 1, 2, 0]] = np.nan
        special[3] = np.nan
        special[4, 0], special[5, 1], special[6] = np.inf, -np.inf, 1e30
        pts = np.concatenate([pts, face, mixed, special]).astype(np.float32)
        got = self.gv.sample_colours(pts)
        want = colour_ref.sample(self.words, geom, pts)
        bad = np.flatnonzero(np.any(got != want, axis=1))
        assert bad.size == 0, "%s: %d sampled colours differ, first at %r: %s vs %s" % (what, bad.size, pts[bad[0]], got[bad[0]], want[bad[0]])
        assert not got[-7:].any()

    def check_cast(self, width, height, cam, what):
        V, N = self.tv.raycast(width, height, cam)     # (the twin casts too: both volumes see the same sequence of calls)
        Vc, Nc, rgb = tsdf_amd.GPURaycaster(width, height).raycast_colour(self.gv, cam)
        assert_same_floats(Vc, V, what + ": coloured cast vertices")
        assert_same_floats(Nc, N, what + ": coloured cast normals")
        assert np.array_equal(rgb, self.gv.sample_colours(Vc)), what + ": cast colours are not the sampled ones"
        assert np.array_equal(rgb, colour_ref.sample(self.words, colour_ref.geometry(self.gv), Vc)), what + ": cast colours vs reference"
        return int((~np.isnan(V[:, 0])).sum())

    def check_mesh(self, what):
        V, Cc = self.gv.extract_coloured_surface()
        assert_same_floats(V, self.tv.extract_surface(), what + ": coloured surface vertices")
        assert np.array_equal(Cc, colour_ref.sample(self.words, colour_ref.geometry(self.gv), V)), what + ": surface colours"
        return len(V)


def noise_rgb(rng, n):
    """Random colours with runs of 0 and 255 in every channel."""
    rgb = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    rgb[rng.random((n, 3)) < 0.15] = 0
    rgb[rng.random((n, 3)) < 0.15] = 255
    return rgb


def random_words(rng, n):
    return rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)


def general_camera(rng, oracle, cam, kind):
    """cam with a skewed, off-centre K ('skew'), a projective last row of the inverse pose ('projective') or a K whose last row
    is not (0, 0, 1) ('k33': surface z is not the depth)."""
    k, ip = cam.k().copy(), cam.inverse_pose().copy()
    if kind == "skew":
        k[3] = float(rng.uniform(-8.0, 8.0))          # K(0,1), column-major
        k[6] += float(rng.uniform(-20.0, 20.0))       # cx
        k[7] += float(rng.uniform(-20.0, 20.0))       # cy
    elif kind == "projective":
        ip[3] = float(rng.uniform(-2e-5, 2e-5))       # inv_pose(3,0)
        ip[7] = float(rng.uniform(-2e-5, 2e-5))       # inv_pose(3,1)
        ip[15] = float(rng.uniform(0.97, 1.03))
    else:
        k[8] = float(rng.choice([1.02, 0.97, 1.03]))  # K(2,2)
    return Cam(cam.pose(), ip, k, oracle.mat3_inverse(k))


def random_case(rng, seed):
    dims = [int(v) for v in rng.integers(5, 73, size=3)]
    if seed % 5 == 1:
        dims[2] = 32 * int(rng.integers(1, 3)) + int(rng.integers(1, 5))    # planes appended to the last brick layer
    elif seed % 5 == 3:
        dims[2] = int(rng.integers(5, 32))                                  # fewer planes than one brick layer
    if rng.random() < 0.5:
        vs = float(rng.uniform(4.0, 60.0))
        phys = tuple(d * vs for d in dims)
    else:
        phys = tuple(float(d * rng.uniform(4.0, 60.0)) for d in dims)
    width, height = int(rng.integers(1, 201)), int(rng.integers(1, 161))
    return tuple(dims), phys, width, height


@pytest.mark.parametrize("seed", range(36))
def test_random_colour_scene(oracle, seed):
    rng = np.random.default_rng(0xC0107 + seed)
    dims, phys, width, height = random_case(rng, seed)
    f = Fusion(oracle, dims, phys)
    shift = None
    if seed % 3 == 0:          # offset baked at clear(), then moved: offset != offset_at_clear
        o0 = tuple(float(v) for v in rng.uniform(-500, 500, size=3))
        o1 = tuple(float(v) for v in rng.uniform(-300, 300, size=3))
        f.offset(o0)
        f.clear()
        f.offset(o1)
        shift = tuple(a + b for a, b in zip(o0, o1))
    if seed % 2 == 1:
        f.set_words(random_words(rng, f.gv.resident_voxels()))
    kind = (None, "skew", None, None, "skew", "projective", None, "skew", None, "k33", None, None)[seed % 12]
    what = "seed %d dims %s image %dx%d camera %s" % (seed, dims, width, height, kind or "standard")
    cams = []
    for _ in range(int(rng.integers(1, 5))):
        cam, dist_to_centre = random_camera(rng, dims, phys, shift, width, height)
        if kind:
            cam = general_camera(rng, oracle, cam, kind)
        depth = random_depth(rng, width, height, max(dist_to_centre, 50.0))
        f.integrate(depth, noise_rgb(rng, width * height), width, height, cam)
        cams.append(cam)
    f.check(what)
    f.check_sampling(rng, what)
    if seed % 2 == 0:
        f.check_cast(width, height, cams[-1], what)
    if seed % 4 == 1:
        f.check_mesh(what)
    _SEEN["scenes"] += 1
    _SEEN["coloured"] += int(f.coloured.any())
    _SEEN["general"] += int(kind is not None and f.coloured.any())
    _SEEN["saturated"] += int(((f.words[f.coloured] >> np.uint32(24)) == 255).any())


def test_the_random_colour_scenes_were_not_vacuous():
    if _SEEN["scenes"] < 30:
        pytest.skip("needs the whole sweep")
    assert _SEEN["coloured"] >= _SEEN["scenes"] // 2, _SEEN
    assert _SEEN["general"] >= 4 and _SEEN["saturated"] >= 3, _SEEN


@pytest.mark.parametrize("planes", [32, 33, 36, 37, 64, 65, 68, 70])
def test_colour_around_the_brick_layers(oracle, planes):
    """Up to 4 planes past the last full brick layer ride on it (z_extra), more get a layer of their own: the second frame puts a
    sloped wall into the last planes."""
    size, phys = (72, 20, planes), (2700.0, 750.0, planes * 37.5)
    rng = np.random.default_rng(planes)
    f = Fusion(oracle, size, phys)
    d, cam = synth.depth_frame(1, 8, seed=5)
    f.integrate(d, noise_rgb(rng, W * H), W, H, cam)
    cam = camera_at((1350.0, 375.0, -1000.0))
    xx = np.tile(np.arange(W), H)
    wall = 1000.0 + (planes - 5) * 37.5 + xx * (6 * 37.5 / W)
    f.integrate(np.rint(wall).astype(np.uint16), noise_rgb(rng, W * H), W, H, cam)
    f.check("%d planes" % planes)
    last = f.coloured.reshape(planes, -1)[-4:]
    assert last.any(), "nothing coloured in the last planes"
    f.check_sampling(rng, "%d planes" % planes)


def _cropped(a, width, height, new_w, new_h, channels=1):
    return np.ascontiguousarray(a.reshape(height, width, channels)[:new_h, :new_w]).reshape(-1)


@pytest.mark.parametrize("size", [(639, 480), (321, 241), (1, 1)])
def test_odd_image_widths(oracle, size):
    w, h = size
    rng = np.random.default_rng(w)
    f = Fusion(oracle, (80, 72, 64), (3000.0, 2700.0, 2400.0))
    for i in (1, 4):
        d, cam = synth.depth_frame(i, 8, seed=9)
        rgb, _ = synth.colour_frame(i, 8, seed=9)
        if (w, h) == (1, 1):      # one pixel on the optical axis of a wide lens
            cam1 = tsdf_amd.Camera(2.0, 2.0, 0.0, 0.0)
            cam1.set_pose(cam.pose())
            cam = cam1
            d, rgb = np.array([1500 + 400 * i], np.uint16), noise_rgb(rng, 1)
        else:
            d, rgb = _cropped(d, W, H, w, h), _cropped(rgb, W, H, w, h, 3)
        f.integrate(d, rgb, w, h, cam)
    f.check("%dx%d image" % size)
    assert f.coloured.any()
    f.check_cast(w, h, cam, "%dx%d image" % size)


def test_unaligned_depth_and_rgb_pointers(oracle):
    """integrate_colour_device with the depth 2 bytes off 4-byte alignment and the rgb at an odd byte offset."""
    import torch
    d, cam = synth.depth_frame(3, 8, seed=11)
    rgb, _ = synth.colour_frame(3, 8, seed=11)
    dbuf = torch.zeros(W * H + 1, dtype=torch.int16, device="cuda")
    dbuf[1:] = torch.from_numpy(d.view(np.int16)).cuda()
    cbuf = torch.zeros(3 * W * H + 1, dtype=torch.uint8, device="cuda")
    cbuf[1:] = torch.from_numpy(np.ascontiguousarray(rgb).reshape(-1)).cuda()
    torch.cuda.synchronize()
    assert (dbuf.data_ptr() + 2) % 4 == 2 and (cbuf.data_ptr() + 1) % 2 == 1
    f = Fusion(oracle, (96, 96, 96), (3000.0,) * 3)
    f.gv.integrate_colour_device(dbuf.data_ptr() + 2, cbuf.data_ptr() + 1, W, H, cam)
    f.gv.synchronize()
    f.words, _, f.coloured = colour_ref.integrate_colour(oracle, f.words, colour_ref.geometry(f.gv), d, rgb, W, H, cam)
    f.tv.integrate(d, W, H, cam)
    f.ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    f.check("unaligned pointers")
    assert f.coloured.sum() > 10000


@pytest.mark.parametrize("ypr", [(0.0, 0.0, 0.0), (0.35, -0.2, 0.15), (1.2, 0.4, -0.7), (3.0, 0.1, 0.0), (-1.57, 1.3, 2.0)])
def test_camera_inside_a_grid_of_many_bricks(oracle, ypr):
    """The bricks that straddle the camera plane, voxels behind the camera included."""
    rng = np.random.default_rng(int(abs(ypr[0]) * 100))
    d, _ = synth.depth_frame(1, 7, seed=21)
    cam = camera_at((1310.0, 1490.0, 1720.0), yaw_pitch_roll=ypr)
    f = Fusion(oracle, (192, 96, 128), (3000.0,) * 3)
    f.set_words(random_words(rng, f.gv.resident_voxels()))
    f.integrate(d, noise_rgb(rng, W * H), W, H, cam)
    f.integrate(synth.wall_depth(700), noise_rgb(rng, W * H), W, H, cam)
    f.check("camera inside, ypr %s" % (ypr,))
    assert f.coloured.sum() > 1000
    f.check_cast(W, H, cam, "camera inside, ypr %s" % (ypr,))


def test_camera_exactly_on_a_voxel_centre(oracle):
    """The voxel under the camera projects to 0 / 0 and takes pixel (0, 0); a depth of 1 there puts it in the band."""
    n = 128
    rng = np.random.default_rng(128)
    for voxel in ((70, 40, 50), (0, 0, 0)):
        f = Fusion(oracle, (n, n, n), (3200.0,) * 3)     # voxel size 25: exact centres
        cam = camera_at(tuple((v + 0.5) * 25.0 for v in voxel))
        rgb = noise_rgb(rng, W * H)
        rgb[0] = (17, 201, 99)
        depth = synth.wall_depth(900).copy()
        depth[0] = 1
        f.integrate(depth, rgb, W, H, cam)
        f.check("camera on voxel %s" % (voxel,))
        i = voxel[0] + n * (voxel[1] + n * voxel[2])
        assert f.coloured[i] and f.words[i] == (17 | 201 << 8 | 99 << 16 | 1 << 24)


def set_trunc(volume, trunc):
    """The truncation distance through tsdf_volume_set_header (offset and the rest kept)."""
    from tsdf_amd import _capi
    i = volume.info()
    f3 = lambda a: (C.c_float * 3)(*a)
    assert _capi.lib.tsdf_volume_set_header(volume._h, f3(i.offset), float(trunc), float(i.max_weight), f3(i.global_translation),
                                            f3(i.global_rotation)) == 0
    assert volume.truncation_distance() == trunc


def voxel_sdf(oracle, volume, depth, width, height, cam):
    """Per voxel: the integrate sdf (NaN where there is none) and the depth of the voxel's pixel (0 where none), from the oracle's
    transforms as colour_ref.update_sets forms them."""
    dims, vs, off, off0, _ = colour_ref.geometry(volume)
    centres = colour_ref.voxel_centres(dims, vs, off, off0)
    pix = oracle.world_to_pixel_n(centres, cam.inverse_pose(), cam.k())
    inb = (pix[:, 0] >= 0) & (pix[:, 0] < width) & (pix[:, 1] >= 0) & (pix[:, 1] < height)
    pidx = np.where(inb, pix[:, 1].astype(np.int64) * width + pix[:, 0], 0)
    d = np.where(inb, depth[pidx], 0).astype(np.uint16)
    sel = np.flatnonzero(d > 0)
    sdf = np.full(len(centres), np.nan, np.float32)
    surf = oracle.pixel_to_camera_n(pix[sel], d[sel].astype(np.float32), cam.kinv())[:, 2]
    sdf[sel] = surf - oracle.world_to_camera_n(centres[sel], cam.inverse_pose())[:, 2]
    return sdf, d


@pytest.mark.parametrize("camera", ["standard", "k33"])
def test_band_edges_at_an_exact_truncation_distance(oracle, camera):
    """trunc = 60 mm, voxel centres 20 i + 10 mm, camera on the -z side looking along +z, integer depths: voxels with sdf exactly
    +trunc (coloured: free space starts above it), exactly -trunc (updated and coloured) and just outside on both sides.  With
    K(2,2) = 1.03 the surface z is the depth only up to an ulp (pixel_to_camera's d / ipz * ipz): there the band decides on those
    ulps, and a kernel that took the depth for the surface z would colour the wrong voxels."""
    trunc = 60.0
    rng = np.random.default_rng(60)
    dims, phys = (40, 40, 40), (800.0,) * 3
    f = Fusion(oracle, dims, phys)
    set_trunc(f.gv, trunc)
    set_trunc(f.tv, trunc)
    f.ov.g.trunc = trunc
    f.clear()
    base = camera_at((400.0, 400.0, -834.0))           # camera z: voxel z = 20 k + 844
    cam = base
    if camera == "k33":
        k = base.k().copy()
        k[8] = 1.03
        cam = Cam(base.pose(), base.inverse_pose(), k, oracle.mat3_inverse(k))
    for frame in range(2):
        # depths 20 j + 4 (sdf = 20 (j - k) exactly for the standard camera) and their neighbours
        depth = (20 * rng.integers(50, 80, size=W * H) + 4 + rng.choice([-1, 0, 0, 0, 1], size=W * H)).astype(np.uint16)
        sdf, d = voxel_sdf(oracle, f.gv, depth, W, H, cam)
        exact = d.astype(np.float32) - (20 * (np.arange(f.gv.resident_voxels()) // (40 * 40)) + 844).astype(np.float32)
        groups = {"+trunc": sdf == trunc, "-trunc": sdf == -trunc,
                  "just above": (sdf > trunc) & (sdf <= trunc + 2), "just below": (sdf < -trunc) & (sdf >= -trunc - 2)}
        for name, g in groups.items():
            assert g.any(), "frame %d: no voxel %s" % (frame, name)
        if camera == "k33":       # some voxels an exact depth puts on the band's edge fall off it by the surface's ulp
            assert ((np.abs(exact) == trunc) & (sdf != exact) & (d > 0)).any()
        f.integrate(depth, noise_rgb(rng, W * H), W, H, cam)
        f.check("%s camera, frame %d" % (camera, frame))
    assert f.words[groups["+trunc"]].any() and f.words[groups["-trunc"]].any()


def test_blend_arithmetic_over_every_count(oracle):
    """Start words with every n in 0..255 and channels 0 / 255 / anything on the voxels the frames colour; pixels 0 and 255."""
    rng = np.random.default_rng(256)
    f = Fusion(oracle, (64, 64, 64), (3000.0,) * 3)
    cam = camera_at((1500.0, 1500.0, -1000.0))
    depths = [synth.config1_depth(), synth.wall_depth(2300)]
    ref = colour_ref.geometry(f.gv)
    will = np.zeros(f.gv.resident_voxels(), bool)
    for d in depths:
        will |= colour_ref.integrate_colour(oracle, np.zeros_like(f.words), ref, d, np.zeros((W * H, 3), np.uint8), W, H, cam)[2]
    idx = np.flatnonzero(will)
    assert idx.size > 256 * 20
    n = np.arange(idx.size, dtype=np.uint32) % np.uint32(256)
    ch = rng.choice(np.array([0, 255, 1, 254, 128], np.uint32), size=(idx.size, 3))
    m = rng.random(idx.size) < 0.3
    ch[m] = rng.integers(0, 256, size=(int(m.sum()), 3)).astype(np.uint32)
    words = random_words(rng, f.gv.resident_voxels())
    words[idx] = ch[:, 0] | (ch[:, 1] << np.uint32(8)) | (ch[:, 2] << np.uint32(16)) | (n << np.uint32(24))
    f.set_words(words)
    start = f.words.copy()
    for d in depths:
        rgb = rng.choice(np.array([0, 255, 1, 254, 127, 128], np.uint8), size=(W * H, 3))
        f.integrate(d, rgb, W, H, cam)
        f.check("blend")
    seen = np.unique(start[f.coloured] >> np.uint32(24))
    assert seen.size == 256, "counts covered: %d" % seen.size
    assert ((f.words[f.coloured] >> np.uint32(24)) == 255).any()


def test_weight_storage_and_colour_lifecycle_on_one_volume(oracle):
    """Plain integrates, then enable_colour (words from zero); 8-bit counts that widen to 16 bits mid-stream; fp32 pinned by
    weight_data(); colour disabled and enabled again (zeroed); clear() with colour on.  The counters equal the twin's frame by
    frame."""
    size, phys = (96, 80, 72), (3000.0, 2500.0, 2250.0)
    f = Fusion(oracle, size, phys, colour=False)
    rng = np.random.default_rng(190)
    f.gv.set_counting(True)
    f.tv.set_counting(True)
    w = np.full(f.gv.resident_voxels(), 190.0, np.float32)
    w[::97] = 252.0
    for v in f.volumes():
        v.set_weight_data(w)
    assert f.gv.weight_storage() == (8, False)
    frames = []
    for i in range(12):
        d, cam = synth.depth_frame(i, 12, seed=0x5EED0401)
        rgb, _ = synth.colour_frame(i, 12, seed=0x5EED0401)
        frames.append((d, rgb, cam))
    modes = []
    for i, (d, rgb, cam) in enumerate(frames):
        if i == 2:
            f.gv.enable_colour()
            f.words = np.zeros(f.gv.resident_voxels(), np.uint32)
            assert not f.gv.get_colour_data().any()
        if i == 6:
            assert f.gv.weight_data() and f.tv.weight_data()       # pinned to fp32
        if i == 8:
            f.gv.enable_colour(False)
            assert not f.gv.colour_enabled()
            f.gv.enable_colour()
            f.words[:] = 0
            assert not f.gv.get_colour_data().any()
        if i == 10:
            f.clear()
            assert not f.gv.get_colour_data().any()
        f.integrate(d, rgb, W, H, cam)
        modes.append(f.gv.weight_storage()[0])
        assert modes[-1] == f.tv.weight_storage()[0]
        assert f.gv.last_updated_voxels() == f.tv.last_updated_voxels() > 0, "frame %d" % i
        assert f.gv.last_distance_stores() == f.tv.last_distance_stores(), "frame %d" % i
        f.check("frame %d (%d-bit weights)" % (i, modes[-1]))
    assert modes[0] == 8 and 16 in modes and modes[-1] == 32, modes
    f.check_sampling(rng, "lifecycle")
    f.check_mesh("lifecycle")


_CAST_PROBE = r"""
import sys
import numpy as np
import tsdf_amd
from tsdf_amd import synth
gv = tsdf_amd.TSDFVolume((96, 96, 96), (3000.0,) * 3)
gv.enable_colour()
def integrate(i):
    d, cam = synth.depth_frame(i, 200, seed=0x5EED0003)
    rgb, _ = synth.colour_frame(i, 200, seed=0x5EED0003)
    gv.integrate_colour(d, rgb, synth.WIDTH, synth.HEIGHT, cam)
for i in range(6):
    integrate(i)
out = {}
cam = synth.camera_for_frame(40, 200)
for w, h in ((17, 9), (800, 600), (640, 480)):
    r = tsdf_amd.GPURaycaster(w, h)
    V, N = r.raycast(gv, cam)
    Vc, Nc, rgb = r.raycast_colour(gv, cam)
    out.update({"V%d" % w: V, "N%d" % w: N, "Vc%d" % w: Vc, "Nc%d" % w: Nc, "rgb%d" % w: rgb, "S%d" % w: gv.sample_colours(Vc)})
integrate(6)
Vc, Nc, rgb = tsdf_amd.GPURaycaster(17, 9).raycast_colour(gv, cam)
out.update({"words": gv.get_colour_data(), "rgb_after": rgb, "S_after": gv.sample_colours(Vc),
            "cells": np.array(gv.last_raycast_cell_parallel())})
np.savez(sys.argv[1], **out)
"""


@pytest.mark.parametrize("cells", ["0", "2"])
def test_coloured_ray_casts_at_other_sizes(oracle, tmp_path, cells):
    """Integrate at 640x480, cast with colour at 17x9, 800x600 and 640x480 (the handle's rgb buffer is reused and grown), integrate
    again into the same buffer, cast again: each cast is the plain cast plus sampling, the words are the reference's.  Both casts,
    each in a process of its own."""
    out = str(tmp_path / "cast.npz")
    e = dict(os.environ, TSDF_RAY_CELLS=cells)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-c", _CAST_PROBE, out], check=True, env=e, cwd=ROOT, timeout=600)
    got = np.load(out)
    assert bool(got["cells"]) == (cells == "2")
    for w in (17, 800, 640):
        assert_same_floats(got["Vc%d" % w], got["V%d" % w], "%d wide: vertices" % w)
        assert_same_floats(got["Nc%d" % w], got["N%d" % w], "%d wide: normals" % w)
        assert np.array_equal(got["rgb%d" % w], got["S%d" % w]), "%d wide: colours" % w
        hit = ~np.isnan(got["V%d" % w][:, 0])
        if w != 17:
            assert hit.mean() > 0.3 and got["rgb%d" % w][hit].any(axis=1).mean() > 0.9
    assert np.array_equal(got["rgb_after"], got["S_after"])
    gv = tsdf_amd.TSDFVolume((96, 96, 96), (3000.0,) * 3)
    words = np.zeros(gv.resident_voxels(), np.uint32)
    geom = colour_ref.geometry(gv)
    for i in range(7):
        d, cam = synth.depth_frame(i, 200, seed=0x5EED0003)
        rgb, _ = synth.colour_frame(i, 200, seed=0x5EED0003)
        words, _, _ = colour_ref.integrate_colour(oracle, words, geom, d, rgb, W, H, cam)
    assert np.array_equal(got["words"], words)
