"""Synthetic RGB-D stream: the TUM-dataset surrogate of SURVEY.md section 8d (no TUM data in the image).

An analytic scene (back wall, sphere, box) inside the default 3000 mm volume is ray traced
exactly from a camera moving on a small closed trajectory; the result is quantised to uint16
millimetres with integer-hash sensor noise and dropouts (0 = invalid), i.e. what
TUMDataLoader + DepthImage::scale_depth(0.2) hand to TSDFVolume::integrate in the reference
(src/DataLoader/TUMDataLoader.cpp:84-99).  Everything is input DATA for the path; numpy only.
"""
import math

import numpy as np

from .api import Camera

WIDTH, HEIGHT = 640, 480

# scene, world millimetres (volume spans 0..3000 on every axis)
WALL_Z = 2400.0
SPHERE_C = np.array([1500.0, 1400.0, 1800.0])
SPHERE_R = 350.0
BOX_MIN = np.array([700.0, 1700.0, 1900.0])
BOX_MAX = np.array([1200.0, 2300.0, 2400.0])
LOOK_AT = (1500.0, 1400.0, 1900.0)


def splitmix64(x):
    """splitmix64 finaliser on uint64 arrays (explicit integer hash so every platform agrees)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def camera_position(i, n):
    """Closed trajectory in front of the volume."""
    a = 2.0 * math.pi * i / n
    return (1500.0 + 200.0 * math.sin(a), 1300.0 + 100.0 * math.sin(2.0 * a), -600.0 + 150.0 * math.cos(a))


def camera_position_inside(i, n):
    """Closed trajectory INSIDE the volume, one metre in front of the wall (BASELINE configs[3]: at 1024^3 a ray covers only
    4402 * 0.279 mm = 1228 mm, Q8, so the scene has to be that close)."""
    a = 2.0 * math.pi * i / n
    return (1500.0 + 120.0 * math.sin(a), 1350.0 + 60.0 * math.sin(2.0 * a), 1400.0 + 80.0 * math.cos(a))


def camera_for_frame(i, n, camera=None, inside=False):
    cam = camera or Camera.default_depth_camera()
    cam.set_pose(np.eye(4, dtype=np.float32).reshape(-1))
    cam.move_to(*(camera_position_inside(i, n) if inside else camera_position(i, n)))
    cam.look_at(*LOOK_AT)
    return cam


# per-object blue of the colour texture (trace_colour); 0 = nothing hit
WALL_B, SPHERE_B, BOX_B = 64, 160, 240


def trace_depth(camera, width=WIDTH, height=HEIGHT):
    """Exact camera-z depth (float64 mm, inf = nothing hit) of the analytic scene."""
    return _trace(camera, width, height)[0]


def _trace(camera, width, height):
    """-> (camera-z depth, blue of the object hit (0: none), camera origin, world ray directions with camera z == 1)."""
    kinv = camera.kinv().astype(np.float64).reshape(3, 3).T
    pose = camera.pose().astype(np.float64).reshape(4, 4).T
    R, o = pose[:3, :3], pose[:3, 3]
    xs, ys = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    pix = np.stack([xs, ys, np.ones_like(xs)], axis=-1)               # (H, W, 3)
    d_cam = pix @ kinv.T                                              # camera-space ray, z == 1
    d = d_cam @ R.T                                                   # world-space, t == camera z
    best = np.full(xs.shape, np.inf)
    obj = np.zeros(xs.shape, np.uint8)

    # wall z = WALL_Z
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (WALL_Z - o[2]) / d[..., 2]
    ok = (t > 0) & np.isfinite(t)
    obj = np.where(ok & (t < best), WALL_B, obj)
    best = np.where(ok & (t < best), t, best)

    # sphere
    oc = o - SPHERE_C
    a = np.sum(d * d, axis=-1)
    b = 2.0 * (d @ oc)
    c = float(oc @ oc) - SPHERE_R ** 2
    disc = b * b - 4.0 * a * c
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(disc)) / (2.0 * a)
    ok = (disc >= 0) & (t > 0)
    obj = np.where(ok & (t < best), SPHERE_B, obj)
    best = np.where(ok & (t < best), t, best)

    # box (slab method)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (BOX_MIN - o) / d
        t1 = (BOX_MAX - o) / d
    tn = np.max(np.minimum(t0, t1), axis=-1)
    tf = np.min(np.maximum(t0, t1), axis=-1)
    ok = (tn <= tf) & (tn > 0)
    obj = np.where(ok & (tn < best), BOX_B, obj)
    best = np.where(ok & (tn < best), tn, best)
    return best, obj, o, d


def texture(points, blue):
    """The scene's colour at world points (..., 3) mm: r = 255 x / 3000, g = 255 y / 3000 (rounded, clamped), b = the object's
    constant blue (WALL_B / SPHERE_B / BOX_B); uint8 (..., 3)."""
    p = np.asarray(points, np.float64)
    r = np.clip(np.rint(255.0 * p[..., 0] / 3000.0), 0, 255)
    g = np.clip(np.rint(255.0 * p[..., 1] / 3000.0), 0, 255)
    return np.stack([r, g, np.asarray(blue, np.float64) + 0 * r], axis=-1).astype(np.uint8)


def trace_colour(camera, width=WIDTH, height=HEIGHT):
    """Per-pixel RGB (uint8 (H*W, 3)) of the analytic scene at the traced hit point (texture()); (0, 0, 0) where nothing is hit."""
    z, obj, o, d = _trace(camera, width, height)
    hit = np.isfinite(z)
    p = o + d * np.where(hit, z, 0.0)[..., None]          # (camera z == ray parameter: d has camera z 1)
    rgb = np.where(hit[..., None], texture(p, obj), 0)
    return rgb.astype(np.uint8).reshape(-1, 3)


def colour_frame(i, n, seed, width=WIDTH, height=HEIGHT, camera=None, inside=False):
    """-> (rgb uint8 (H*W, 3), camera): the colour frame registered to depth_frame(i, n, seed, ...) -- same camera, same pixels (a
    depth dropout keeps its colour).  Noise-free: `seed` is accepted for symmetry with depth_frame."""
    del seed
    cam = camera_for_frame(i, n, camera, inside)
    return trace_colour(cam, width, height), cam


# per-object class id of the class image (trace_classes); CLASS_VOID = nothing hit (TSDF_CLASS_VOID of include/tsdf_amd.h)
WALL_CLASS, SPHERE_CLASS, BOX_CLASS, CLASS_VOID = 1, 2, 3, 0xFFFF


def trace_classes(camera, width=WIDTH, height=HEIGHT):
    """Per-pixel class (uint16 (H*W,)) of the analytic scene, from _trace's object map: WALL_CLASS / SPHERE_CLASS / BOX_CLASS,
    CLASS_VOID where nothing is hit (exactly where trace_depth is infinite)."""
    obj = _trace(camera, width, height)[1]
    lut = np.full(256, CLASS_VOID, np.uint16)
    lut[WALL_B], lut[SPHERE_B], lut[BOX_B] = WALL_CLASS, SPHERE_CLASS, BOX_CLASS
    return lut[obj].reshape(-1)


def class_frame(i, n, seed, width=WIDTH, height=HEIGHT, camera=None, inside=False):
    """-> (classes uint16 (H*W,), camera): the class frame registered to depth_frame(i, n, seed, ...) -- same camera, same pixels (a
    depth dropout keeps its class).  Noise-free: `seed` is accepted for symmetry with depth_frame."""
    del seed
    cam = camera_for_frame(i, n, camera, inside)
    return trace_classes(cam, width, height), cam


def depth_frame(i, n, seed, width=WIDTH, height=HEIGHT, camera=None, noise=True, inside=False):
    """-> (depth uint16 (H*W,), camera) for frame i of an n-frame stream (inside: the config-4 trajectory within the volume)."""
    cam = camera_for_frame(i, n, camera, inside)
    z = trace_depth(cam, width, height)
    mm = np.where(np.isfinite(z), np.rint(z), 0.0)
    if noise:
        idx = (np.arange(width * height, dtype=np.uint64).reshape(height, width)
               + np.uint64(i) * np.uint64(width * height))
        h = splitmix64(idx ^ np.uint64(seed))
        jitter = (h % np.uint64(7)).astype(np.int64) - 3                 # +-3 mm
        drop = ((h >> np.uint64(20)) % np.uint64(1000)) < np.uint64(15)  # 1.5 % dropouts
        mm = np.where(mm > 0, mm + jitter, 0.0)
        mm = np.where(drop, 0.0, mm)
    depth = np.clip(mm, 0, 65535).astype(np.uint16).reshape(-1)
    return depth, cam


def moving_disc_frame(i, n, seed, width=WIDTH, height=HEIGHT, camera=None, noise=True, inside=False, disc_depth=900, radius=None):
    """depth_frame with something that moves: a disc of constant depth `disc_depth` (mm, nearer than the scene) pasted over the frame,
    its centre moving with i from the left third to the right third of the image on the middle row; radius: pixels (default
    height / 6).  -> (depth uint16 (H*W,), camera, disc (H*W,) bool: the pasted pixels)."""
    depth, cam = depth_frame(i, n, seed, width, height, camera, noise, inside)
    r = max(int(radius if radius is not None else height // 6), 1)
    cx = width // 3 + ((width // 3) * int(i)) // max(int(n) - 1, 1)
    cy = height // 2
    y, x = np.mgrid[0:height, 0:width]
    disc = ((x - cx) ** 2 + (y - cy) ** 2 <= r * r).reshape(-1)
    depth = np.where(disc, np.uint16(disc_depth), depth).astype(np.uint16)
    return depth, cam, disc


def wall_depth(mm=2500, width=WIDTH, height=HEIGHT):
    """The survey probe's frame: a wall at constant depth everywhere."""
    return np.full(width * height, mm, np.uint16)


def config1_depth(seed=1, width=WIDTH, height=HEIGHT):
    """BASELINE config 1 frame: wall at 2500 mm, a centred bulge of radius 120 px, hash dropouts."""
    xs, ys = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    dx, dy = xs - width / 2.0, ys - height / 2.0
    r2 = dx * dx + dy * dy
    d = np.full((height, width), 2500.0)
    inside = r2 < 120.0 ** 2
    bulge = 2000.0 - np.sqrt(np.maximum(120.0 ** 2 - r2, 0.0)) * 2.0
    d = np.where(inside, np.maximum(bulge, 400.0), d)
    h = splitmix64((np.arange(width * height, dtype=np.uint64).reshape(height, width)) ^ np.uint64(seed))
    d = np.where(h % np.uint64(50) == 0, 0.0, d)
    return np.rint(d).astype(np.uint16).reshape(-1)


def _write_png16(path, image):
    """16-bit greyscale PNG (big-endian samples, filter 0), enough for TUM-style depth maps."""
    import struct
    import zlib
    h, w = image.shape
    raw = b"".join(b"\x00" + image[y].astype(">u2").tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(chunk(b"IEND", b""))


def _write_png_rgb(path, image):
    """8-bit RGB PNG (filter 0): the colour frames of a TUM-style directory."""
    import struct
    import zlib
    h, w, _ = image.shape
    raw = b"".join(b"\x00" + image[y].astype(np.uint8).tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(chunk(b"IEND", b""))


def write_tum_directory(directory, n_frames, seed, stream_frames=None, width=WIDTH, height=HEIGHT, colour=False):
    """Writes the layout the reference's TUMDataLoader expects (src/DataLoader/TUMDataLoader.cpp:20,111-128):
    <dir>/depth/<stem>.png (uint16, 5 units per mm) and <dir>/ground_truth.txt with lines
    '<stem> tx ty tz qx qy qz qw' (metres, TUM quaternion order).  Returns the per-frame (depth_mm, pose16).
    colour=True also writes <dir>/rgb/<stem>.png (8-bit RGB, colour_frame) for TUMDataLoader::next(pose, rgb)."""
    import os
    os.makedirs(os.path.join(directory, "depth"), exist_ok=True)
    if colour:
        os.makedirs(os.path.join(directory, "rgb"), exist_ok=True)
    frames = []
    lines = ["# synthetic TUM surrogate (tsdf_amd.synth), seed 0x%X" % seed]
    total = stream_frames or n_frames
    for i in range(n_frames):
        depth, cam = depth_frame(i, total, seed, width, height)
        stem = "%010.6f" % (1305031102.0 + i / 30.0)
        _write_png16(os.path.join(directory, "depth", stem + ".png"), (depth.astype(np.uint32) * 5).clip(0, 65535)
                     .astype(np.uint16).reshape(height, width))
        if colour:
            _write_png_rgb(os.path.join(directory, "rgb", stem + ".png"), trace_colour(cam, width, height).reshape(height, width, 3))
        P = cam.pose().astype(np.float64).reshape(4, 4).T
        R, t = P[:3, :3], P[:3, 3] / 1000.0
        # rotation -> quaternion (w largest-branch free form is enough for these small rotations)
        qw = math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
        qx = (R[2, 1] - R[1, 2]) / (4.0 * qw)
        qy = (R[0, 2] - R[2, 0]) / (4.0 * qw)
        qz = (R[1, 0] - R[0, 1]) / (4.0 * qw)
        lines.append("%s %.9f %.9f %.9f %.9f %.9f %.9f %.9f" % (stem, t[0], t[1], t[2], qx, qy, qz, qw))
        frames.append((depth, cam.pose().copy()))
    with open(os.path.join(directory, "ground_truth.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return frames
