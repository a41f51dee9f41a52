"""Inputs of the scene-flow tests (no expectations live here): a pinhole camera of 40 x 30 pixels that looks along +z from a
position in the world, analytic depth frames of a sphere and of a tilted plane seen from it, and flow images."""
import numpy as np

from tests.helpers import Cam

F32 = np.float32
WIDTH, HEIGHT = 40, 30
FOCAL, CX, CY = 35.0, 20.0, 15.0


def camera(position):
    """Identity rotation, the given position: pose, its inverse, K and K^-1 as column-major float32."""
    pose = np.eye(4)
    pose[:3, 3] = position
    K = np.array([[FOCAL, 0.0, CX], [0.0, FOCAL, CY], [0.0, 0.0, 1.0]])
    col = lambda m: np.ascontiguousarray(np.asarray(m, np.float64).T, F32).reshape(-1)
    return Cam(col(pose), col(np.linalg.inv(pose)), col(K), col(np.linalg.inv(K)))


def _rays():
    u, v = np.meshgrid(np.arange(WIDTH, dtype=np.float64), np.arange(HEIGHT, dtype=np.float64))
    return np.stack([(u - CX) / FOCAL, (v - CY) / FOCAL, np.ones_like(u)], axis=-1)      # z = 1: the ray parameter is the depth


def _to_depth(t):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(t) & (t >= 1.0) & (t <= 65535.0)
    return np.where(ok, np.rint(np.where(ok, t, 0.0)), 0).astype(np.uint16)


def sphere_depth(position, centre, radius):
    """(HEIGHT, WIDTH) uint16: the depth of the near side of the sphere, 0 where the ray misses it."""
    d = _rays()
    oc = np.asarray(position, np.float64) - np.asarray(centre, np.float64)
    a = (d * d).sum(-1)
    b = 2.0 * (d * oc).sum(-1)
    c = (oc * oc).sum() - radius * radius
    disc = b * b - 4.0 * a * c
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(disc)) / (2.0 * a)
    return _to_depth(np.where(disc > 0, t, np.nan))


def plane_depth(position, point, normal):
    """(HEIGHT, WIDTH) uint16: the depth at which each ray meets the plane through `point` with `normal`."""
    d = _rays()
    n = np.asarray(normal, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((np.asarray(point, np.float64) - np.asarray(position, np.float64)) * n).sum() / (d * n).sum(-1)
    return _to_depth(t)


def constant_flow(f):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(f, F32), (HEIGHT, WIDTH, 3)))


def random_flow(seed, scale=4.0):
    return np.random.default_rng(seed).uniform(-scale, scale, (HEIGHT, WIDTH, 3)).astype(F32)


def sphere_field(size, voxel, offset, centre, radius, trunc):
    """A sphere's truncated distance at the voxel centres (i + 0.5) * voxel + offset, x fastest."""
    ax = [(np.arange(n, dtype=np.float64) + 0.5) * voxel + o for n, o in zip(size, offset)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return np.clip(d, -trunc, trunc).astype(F32).reshape(-1)
