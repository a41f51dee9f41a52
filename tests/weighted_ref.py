"""CPU reference of weighted integration (include/tsdf_amd.h, "weighted integration"), over the oracle's integrate.  Test infrastructure only.

The frame's voxel set and its tsdf values come from tests/deintegrate_ref.frame_set on the MASKED image (depth zeroed wherever the pixel's
weight is not finite and > 0); each voxel's pixel comes from tests/colour_ref.update_sets on the same image, and the two sets are asserted
to agree.  The blend and the two weight models are the header's formulas in numpy fp32, every operation rounded on its own.
"""
import numpy as np

from tests import colour_ref
from tests.deintegrate_ref import frame_set
from tests.helpers import H, W

F = np.float32
INVERSE_SQUARE, COSINE = 1, 2


def valid_pixels(depth, weights):
    d = np.asarray(depth, np.uint16).reshape(-1)
    p = np.asarray(weights, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (d > 0) & np.isfinite(p) & (p > F(0.0))


def masked_depth(depth, weights):
    d = np.asarray(depth, np.uint16).reshape(-1)
    return np.where(valid_pixels(d, weights), d, np.uint16(0)).astype(np.uint16)


def centres_of(ov):
    """(N, 3) fp32 voxel centres of an oracle.Volume as integrate forms them (whole volumes)."""
    g = ov.g
    if ov.translation is not None:
        return (np.asarray(ov.translation, F).reshape(-1, 3) + np.array(g.offset, F)).astype(F)
    return colour_ref.voxel_centres(tuple(g.dims), np.array(g.vs, F), np.array(g.offset, F), np.array(g.offset_at_clear, F))


def frame(O, ov, depth, weights, cam, width=W, height=H):
    """-> (in_set, tsdf, pixel index) of a weighted frame on `ov`'s grid (`ov` is left as it was)."""
    md = masked_depth(depth, weights)
    in_set, tsdf = frame_set(O, ov, md, cam, width, height)
    updated, _, pidx = colour_ref.update_sets(O, centres_of(ov), F(ov.truncation_distance()), md, width, height, cam.inverse_pose(), cam.k(),
                                              cam.kinv())
    assert np.array_equal(updated, in_set), "the oracle's integrate and colour_ref.update_sets disagree about the frame's voxels"
    return in_set, tsdf, pidx


def blend(ov, in_set, tsdf, p_voxel, cap=0):
    """The header's blend on ov.dist / ov.weight.  Returns (voxels updated, distance stores made)."""
    with np.errstate(all="ignore"):
        w, D = ov.weight, ov.dist
        p = np.where(in_set, p_voxel, F(1.0)).astype(F)
        nw = (w + p).astype(F)
        new_d = (((D * w).astype(F) + (tsdf * p).astype(F)).astype(F) / nw).astype(F)
        stored = nw if not cap else np.where(nw > F(cap), F(cap), nw).astype(F)
    stores = int((in_set & (new_d.view(np.uint32) != D.view(np.uint32))).sum())
    ov.dist[:] = np.where(in_set, new_d, D)
    ov.weight[:] = np.where(in_set, stored, w)
    return int(in_set.sum()), stores


def integrate(O, ov, depth, weights, cam, cap=0, width=W, height=H):
    """One weighted integrate of `ov` (oracle.Volume).  Returns (updated voxels, distance stores)."""
    in_set, tsdf, pidx = frame(O, ov, depth, weights, cam, width, height)
    p = np.asarray(weights, F).reshape(-1)[pidx]
    return blend(ov, in_set, tsdf, p, cap)


def _points(d, kinv, width, height):
    """pixel_to_camera of every pixel as tsdf_depth_to_points_device forms it; (h, w) arrays x, y, z (garbage where d == 0)."""
    k = np.asarray(kinv, F).reshape(-1)          # column-major: m11 = k[0], m21 = k[1], m31 = k[2], m12 = k[3], ...
    px, py = np.meshgrid(np.arange(width).astype(F), np.arange(height).astype(F))
    ip = [((k[r] * px).astype(F) + (k[3 + r] * py).astype(F)).astype(F) + k[6 + r] for r in range(3)]
    scale = (d / ip[2]).astype(F)
    return [(c * scale).astype(F) for c in ip]


def depth_weights(depth, width, height, kinv, flags, z_ref=0.0):
    """tsdf_depth_weights in numpy fp32, in the header's operation order: (height, width) float32."""
    raw = np.asarray(depth, np.uint16).reshape(height, width)
    d = raw.astype(F)
    has = raw != 0
    with np.errstate(all="ignore"):
        w = np.ones((height, width), F)
        if flags & INVERSE_SQUARE:
            r = (F(z_ref) / d).astype(F)
            f = (r * r).astype(F)
            f = np.where(f > F(1.0), F(1.0), f).astype(F)
            w = (w * f).astype(F)
        if flags & COSINE:
            X, Y, Z = _points(d, kinv, width, height)
            ok = np.zeros((height, width), bool)
            ok[1:-1, 1:-1] = has[1:-1, 1:-1] & has[1:-1, :-2] & has[1:-1, 2:] & has[:-2, 1:-1] & has[2:, 1:-1]
            sh = lambda A, dy, dx: np.roll(A, (-dy, -dx), (0, 1))            # A(x + dx, y + dy); the wrapped border is masked by `ok`
            a = [(sh(A, 0, 1) - sh(A, 0, -1)).astype(F) for A in (X, Y, Z)]
            b = [(sh(A, 1, 0) - sh(A, -1, 0)).astype(F) for A in (X, Y, Z)]
            mul = lambda u, v: (u * v).astype(F)
            nx = (mul(a[1], b[2]) - mul(a[2], b[1])).astype(F)
            ny = (mul(a[2], b[0]) - mul(a[0], b[2])).astype(F)
            nz = (mul(a[0], b[1]) - mul(a[1], b[0])).astype(F)
            dot3 = lambda u, v: ((mul(u[0], v[0]) + mul(u[1], v[1])).astype(F) + mul(u[2], v[2])).astype(F)
            n, P = (nx, ny, nz), (X, Y, Z)
            np_, nn, pp = dot3(n, P), dot3(n, n), dot3(P, P)
            c = (np.abs(np_) / (np.sqrt(nn).astype(F) * np.sqrt(pp).astype(F)).astype(F)).astype(F)
            c = np.where(c > F(1.0), F(1.0), c).astype(F)
            c = np.where(ok & (c > F(0.0)), c, F(0.0)).astype(F)
            w = (w * c).astype(F)
    return np.where(has, w, F(0.0)).astype(F)
