"""CPU reference of colour fusion (include/tsdf_amd.h, "colour fusion"), pure numpy over the oracle's pinned transforms.

The voxels a colour integrate updates are the ones the distance update touches -- pixel from world_to_pixel_n, frustum test,
depth > 0, sdf = pixel_to_camera_n(...).z - world_to_camera_n(...).z >= -trunc (src/TSDF/TSDFVolume.cu:337-366) -- with
sdf <= +trunc as well; the blend is integer arithmetic.  Test infrastructure only (uses oracle/).
"""
import numpy as np


def voxel_centres(dims, vs, offset, offset_at_clear):
    """(N, 3) float32 centres, x fastest: ((i + 0.5) * vs + offset_at_clear) + offset per axis, each op rounded to fp32."""
    axes = []
    for a in range(3):
        i = np.arange(dims[a], dtype=np.float32)
        axes.append(((i + np.float32(0.5)) * np.float32(vs[a]) + np.float32(offset_at_clear[a])) + np.float32(offset[a]))
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)


def geometry(volume):
    """(dims, vs, offset, offset_at_clear, trunc) of a tsdf_amd.TSDFVolume."""
    i = volume.info()
    return (tuple(int(s) for s in i.size), np.array(i.voxel_size, np.float32), np.array(i.offset, np.float32),
            np.array(i.offset_at_clear, np.float32), np.float32(i.truncation_distance))


def update_sets(O, centres, trunc, depth, width, height, inv_pose, k, kinv):
    """-> (updated, coloured, pixel): the distance update's voxels, the colour update's voxels (a subset) and each voxel's pixel
    index (valid where updated)."""
    pix = O.world_to_pixel_n(centres, inv_pose, k)
    inb = (pix[:, 0] >= 0) & (pix[:, 0] < width) & (pix[:, 1] >= 0) & (pix[:, 1] < height)
    pidx = np.where(inb, pix[:, 1].astype(np.int64) * width + pix[:, 0], 0)
    d = np.asarray(depth, np.uint16).reshape(-1)[pidx]
    sel = np.nonzero(inb & (d > 0))[0]
    surf_z = O.pixel_to_camera_n(pix[sel], d[sel].astype(np.float32), kinv)[:, 2]
    cam_z = O.world_to_camera_n(centres[sel], inv_pose)[:, 2]
    sdf = (surf_z - cam_z).astype(np.float32)
    up = sdf >= -np.float32(trunc)
    updated = np.zeros(len(centres), bool)
    coloured = np.zeros(len(centres), bool)
    updated[sel[up]] = True
    coloured[sel[up & (sdf <= np.float32(trunc))]] = True
    return updated, coloured, pidx


def blend(colour, coloured, pidx, rgb):
    """The integer blend of include/tsdf_amd.h on uint32 {r, g, b, n} words: a new array."""
    out = np.array(colour, np.uint32, copy=True)
    idx = np.nonzero(coloured)[0]
    old = out[idx]
    n = old >> np.uint32(24)
    n1 = n + np.uint32(1)
    half = n1 >> np.uint32(1)
    c = np.asarray(rgb, np.uint8).reshape(-1, 3)[pidx[idx]].astype(np.uint32)
    new = np.minimum(n1, np.uint32(255)) << np.uint32(24)
    for ch in range(3):
        o = (old >> np.uint32(8 * ch)) & np.uint32(0xFF)
        new |= ((o * n + c[:, ch] + half) // n1) << np.uint32(8 * ch)
    out[idx] = new
    return out


def integrate_colour(O, colour, geom, depth, rgb, width, height, camera):
    """One colour integrate on the CPU: -> (new colour words, updated mask, coloured mask)."""
    dims, vs, offset, offset_at_clear, trunc = geom
    centres = voxel_centres(dims, vs, offset, offset_at_clear)
    updated, coloured, pidx = update_sets(O, centres, trunc, depth, width, height, camera.inverse_pose(), camera.k(), camera.kinv())
    return blend(colour, coloured, pidx, rgb), updated, coloured


def sample(colour, geom, points):
    """sample_colours on the CPU: (n, 3) float32 points -> (n, 3) uint8."""
    dims, vs, offset, offset_at_clear, _ = geom
    p = np.asarray(points, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(((p - offset) - offset_at_clear) / vs).astype(np.float32)
        ok = np.all((f >= 0) & (f < np.array(dims, np.float32)), axis=1)
    fi = np.where(ok[:, None], f, 0).astype(np.int64)
    w = np.asarray(colour, np.uint32)[fi[:, 0] + dims[0] * (fi[:, 1] + dims[1] * fi[:, 2])]
    w = np.where(ok & ((w >> np.uint32(24)) != 0), w, np.uint32(0))
    return np.stack([(w >> np.uint32(8 * ch)) & np.uint32(0xFF) for ch in range(3)], axis=1).astype(np.uint8)
