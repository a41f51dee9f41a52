"""CPU reference of de-integration (include/tsdf_amd.h, "de-integration"), over the oracle's integrate.  Test infrastructure only.

The frame's voxel set and its tsdf values come from ONE ORACLE INTEGRATE OF THE SAME VOLUME OBJECT WITH ITS ARRAYS CLEARED (same grid,
offsets, slab and deformation nodes): where the weight became 1 the voxel is in the set and its distance is the frame's tsdf.  The oracle
computes (trunc * 0 + tsdf * 1) / (0 + 1) there: trunc * 0 = +0, tsdf * 1 = tsdf, / 1 keeps the bits, and +0 + tsdf = tsdf bit for bit
unless tsdf is -0, which would come out as +0.  The kernels' sdf is a difference a - b of a surface depth a > 0 ((float)depth, or
ipz * (depth / ipz) for a general camera -- positive, as both factors carry ipz's sign) and the voxel's camera z: IEEE subtraction
gives -0 only for (-0) - (+0), and a is not a zero, so sdf -- and min(sdf, trunc) -- is never -0 and nothing is lost.  (Checked on the
frames of tests/test_deintegrate_host.py: no tsdf in a set has the bits of either zero's negative.)

The removal itself is the header's formula in numpy fp32, every operation rounded on its own.
"""
import numpy as np

from tests.helpers import H, W


def frame_set(O, ov, depth, cam, width=W, height=H):
    """(in_set, tsdf) of a frame on `ov`'s grid: boolean mask and the fp32 tsdf values (valid inside the mask).  `ov` is left as it was."""
    keep_d, keep_w = ov.dist.copy(), ov.weight.copy()
    ov.dist[:] = np.float32(ov.truncation_distance())
    ov.weight[:] = 0.0
    ov.integrate(depth, width, height, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=O.max_threads())
    in_set = ov.weight == 1.0
    tsdf = ov.dist.copy()
    ov.dist[:] = keep_d
    ov.weight[:] = keep_w
    assert not np.any(tsdf[in_set].view(np.uint32) == 0x80000000), "a tsdf of -0: the set's values need another source"
    return in_set, tsdf


def remove(ov, in_set, tsdf):
    """Apply the header's formula to ov.dist / ov.weight.  Returns (voxels whose weight went down, distance stores made)."""
    trunc = np.float32(ov.truncation_distance())
    with np.errstate(all="ignore"):
        w, D = ov.weight, ov.dist
        act = in_set & (w >= np.float32(1.0))                     # (False for NaN)
        nw = (w - np.float32(1.0)).astype(np.float32)
        inv = (((D * w).astype(np.float32) - (tsdf * np.float32(1.0)).astype(np.float32)).astype(np.float32) / nw).astype(np.float32)
        new_d = np.where(nw > np.float32(0.0), inv, trunc).astype(np.float32)
        new_w = np.where(nw > np.float32(0.0), nw, np.float32(0.0)).astype(np.float32)
    stores = int((act & (new_d.view(np.uint32) != D.view(np.uint32))).sum())
    ov.dist[:] = np.where(act, new_d, D)
    ov.weight[:] = np.where(act, new_w, w)
    return int(act.sum()), stores


def oracle_remove(O, ov, depth, cam, width=W, height=H):
    """One de-integrate of `ov` (oracle.Volume).  Returns (updated voxels, distance stores)."""
    in_set, tsdf = frame_set(O, ov, depth, cam, width, height)
    return remove(ov, in_set, tsdf)
