"""CPU reference of the weight cap (include/tsdf_amd.h, "weight cap"), over the oracle's integrate.  Test infrastructure only.

The capped integrate is ONE ORACLE INTEGRATE FOLLOWED BY A CLAMP OF THE ORACLE'S WEIGHT ARRAY: the oracle blends with the prior
weight -- the divisor is prior + 1, never clamped -- and the clamp only touches what the next frame will read.  The clamp is
np.minimum(weight, cap) on the voxels the frame updated (the ones whose weight the integrate changed); where no weight exceeds the
cap beforehand that is np.minimum over the whole array.  A voxel the frame did not update keeps an uploaded weight above the cap, as
the header says.  (An fp32 weight of 2^24 and more, which + 1 leaves as it is, would pass for not updated: not used here.)
np.minimum keeps a NaN a NaN, like the kernels' comparison.
"""
import numpy as np

from tests.helpers import H, W


def oracle_step(O, ov, depth, cam, cap=0, width=W, height=H):
    """One integrate of `ov` (oracle.Volume) with weight cap `cap` (0: none)."""
    before = ov.weight.view(np.uint32).copy()
    ov.integrate(depth, width, height, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=O.max_threads())
    if cap:
        updated = ov.weight.view(np.uint32) != before
        w = ov.weight.copy()
        w[updated] = np.minimum(w[updated], np.float32(cap))
        ov.set_weight_data(w)
    return ov
