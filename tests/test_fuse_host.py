"""Volume fusion off the GPU: the header declares tsdf_volume_fuse and the built library exports it, and the CPU reference the GPU
tests compare against (tests/fuse_ref.py) on a grid small enough to do by hand."""
import ctypes
import os
import re

import numpy as np

from tests import fuse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_header_declares_and_library_exports_tsdf_volume_fuse():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsdf_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+tsdf_volume_fuse\s*\(\s*tsdf_volume\s*\*\s*dst\s*,\s*const\s+tsdf_volume\s*\*\s*src\s*,\s*"
                     r"const\s+float\s+dst_to_src\s*\[16\]\s*,\s*uint64_t\s*\*\s*fused_voxels\s*\)\s*;", text)
    lib = ctypes.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    assert hasattr(lib, "tsdf_volume_fuse")
    from tsdf_amd import _capi
    assert "tsdf_volume_fuse" in _capi.EXPORTS
    import tsdf_amd
    assert callable(tsdf_amd.TSDFVolume.fuse)


# A 2 x 2 x 2 source with three different voxel edges: voxel (x, y, z) holds D = 1 + x + 2 y + 4 z and the weight D, except voxel
# (0, 0, 0), which was never observed (weight 0).  The destination is 3 x 2 x 2 with the same edges, distance 0.5 and weight 2
# everywhere, truncation distance 4.  The transform shifts by half a voxel along x: q.x = c.x - 5 = 0, 10, 20 for x = 0, 1, 2.
#   x = 2: q.x = 20 is the source's upper bound 2 * 10 -- outside, skipped (four voxels).
#   y and z sit on voxel centres, so only the two x taps have a non-zero share: u = (0 - 5) / 10 = -0.5 at x = 0 (the sample
#   extrapolates: 1.5 D(0, y, z) - 0.5 D(1, y, z) = D(0, y, z) - 0.5) and u = (10 - 5) / 10 = 0.5 at x = 1 (D(0, y, z) + 0.5).
#   The taps of a voxel on a centre reach one voxel up along y and z (clamped at the far face), so (x, 0, 0) reads all eight source
#   voxels, the unobserved one among them: (0, 0, 0) and (1, 0, 0) are skipped.  No other voxel has (0, 0, 0) among its taps.
#   ws is the weight of the voxel q lies in: D(0, y, z) at x = 0 (q.x = 0), D(1, y, z) at x = 1 (q.x = 10).
SRC_GEOM = ((2, 2, 2), np.array([10, 20, 40], F), np.array([0, 0, 0], F))
DST_GEOM = ((3, 2, 2), np.array([10, 20, 40], F), np.array([0, 0, 0], F))
SRC_DIST = np.arange(1, 9, dtype=F)
SRC_WEIGHT = np.array([0, 2, 3, 4, 5, 6, 7, 8], F)
SHIFT = np.eye(4, dtype=F)
SHIFT[0, 3] = -5
SHIFT = SHIFT.T.reshape(-1).copy()      # column-major
# (x, y, z): (s after the clamp to +-4, ws) -> d' = (0.5 * 2 + s ws) / (2 + ws), w' = 2 + ws
EXPECTED = {(0, 1, 0): (8.5 / 5, 5), (1, 1, 0): (15.0 / 6, 6),        # s = 2.5, 3.5
            (0, 0, 1): (21.0 / 7, 7), (1, 0, 1): (25.0 / 8, 8),       # s = 4.5, 5.5 -> 4
            (0, 1, 1): (29.0 / 9, 9), (1, 1, 1): (33.0 / 10, 10)}     # s = 6.5, 7.5 -> 4


def _hand(oracle, cap=0):
    return fuse_ref.fuse(oracle, DST_GEOM, 4.0, np.full(12, 0.5, F), np.full(12, 2, F), SRC_GEOM, SRC_DIST, SRC_WEIGHT, SHIFT, cap=cap)


def test_reference_on_a_hand_computed_grid(oracle):
    d, w, updated = _hand(oracle)
    at = lambda x, y, z: x + 3 * (y + 2 * z)
    want_d, want_w = np.full(12, 0.5, F), np.full(12, 2, F)
    for (x, y, z), (dn, wn) in EXPECTED.items():
        want_d[at(x, y, z)] = F(dn)
        want_w[at(x, y, z)] = F(wn)
    assert d.tolist() == want_d.tolist()
    assert w.tolist() == want_w.tolist()
    assert sorted(np.flatnonzero(updated).tolist()) == sorted(at(*v) for v in EXPECTED)
    # skipped for an unobserved tap, skipped for lying outside: distance and weight as they were
    for v in ((0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0), (2, 0, 1), (2, 1, 1)):
        assert d[at(*v)] == F(0.5) and w[at(*v)] == F(2) and not updated[at(*v)]


def test_reference_weight_cap_on_the_hand_computed_grid(oracle):
    """A cap of 6 stores min(w + ws, 6); the divisor stays w + ws, so the distances are those of the uncapped fuse."""
    d, w, updated = _hand(oracle, cap=6)
    d0, w0, updated0 = _hand(oracle)
    assert d.tolist() == d0.tolist() and updated.tolist() == updated0.tolist()
    assert w.tolist() == np.minimum(w0, F(6)).tolist()
    assert sorted(set(w[updated].tolist())) == [5.0, 6.0]


def test_reference_identity_default_and_rotation_helper(oracle):
    """m=None is the identity: source voxels on their own centres come back as they are where all taps are observed."""
    src_w = np.full(8, 3, F)
    d, w, updated = fuse_ref.fuse(oracle, SRC_GEOM, 100.0, np.full(8, 9, F), np.zeros(8, F), SRC_GEOM, SRC_DIST, src_w)
    assert updated.all() and d.tolist() == SRC_DIST.tolist() and w.tolist() == src_w.tolist()
    m = fuse_ref.rotation((0, 0, 1), 90.0, (1, 2, 3)).reshape(4, 4).T    # rows again
    assert np.allclose(m[:3, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-7) and m[:3, 3].tolist() == [1, 2, 3]
    assert m[3].tolist() == [0, 0, 0, 1]
