"""The inputs of the fusion-across-a-shift tests (tests/test_rolling.py on the GPU; that its identities hold for these inputs is checked
with the oracle's integrate in tests/test_rolling_ref_host.py): voxels of exactly 4 mm, integer offsets and offset_at_clear zero, so
every voxel centre (((i + 0.5) 4) + 0) + offset is exact in fp32 and a voxel of the rolling volume has the centre of the static
volume's voxel it lies on, bit for bit.  Inputs only; no expectations live here."""
import numpy as np

import tsdf_amd

W, H = 640, 480
VOXEL = 4.0
STATIC_SIZE, ROLLING_SIZE = (48, 32, 32), (32, 32, 32)
OFFSET = (-96.0, -64.0, 300.0)          # the camera sits at the origin and looks along +z: the volumes are 300 mm in front of it
BOX_SHIFT = (1, 0, 0)
FRAMES = 6                               # three before the shift, three after


def physical(size):
    return tuple(VOXEL * s for s in size)


def camera():
    cam = tsdf_amd.Camera.default_depth_camera()
    cam.set_pose(np.eye(4, dtype=np.float32).reshape(-1))
    return cam


def depth_frame(f):
    """A stepped, slanted surface 340 .. 390 mm from the camera that moves 5 mm a frame; covers the whole image."""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (340 + (u // 16) % 8 + v // 60 + 5 * f + 20 * (u > 400)).astype(np.uint16).reshape(-1)
