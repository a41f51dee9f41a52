"""The inputs of the sparse-snapshot tests (tests/test_snapshot.py on the GPU; their properties are checked on the CPU in
tests/test_snapshot_ref_host.py): grids, the anisotropic geometry and the random fields per grid and
storage.  Inputs only; no expectations live here."""
import numpy as np

from tests import snapshot_ref as R

F32 = np.float32
# The smallest grids at which the kernels can go wrong: less than a brick, one brick, a second brick one voxel wide; partial bricks on
# every axis with Z no multiple of 4 or 2 (the packed z-groups); rows shorter than, equal to and longer than a wave (the flag kernel's
# lanes run along x, 64 at a time); a mid-sized odd grid; and 1320 bricks, more than the 1024 chunks of one scan workgroup.
GRIDS = [(2, 2, 2), (8, 8, 8), (9, 8, 8), (7, 9, 17), (64, 8, 8), (65, 3, 5), (129, 7, 3), (40, 33, 21), (264, 64, 40)]
VS = np.array([10.0, 12.5, 9.0], F32)
OFFSET = (100.0, -50.0, 25.0)
# 1.1 * |VS| in fp32, as the library forms it (checked against the volume's own value on the GPU)
FILL = F32(1.1) * np.sqrt(VS[0] * VS[0] + VS[1] * VS[1] + VS[2] * VS[2], dtype=F32)


def physical(size):
    return (size[0] * 10.0, size[1] * 12.5, size[2] * 9.0)


def total_bricks(size):
    nb = R.bricks_per_axis(size)
    return nb[0] * nb[1] * nb[2]


def seed_of(size, bits):
    return 9108 + 13 * size[0] + 5 * size[1] + size[2] + bits


def random_case(size, bits, colour, fill=FILL):
    """(dist, weight, colour or None) for a grid and a weight storage; with more than one brick some are live and some are not."""
    share = 1.0 if total_bricks(size) == 1 else 0.45
    return R.random_field(size, seed_of(size, bits), bits, colour, fill, live_share=share)
