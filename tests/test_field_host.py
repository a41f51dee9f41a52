"""Field queries off the GPU: the PLY writers with normals through the flat host wrappers, the unchanged bytes of the writers that
were there before, and the CPU reference the GPU tests compare against (tests/field_ref.py) on a grid small enough to do by hand."""
import numpy as np

from tests import field_ref

F = np.float32
MESH_V = np.array([[0, 0, 0], [1.5, 0, 0], [0, 2.25, 0], [1.5, 2.25, -0.5]], np.float32)
MESH_T = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
MESH_C = np.array([[255, 0, 0], [0, 128, 0], [0, 0, 7], [10, 20, 30]], np.uint8)
MESH_N = np.array([[0, 0, 1], [0.5, -0.25, 0.125], [np.nan, np.nan, np.nan], [-1, 1e-7, 3.0e10]], np.float32)
HEAD = "ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
FACES = "element face 2\nproperty list uchar int vertex_indices\nend_header\n"
TAIL = "3 0 1 2\n3 1 3 2\n"
# what the three-argument and the coloured writer produced for this mesh before the writers with normals were added
PLAIN_BEFORE = HEAD + FACES + "0 0 0\n1.5 0 0\n0 2.25 0\n1.5 2.25 -0.5\n" + TAIL
COLOURED_BEFORE = (HEAD + "property uchar red\nproperty uchar green\nproperty uchar blue\n" + FACES +
                   "0 0 0 255 0 0\n1.5 0 0 0 128 0\n0 2.25 0 0 0 7\n1.5 2.25 -0.5 10 20 30\n" + TAIL)


def test_ply_with_normals_header_order_and_line_format(tmp_path):
    from tsdf_amd import _capi
    path = str(tmp_path / "n.ply")
    assert _capi.host.tsdf_host_write_ply_normals(path.encode(), MESH_V.ctypes.data, 4, MESH_T.ctypes.data, 2, MESH_N.ctypes.data) == 0
    # nx / ny / nz after z; values printed like the coordinates (the stream's default float format)
    assert open(path, "rb").read() == (HEAD + "property float nx\nproperty float ny\nproperty float nz\n" + FACES +
                                       "0 0 0 0 0 1\n1.5 0 0 0.5 -0.25 0.125\n0 2.25 0 nan nan nan\n1.5 2.25 -0.5 -1 1e-07 3e+10\n" +
                                       TAIL).encode()
    both = str(tmp_path / "nc.ply")
    assert _capi.host.tsdf_host_write_ply_normals_coloured(both.encode(), MESH_V.ctypes.data, 4, MESH_T.ctypes.data, 2,
                                                           MESH_N.ctypes.data, MESH_C.ctypes.data) == 0
    # ... and before the colour properties
    assert open(both, "rb").read() == (HEAD + "property float nx\nproperty float ny\nproperty float nz\n"
                                       "property uchar red\nproperty uchar green\nproperty uchar blue\n" + FACES +
                                       "0 0 0 0 0 1 255 0 0\n1.5 0 0 0.5 -0.25 0.125 0 128 0\n0 2.25 0 nan nan nan 0 0 7\n"
                                       "1.5 2.25 -0.5 -1 1e-07 3e+10 10 20 30\n" + TAIL).encode()
    # null arrays are refused, not dereferenced
    assert _capi.host.tsdf_host_write_ply_normals(path.encode(), MESH_V.ctypes.data, 4, MESH_T.ctypes.data, 2, None) == -1
    assert _capi.host.tsdf_host_write_ply_normals_coloured(both.encode(), MESH_V.ctypes.data, 4, MESH_T.ctypes.data, 2,
                                                           MESH_N.ctypes.data, None) == -1


def test_the_earlier_ply_writers_still_write_the_same_bytes(tmp_path):
    from tsdf_amd import _capi
    plain, coloured = str(tmp_path / "p.ply"), str(tmp_path / "c.ply")
    _capi.host.tsdf_host_write_ply(plain.encode(), MESH_V.ctypes.data, 4, MESH_T.ctypes.data, 2)
    assert open(plain, "rb").read() == PLAIN_BEFORE.encode()
    assert _capi.host.tsdf_host_write_ply_coloured(coloured.encode(), MESH_V.ctypes.data, 4, MESH_T.ctypes.data, 2,
                                                   MESH_C.ctypes.data) == 0
    assert open(coloured, "rb").read() == COLOURED_BEFORE.encode()


# a 2 x 2 x 2 grid with three different voxel edges; voxel (x, y, z) holds 1 + x + 2 y + 4 z, its weight ten times that
DIMS, VS, OFFSET = (2, 2, 2), np.array([10, 20, 40], F), np.array([100, -50, 7], F)
DIST = np.arange(1, 9, dtype=F)
WEIGHT = DIST * F(10)


def _sample(oracle, q, offset=OFFSET, **kw):
    """field_ref at grid points q.  The offset is added here and subtracted again by the query: exact for the round values of the
    tests that keep it, zero where a test is about the last bit of q."""
    offset = np.asarray(offset, F)
    return field_ref.sample(oracle, (DIMS, VS, offset), DIST, WEIGHT, np.asarray(q, F).reshape(-1, 3) + offset, **kw)


def test_reference_on_a_hand_computed_grid_voxel_centres(oracle):
    """At a voxel's centre the sample is the voxel's own distance exactly: weight (1 - 0) on it, zeros on the other seven taps."""
    q = [[(x + 0.5) * 10, (y + 0.5) * 20, (z + 0.5) * 40] for z in range(2) for y in range(2) for x in range(2)]
    d, g, w = _sample(oracle, q)
    assert d.tolist() == DIST.tolist()
    assert w.tolist() == WEIGHT.tolist()
    # every point of a grid two voxels wide is within one voxel of a face: no gradient anywhere
    assert np.isnan(g).all()
    assert np.isnan(_sample(oracle, q, unit_gradient=True)[1]).all()


def test_reference_on_a_hand_computed_grid_invalid_points(oracle):
    bad = [[20, 10, 20], [5, 40, 20], [5, 10, 80],            # the exact upper bound size * voxel_size, per axis
           [-0.001, 10, 20], [5, -1, 20], [5, 10, -1e-30],
           [np.nan, 10, 20], [5, np.inf, 20], [5, 10, -np.inf]]
    d, g, w = _sample(oracle, bad, offset=(0, 0, 0))
    assert np.isnan(d).all() and np.isnan(g).all()
    assert w.tolist() == [0.0] * len(bad)
    # -0.0 is >= 0: valid, in voxel 0 of that axis; the largest float below the bound is valid too
    ok = [[-0.0, 10, 20], [np.nextafter(F(20), F(0)), 10, 20]]
    d, g, w = _sample(oracle, ok, offset=(0, 0, 0))
    assert not np.isnan(d).any() and np.isnan(g).all()
    assert w.tolist() == [10.0, 20.0]


def test_reference_on_a_hand_computed_grid_tap_clamping_at_the_far_faces(oracle):
    """Beyond the last voxel centre the upper tap is clamped onto the lower one: along x at (17, 10, 20) both taps are voxel
    (1, 0, 0) = 2, weighted 1 - u and u with u = (17 - 15) / 10; v = w = 0 on the centres of y and z."""
    u = F(F(F(17) - F(15)) / F(10))
    expected = F(F(F(2) * F(F(1) - u)) + F(F(2) * u))
    d, _, w = _sample(oracle, [[17, 10, 20]])
    assert d[0] == expected and abs(float(d[0]) - 2.0) < 1e-6
    assert w[0] == 20.0
    # the same along y and z: voxel (0, 1, 0) = 3 at (5, 36, 20), voxel (0, 0, 1) = 5 at (5, 10, 72)
    d, _, w = _sample(oracle, [[5, 36, 20], [5, 10, 72]])
    assert abs(float(d[0]) - 3.0) < 1e-6 and abs(float(d[1]) - 5.0) < 1e-6
    assert w.tolist() == [30.0, 50.0]
    # below the first centre the reference extrapolates from the first two voxels (u < 0): (2, 10, 20) -> 1 + (2 - 5) / 10 = 0.7
    d, _, _ = _sample(oracle, [[2, 10, 20]])
    assert abs(float(d[0]) - 0.7) < 1e-6
