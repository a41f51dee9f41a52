"""ICP (tsdf_amd/csrc/icp.hip) against the CPU oracle at the sizes where its kernels take other paths than at 640 x 480, and at poses
that push its gates and guards.  tests/icp_cases.py has the scene, the sizes and why each is there; tests/test_icp_cases_host.py checks
without a GPU that those inputs are sound.

  * pyramid and maps, every size: floor-halved levels, odd source widths in icp_pyr_down_kernel, images narrower or flatter than the
    64 x 4 tile of the map kernels -- bit for bit;
  * one step, every size x level: fewer pixels than a workgroup / than one pass of the 256 x 256 grid, the first pixels of the second
    grid-stride trip (321 x 205) -- the same inliers as the oracle, sums within test_parity_icp.py's rule;
  * gates and guards: p2 <= 0, 0/0 at the principal point, projections that saturate float2int_rn, NaN, both sides of the distance and
    the angle gate;
  * chains: identical frames and an all-zero frame at every size / exactly, a moving scene against the oracle's chain at the sizes
    whose levels are all healthy (SIZES_CHAIN) -- only there: below 37 x 21 the system has a condition number of 1e9 .. 1e10, the oracle's
    own chain ends metres away, and the device (unpivoted solve where the pivots allow it) legitimately differs from it.
"""
import numpy as np
import pytest

import tsdf_amd
from tests import icp_cases as K
from tests.helpers import assert_same_floats

pytestmark = pytest.mark.gpu
_size_id = lambda s: "%dx%d" % s
_MAPS = ("vmap_curr", "nmap_curr", "vmap_prev", "nmap_prev")


def _odometry(size, intr=None):
    W, H = size
    return tsdf_amd.ICPOdometry(W, H, *(intr or K.intrinsics(W)))


_rigs = {}


def _rig(size):
    """One ICPOdometry a size, model and current frame of the moving scene initialised (shared by the step tests: nothing changes it)."""
    if size not in _rigs:
        W, H = size
        icp = _odometry(size)
        icp.init_icp_model(K.depth_frame(W, H, K.MODEL_SHIFT))
        icp.init_icp(K.depth_frame(W, H, K.CURRENT_SHIFT))
        _rigs[size] = icp
    return _rigs[size]


@pytest.mark.parametrize("size", K.SIZES_ALL, ids=_size_id)
def test_pyramid_and_maps_are_bit_exact(oracle, size):
    W, H = size
    intr = K.intrinsics(W)
    icp = _odometry(size)
    for shift, init, vmap, nmap in ((K.MODEL_SHIFT, icp.init_icp_model, "vmap_prev", "nmap_prev"),
                                    (K.CURRENT_SHIFT, icp.init_icp, "vmap_curr", "nmap_curr")):
        d = K.depth_frame(W, H, shift)
        init(d)
        for level, (do, vo, no) in enumerate(K.oracle_pyramid(oracle, d, W, H, intr)):
            assert do.shape == (H >> level, W >> level)
            assert np.array_equal(icp.get_depth_level(level), do), "%s depth level %d" % (vmap, level)
            assert_same_floats(icp.get_map(vmap, level), vo, "%s level %d" % (vmap, level))
            assert_same_floats(icp.get_map(nmap, level), no, "%s level %d" % (nmap, level))


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("size", K.SIZES_ALL, ids=_size_id)
def test_one_step_matches_the_oracle_sums(oracle, size, level):
    W, H = size
    icp = _rig(size)
    T = oracle.se3_exp(K.PROBE_TWIST)
    R, t = K.pose_floats(T)
    A, b, res, inl = icp.estimate_step(level, R, t)
    maps = [icp.get_map(k, level) for k in _MAPS]
    Ao, bo, reso, inlo = K.oracle_step(oracle, T, maps, W, H, K.intrinsics(W), level)
    print("%dx%d level %d: %d inliers of %d pixels" % (W, H, level, inl, (H >> level) * (W >> level)))
    assert inl == inlo                                  # the same pixels pass the gates
    if size in K.SIZES_CHAIN:
        assert inl >= 0.5 * (H >> level) * (W >> level)
    if inlo > 0:
        K.sums_close(A, b, res, Ao, bo, reso)
    else:
        assert not A.any() and not b.any() and res == 0
    assert np.array_equal(A, A.T)
    A2, b2, res2, inl2 = icp.estimate_step(level, R, t)      # deterministic: a second call gives the same bits
    assert np.array_equal(A.view(np.uint32), A2.view(np.uint32)) and np.array_equal(b.view(np.uint32), b2.view(np.uint32))
    assert res == res2 and inl == inl2


@pytest.mark.parametrize("case", K.GATE_CASES, ids=lambda c: c[0])
def test_gates_and_guards(oracle, case):
    """A 2 m plane against itself, the principal point on a pixel.  None of these poses can make the kernel read out of bounds: the
    range test on px / py (float2int_rn saturates, NaN -> 0) comes before every load through them; the test pins the arithmetic."""
    _, T, _ = case
    W, H = K.GATE_SIZE
    if "gate" not in _rigs:
        icp = _odometry(K.GATE_SIZE, K.GATE_INTRINSICS)
        icp.init_icp_model(K.gate_depth())
        icp.init_icp(K.gate_depth())
        _rigs["gate"] = icp
    icp = _rigs["gate"]
    R, t = K.pose_floats(T)
    A, b, res, inl = icp.estimate_step(0, R, t)
    maps = [icp.get_map(k, 0) for k in _MAPS]
    Ao, bo, reso, inlo = K.oracle_step(oracle, T, maps, W, H, K.GATE_INTRINSICS, 0)
    assert inl == inlo
    if inlo > 0:
        K.sums_close(A, b, res, Ao, bo, reso)
    else:
        assert not A.any() and not b.any() and res == 0


@pytest.mark.parametrize("size", K.SIZES_ALL, ids=_size_id)
def test_identical_frames_give_the_identity_exactly(oracle, size):
    W, H = size
    d = K.depth_frame(W, H, K.MODEL_SHIFT)
    icp = _odometry(size)
    icp.init_icp_model(d)
    icp.init_icp(d)
    T = icp.get_incremental_transformation()
    _, _, inlo = oracle.icp_incremental_transformation(d, d, W, H, *K.intrinsics(W))
    assert np.array_equal(T, np.eye(4)), T
    assert icp.last_error == 0.0
    assert icp.last_inliers == inlo and inlo > 0


def test_all_zero_current_frame_leaves_the_pose_alone(oracle):
    W, H = K.GATE_SIZE
    icp = _odometry(K.GATE_SIZE)
    icp.init_icp_model(K.depth_frame(W, H, K.MODEL_SHIFT))
    icp.init_icp(np.zeros((H, W), np.uint16))
    start = oracle.se3_exp(K.ZERO_FRAME_START_TWIST)
    T = icp.get_incremental_transformation(start)
    assert np.array_equal(T.view(np.uint64), start.view(np.uint64))
    assert icp.last_inliers == 0 and np.isnan(icp.last_error)        # sqrt(0) / 0, as in the oracle


@pytest.mark.parametrize("size", K.SIZES_CHAIN, ids=_size_id)
def test_moving_scene_chain_matches_the_oracle(oracle, size):
    W, H = size
    model, current = K.depth_frame(W, H, K.MODEL_SHIFT), K.depth_frame(W, H, K.CURRENT_SHIFT)
    icp = _odometry(size)
    runs = []
    for rep in range(2):                                             # twice on one object: its buffers are used again
        icp.init_icp_model(model)
        icp.init_icp(current)
        runs.append((icp.get_incremental_transformation(), icp.last_error, icp.last_inliers))
    T, err, inl = runs[0]
    To, erro, inlo = oracle.icp_incremental_transformation(current, model, W, H, *K.intrinsics(W))
    dt, dr = np.max(np.abs(T[:3, 3] - To[:3, 3])), np.max(np.abs(T[:3, :3] - To[:3, :3]))
    print("%dx%d chain against the oracle: translation %.3g, rotation %.3g, inliers %d / %d" % (W, H, dt, dr, inl, inlo))
    assert dt < K.CHAIN_TOL_T and dr < K.CHAIN_TOL_R, (T, To)
    assert abs(inl - inlo) <= max(0.002 * inlo, 2)
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12, rtol=0) and np.array_equal(T[3], [0, 0, 0, 1])
    assert np.max(np.abs(T[:3, 3])) > 1e-3                           # (a real motion was estimated)
    T2, err2, inl2 = runs[1]
    assert np.array_equal(T.view(np.uint64), T2.view(np.uint64)) and err == err2 and inl == inl2
