"""The inputs of test_icp_sizes.py and test_gn_finish.py are sound (tests/icp_cases.py; oracle, numpy and mpmath only, no GPU): the sizes
whose chain poses are compared are healthy at every level, the gate cases sit on the side of their gate they are named for, the
restated second stage depends on the order it pins, and the numpy restatement of the device's exponential is accurate against a
60-digit evaluation.  A size or case that fails one of these is replaced in icp_cases.py, never excused here."""
import numpy as np
import pytest

from tests import icp_cases as K


def _frames(size):
    W, H = size
    return K.depth_frame(W, H, K.MODEL_SHIFT), K.depth_frame(W, H, K.CURRENT_SHIFT)


@pytest.mark.parametrize("size", K.SIZES_CHAIN, ids=lambda s: "%dx%d" % s)
def test_chain_sizes_are_healthy_at_every_level(oracle, size):
    """cond2(A) <= 1e3 and at least half of the level's pixels inliers, at the probe pose (observed: 38 .. 250, 68 .. 87 %)."""
    W, H = size
    intr = K.intrinsics(W)
    model, current = _frames(size)
    pm, pc = K.oracle_pyramid(oracle, model, W, H, intr), K.oracle_pyramid(oracle, current, W, H, intr)
    T = oracle.se3_exp(K.PROBE_TWIST)
    for level in range(3):
        A, b, res, inl = K.oracle_step(oracle, T, (pc[level][1], pc[level][2], pm[level][1], pm[level][2]), W, H, intr, level)
        cond, share = np.linalg.cond(A.astype(np.float64), 2), inl / ((H >> level) * (W >> level))
        print("%dx%d level %d: cond %.1f, inliers %.1f %%" % (W, H, level, cond, 100 * share))
        assert cond <= 1e3 and share >= 0.5


@pytest.mark.parametrize("size", K.SIZES_CHAIN, ids=lambda s: "%dx%d" % s)
def test_chain_sizes_contract(oracle, size):
    """The oracle's chain forgets a 1e-6 perturbation of its start pose along every axis of the twist: it ends within 1/100 of the
    bounds the device is held to, with the same inliers (observed: <= 7e-8) -- so those bounds measure the device, not the scene."""
    W, H = size
    cx, cy, fx, fy = K.intrinsics(W)
    model, current = _frames(size)
    T0, _, inl0 = oracle.icp_incremental_transformation(current, model, W, H, cx, cy, fx, fy)
    assert np.max(np.abs(T0[:3, 3])) > 1e-3      # (a real motion)
    worst = 0.0
    for k in range(6):
        T, _, inl = oracle.icp_incremental_transformation(current, model, W, H, cx, cy, fx, fy, T=oracle.se3_exp(1e-6 * np.eye(6)[k]))
        worst = max(worst, np.max(np.abs(T - T0)))
        assert np.max(np.abs(T[:3, 3] - T0[:3, 3])) <= K.CHAIN_TOL_T / 100 and np.max(np.abs(T[:3, :3] - T0[:3, :3])) <= K.CHAIN_TOL_R / 100
        assert inl == inl0
    print("%dx%d: a 1e-6 start perturbation moves the final pose by %.2e" % (W, H, worst))


@pytest.mark.parametrize("size", K.SIZES_ALL, ids=lambda s: "%dx%d" % s)
def test_identical_frames_give_the_identity_exactly(oracle, size):
    W, H = size
    cx, cy, fx, fy = K.intrinsics(W)
    d = K.depth_frame(W, H, K.MODEL_SHIFT)
    T, err, inl = oracle.icp_incremental_transformation(d, d, W, H, cx, cy, fx, fy)
    assert np.array_equal(T, np.eye(4)) and err == 0.0 and inl > 0
    observed = {(4, 4): 9, (5, 7): 22, (37, 21): 691, (65, 47): 2774, (131, 97): 11747}
    if size in observed:
        assert inl == observed[size]


def test_all_zero_frame_leaves_the_oracle_pose_alone(oracle):
    W, H = K.GATE_SIZE
    cx, cy, fx, fy = K.intrinsics(W)
    start = oracle.se3_exp(K.ZERO_FRAME_START_TWIST)
    T, err, inl = oracle.icp_incremental_transformation(np.zeros((H, W), np.uint16), K.depth_frame(W, H, K.MODEL_SHIFT), W, H, cx, cy,
                                                        fx, fy, T=start)
    assert np.array_equal(T, start) and inl == 0 and np.isnan(err)


@pytest.mark.parametrize("case", K.GATE_CASES, ids=lambda c: c[0])
def test_gate_cases_sit_where_they_are_named(oracle, case):
    _, T, expected = case
    W, H = K.GATE_SIZE
    p = K.oracle_pyramid(oracle, K.gate_depth(), W, H, K.GATE_INTRINSICS)
    A, b, res, inl = K.oracle_step(oracle, T, (p[0][1], p[0][2], p[0][1], p[0][2]), W, H, K.GATE_INTRINSICS, 0)
    assert inl == expected


@pytest.mark.parametrize("n_blocks", K.N_BLOCKS_CASES)
def test_second_stage_restatement(n_blocks):
    p = K.random_partials(n_blocks, 1000 + n_blocks)
    assert 1e-6 <= np.abs(p).min() and np.abs(p).max() <= 1e6 and (p > 0).any() and (p < 0).any()
    total = K.second_stage(p, n_blocks)
    # against an exact sum, it is a sum: within the rounding of 256 double additions and the one to float
    import math
    for e in range(29):
        exact = math.fsum(float(v) for v in p[:, e])
        assert abs(float(total[e]) - exact) <= 256 * 2.0 ** -53 * float(np.abs(p[:, e]).sum()) + 2.0 ** -24 * abs(exact)
    # blocks past n_blocks do not count, whatever they hold
    wide = np.concatenate([p, np.full((K.GN_BLOCKS - n_blocks, 32), 1.0e30, np.float32)])
    assert np.array_equal(K.second_stage(wide[:n_blocks], n_blocks), total)
    # not vacuous: the totals depend on the order of the blocks (one block has no order)
    if n_blocks > 1:
        assert not np.array_equal(K.second_stage(p[::-1], n_blocks), total)
    else:
        assert np.array_equal(total, p[0, :29])
    A, b, res, inl = K.unpack_totals(total)
    assert np.array_equal(A, A.T) and res == total[27] and inl == total[28] and b[5] == total[26] and A[0, 5] == total[5]
    assert np.array_equal(K.unpack_totals(K.second_stage(K.pack_system(A, b, res, inl), 1))[0], A)


def test_exponential_restatement_against_60_digits():
    """device_exp (gn_solve.hpp's series below th^2 = 0.0625, closed forms above) within 4 x 2^-53 x max(1, |a|inf) of the true
    exponential over the whole angle list (observed: 2.9)."""
    worst = 0.0
    for a in K.exp_cases():
        err = K.max_abs_diff(K.device_exp(a), K.true_exp(a)) / K.exp_bound(a, 1.0)
        worst = max(worst, err)
    print("numpy restatement of the device's se3_exp: worst %.2f x 2^-53 x max(1, |a|inf)" % worst)
    assert worst <= K.EXP_RESTATEMENT_UNITS


def test_oracle_exponential_is_no_precision_reference(oracle):
    """Recorded discrepancy: the oracle restates Sophus's closed form, whose (1 - cos th) / th^2 cancels for small th.  At th = 1e-8 it
    is some 1e7 units off where the device's series stays within a few -- so nothing in these tests compares an exponential with it."""
    worst = 0.0
    for a in K.exp_cases():
        if abs(np.linalg.norm(a[3:]) - 1e-8) < 1e-10:
            worst = max(worst, K.max_abs_diff(oracle.se3_exp(a), K.true_exp(a)) / K.exp_bound(a, 1.0))
    print("oracle se3_exp at th = 1e-8: worst %.3g x 2^-53 x max(1, |a|inf)" % worst)
    assert worst > 1e3


def test_solve_families_are_what_they_claim():
    for A, b in K.well_conditioned_systems():
        assert np.array_equal(A, A.T) and np.linalg.cond(A.astype(np.float64), 2) < 1e4
        x = np.array([float(v) for v in K.true_solve(A, b)])
        assert np.max(np.abs(x)) < 0.2
        d = np.diag(A).astype(np.float64)
        assert d.min() > 1e-9 * d.max()
    for A, b in K.fallback_systems():
        assert np.array_equal(A, A.T)
        d = np.diag(A).astype(np.float64)
        assert 0 < d[0] <= 1e-9 * d.max()           # the unpivoted factorisation's first pivot: refused
        x = np.array([float(v) for v in K.true_solve(A, b)])
        assert np.max(np.abs(x)) < 0.2
    x = K.semidefinite_x()
    assert np.allclose(K.SEMIDEFINITE_A.astype(np.float64) @ x, K.SEMIDEFINITE_B * (np.diag(K.SEMIDEFINITE_A) != 0))
    T = K.random_rigid(7)
    assert np.max(np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3))) < 1e-14 and np.array_equal(T[3], [0, 0, 0, 1])
