"""The Gauss-Newton back end (tsdf_amd/csrc/gn_solve.hpp: icp_finish_step) on its own, through tsdf_selftest_gn_finish: one launch of
the kernel ICP and the plain field aligner finish a step with, on sums made up here.

  * second stage of the reduction: bit for bit against its numpy restatement, for block counts either side of the groups of 32 (blocks
    past n_blocks hold 1e30 in the device buffer: the kernel has to leave them out);
  * SE3 exponential: against a 60-digit evaluation (mpmath), over the series branch, the switch at th^2 = 0.0625 and the sin / cos branch.
    NOT against the oracle: its closed form is some 1e7 units off at th = 1e-8 (tests/icp_cases.py);
  * solve: well-conditioned systems (the unpivoted LDL^T), then systems it has to refuse -- zero pivots, a tiny first pivot under a
    shuffled permutation, the zero matrix -- so that the pivoted factorisation's exchanges and its un-permutation are exercised;
  * T <- exp(x) * T_in for a rigid T_in.
The bounds are in units of 2^-53 and come from the arithmetic (tests/icp_cases.py, test_icp_cases_host.py), not from what the device gave;
each test prints the device's worst, LABNOTES.md records them.
"""
import numpy as np
import pytest

from tests import icp_cases as K
from tsdf_amd import _capi

pytestmark = pytest.mark.gpu
I6 = np.eye(6, dtype=np.float32)


def gn_finish(partial, n_blocks, T_in=None, update=1):
    """-> state_out[64]: [0, 16) pose (column-major), [16] residual, [17] inliers, [18, 54) A, [54, 60) b"""
    p = np.ascontiguousarray(partial, np.float32).reshape(n_blocks, 32)
    Tc = np.ascontiguousarray((np.eye(4) if T_in is None else np.asarray(T_in, np.float64)).T.reshape(-1))
    out = np.full(64, np.nan)
    _capi.check(_capi.lib.tsdf_selftest_gn_finish(p.ctypes.data, n_blocks, Tc.ctypes.data, update, out.ctypes.data))
    return out


def pose_of(state):
    return np.ascontiguousarray(state[:16].reshape(4, 4).T)


def step(A, b, T_in=None):
    """the pose after one update with the system (A, b), all of it in block 0"""
    return pose_of(gn_finish(K.pack_system(A, b), 1, T_in))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("n_blocks", K.N_BLOCKS_CASES)
def test_second_stage_equals_its_restatement_bit_for_bit(n_blocks):
    p = K.random_partials(n_blocks, 1000 + n_blocks)
    T_in = K.random_rigid(n_blocks)
    out = gn_finish(p, n_blocks, T_in, update=0)
    A, b, res, inl = K.unpack_totals(K.second_stage(p, n_blocks))
    got = out[16:60].astype(np.float32)
    assert np.array_equal(got.astype(np.float64), out[16:60])                       # float values, held in doubles
    assert np.array_equal(_bits(got[2:38]), _bits(A.reshape(-1)))
    assert np.array_equal(_bits(got[38:44]), _bits(b))
    assert _bits(got[0:1]) == _bits(np.float32(res).reshape(1)) and _bits(got[1:2]) == _bits(np.float32(inl).reshape(1))
    Ad = out[18:54].reshape(6, 6)
    assert np.array_equal(Ad, Ad.T)                                                 # mirrored from the upper triangle
    assert np.array_equal(_bits(pose_of(out)), _bits(T_in))                         # update = 0: the pose comes back as given


def test_system_in_the_last_block_is_counted():
    """the mask is b < n_blocks at both ends: the last block counts, the first one past it (poisoned) does not"""
    (A, b) = K.well_conditioned_systems(1)[0]
    for n_blocks in K.N_BLOCKS_CASES:
        out = gn_finish(K.pack_system(A, b, 0.25, 7.0, n_blocks, n_blocks - 1), n_blocks, update=0)
        assert np.array_equal(out[18:54].reshape(6, 6), A.astype(np.float64)) and np.array_equal(out[54:60], b.astype(np.float64))
        assert out[16] == 0.25 and out[17] == 7.0


def test_exponential_against_60_digits():
    """A = I, everything in block 0: the unpivoted solve returns x = b exactly, so pose = exp(b)."""
    worst, worst_at, worst_orth = 0.0, None, 0.0
    for a in K.exp_cases():
        b = a.astype(np.float32)
        assert np.array_equal(b.astype(np.float64), a)
        T = step(I6, b)
        err = K.max_abs_diff(T, K.true_exp(a)) / K.exp_bound(a, 1.0)
        if err > worst:
            worst, worst_at = err, (float(np.linalg.norm(a[3:])), float(np.max(np.abs(a[:3]))))
        worst_orth = max(worst_orth, float(np.max(np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)))))
        assert np.array_equal(T[3], [0, 0, 0, 1])
        assert err <= K.EXP_BOUND_UNITS, (a, err)
        assert worst_orth <= 1e-14, a
    print("se3_exp on the device: worst %.2f x 2^-53 x max(1, |a|inf) at (angle, |upsilon|inf) = %r; R R^T - I <= %.2e"
          % (worst, worst_at, worst_orth))


def _solve_family(systems, what):
    worst, worst_cond = 0.0, 0.0
    for A, b in systems:
        x = K.true_solve(A, b)
        xf = np.array([float(v) for v in x])
        T = step(A, b)
        err, bound = K.max_abs_diff(T, K.true_exp(x)), K.solve_bound(A, xf)       # (x stays at 60 digits)
        cond = np.linalg.cond(A.astype(np.float64), 2)
        worst, worst_cond = max(worst, err / bound), max(worst_cond, err / (cond * K.U * np.max(np.abs(xf))))
        assert err <= bound, (A, b, err, bound)
    print("%s: worst error %.3g of the bound, %.3g of cond2 x 2^-53 x |x|inf" % (what, worst, worst_cond))


def test_solve_well_conditioned():
    """|pose - exp(A^-1 b)| <= (cond2(A) |x|inf + 8 max(1, |x|inf)) 2^-53: loose for rounding -- a wrong sign, index or order is O(1)."""
    _solve_family(K.well_conditioned_systems(), "unpivoted solve, 50 systems with cond2 up to 7e3")


def test_solve_falls_back_on_zero_pivots():
    x = K.semidefinite_x()
    T = step(K.SEMIDEFINITE_A, K.SEMIDEFINITE_B)
    err = K.max_abs_diff(T, K.true_exp(x))
    print("semidefinite system: error %.3g x 2^-53" % (err / K.U))
    # (cond2 of a singular matrix is no bound: the non-zero part has cond 4)
    assert err <= (4.0 * np.max(np.abs(x)) + 8.0) * K.U


def test_solve_falls_back_on_a_tiny_first_pivot():
    _solve_family(K.fallback_systems(), "pivoted solve, 50 permuted systems with one entry 1e-12 of the largest")


def test_zero_system_leaves_the_pose_alone():
    T_in = K.random_rigid(11)
    assert np.max(np.abs(T_in - np.eye(4))) > 0.1
    for b in (np.zeros(6, np.float32), np.full(6, 0.1, np.float32)):
        T = step(np.zeros((6, 6), np.float32), b, T_in)
        assert np.array_equal(_bits(T), _bits(T_in))


def test_composition_with_a_rigid_pose():
    worst = 0.0
    rng = np.random.default_rng(0xC0)
    for seed in range(10):
        T_in = K.random_rigid(100 + seed, translation=3.0)
        b = (rng.normal(size=6) * 0.05).astype(np.float32)
        T = step(I6, b, T_in)
        ref = K.true_exp(b.astype(np.float64)) * K.mp_matrix(T_in)
        err = K.max_abs_diff(T, ref) / (K.U * np.max(np.abs(T_in)))
        worst = max(worst, err)
        assert err <= 16.0, (seed, err)
        assert np.array_equal(T[3], [0, 0, 0, 1])
    print("T <- exp(x) T: worst %.2f x 2^-53 x max|T_in|" % worst)


def test_refusals():
    p, T, out = np.zeros((256, 32), np.float32), np.eye(4).reshape(-1), np.zeros(64)
    f = _capi.lib.tsdf_selftest_gn_finish
    for n_blocks in (0, 257, -1):
        assert f(p.ctypes.data, n_blocks, T.ctypes.data, 1, out.ctypes.data) == _capi.TSDF_ERR_INVALID
    assert f(None, 1, T.ctypes.data, 1, out.ctypes.data) == _capi.TSDF_ERR_INVALID
    assert f(p.ctypes.data, 1, None, 1, out.ctypes.data) == _capi.TSDF_ERR_INVALID
    assert f(p.ctypes.data, 1, T.ctypes.data, 1, None) == _capi.TSDF_ERR_INVALID
    assert not out.any()
    with pytest.raises(ValueError, match="tsdf_selftest_gn_finish"):
        _capi.check(f(p.ctypes.data, 0, T.ctypes.data, 1, out.ctypes.data))
