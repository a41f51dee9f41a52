"""Shared inputs and references of the ICP size / gate tests (test_icp_sizes.py) and the Gauss-Newton back-end tests (test_gn_finish.py);
test_icp_cases_host.py checks, without a GPU, that the inputs are sound.  Nothing here touches the device.

Two references are used, for different things:
  * the CPU oracle (oracle/icp_oracle.c) for pyramids, maps, the sums of a step and whole chains.  Its se3_exp restates Sophus's closed
    form, whose (1 - cos th) / th^2 loses everything for th between 1e-10 and about 1e-3: against the 60-digit evaluation below its worst
    error is 5e7 .. 6e7 x 2^-53 x max(1, |a|inf), at th = 1e-8 (test_icp_cases_host.py measures it; LABNOTES.md 17).  The device's series is the more
    accurate of the two, so the oracle is NOT the reference for the exponential or the solve;
  * mpmath at 60 digits (true_exp, true_solve) for those.
"""
import math

import numpy as np

U = 2.0 ** -53          # the unit the exponential's and the solve's bounds are stated in

# (width, height).  (4, 4) is the smallest size tsdf_icp_create accepts; 37 x 21 .. 257 x 129 have odd widths and floor-halved levels;
# (300, 4) and (4, 300) are flatter / narrower than the map kernels' 64 x 4 tile; (4, 4) .. (65, 47) have fewer pixels than one pass of
# the 256 x 256 reduction grid (the first three fewer than ONE workgroup at some level); (321, 205) has 65 805: one pass plus 269.
SIZES_ALL = ((4, 4), (5, 7), (37, 21), (63, 33), (65, 47), (131, 97), (257, 129), (300, 4), (4, 300), (321, 205))
# Sizes whose three levels are all healthy (test_icp_cases_host.py asserts it): only here are chain poses compared with the oracle's.
# Below 37 x 21 the normal matrix has a condition number of 1e9 .. 1e10 (no inliers at all at level 2), the oracle's own chain ends
# metres away, and device and oracle legitimately differ: the device solves without pivoting whenever every pivot exceeds 1e-9 of the
# largest diagonal entry, the oracle always pivots.
SIZES_CHAIN = ((37, 21), (65, 47), (131, 97))
CHAIN_TOL_T, CHAIN_TOL_R = 2e-4, 1e-4      # test_parity_icp.py's bounds at 640 x 480

MODEL_SHIFT, CURRENT_SHIFT = (0.0, 0.0, 0.0), (0.6, -0.4, 3.0)
PROBE_TWIST = (0.004, -0.003, 0.002, 0.002, -0.001, 0.0015)
ZERO_FRAME_START_TWIST = (0.01, -0.02, 0.03, 0.02, 0.01, -0.015)
DIST_THRESH = 0.10


def icp_angle():
    """sinf(20.f * 3.14159254f / 180.f), ICPOdometry.h:27"""
    return float(np.float32(math.sin(np.float32(20.0) * np.float32(3.14159254) / np.float32(180.0))))


def intrinsics(width):
    """(cx, cy, fx, fy), the order of the ICPOdometry constructor: the default depth camera scaled to the image width."""
    k = width / 640.0
    return (331.0 * k, 234.6 * k, 591.1 * k, 590.1 * k)


def depth_frame(width, height, shift):
    """A tilted, gently waved surface 1.5 m away, the same in every size (coordinates scaled by 640 / width), 2 % dropouts."""
    dx, dy, dz = shift
    s = 640.0 / width
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    X, Y = (x + dx) * s, (y + dy) * s
    z = 1500 + 0.3 * (X - 320) + 0.2 * (Y - 240) + 80 * np.sin(X / 40) * np.cos(Y / 55) + dz
    d = np.rint(z).astype(np.uint16)
    d[np.random.default_rng(width * 1000 + height).random((height, width)) < 0.02] = 0
    return d


def level_intrinsics(intr, level):
    """Intr::operator()(level) in fp32: (fx, fy, cx, cy) / 2^level, the order of the oracle's arguments."""
    cx, cy, fx, fy = intr
    div = 1 << level
    return (np.float32(fx) / div, np.float32(fy) / div, np.float32(cx) / div, np.float32(cy) / div)


def oracle_pyramid(O, depth, width, height, intr, depth_cutoff=20.0):
    """[(depth, vmap, nmap)] of levels 0..2 from the oracle alone."""
    out = []
    d = np.ascontiguousarray(depth, np.uint16).reshape(height, width)
    for level in range(3):
        rows, cols = height >> level, width >> level
        if level > 0:
            d = O.icp_pyr_down(d, height >> (level - 1), width >> (level - 1))
        v = O.icp_vmap(d, rows, cols, *level_intrinsics(intr, level), depth_cutoff)
        out.append((d, v, O.icp_nmap(v, rows, cols)))
    return out


def oracle_step(O, T, maps, width, height, intr, level):
    """The oracle's sums of one step at the float-narrowed pose T (4 x 4); maps = (vmap_curr, nmap_curr, vmap_prev, nmap_prev) of
    `level`.  -> (A, b, residual, inliers)."""
    R, t = pose_floats(T)
    A, b, res, inl, _ = O.icp_step(R.T.reshape(-1), t, *maps, height >> level, width >> level, *level_intrinsics(intr, level),
                                   DIST_THRESH, icp_angle())
    return A, b, res, inl


def pose_floats(T):
    T = np.asarray(T)
    return np.ascontiguousarray(T[:3, :3], np.float32), np.ascontiguousarray(T[:3, 3], np.float32)


def sums_close(A, b, res, Ao, bo, reso, tol=1e-4):
    """test_parity_icp.py's rule for the fp32 sums against the oracle's double ones: tol of the largest entry, the same floor for b."""
    assert np.max(np.abs(A - Ao)) <= tol * np.max(np.abs(Ao)), (A, Ao)
    assert np.max(np.abs(b - bo)) <= tol * max(np.max(np.abs(bo)), 1e-6 * np.max(np.abs(Ao))), (b, bo)
    assert abs(res - reso) <= tol * reso, (res, reso)


# ---- gates and guards: a 2 m plane seen by a camera whose principal point is a pixel centre -------------------------------------
GATE_SIZE = (65, 47)
GATE_INTRINSICS = (33.0, 23.0, 591.1 * 65 / 640, 590.1 * 65 / 640)      # cx, cy, fx, fy


def gate_depth():
    return np.full((GATE_SIZE[1], GATE_SIZE[0]), 2000, np.uint16)


def _rot_y(degrees):
    a = math.radians(degrees)
    T = np.eye(4)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
    return T


def _shift(x, y, z):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


# (name, pose, the oracle's inliers -- asserted in test_icp_cases_host.py, so every case stays on the side of its gate it is named for)
GATE_CASES = (
    ("p2_exactly_zero_and_0_over_0_at_the_principal_pixel", _shift(0, 0, -2.0), 0),
    ("behind_the_camera", _shift(0, 0, -5), 0),
    ("projection_far_outside", _shift(0.5, 0.5, -1.9999999), 0),
    ("translation_1e12", _shift(1e12, -1e12, 0), 0),
    ("nan_translation", _shift(float("nan"), 0, 0), 0),
    ("quarter_turn_about_y", _rot_y(90), 0),
    ("half_turn_about_y", _rot_y(180), 0),
    ("inside_the_distance_gate", _shift(0, 0, 0.09), 2001),
    ("outside_the_distance_gate", _shift(0, 0, 0.11), 0),
    ("inside_the_angle_gate", _rot_y(19), 794),
    ("outside_the_angle_gate", _rot_y(21), 0),
)


# ---- the second stage of the reduction (icp_finish_step) restated ----------------------------------------------------------------
GN_BLOCKS = 256
N_BLOCKS_CASES = (1, 31, 32, 33, 255, 256)


def second_stage(partial, n_blocks):
    """The 29 fp32 totals icp_finish_step forms of `partial` ((n_blocks, 32) float32): per entry eight float64 sums of 32 blocks each,
    in block order, blocks at or past n_blocks counting as +0.0f; then the eight group sums in order; then float32."""
    p = np.zeros((GN_BLOCKS, 32), np.float32)
    p[:n_blocks] = np.asarray(partial, np.float32).reshape(n_blocks, 32)
    blocks = p.reshape(8, 32, 32).astype(np.float64)       # [group][block in group][entry]
    g = np.zeros((8, 32), np.float64)
    for i in range(32):
        g += blocks[:, i, :]
    s = np.zeros(32, np.float64)
    for k in range(8):
        s += g[k]
    return s.astype(np.float32)[:29]


def unpack_totals(total):
    """-> (A 6 x 6, b 6, residual, inliers): the upper triangle of (A | b) row by row, then the two scalars."""
    A, b = np.zeros((6, 6), np.float32), np.zeros(6, np.float32)
    k = 0
    for i in range(6):
        for j in range(i, 7):
            if j == 6:
                b[i] = total[k]
            else:
                A[i, j] = A[j, i] = total[k]
            k += 1
    return A, b, total[27], total[28]


def pack_system(A, b, residual=0.0, inliers=0.0, n_blocks=1, block=0):
    """(n_blocks, 32) float32 partial sums with the system in one block and zeros elsewhere."""
    p = np.zeros((n_blocks, 32), np.float32)
    k = 0
    for i in range(6):
        for j in range(i, 7):
            p[block, k] = b[i] if j == 6 else A[i][j]
            k += 1
    p[block, 27], p[block, 28] = residual, inliers
    return p


def random_partials(n_blocks, seed):
    """Mixed signs, magnitudes 1e-6 .. 1e6.  Every value above 1e-3 is taken back by the block after it, so a total is the sum of the
    small values while the running sums pass through large ones: which double additions round -- the order -- shows in the fp32
    totals (the host test asserts that it does).  A single block is the plain draw."""
    rng = np.random.default_rng(seed)

    def draw(lo, hi):
        return (rng.choice([-1.0, 1.0], 32) * 10.0 ** rng.uniform(lo, hi, 32)).astype(np.float32)
    p = np.zeros((n_blocks, 32), np.float32)
    for k in range(0, n_blocks, 2):
        p[k] = draw(-6, 6) if k + 1 < n_blocks or n_blocks == 1 else draw(-6, -3)
        if k + 1 < n_blocks:
            large = np.abs(p[k]) > 1e-3
            p[k + 1] = np.where(large, -p[k], draw(-6, -3))
    return p


# ---- 60-digit references ----------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 60
    return mpmath


def true_exp(a):
    """Sophus::SE3d::exp(a), a = (upsilon, omega) as floats or mpf, at 60 digits -> mpmath 4 x 4 matrix."""
    mp = _mp()
    a = [v if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in a]
    wx, wy, wz = a[3:]
    th2 = wx * wx + wy * wy + wz * wz
    th = mp.sqrt(th2)
    if th == 0:
        A, B, Cc = mp.mpf(1), mp.mpf(1) / 2, mp.mpf(1) / 6
    else:
        A, B, Cc = mp.sin(th) / th, (1 - mp.cos(th)) / th2, (th - mp.sin(th)) / (th2 * th)
    W = mp.matrix([[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]])
    W2 = W * W
    I = mp.eye(3)
    R, V = I + A * W + B * W2, I + B * W + Cc * W2
    t = V * mp.matrix(a[:3])
    E = mp.eye(4)
    for i in range(3):
        for j in range(3):
            E[i, j] = R[i, j]
        E[i, 3] = t[i]
    return E


def true_solve(A, b):
    """x = A^-1 b of the float32 inputs at 60 digits (A non-singular) -> list of mpf."""
    mp = _mp()
    A = np.asarray(A, np.float32)
    b = np.asarray(b, np.float32)
    x = mp.lu_solve(mp.matrix([[mp.mpf(float(v)) for v in row] for row in A]), mp.matrix([mp.mpf(float(v)) for v in b]))
    return [x[i] for i in range(6)]


def mp_matrix(T):
    mp = _mp()
    T = np.asarray(T, np.float64)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in T])


def max_abs_diff(T, E):
    """max |T - E| over the 16 entries, T a float64 4 x 4, E an mpmath one, evaluated at 60 digits -> float"""
    mp = _mp()
    T = np.asarray(T, np.float64)
    return float(max(abs(mp.mpf(float(T[i, j])) - E[i, j]) for i in range(4) for j in range(4)))


def device_exp(a):
    """gn_solve.hpp's se3_exp restated in numpy float64: power series in th^2 below th^2 = 0.0625, the closed forms above."""
    a = np.asarray(a, np.float64)
    wx, wy, wz = a[3], a[4], a[5]
    t = wx * wx + wy * wy + wz * wz
    th = np.sqrt(t)
    W = np.array([[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]], np.float64)
    W2 = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            for k in range(3):
                W2[i, j] += W[i, k] * W[k, j]

    def horner(first, dens):
        s = 1.0
        for d in reversed(dens):
            s = 1.0 - t * (1.0 / d) * s
        return first * s
    if t < 0.0625:
        A = horner(1.0, (6.0, 20.0, 42.0, 72.0, 110.0, 156.0, 210.0))
        B = horner(0.5, (12.0, 30.0, 56.0, 90.0, 132.0, 182.0, 240.0))
        Cc = horner(1.0 / 6.0, (20.0, 42.0, 72.0, 110.0, 156.0, 210.0, 272.0))
    else:
        A, B, Cc = np.sin(th) / th, (1.0 - np.cos(th)) / t, (th - np.sin(th)) / (t * th)
    E = np.eye(4)
    for i in range(3):
        ti = 0.0
        for j in range(3):
            I = 1.0 if i == j else 0.0
            E[i, j] = I + A * W[i, j] + B * W2[i, j]
            ti += (I + B * W[i, j] + Cc * W2[i, j]) * a[j]
        E[i, 3] = ti
    return E


# ---- the exponential's and the solve's cases ----------------------------------------------------------------------------------------
EXP_ANGLES = (0.0, 1e-12, 1e-10, 1e-8, 1e-5, 1e-3, 0.01, 0.1, 0.2499, 0.25, 0.2501, 0.5, 1.0, 3.0, 3.14159, 6.0)
EXP_TRANSLATION_SCALES = (1e-3, 1.0, 100.0)
EXP_BOUND_UNITS, EXP_RESTATEMENT_UNITS = 8.0, 4.0


def exp_cases():
    """Twists a = (upsilon, omega), fp32-representable (the device receives them as the b of an identity system): every angle x 20
    random axes, the translation scale cycling over EXP_TRANSLATION_SCALES so that each angle meets each scale."""
    rng = np.random.default_rng(0x5E3)
    out = []
    for th in EXP_ANGLES:
        for k in range(20):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            a = np.concatenate([rng.normal(size=3) * EXP_TRANSLATION_SCALES[k % 3], axis * th]).astype(np.float32)
            out.append(a.astype(np.float64))
    return out


def exp_bound(a, units=EXP_BOUND_UNITS):
    return units * U * max(1.0, float(np.max(np.abs(a))))


def well_conditioned_systems(n=50, seed=0x6A55):
    """[(A float32 6 x 6, b float32 6)]: A = J^T J of a 40 x 6 normal J whose columns are scaled (1, 1, 1, 30, 30, 30) -- the shape of an
    ICP normal matrix, cond2 up to about 7e3 -- and b = A x0 with |x0| < 0.2."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        J = rng.normal(size=(40, 6)) * np.array([1, 1, 1, 30, 30, 30.0])
        A = (J.T @ J).astype(np.float32)
        b = rng.normal(size=6)
        x = np.linalg.solve(A.astype(np.float64), b)
        b = (b * (0.15 / np.max(np.abs(x)))).astype(np.float32)
        out.append((A, b))
    return out


def fallback_systems(n=50, seed=0x6A56):
    """[(A, b)] that the unpivoted factorisation has to refuse: block diag(SPD 5 x 5, 1e-12 x the largest diagonal entry) under a
    symmetric permutation that puts the tiny entry FIRST -- the first pivot is below 1e-9 of the largest -- and shuffles the rest,
    so the pivoted solve exchanges rows and has to undo its permutation.  b = A x0 with |x0| < 0.2, so the true x stays small."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        J = rng.normal(size=(40, 5)) * np.array([1, 1, 30, 30, 30.0])[rng.permutation(5)]
        M = np.zeros((6, 6))
        M[:5, :5] = J.T @ J
        M[5, 5] = 1e-12 * np.max(np.diag(M))
        perm = np.concatenate([[5], rng.permutation(5)])
        A = M[np.ix_(perm, perm)].astype(np.float32)
        x0 = rng.uniform(-0.15, 0.15, 6)
        b = (A.astype(np.float64) @ x0).astype(np.float32)
        out.append((A, b))
    return out


def solve_bound(A, x):
    """(cond2(A) |x|inf + 8 max(1, |x|inf)) x 2^-53 for the float32 A as given"""
    xinf = float(np.max(np.abs(x)))
    return (np.linalg.cond(np.asarray(A, np.float64), 2) * xinf + 8.0 * max(1.0, xinf)) * U


SEMIDEFINITE_A = np.diag([4.0, 0.0, 2.0, 0.0, 1.0, 0.0]).astype(np.float32)
SEMIDEFINITE_B = np.full(6, 0.1, np.float32)


def semidefinite_x():
    """zero pivots give zero components; the others are b_i / A_ii of the float32 values"""
    b = SEMIDEFINITE_B.astype(np.float64)
    return np.array([b[0] / 4.0, 0.0, b[2] / 2.0, 0.0, b[4] / 1.0, 0.0])


def random_rigid(seed, translation=1.0):
    """A rigid 4 x 4 (float64, orthonormal to rounding) with a rotation of about a radian"""
    rng = np.random.default_rng(seed)
    T = device_exp(np.concatenate([rng.normal(size=3) * translation, rng.normal(size=3) * 0.6]))
    return T
