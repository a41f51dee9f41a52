"""Seeded inputs for the volume-fusion sweep (tests/test_fuse_sweep.py): case(seed) is pure -- numpy arrays and plain numbers, no GPU,
no oracle -- and reference(O, case) is the CPU reference's answer for it (tests/fuse_ref.py), computed once a seed and shared.

What a seed fixes by its index, so that every kind occurs in range(N_SEEDS) whatever the random draws do: the kind of matrix
(seed % 8), the pattern of source weights (seed % 7), the pair of weight storages (seed % 9), the cap ((seed // 3) % 5), the forced
grid dimensions (FORCED), a one-voxel source axis (seed % 8 == 5) and a sub-millimetre scene (seed % 5 == 2).  Everything else comes from numpy's default_rng(seed).

The source's voxel edges are derived, not drawn: the destination's box goes through the matrix, and the source is sized so that it
covers 0.5 - 1.4 of that image an axis -- as far as the ratio of edges (kept within about 1/6 .. 6) and the 48 voxels an axis allow.
That keeps most seeds between "nothing is updated" and "everything is"."""
import functools

import numpy as np

from tests import fuse_ref

F = np.float32
N_SEEDS = 64
SEEDS = tuple(range(N_SEEDS))
MATRIX_KINDS = ("identity", "translation", "turn", "rotation", "scaled", "affine", "rank2", "point")
WEIGHT_KINDS = ("full", "blocks", "speckle", "c250", "c60000", "fractional", "signed")
STORAGES = (8, 16, 32)
CAPS = (0, 1, 5, 255, 300)
MAX_DST, MAX_SRC = 40000, 60000
DST_LIMITS, SRC_LIMIT = (140, 23, 70), 48
# (X, Y, Z) of the destination, None = drawn: one wave exactly / one lane short / one over, the rows of a brick likewise, one layer of
# bricks exactly / one plane short / one over, an odd Z in the second layer, and single-voxel axes
FORCED = {0: (63, None, 31), 1: (64, 4, 32), 2: (65, 5, 33), 3: (None, 1, 47), 4: (64, 5, 65), 5: (1, 1, 35), 6: (None, None, 1)}
BRICK = (64, 4, 32)      # integrate's brick, the cull's unit (tsdf_amd/csrc/common.hpp: kIntBrickX / Y / Z)
SUMMARY = 8              # the source summary's brick (fuse.hip: kSumBrick)


def _shrink(dims, limits_fixed, most):
    """Scale the free axes down until the grid has at most `most` voxels."""
    dims = list(dims)
    while dims[0] * dims[1] * dims[2] > most:
        free = [a for a in range(3) if not limits_fixed[a] and dims[a] > 1]
        a = max(free, key=lambda i: dims[i])
        dims[a] = max(1, int(dims[a] * 0.8))
    return tuple(dims)


def _edges(rng, kind, base):
    """Three voxel edges around `base` (mm): `kind` = (round, anisotropic)."""
    round_, aniso = kind
    e = np.array(base, np.float64) * (rng.uniform(0.6, 1.6, 3) if aniso else np.ones(3))
    if round_:
        e = 2.0 ** np.round(np.log2(e))
    return e


def _offset(rng, kinds=3):
    how = rng.integers(kinds)
    if how == 0:
        return np.zeros(3)
    if how == 1:
        return np.round(rng.uniform(-400, 400, 3))
    return rng.choice([-1.0, 1.0], 3) * rng.uniform(5000, 20000, 3)


def _rotation(rng):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    t = rng.uniform(0, 2 * np.pi)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _turn(rng):
    """One of the 23 proper rotations by multiples of 90 degrees other than the identity: entries exactly 0 and +-1."""
    while True:
        A = np.zeros((3, 3))
        A[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
        if np.linalg.det(A) > 0 and not np.array_equal(A, np.eye(3)):
            return A


def _linear(rng, kind):
    if kind in ("identity", "translation"):
        return np.eye(3)
    if kind == "turn":
        return _turn(rng)
    if kind == "rotation":
        return _rotation(rng)
    if kind == "scaled":
        return _rotation(rng) * np.exp(rng.uniform(np.log(0.3), np.log(3.0)))
    if kind == "point":
        return np.zeros((3, 3))
    shear = np.eye(3) + np.triu(rng.uniform(-0.5, 0.5, (3, 3)), 1)
    A = _rotation(rng) @ shear @ np.diag(rng.choice([-1.0, 1.0], 3) * rng.uniform(0.6, 1.5, 3))   # reflection where the signs say so
    if kind == "rank2":
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        A = A @ (np.eye(3) - np.outer(n, n))
    return A


def _source_weights(rng, kind, sdims):
    sX, sY, sZ = sdims
    n = sX * sY * sZ
    if kind == "full":
        return rng.integers(1, 4, n).astype(F)
    if kind == "blocks":   # a few observed boxes and balls in an unobserved grid
        w = np.zeros((sZ, sY, sX), F)
        zi, yi, xi = np.meshgrid(np.arange(sZ), np.arange(sY), np.arange(sX), indexing="ij")
        for _ in range(int(rng.integers(1, 4))):
            c = [rng.uniform(0, d) for d in (sX, sY, sZ)]
            r = [max(2.0, d * rng.uniform(0.15, 0.35)) for d in (sX, sY, sZ)]
            u = [np.abs(g - c[a]) / r[a] for a, g in enumerate((xi, yi, zi))]
            inside = (u[0] ** 2 + u[1] ** 2 + u[2] ** 2 <= 1.0) if rng.integers(2) else ((u[0] <= 1) & (u[1] <= 1) & (u[2] <= 1))
            w[inside] = F(rng.integers(1, 6))
        return w.reshape(-1)
    if kind == "speckle":
        return np.where(rng.random(n) < rng.uniform(0.6, 0.8), rng.integers(1, 4, n), 0).astype(F)
    if kind in ("c250", "c60000"):
        top = 250 if kind == "c250" else 60000
        w = rng.integers(1, top + 1, n).astype(F)
        w[rng.integers(n)] = top
        return w
    if kind == "fractional":
        return np.where(rng.random(n) < 0.9, rng.uniform(0.25, 4.0, n), 0.0).astype(F)
    w = rng.integers(1, 4, n).astype(F)            # "signed": fp32 with a few weights that are not > 0
    bad = rng.random(n)
    w[bad < 0.02] = F(-2.0)
    w[(bad >= 0.02) & (bad < 0.03)] = F(np.nan)
    return w


def needed_storage(weights):
    """The storage set_weight_data gives these weights (weights.hip: counts are packed into the narrowest mode that holds them)."""
    w = np.asarray(weights, F)
    counts = bool(np.all((w >= 0) & (w <= 65535) & (w == np.trunc(w)) & ~(np.signbit(w) & (w == 0))))
    return 32 if not counts else (8 if w.max() <= 255 else 16)


def storage_after(dst_bits, dst_weight, cap, src_weight):
    """The destination's weight storage after a fuse, by the header's rule (include/tsdf_amd.h, "Weight storage of dst")."""
    if dst_bits == 32 or needed_storage(src_weight) == 32:
        return 32
    if cap and (dst_bits == 16 or cap <= 255):          # a cap that fits the field needs no room
        return dst_bits
    need = int(np.max(dst_weight)) + int(np.max(src_weight))
    return 32 if need > 65535 else (16 if need > 255 else dst_bits)


def case(seed):
    rng = np.random.default_rng(seed)
    c = {"seed": seed, "matrix_kind": MATRIX_KINDS[seed % 8], "weight_kind": WEIGHT_KINDS[seed % 7],
         "dst_storage_wanted": STORAGES[(seed % 9) // 3], "src_storage_wanted": STORAGES[(seed % 9) % 3], "cap": CAPS[(seed // 3) % 5]}
    # ---- destination grid
    forced = FORCED.get(seed, (None, None, None))
    drawn = [int(rng.integers(1, lim + 1)) for lim in DST_LIMITS]
    if rng.random() < 0.6:
        drawn[2] |= 1                                  # odd Z more often than not: the last 16-bit weight dword is then partial
    ddims = _shrink([f if f is not None else d for f, d in zip(forced, drawn)], [f is not None for f in forced], MAX_DST)
    dkind = (bool(rng.integers(2)), rng.random() < 0.4)
    # every fifth seed is a sub-millimetre scene: a divisor below 1 fails the fast-division proof (a / b overflows for large a), so
    # the source of such a seed takes the IEEE instance of the kernel.  Its offsets stay small: 2^-19 of 20 m is a voxel there.
    small = seed % 5 == 2
    dvs = _edges(rng, dkind, rng.uniform(0.3, 0.8) if small else rng.uniform(8.0, 50.0))
    doff = _offset(rng, 2 if small else 3)
    dext = np.array(ddims) * dvs
    dtrunc = None if rng.integers(2) else float(F(np.linalg.norm(dvs) * rng.uniform(0.7, 2.5)))
    trunc_about = dtrunc if dtrunc else 1.1 * np.linalg.norm(dvs)
    # ---- the matrix's linear part, and the image of the destination's box
    A = _linear(rng, c["matrix_kind"])
    image = np.abs(A) @ dext
    # ---- source grid
    sdims = [int(rng.integers(1, SRC_LIMIT + 1)) for _ in range(3)]
    if seed % 8 == 5:
        sdims[(seed // 8) % 3] = 1
    sdims = _shrink(sdims, [False] * 3, MAX_SRC)
    skind = (bool(rng.integers(2)), rng.random() < 0.5)
    want = image * rng.uniform(0.5, 1.4, 3) / np.array(sdims)
    want = np.clip(want, dvs.mean() / 6.0, 0.7) if small else np.clip(want, max(2.0, dvs.mean() / 6.0), dvs.mean() * 6.0)
    svs = want if skind[1] else np.full(3, np.exp(np.log(want).mean()))
    if skind[0]:
        svs = 2.0 ** np.round(np.log2(svs))
    soff = _offset(rng, 2 if small else 3)
    sext = np.array(sdims) * svs
    strunc = None if rng.integers(2) else float(F(trunc_about * rng.choice([0.5, 2.0])))
    # ---- translation: the centre of the destination's box lands near the centre of the source's
    t = soff + sext * (0.5 + rng.uniform(-0.2, 0.2, 3)) - A @ (doff + dext / 2)
    if c["matrix_kind"] == "identity":
        t = np.zeros(3)
        soff = doff + (dext - sext) / 2 if rng.integers(2) else doff.copy()     # (the two boxes share a centre, or a corner)
    elif c["matrix_kind"] in ("translation", "turn"):
        t = np.round(t / (svs / 2)) * (svs / 2)        # whole and half source voxels
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = A, t
    c["matrix"] = M.T.astype(F).reshape(-1).copy()      # column-major
    c["dst"] = {"dims": tuple(ddims), "physical": tuple(float(F(e)) for e in dext), "offset": tuple(float(F(o)) for o in doff), "trunc": dtrunc}
    c["src"] = {"dims": tuple(sdims), "physical": tuple(float(F(e)) for e in sext), "offset": tuple(float(F(o)) for o in soff), "trunc": strunc}
    # ---- source content: a smooth field plus noise, beyond the destination's truncation in many seeds
    sX, sY, sZ = sdims
    zi, yi, xi = np.meshgrid(np.arange(sZ), np.arange(sY), np.arange(sX), indexing="ij")
    k = rng.uniform(0.1, 0.6, 3)
    amp = trunc_about * rng.uniform(0.5, 1.6)
    d = amp * np.sin(k[0] * xi + k[1] * yi + k[2] * zi + rng.uniform(0, 6)) + rng.normal(0, 0.1 * amp, xi.shape)
    d = d.astype(F).reshape(-1)
    c["small"] = small
    c["specials"] = seed % 3 == 0
    if c["specials"]:
        at = rng.choice(d.size, min(d.size, 14), replace=False)
        d[at] = np.resize(np.array([np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, 1e30, -1e30, 0.0, -0.0, 5 * trunc_about, -5 * trunc_about,
                                    np.nan, 1e30], F), at.size)
    c["src_dist"] = d
    c["src_weight"] = _source_weights(rng, c["weight_kind"], sdims)
    c["src_storage"] = max(c["src_storage_wanted"], needed_storage(c["src_weight"]))
    # ---- destination content: cleared, or uploaded distances and counts
    n = ddims[0] * ddims[1] * ddims[2]
    c["dst_cleared"] = rng.random() < 0.3
    if c["dst_cleared"]:
        c["dst_dist"], c["dst_weight"] = None, np.zeros(n, F)
    else:
        c["dst_dist"] = rng.uniform(-trunc_about, trunc_about, n).astype(F)
        top = int(rng.choice([3, 40, 200]))
        c["dst_weight"] = np.where(rng.random(n) < 0.7, rng.integers(1, top + 1, n), 0).astype(F)
    c["dst_storage"] = max(c["dst_storage_wanted"], needed_storage(c["dst_weight"]))
    return c


# ---- the reference's answer ---------------------------------------------------------------------------------------------------------
class Reference:
    pass


def oracle_volume(O, spec):
    v = O.Volume(spec["dims"], spec["physical"])
    v.offset(*spec["offset"])
    if spec["trunc"]:
        v.g.trunc = spec["trunc"]
        v.clear()
    return v


def reference_of(O, c):
    """fuse_ref.fuse of a case (a dict like case()'s): geometry and truncation from the oracle's volumes."""
    r = Reference()
    dv, sv = oracle_volume(O, c["dst"]), oracle_volume(O, c["src"])
    r.dgeom, r.sgeom, r.trunc = fuse_ref.geometry(dv), fuse_ref.geometry(sv), float(dv.g.trunc)
    r.start_d = dv.dist.copy() if c["dst_dist"] is None else c["dst_dist"]
    r.detail = {}
    with np.errstate(all="ignore"):
        r.dist, r.weight, r.updated = fuse_ref.fuse(O, r.dgeom, r.trunc, r.start_d, c["dst_weight"], r.sgeom, c["src_dist"], c["src_weight"],
                                                    c["matrix"], cap=c["cap"], detail=r.detail)
    for a in (r.start_d, r.dist, r.weight, r.updated):
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _cached(seed):
    import oracle as O
    O.build()
    c = case(seed)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c, reference_of(O, c)


def reference(seed):
    """(case(seed), its Reference): computed once a process, read-only."""
    return _cached(seed)


# ---- bricks -------------------------------------------------------------------------------------------------------------------------
def brick_counts(dims):
    return tuple(-(-dims[a] // BRICK[a]) for a in range(3))


def bricks_updated(updated, dims):
    """A bool array (nz, ny, nx): the destination bricks that hold an updated voxel."""
    X, Y, Z = dims
    nx, ny, nz = brick_counts(dims)
    g = np.zeros((nz * BRICK[2], ny * BRICK[1], nx * BRICK[0]), bool)
    g[:Z, :Y, :X] = np.asarray(updated).reshape(Z, Y, X)
    return g.reshape(nz, BRICK[2], ny, BRICK[1], nx, BRICK[0]).any(axis=(1, 3, 5))


def cull_upper_bound(dgeom, sgeom, m, src_weight, grow=4):
    """-> (bricks, finite): how many destination bricks the cull may list at the most, in float64 from the documented design
    (DESIGN.md 13): the centres of a brick's eight corner voxels through the matrix, their bounding box in source voxels grown by
    `grow` voxels a side (the design allows 2 and less than one of slack), outward to whole 8-voxel summary bricks, clamped to the
    grid; the brick counts when that box holds a source weight > 0.  finite = False when some box is not finite or lies beyond 1e9
    voxels, where the design makes no statement and keeps the brick: no bound then."""
    ddims, dvs, doff = dgeom
    sdims, svs, soff = sgeom
    dvs, doff, svs, soff = (np.asarray(a, F).astype(np.float64) for a in (dvs, doff, svs, soff))
    M = np.asarray(m, F).astype(np.float64).reshape(4, 4).T
    observed = (np.asarray(src_weight, F) > 0).reshape(sdims[2], sdims[1], sdims[0])
    n, finite = 0, True
    nb = brick_counts(ddims)
    with np.errstate(all="ignore"):
        for bz in range(nb[2]):
            for by in range(nb[1]):
                for bx in range(nb[0]):
                    v0 = np.array([bx, by, bz]) * BRICK
                    v1 = np.minimum(v0 + BRICK, ddims) - 1
                    corners = np.array([[(v1 if (k >> a) & 1 else v0)[a] for a in range(3)] for k in range(8)], np.float64)
                    q = ((corners + 0.5) * dvs + doff) @ M[:3, :3].T + M[:3, 3] - soff
                    lo, hi = np.floor(q.min(axis=0) / svs) - grow, np.floor(q.max(axis=0) / svs) + grow
                    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (np.abs(lo) < 1e9).all() and (np.abs(hi) < 1e9).all()):
                        finite = False
                        continue
                    lo = np.maximum(np.floor(lo / SUMMARY) * SUMMARY, 0)
                    hi = np.minimum(np.floor(hi / SUMMARY) * SUMMARY + SUMMARY - 1, np.array(sdims) - 1)
                    if (lo > hi).any():
                        continue
                    lo, hi = lo.astype(np.int64), hi.astype(np.int64)
                    n += bool(observed[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].any())
    return n, finite
