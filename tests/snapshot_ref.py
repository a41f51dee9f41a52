"""CPU reference of the sparse snapshot (include/tsdf_amd.h, "sparse snapshot"): dense arrays and the fill distance -> the ascending
list of live brick ids and the brick arrays, and back.  Words are compared as bits throughout: a distance is cleared only with exactly
the bits of fill, an fp32 weight only with the bits 0x00000000 (-0.0 and NaN are not cleared).  The checker, never the thing under test.
"""
import numpy as np

F32, U32 = np.float32, np.uint32
BRICK = 8
WEIGHT_DTYPES = {8: np.uint8, 16: np.uint16, 32: np.float32}


def bricks_per_axis(size):
    return tuple((int(s) + BRICK - 1) // BRICK for s in size)


def _bits(a):
    """An array's words as unsigned integers of its own width (floats as their bits)."""
    a = np.ascontiguousarray(a)
    return a.view(U32) if a.dtype == np.float32 else a


def _bricked(dense, size, pad):
    """(X * Y * Z,) in index order x + y X + z X Y -> (bricks, 512): brick b = bx + by nb[0] + bz nb[0] nb[1], voxel lx + 8 ly + 64 lz,
    positions beyond the grid holding `pad`."""
    X, Y, Z = (int(s) for s in size)
    nbx, nby, nbz = bricks_per_axis(size)
    full = np.full((nbz * BRICK, nby * BRICK, nbx * BRICK), pad, dtype=dense.dtype)
    full[:Z, :Y, :X] = dense.reshape(Z, Y, X)
    b = full.reshape(nbz, BRICK, nby, BRICK, nbx, BRICK).transpose(0, 2, 4, 1, 3, 5)   # bz, by, bx, lz, ly, lx
    return np.ascontiguousarray(b).reshape(nbx * nby * nbz, BRICK ** 3)


def _unbricked(bricks, size):
    X, Y, Z = (int(s) for s in size)
    nbx, nby, nbz = bricks_per_axis(size)
    full = bricks.reshape(nbz, nby, nbx, BRICK, BRICK, BRICK).transpose(0, 3, 1, 4, 2, 5).reshape(nbz * BRICK, nby * BRICK, nbx * BRICK)
    return np.ascontiguousarray(full[:Z, :Y, :X]).reshape(-1)


def take(dist, weight, size, fill, weight_bits, colour=None):
    """dist (float32), weight (float32 as every accessor reports it), colour (uint32 words or None) of a whole volume whose weights
    are stored in `weight_bits` bits -> (ids uint32 (n,), distances float32 (n, 512), weights (n, 512) of the storage's element type,
    colours uint32 (n, 512) or None)."""
    dist = np.ascontiguousarray(dist, F32).reshape(-1)
    weight = np.ascontiguousarray(weight, F32).reshape(-1)
    fill = F32(fill)
    if weight_bits == 32:
        w = weight
    else:
        w = weight.astype(WEIGHT_DTYPES[weight_bits])
        assert np.array_equal(w.astype(F32), weight), "weights are not counts of %d bits" % weight_bits
    live = (_bits(dist) != fill.reshape(1).view(U32)[0]) | (_bits(w) != 0)
    if colour is not None:
        colour = np.ascontiguousarray(colour, U32).reshape(-1)
        live |= colour != 0
    # (padding is never live: it is False here)
    ids = np.flatnonzero(_bricked(live, size, False).any(axis=1)).astype(U32)
    d = _bricked(dist.view(U32), size, fill.reshape(1).view(U32)[0])[ids].view(F32)
    wb = _bricked(_bits(w), size, 0)[ids]
    wb = wb.view(F32) if weight_bits == 32 else wb
    c = None if colour is None else _bricked(colour, size, 0)[ids]
    return ids, d, wb, c


def put(ids, distances, weights, colours, size, fill):
    """The inverse: (dist float32, weight float32, colour uint32 or None) dense arrays; voxels of bricks that are not stored get fill,
    weight 0 and colour 0."""
    nb = bricks_per_axis(size)
    total = nb[0] * nb[1] * nb[2]
    ids = np.asarray(ids, np.int64)
    fill_bits = F32(fill).reshape(1).view(U32)[0]
    d = np.full((total, BRICK ** 3), fill_bits, U32)
    d[ids] = np.ascontiguousarray(distances, F32).reshape(-1, BRICK ** 3).view(U32)
    weights = np.ascontiguousarray(weights).reshape(-1, BRICK ** 3)
    if weights.dtype == np.float32:
        w = np.zeros((total, BRICK ** 3), U32)
        w[ids] = weights.view(U32)
        w_dense = _unbricked(w, size).view(F32)
    else:
        w = np.zeros((total, BRICK ** 3), weights.dtype)
        w[ids] = weights
        w_dense = _unbricked(w, size).astype(F32)
    c_dense = None
    if colours is not None:
        c = np.zeros((total, BRICK ** 3), U32)
        c[ids] = np.ascontiguousarray(colours, U32).reshape(-1, BRICK ** 3)
        c_dense = _unbricked(c, size)
    return _unbricked(d, size).view(F32), w_dense, c_dense


def random_field(size, seed, weight_bits, colour, fill, live_share=0.4):
    """A random volume state with whole blocks of 8^3 left cleared: (dist, weight float32, colour or None).  About `live_share` of the
    bricks get random voxels (a third of them cleared again); weights are counts the storage holds, or any floats for 32 bits."""
    rng = np.random.default_rng(seed)
    X, Y, Z = (int(s) for s in size)
    n = X * Y * Z
    nb = bricks_per_axis(size)
    brick_live = rng.random(nb[0] * nb[1] * nb[2]) < live_share
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    b = (x // BRICK + (y // BRICK) * nb[0] + (z // BRICK) * nb[0] * nb[1]).reshape(-1)
    on = brick_live[b] & (rng.random(n) < 0.66)
    dist = np.where(on, rng.uniform(-1.0, 1.0, n).astype(F32) * F32(fill), F32(fill)).astype(F32)
    top = {8: 255, 16: 65535, 32: 1000}[weight_bits]
    weight = np.where(on & (rng.random(n) < 0.8), rng.integers(0, top + 1, n), 0).astype(F32)
    if weight_bits == 32:
        weight = np.where(on & (rng.random(n) < 0.2), rng.uniform(0.0, 3.0, n).astype(F32), weight).astype(F32)
    col = None
    if colour:
        col = np.where(on & (rng.random(n) < 0.5), rng.integers(0, 2 ** 32, n, dtype=np.uint64), 0).astype(U32)
    return dist, weight, col
