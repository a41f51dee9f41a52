"""CPU reference of the distance field (include/tsdf_amd.h, "distance field") in numpy, every operation in float32 as the header
writes it: sites(), the three unwindowed passes, finish(), and the brute-force minimum of c(v, s) over all sites for small grids.
Arrays are flat in the volume's index order x + y X + z X Y (reshaped (Z, Y, X) inside); size = (X, Y, Z)."""
import numpy as np

F32 = np.float32
INF = F32(np.inf)


def _zyx(a, size):
    return np.ascontiguousarray(a, F32).reshape(int(size[2]), int(size[1]), int(size[0]))


def observed(weights):
    """w > 0; a NaN weight is not observed."""
    with np.errstate(invalid="ignore"):
        return np.asarray(weights, F32) > F32(0.0)


def negative(distances):
    """d < 0, the mesh's sign test: NaN and both zeros are not negative."""
    with np.errstate(invalid="ignore"):
        return np.asarray(distances, F32) < F32(0.0)


def sites(distances, weights, size):
    """The boolean site mask, flat: observed voxels with an observed 6-neighbour inside the grid of the other sign."""
    obs, neg = observed(_zyx(weights, size)), negative(_zyx(distances, size))
    site = np.zeros(obs.shape, bool)
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = obs[lo] & obs[hi] & (neg[lo] != neg[hi])
        site[lo] |= cross
        site[hi] |= cross
    return site.reshape(-1)


def areas(voxel_size):
    """A[a] = vs[a] * vs[a], one fp32 multiply each."""
    vs = np.asarray(voxel_size, F32)
    return vs * vs


def _pass(prev, axis, a):
    """min_j (a * (float)(j * j) + prev[i +- j]) along `axis` of a (Z, Y, X) array, unwindowed."""
    n = prev.shape[axis]
    out = prev.copy()   # j = 0: a * 0 + prev
    for j in range(1, n):
        t = F32(a) * F32(j * j)
        src_lo = [slice(None)] * 3
        dst_lo = [slice(None)] * 3
        src_lo[axis], dst_lo[axis] = slice(0, n - j), slice(j, n)
        src_lo, dst_lo = tuple(src_lo), tuple(dst_lo)
        out[dst_lo] = np.minimum(out[dst_lo], t + prev[src_lo])     # the neighbour j below
        out[src_lo] = np.minimum(out[src_lo], t + prev[dst_lo])     # the neighbour j above
    return out


def pass_x(site, size, voxel_size):
    w0 = np.where(np.asarray(site, bool), F32(0.0), INF).astype(F32).reshape(int(size[2]), int(size[1]), int(size[0]))
    return _pass(w0, 2, areas(voxel_size)[0])


def pass_y(prev, voxel_size):
    return _pass(prev, 1, areas(voxel_size)[1])


def pass_z(prev, voxel_size):
    return _pass(prev, 0, areas(voxel_size)[2])


def squared(site, size, voxel_size):
    """q, flat: the three passes."""
    return pass_z(pass_y(pass_x(site, size, voxel_size), voxel_size), voxel_size).reshape(-1)


def brute_force(site, size, voxel_size):
    """q, flat: min over sites of A[2]*(float)(dz*dz) + (A[1]*(float)(dy*dy) + A[0]*(float)(dx*dx)); small grids only."""
    X, Y, Z = (int(s) for s in size)
    A = areas(voxel_size)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    x, y, z = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    q = np.full(X * Y * Z, INF, F32)
    for s in np.flatnonzero(np.asarray(site, bool)):
        dx, dy, dz = x - x[s], y - y[s], z - z[s]
        c = A[2] * (dz * dz).astype(F32) + (A[1] * (dy * dy).astype(F32) + A[0] * (dx * dx).astype(F32))
        q = np.minimum(q, c)
    return q


def finish(q, distances, weights, max_distance, fill_unknown=False):
    """sqrtf, the cap, the sign and the rule for unobserved voxels."""
    md = F32(max_distance)
    e = np.sqrt(np.asarray(q, F32))
    with np.errstate(invalid="ignore"):
        e = np.where(e < md, e, md).astype(F32)
    obs, neg = observed(weights).reshape(-1), negative(distances).reshape(-1)
    out = np.where(neg, -e, e).astype(F32)
    unknown = e if fill_unknown else np.full(e.shape, np.nan, F32)
    return np.where(obs, out, unknown).astype(F32)


def esdf(distances, weights, size, voxel_size, max_distance=np.inf, fill_unknown=False):
    """(the field flat, the number of sites)"""
    site = sites(distances, weights, size)
    return finish(squared(site, size, voxel_size), distances, weights, max_distance, fill_unknown), int(site.sum())


def random_field(size, seed, negative_share=0.5, unobserved_share=0.3, nan_weight=True):
    """(distances, weights), flat: signed noise, `negative_share` of it negative (a small share leaves few sites and long scans),
    about `unobserved_share` of the weights zero (the others small whole numbers), and 0.0, -0.0 and NaN distances and -- unless
    nan_weight is off -- a NaN weight planted."""
    rng = np.random.default_rng(seed)
    n = int(size[0]) * int(size[1]) * int(size[2])
    D = rng.uniform(0.05, 1.0, n).astype(F32)
    D[rng.random(n) < negative_share] *= F32(-1.0)
    Wt = rng.integers(1, 9, n).astype(F32)
    Wt[rng.random(n) < unobserved_share] = F32(0.0)
    k = min(6, n // 4)             # (a tiny grid keeps most of its noise)
    at = rng.choice(n, k + 1, replace=False)
    D[at[:k]] = np.array([0.0, -0.0, np.nan, 0.0, -0.0, np.nan], F32)[:k]
    Wt[at[:k]] = F32(3.0)          # the planted distances are observed ...
    if nan_weight:
        Wt[at[k]] = F32(np.nan)    # ... and one weight is NaN: not observed
    return D, Wt
