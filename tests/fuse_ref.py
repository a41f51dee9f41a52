"""CPU reference of volume fusion (include/tsdf_amd.h, "volume fusion"): every sample S is the oracle's orc_trilinear, everything else
numpy float32 operations -- each rounded on its own -- in the order the header states.  Test infrastructure only (uses oracle/).
"""
import numpy as np

from tests.field_ref import bounds, geometry, valid  # noqa: F401  (geometry: re-exported for the tests)

F = np.float32


def rotation(axis, degrees, translation=(0.0, 0.0, 0.0)):
    """A rigid 4 x 4 transform as 16 float32, column-major like a pose: a rotation about `axis` and a translation."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    M[:3, 3] = translation
    return M.T.astype(F).reshape(-1).copy()   # (the transpose of the rows, flattened: column-major)


def fuse(O, dst_geom, dst_trunc, dist, weight, src_geom, src_dist, src_weight, m=None, cap=0, detail=None):
    """-> (distances, weights, updated) of dst after the fuse: float32 copies of the whole grid (x fastest) and a bool mask.
    dst_geom / src_geom = (dims, vs, offset) as geometry() gives them; m: 16 floats, column-major dst -> src (None: identity).
    detail: a dict that receives what the tests' preconditions count -- "q" (the three float32 arrays of step 3), "tapped" (the mask
    after step 5) and "sample" (S at those voxels before step 7, NaN elsewhere)."""
    (X, Y, Z), dvs, doff = dst_geom
    sdims, svs, soff = src_geom
    dvs, doff, svs, soff = (np.asarray(a, F) for a in (dvs, doff, svs, soff))
    m = np.eye(4, dtype=F).reshape(-1) if m is None else np.ascontiguousarray(m, F).reshape(-1)
    dist = np.array(dist, F).reshape(-1)
    weight = np.array(weight, F).reshape(-1)
    src_dist = np.ascontiguousarray(src_dist, F).reshape(-1)
    src_weight = np.ascontiguousarray(src_weight, F).reshape(-1)
    trunc = F(dst_trunc)
    mx = bounds(sdims, svs)
    sX, sY, sZ = sdims
    half, zero = F(0.5), F(0)
    with np.errstate(all="ignore"):
        # 1. centres, one float32 array per axis over the whole grid (x fastest)
        zi, yi, xi = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
        c = [((idx.reshape(-1).astype(F) + half) * dvs[a]) + doff[a] for a, idx in enumerate((xi, yi, zi))]
        # 2. transform, 3. source point
        q = [(((m[r] * c[0] + m[4 + r] * c[1]) + m[8 + r] * c[2]) + m[12 + r]) - soff[r] for r in range(3)]
        assert all(a.dtype == F for a in q)
        ok = np.ones(X * Y * Z, bool)
        for a in range(3):
            ok &= (q[a] >= zero) & (q[a] < mx[a])
        # the voxel q lies in, the lower corner on the unclamped point, the +1 taps clamped at the far faces
        v, lo, hi = [], [], []
        for a in range(3):
            va = np.floor(np.where(ok, q[a], zero) / svs[a]).astype(np.int64)
            ok &= va < sdims[a]          # (within rounding of the upper bound: no such voxel, the sample is NaN)
            va = np.minimum(va, sdims[a] - 1)
            centre = (va.astype(F) + half) * svs[a] + zero
            la = np.maximum(np.where(q[a] < centre, va - 1, va), 0)
            v.append(va)
            lo.append(la)
            hi.append(np.where(la + 1 < sdims[a], la + 1, la))
        at = lambda x, y, z: x + sX * (y + sY * z)
        # 5. all eight tap weights > 0 (False for NaN), 6. the weight of q's own voxel
        for tx in (lo[0], hi[0]):
            for ty in (lo[1], hi[1]):
                for tz in (lo[2], hi[2]):
                    ok &= src_weight[at(tx, ty, tz)] > zero
        ws = src_weight[at(v[0], v[1], v[2])]
        # 4. the sample, through the oracle, where it is needed
        s = np.full(X * Y * Z, np.nan, F)
        s[ok] = O.trilinear_n(np.stack([a[ok] for a in q], axis=1), sdims, svs, src_dist)
        if detail is not None:
            detail.update(q=q, tapped=ok.copy(), sample=s.copy())
        # 7. NaN skips, then the clamp
        ok &= ~np.isnan(s)
        s = np.minimum(np.maximum(s, -trunc), trunc)
        # 8. blend, 9. cap
        wn = weight + ws
        dn = ((dist * weight) + (s * ws)) / wn
        if cap:
            wn = np.where(wn > F(cap), F(cap), wn)
        assert dn.dtype == F and wn.dtype == F
        dist[ok] = dn[ok]
        weight[ok] = wn[ok]
    return dist, weight, ok
