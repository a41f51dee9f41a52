"""The CPU reference of the distance field (tests/esdf_ref.py) checked on its own, no GPU: the three passes equal the brute-force
minimum over sites bit for bit, sqrt(q) agrees with scipy's double-precision EDT, the analytic sphere stays inside the accuracy bound
the header states, and the sign, NaN, fill and cap rules hold."""
import numpy as np
import pytest

from tests import esdf_ref

F32 = np.float32
VS = np.array([10.0, 12.5, 9.0], F32)
SMALL = [(7, 5, 4), (13, 9, 6)]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("size", SMALL)
@pytest.mark.parametrize("negative_share", [0.5, 0.04])
def test_passes_equal_brute_force_bit_for_bit(size, negative_share):
    D, Wt = esdf_ref.random_field(size, 11 + size[0], negative_share)
    site = esdf_ref.sites(D, Wt, size)
    assert 0 < site.sum() < site.size
    q = esdf_ref.squared(site, size, VS)
    assert np.array_equal(bits(q), bits(esdf_ref.brute_force(site, size, VS)))
    assert np.isfinite(q).all() and (q[site] == 0).all() and (q[~site] > 0).all()


@pytest.mark.parametrize("size", SMALL)
def test_sqrt_agrees_with_scipy_edt(size):
    from scipy import ndimage
    D, Wt = esdf_ref.random_field(size, 23 + size[0], 0.1)
    site = esdf_ref.sites(D, Wt, size)
    assert site.any()
    e = np.sqrt(esdf_ref.squared(site, size, VS)).astype(np.float64)
    X, Y, Z = size
    edt = ndimage.distance_transform_edt(~site.reshape(Z, Y, X), sampling=(float(VS[2]), float(VS[1]), float(VS[0]))).reshape(-1)
    err = np.abs(e - edt) / np.maximum(edt, 1e-30)
    err[edt == 0] = np.abs(e[edt == 0])
    print("largest relative difference from scipy's EDT at %s: %.3g" % (size, err.max()))
    assert err.max() <= 1e-6   # four fp32 roundings


def test_sites_are_crossings_between_observed_voxels_only():
    size = (4, 1, 1)
    D = np.array([1.0, -1.0, -1.0, 1.0], F32)
    assert esdf_ref.sites(D, np.ones(4, F32), size).tolist() == [True, True, True, True]
    # an unobserved voxel neither is a site nor makes one: the crossing 2|3 stays, the crossing 0|1 goes
    assert esdf_ref.sites(D, np.array([1, 0, 1, 1], F32), size).tolist() == [False, False, True, True]
    assert esdf_ref.sites(D, np.array([1, np.nan, 1, 1], F32), size).tolist() == [False, False, True, True]
    # 0.0, -0.0 and NaN distances are not negative
    for planted in (0.0, -0.0, np.nan):
        assert esdf_ref.sites(np.array([planted, 1.0, 1.0, 1.0], F32), np.ones(4, F32), size).tolist() == [False] * 4
        assert esdf_ref.sites(np.array([planted, -1.0, 1.0, 1.0], F32), np.ones(4, F32), size).tolist() == [True, True, True, False]


def test_sign_nan_and_fill_rules():
    size = (6, 1, 1)
    D = np.array([2.0, 1.0, -1.0, -2.0, -0.0, np.nan], F32)
    Wt = np.array([1.0, 1.0, 1.0, 0.0, 1.0, np.nan], F32)
    out, n_sites = esdf_ref.esdf(D, Wt, size, VS)
    assert n_sites == 2
    # sites are +0.0 and -0.0; voxel 3 is unobserved, so the crossing 3|4 is none and voxel 4 (-0.0: not negative) is positive
    assert bits(out[:3]).tolist() == bits(np.array([10.0, 0.0, -0.0], F32)).tolist()
    assert np.isnan(out[3]) and out[4] == F32(20.0) and np.isnan(out[5])
    filled, _ = esdf_ref.esdf(D, Wt, size, VS, fill_unknown=True)
    assert np.array_equal(bits(filled[[0, 1, 2, 4]]), bits(out[[0, 1, 2, 4]]))
    assert filled[3] == F32(10.0) and filled[5] == F32(30.0)    # unknown voxels get the positive distance, whatever their sign


def test_a_grid_without_sites():
    size = (3, 2, 2)
    D, Wt = np.full(12, 0.5, F32), np.ones(12, F32)
    Wt[5] = 0.0
    out, n_sites = esdf_ref.esdf(D, Wt, size, VS)
    assert n_sites == 0 and np.isnan(out[5]) and np.isposinf(np.delete(out, 5)).all()
    assert np.isposinf(esdf_ref.esdf(D, Wt, size, VS, fill_unknown=True)[0]).all()
    capped, _ = esdf_ref.esdf(D, Wt, size, VS, max_distance=25.0)
    assert (np.delete(capped, 5) == F32(25.0)).all() and np.isnan(capped[5])


@pytest.mark.parametrize("cap", [35.0, 5.0, float(VS[0])])
def test_capping_never_changes_a_value_below_the_cap(cap):
    size = (13, 9, 6)
    D, Wt = esdf_ref.random_field(size, 77, 0.04)
    free, _ = esdf_ref.esdf(D, Wt, size, VS)
    capped, _ = esdf_ref.esdf(D, Wt, size, VS, max_distance=cap)
    with np.errstate(invalid="ignore"):
        below = np.abs(free) < F32(cap)
    assert below.any() and (~below & ~np.isnan(free)).any()
    assert np.array_equal(bits(capped[below]), bits(free[below]))
    rest = ~below & ~np.isnan(free)
    assert (np.abs(capped[rest]) == F32(cap)).all() and np.array_equal(np.signbit(capped[rest]), np.signbit(free[rest]))
    assert np.array_equal(np.isnan(capped), np.isnan(free))


def test_the_analytic_sphere_stays_inside_the_stated_bound():
    n, vs, radius = 40, F32(7.0), 80.0
    c = (np.arange(n, dtype=np.float64) + 0.5) * float(vs) - n * float(vs) / 2.0
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    signed = (np.sqrt(x * x + y * y + z * z) - radius).reshape(-1)
    D = signed.astype(F32)
    out, n_sites = esdf_ref.esdf(D, np.ones(n ** 3, F32), (n, n, n), (vs, vs, vs))
    assert n_sites > 1000 and np.isfinite(out).all()
    assert np.array_equal(np.signbit(out), signed < 0)
    diff = (np.abs(out.astype(np.float64)) - np.abs(signed)) / float(vs)    # e - t, in voxels
    print("sphere: e - t in [%.4f, %.4f] voxels" % (diff.min(), diff.max()))
    assert -1.0 - 1e-3 <= diff.min() and diff.max() <= np.sqrt(3.0) + 1e-3


def windowed(prev, axis, a, jmax):
    """esdf_ref._pass with the scan cut off behind j = jmax, as the kernels cut it under a cap."""
    n = prev.shape[axis]
    out = prev.copy()
    for j in range(1, min(n - 1, jmax) + 1):
        t = F32(a) * F32(j * j)
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - j), slice(j, n)
        lo, hi = tuple(lo), tuple(hi)
        out[hi] = np.minimum(out[hi], t + prev[lo])
        out[lo] = np.minimum(out[lo], t + prev[hi])
    return out


@pytest.mark.parametrize("cap", [35.0, 5.0, float(VS[0]), 12.4, 1e9])
def test_a_scan_window_of_the_cap_plus_one_voxel_changes_nothing_under_the_cap(cap):
    """The kernels stop a scan at j = ceil(max_distance / voxel_size) + 1 (include/tsdf_amd.h: max_distance only caps)."""
    size = (13, 9, 6)
    D, Wt = esdf_ref.random_field(size, 78, 0.02)
    site = esdf_ref.sites(D, Wt, size)
    A = esdf_ref.areas(VS)
    jmax = [int(np.ceil(cap / float(v))) + 1 for v in VS]
    w = np.where(site, F32(0.0), esdf_ref.INF).astype(F32).reshape(size[2], size[1], size[0])
    q = windowed(windowed(windowed(w, 2, A[0], jmax[0]), 1, A[1], jmax[1]), 0, A[2], jmax[2]).reshape(-1)
    assert np.array_equal(bits(esdf_ref.finish(q, D, Wt, cap)), bits(esdf_ref.finish(esdf_ref.squared(site, size, VS), D, Wt, cap)))
