"""Ray queries off the GPU: the reference the GPU tests compare against (tests/ray_ref.py: the oracle's 1 x 1 image cast per ray) equals
the oracle's own image cast on the pixel rays, every ray set of tests/ray_cases.py keeps the coverage it is there for -- conditions on
the reference alone, met by the choice of seeds -- and the refusals that need no device."""
import numpy as np

from tests import ray_cases, ray_ref
from tests.helpers import assert_same_floats

F = np.float32


def hits_of(ref):
    return ~np.isnan(ref[1])


def test_the_per_ray_reference_equals_the_oracles_image_cast(oracle):
    s = ray_cases.scene(oracle)
    V, _ = s.ov.raycast(ray_cases.CAST_W, ray_cases.CAST_H, s.cam.pose(), s.cam.kinv(), nthreads=oracle.max_threads())
    assert_same_floats(s.ref["pixels"][0], V, "1 x 1 casts against the 80 x 60 cast")
    # t is the parameter of the point: origin + t * dir is the point to within the rounding of the three adds
    o, d, _ = s.sets["pixels"]
    P, T, _ = s.ref["pixels"]
    h = hits_of(s.ref["pixels"])
    back = o[h].astype(np.float64) + T[h, None].astype(np.float64) * d[h].astype(np.float64)
    assert np.abs(back - P[h]).max() < 1e-2


def test_every_ray_set_keeps_its_coverage(oracle):
    s = ray_cases.scene(oracle)
    for name, (o, d, m) in s.sets.items():
        assert len(o) == len(d) and (m is None or len(m) == len(o))
        assert name == "pixels" or len(o) % 64 != 0, name              # (4 800 pixels are 75 waves: the other sets end in a partial wave)
        P, T, N = s.ref[name]
        assert (np.isnan(P).any(axis=1) == np.isnan(T)).all() and (np.isnan(P).all(axis=1) == np.isnan(T)).all()
        assert np.isnan(N[np.isnan(T)]).all()
    h1 = hits_of(s.ref["pixels"])
    assert h1.sum() >= 800 and (~h1).sum() >= 800
    assert len(s.sets["shuffled"][0]) == len(h1) - 3
    h3 = hits_of(s.ref["inside"])
    assert h3.sum() >= 300 and (~h3).sum() >= 200
    # some origins are behind the surface: a hit at sample 0 is t == near_t == 0 refined backwards or not at all
    assert (s.ref["inside"][1][h3] <= 0).sum() >= 1
    h4 = hits_of(s.ref["outside"])
    assert (~s.outside_meets_box).sum() >= 100 and h4.sum() >= 200
    assert not h4[~s.outside_meets_box].any()
    h5 = hits_of(s.ref["edges"])
    assert h5.sum() >= 10 and (~h5).sum() >= 10
    o5, d5, _ = s.sets["edges"]
    assert (np.signbit(d5) & (d5 == 0)).any() and ((d5 == 0) & ~np.signbit(d5)).any()
    assert ((o5 == s.smin) | (o5 == s.smax)).all(axis=1).sum() >= 8      # corners
    # set 6: per scale, a ray that hits unscaled and whose scaled answer differs
    n = ray_cases.N_SCALED
    P3 = s.ref["inside"][0][:n]
    for j, scale in enumerate(ray_cases.SCALES):
        Pk = s.ref["scaled"][0][j * n:(j + 1) * n]
        differs = (P3.view(np.uint32) != Pk.view(np.uint32)).any(axis=1) & ~(np.isnan(P3).all(axis=1) & np.isnan(Pk).all(axis=1))
        assert (h3[:n] & differs).sum() >= 1, scale
    # the longest scale steps over surfaces the unscaled march stops at
    far = s.ref["scaled"][1][2 * n:]
    assert (h3[:n] & np.isnan(far)).sum() >= 1
    h7 = hits_of(s.ref["decreed"])
    assert not h7[:-1].any() and len(h7) >= 20
    h8 = hits_of(s.ref["limited"])
    assert h8.any() and (~h8).any()
    k = h3.sum()
    assert len(h8) in (6 * k, 6 * k - 1)
    assert h8[:k].all() and not h8[k:2 * k].any() and h8[2 * k:3 * k].all()         # t itself, just below, just above
    assert not h8[4 * k:5 * k].any() and h8[5 * k:6 * k - 1].all()                   # NaN, +inf
    # t_max = 0 keeps exactly the hits with t <= 0
    assert (h8[3 * k:4 * k] == (s.ref["inside"][1][h3] <= 0)).all()


def test_the_reference_applies_the_decreed_misses_and_the_range_limit(oracle):
    s = ray_cases.scene(oracle)
    o, d, _ = s.sets["inside"]
    h = np.flatnonzero(hits_of(s.ref["inside"]))[:5]
    # the limit through ray_ref.cast itself equals ray_ref.limit on the unlimited answers
    m = s.ref["inside"][1][h].copy()
    m[1] = np.nextafter(m[1], F(-np.inf))
    m[2] = np.nan
    a = ray_ref.cast(oracle, s.ov, o[h], d[h], t_max=m, normals=True)
    b = ray_ref.limit(*(x[h] for x in s.ref["inside"]), m)
    for x, y, name in zip(a, b, ("points", "t", "normals")):
        assert_same_floats(x, y, name)
    assert np.isnan(a[1][[1, 2]]).all() and not np.isnan(a[1][[0, 3, 4]]).any()
    assert ray_ref.decreed_miss(np.array([0, np.nan, 0], F), np.ones(3, F))
    assert ray_ref.decreed_miss(np.zeros(3, F), np.array([0.0, -0.0, 0.0], F))
    assert not ray_ref.decreed_miss(np.zeros(3, F), np.array([0.0, -0.0, 1e-30], F))


def test_refusals_that_need_no_device():
    from tsdf_amd import _capi
    buf = np.zeros(12, F)
    p = buf.ctypes.data
    for fn in (_capi.lib.tsdf_volume_cast_rays, _capi.lib.tsdf_volume_cast_rays_device):
        assert fn(None, 1, p, p, None, p, None, None) == _capi.TSDF_ERR_INVALID
        assert "null volume" in _capi.last_error()
        assert fn(None, 0, None, None, None, None, None, None) == _capi.TSDF_ERR_INVALID


def test_host_normalisation_is_fp32():
    from tsdf_amd import api
    d = np.array([[3, 4, 0], [1e-3, 2e-3, -2e-3], [0, 0, 0], [np.inf, 1, 1]], F)
    ln = api.direction_lengths(d)
    assert ln.dtype == F and ln[0] == F(5) and ln[2] == 0
    expected = np.sqrt(F(F(d[1, 0] * d[1, 0]) + F(d[1, 1] * d[1, 1])) + F(d[1, 2] * d[1, 2]))
    assert ln[1] == expected
    u = api.unit_directions(d)
    assert u.dtype == F and (u[0] == np.array([0.6, 0.8, 0.0], F)).all()
    assert (u[1] == d[1] / ln[1]).all()
    assert not np.isfinite(u[2]).all() and not np.isfinite(u[3]).all()      # a ray query answers these with a miss
