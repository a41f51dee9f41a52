"""Weighted integration without a GPU (include/tsdf_amd.h, "weighted integration"): the CPU reference (tests/weighted_ref.py) has the
unit property against the oracle, treats a pixel of invalid weight as a pixel without depth, and its weight models have the values the
header promises at dropouts, borders and below z_ref."""
import numpy as np

from tests import weighted_ref as R
from tests.helpers import H, W, assert_same_floats
from tsdf_amd import synth

SIZE, PHYS = (64, 56, 50), (3000.0, 2625.0, 2343.75)
SEED, PERIOD = 0x5EED0C01, 60
SPECIALS = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf], np.float32)


def frames(n):
    return [synth.depth_frame(i, PERIOD, seed=SEED) for i in range(n)]


def test_unit_weights_are_the_oracles_integrate(oracle):
    ov, rv = oracle.Volume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    ones = np.ones(W * H, np.float32)
    total = 0
    for d, cam in frames(6):
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
        total += R.integrate(oracle, rv, d, ones, cam)[0]
    assert total > 10000 and ov.weight.max() == 6.0
    assert_same_floats(rv.weight, ov.weight, "unit weights: weights")
    assert_same_floats(rv.dist, ov.dist, "unit weights: distances")


def test_a_pixel_of_invalid_weight_is_a_pixel_without_depth(oracle):
    rng = np.random.RandomState(7)
    a, b = oracle.Volume(SIZE, PHYS), oracle.Volume(SIZE, PHYS)
    for i, (d, cam) in enumerate(frames(3)):
        p = rng.uniform(1 / 64, 64, W * H).astype(np.float32)
        stripe = (np.arange(W * H) // 7) % 3 == i % 3
        p[stripe] = SPECIALS[np.arange(stripe.sum()) % SPECIALS.size]
        zeroed = np.where(stripe, 0, d).astype(np.uint16)
        assert np.array_equal(R.masked_depth(d, p), zeroed)
        q = np.where(stripe, np.float32(1.0), p)                       # (any valid weight: those pixels have no depth)
        ua = R.integrate(oracle, a, d, p, cam)
        ub = R.integrate(oracle, b, zeroed, q, cam)
        assert ua == ub and ua[0] > 1000
    assert_same_floats(a.weight, b.weight, "masked: weights")
    assert_same_floats(a.dist, b.dist, "masked: distances")
    assert not np.isnan(a.weight).any() and np.isfinite(a.weight).all()


def test_the_model_reference_has_the_promised_values():
    d, cam = synth.depth_frame(0, PERIOD, seed=SEED)
    d = d.copy().reshape(H, W)
    d[100:110, 200:260] = 0                                            # dropouts
    kinv = cam.kinv()
    z_ref = 2000.0
    for flags in (0, 1, 2, 3):
        w = R.depth_weights(d, W, H, kinv, flags, z_ref)
        assert w.dtype == np.float32 and w.shape == (H, W)
        assert np.all(w[d == 0] == 0.0) and not np.signbit(w[d == 0]).any()
        assert np.all(w <= 1.0) and np.all(w >= 0.0)
        if flags & R.COSINE:
            border = np.ones((H, W), bool)
            border[1:-1, 1:-1] = False
            assert np.all(w[border] == 0.0)
            hole = np.zeros((H, W), bool)
            hole[99:111, 199:261] = True                                # the dropouts and their 4-neighbours
            assert np.all(w[99:111, 200:260][d[99:111, 200:260] == 0] == 0.0)
            assert np.all(w[99, 200:260] == 0.0) and np.all(w[110, 200:260] == 0.0) and np.all(w[100:110, 199] == 0.0)
            assert (w > 0).sum() > 1000
        else:
            assert np.all(w[d != 0] > 0.0)
    w = R.depth_weights(d, W, H, kinv, R.INVERSE_SQUARE, z_ref)
    near = (d != 0) & (d <= z_ref)
    assert near.sum() > 0 and np.all(w[near] == 1.0)
    far = d > z_ref * 1.01
    assert far.sum() > 0 and np.all(w[far] < 1.0)
    assert np.all(R.depth_weights(d, W, H, kinv, 0)[d != 0] == 1.0)


def test_kinfu_stream_checks_the_weights_options():
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "kinfu_stream")
    assert os.path.exists(exe), "build/kinfu_stream missing: run `make cpptest` (build() does)"
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert "--weights" in r.stdout + r.stderr and "--weight-ref" in r.stdout + r.stderr
    for extra in (["--weights", "cosine"], ["--track", "--weights", "bogus"], ["--track", "--weights", "inverse-square"],
                  ["--track", "--weights", "inverse-square", "--weight-ref", "-5"], ["--track", "--window", "3", "--weights", "cosine"],
                  ["--track", "--weight-ref", "2000"]):
        r = subprocess.run([exe, "-d", "nowhere"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--weight" in r.stderr, (extra, r.stderr)
    # accepted options get as far as the missing directory
    r = subprocess.run([exe, "-d", "nowhere", "--track", "--weights", "inverse-square,cosine", "--weight-ref", "2000"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--weight" not in r.stderr, r.stderr
