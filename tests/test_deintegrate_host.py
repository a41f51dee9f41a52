"""De-integration without a GPU (include/tsdf_amd.h, "de-integration"): the CPU reference (tests/deintegrate_ref.py) has the sequence
property and keeps the one-removal bound; the entry points are declared, exported and bound; null arguments are refused."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.deintegrate_ref import frame_set, oracle_remove, remove
from tests.helpers import H, W
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tsdf_amd.h")
LIB = os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so")
SYMBOLS = ("tsdf_deintegrate", "tsdf_deintegrate_device")
BIN = os.path.join(ROOT, "build", "kinfu_stream")
SIZE, PHYS = (64, 56, 50), (3000.0, 2625.0, 2343.75)
SEED, PERIOD, K = 0x5EED0B01, 60, 7
U = 2.0 ** -24


def frames(n):
    return [synth.depth_frame(i, PERIOD, seed=SEED) for i in range(n)]


def integrated(oracle, fr):
    ov = oracle.Volume(SIZE, PHYS)
    for d, cam in fr:
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    return ov


@pytest.mark.parametrize("order", ["forward", "reverse", "shuffled"])
def test_removing_every_frame_gives_the_cleared_volume_back(oracle, order):
    fr = frames(K)
    ov = integrated(oracle, fr)
    assert ov.weight.max() == float(K)
    idx = {"forward": list(range(K)), "reverse": list(range(K))[::-1], "shuffled": list(np.random.RandomState(5).permutation(K))}[order]
    total = 0
    for i in idx:
        total += oracle_remove(oracle, ov, *fr[i])[0]
    cleared = oracle.Volume(SIZE, PHYS)
    assert total > 10000
    assert np.array_equal(ov.weight.view(np.uint32), cleared.weight.view(np.uint32))
    assert np.array_equal(ov.dist.view(np.uint32), cleared.dist.view(np.uint32))


def test_removing_the_last_frame_keeps_the_header_bound(oracle):
    """The header's derivation: (5 w / (w - 1) + 1) u T <= 11 u T for w >= 2, asserted as 6 * 2^-23 * T.  Largest deviation the
    reference shows over k = 2 .. 7 frames on this grid: printed below, recorded in DESIGN.md section 11."""
    fr = frames(K)
    worst = 0.0
    for k in range(2, K + 1):
        ov, before = integrated(oracle, fr[:k]), integrated(oracle, fr[:k - 1])
        T = ov.truncation_distance()
        oracle_remove(oracle, ov, *fr[k - 1])
        assert np.array_equal(ov.weight.view(np.uint32), before.weight.view(np.uint32))
        dev = float(np.abs(ov.dist.astype(np.float64) - before.dist.astype(np.float64)).max())
        worst = max(worst, dev / T)
        print("k = %d: max |D' - D_before| = %.3g = %.2f * 2^-23 * trunc" % (k, dev, dev / T * 2 ** 23))
        assert dev <= 6 * 2.0 ** -23 * T
    assert worst > 0.0                                             # (the inverse is not exact: the bound is exercised)


@pytest.mark.parametrize("which", [0, 3])
def test_removing_an_earlier_frame_gives_the_other_frames_average(oracle, which):
    """Against the oracle's volume of the K - 1 other frames (another order of averaging).  In the sum D * w an integrate at new count j
    errs by at most (3 j - 1) u T and a removal at count w by 3 w u T (header); a voxel seen w times carries S(w) + 3 w from the one side
    and S(w - 1) from the other, S(n) = n (3 n + 1) / 2, over the final count w - 1."""
    fr = frames(K)
    ov = integrated(oracle, fr)
    others = integrated(oracle, fr[:which] + fr[which + 1:])
    w = ov.weight.astype(np.float64)
    in_set, tsdf = frame_set(oracle, ov, *fr[which])
    remove(ov, in_set, tsdf)
    assert np.array_equal(ov.weight.view(np.uint32), others.weight.view(np.uint32))
    T = ov.truncation_distance()
    S = lambda n: n * (3 * n + 1) / 2
    bound = np.where(in_set & (w >= 2), (S(w) + 3 * w + S(w - 1)) / np.maximum(w - 1, 1), 0.0) * U * T
    dev = np.abs(ov.dist.astype(np.float64) - others.dist.astype(np.float64))
    print("frame %d: max deviation %.2f * 2^-23 * trunc" % (which, dev.max() / T * 2 ** 23))
    assert np.all(dev <= bound)
    assert dev.max() > 0.0


def test_a_frame_that_was_never_integrated_leaves_unfused_voxels_alone(oracle):
    fr = frames(3)
    ov = integrated(oracle, fr[:2])
    d0, w0 = ov.dist.copy(), ov.weight.copy()
    other = synth.depth_frame(20, PERIOD, seed=SEED)
    in_set, _ = frame_set(oracle, ov, *other)
    updated, stores = oracle_remove(oracle, ov, *other)
    assert updated == int((in_set & (w0 >= 1)).sum()) and 0 < stores <= updated
    untouched = ~(in_set & (w0 >= 1))
    assert np.array_equal(ov.dist[untouched].view(np.uint32), d0[untouched].view(np.uint32))
    assert np.array_equal(ov.weight[untouched].view(np.uint32), w0[untouched].view(np.uint32))
    assert (in_set & (w0 == 0)).sum() > 100


def test_the_entry_points_are_declared_exported_and_bound():
    with open(HEADER) as f:
        text = f.read()
    for s in SYMBOLS:
        assert re.search(r"int\s+%s\s*\(\s*tsdf_volume\s*\*\s*volume\s*," % s, text), s
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    from tsdf_amd import _capi, api
    for s in SYMBOLS:
        assert s in exported, s + " is not exported by libtsdf_hip.so"
        assert s in _capi.EXPORTS and getattr(_capi.lib, s).argtypes is not None, s
    assert callable(api.TSDFVolume.deintegrate) and callable(api.TSDFVolume.deintegrate_device)


def test_null_arguments_are_refused_without_a_device():
    from tsdf_amd import _capi
    for s in SYMBOLS:
        assert getattr(_capi.lib, s)(None, None, 640, 480, None, None, None, None) == _capi.TSDF_ERR_INVALID
        assert "tsdf_deintegrate: null argument" in _capi.last_error()


def test_the_header_states_the_rule():
    with open(HEADER) as f:
        text = f.read()
    flat = " ".join(text[text.index("---- de-integration"):text.index("---- colour fusion")].split())
    assert "if (!(w >= 1.0f))" in flat
    assert "new_distance = ((D * w) - (tsdf * 1.0f)) / nw" in flat
    assert "TSDF_ERR_INVALID" in flat and "not invertible" in flat and "6 * 2^-23" in flat


def test_kinfu_stream_checks_the_window_option():
    assert os.path.exists(BIN), "build/kinfu_stream missing: run `make cpptest` (build() does)"
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert "--window" in r.stdout + r.stderr
    for extra in ([], ["--track", "--weight-cap", "15"], ["--ranks", "2"], ["--track", "--ranks", "2"]):
        r = subprocess.run([BIN, "-d", "nowhere", "--window", "30"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and ("--window" in r.stderr or "--track is single-volume" in r.stderr), (extra, r.stderr)
    r = subprocess.run([BIN, "-d", "nowhere", "--track", "--window", "65536"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--window" in r.stderr


def test_the_tracker_window_is_declared_exported_and_bound():
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"int\s+tsdf_tracker_set_window\s*\(\s*tsdf_tracker\s*\*\s*tracker\s*,\s*uint32_t\s+n\s*\)\s*;", text)
    assert re.search(r"int\s+tsdf_tracker_window\s*\(\s*const\s+tsdf_tracker\s*\*\s*tracker\s*,\s*uint32_t\s*\*\s*n\s*\)\s*;", text)
    from tsdf_amd import _capi, tracking
    assert _capi.lib.tsdf_tracker_set_window(None, 3) == _capi.TSDF_ERR_INVALID
    assert _capi.lib.tsdf_tracker_window(None, None) == _capi.TSDF_ERR_INVALID
    assert callable(tracking.FrameToModelTracker.set_window) and callable(tracking.FrameToModelTracker.window)
