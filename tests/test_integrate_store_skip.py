"""integrate stores a distance only when the blend changes its bits (integrate_packed.hip / integrate.hip, blend_and_store).

A voxel that has only seen free space holds +trunc, and the reference's blend (D w + trunc) / (w + 1) (src/TSDF/TSDFVolume.cu:375-381)
gives +trunc back bit for bit at most counts -- it moves at counts 6, 7, 9, 12, 22, 25, ... -- so most stores would write what memory
holds.  Skipping them must not show in a single bit: long streams in every weight storage against the CPU oracle, uploaded special
values (-0, +0, NaN, denormals), the incremental occupancy rebuild (a brick whose every store was skipped is no longer marked for it)
and both ray casts.  The store count the volume keeps with counting on is pinned exactly against the distances' own bits.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import tsdf_amd
from tests.helpers import H, W, assert_same_floats, camera_at
from tests.test_occupancy import _expected
from tsdf_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0003            # bench.py's stream (config 3)
N_FRAMES = 32                # free-space voxels in view all along reach counts past 25


def stream(n_frames=N_FRAMES, period=200):
    """The first frames of bench.py's 200-frame trajectory: a slow camera, so a voxel in view is updated by nearly every frame."""
    return [synth.depth_frame(i, period, seed=SEED) for i in range(n_frames)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def step(oracle, gv, ov, depth, cam):
    gv.integrate(depth, W, H, cam)
    ov.integrate(depth, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())


def storage(gv, ov, mode):
    """Put the pair into weight storage `mode` (8: the default; 16: counts that do not fit a byte, uploaded out of view; 32: the
    device pointer taken, the reference's fp32 layout for good)."""
    if mode == 16:
        w = np.zeros(gv.resident_voxels(), np.float32)
        w[0] = 300.0                                        # (the grid's corner voxel: behind the camera of every frame here)
        gv.set_weight_data(w); ov.set_weight_data(w)
    elif mode == 32:
        assert gv.weight_data()
    assert gv.weight_storage()[0] == mode


@pytest.mark.parametrize("mode", [8, 16, 32])
@pytest.mark.parametrize("n", [128, 256])
def test_a_long_stream_is_the_oracles_in_every_weight_storage(oracle, n, mode):
    gv, ov = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3), oracle.Volume((n,) * 3, (3000.0,) * 3)
    storage(gv, ov, mode)
    frames = stream()
    gv.set_counting(True)
    prev = gv.get_distance_data()
    skipped = 0
    for i, (d, cam) in enumerate(frames):
        step(oracle, gv, ov, d, cam)
        cur = gv.get_distance_data()
        updated, stores = gv.last_updated_voxels(), gv.last_distance_stores()
        # a store is issued exactly where the bits change (every voxel the frame changes is one it updates)
        assert stores == int((bits(cur) != bits(prev)).sum()), "frame %d: distance stores" % i
        assert stores <= updated
        skipped += updated - stores
        prev = cur
        if i % 8 == 7 or i == N_FRAMES - 1:
            assert_same_floats(cur, ov.dist, "%d^3, %d-bit weights, frame %d: distances" % (n, mode, i))
            assert_same_floats(gv.get_weight_data(), ov.weight, "%d^3, %d-bit weights, frame %d: weights" % (n, mode, i))
    gv.set_counting(False)
    assert gv.weight_storage()[0] == mode
    w = ov.weight[ov.weight < 256]
    assert w.max() >= 26, "no voxel crossed counts 6, 7, 9, 12, 22, 25: the stream proves nothing"
    assert skipped > 0, "no store was skipped: the stream proves nothing"
    # the picture of the last pose, whichever cast this process takes
    cam = frames[-1][1]
    V, N = gv.raycast(W, H, cam)
    Vo, No = ov.raycast(W, H, cam.pose(), cam.kinv(), nthreads=oracle.max_threads())
    assert_same_floats(V, Vo, "vertices")
    assert_same_floats(N, No, "normals")
    assert int((~np.isnan(Vo[:, 0])).sum()) > 1000


def test_uploaded_special_distances_keep_their_bits(oracle):
    """-0.0, +0.0, NaNs with payloads and denormals uploaded as distances, under small counts; a camera looking straight down +z with
    a flat depth image: plane z = 20 of a 64^3 grid of 10 mm voxels lies exactly at the depth (sdf = +0 there).  A -0 there blends to
    +0 -- equal as floats, not as bits: it must be stored -- and a +0 blends to +0 (skipped).  Where the frame updates nothing the
    uploaded bits stay as they are, NaN payloads included; everywhere the result is the oracle's."""
    n = 64
    gv, ov = tsdf_amd.TSDFVolume((n,) * 3, (640.0,) * 3), oracle.Volume((n,) * 3, (640.0,) * 3)
    trunc = np.float32(gv.truncation_distance())
    special = np.array([0x80000000, 0x00000000, 0x7fc01234, 0xffc00007, 0x7f800001, 0x00000001, 0x807fffff, 0x00800000,
                        int(trunc.view(np.uint32)), int((-trunc).view(np.uint32))], np.uint32)
    i = np.arange(n ** 3)
    D = special[(i + i // n + i // (n * n)) % special.size].view(np.float32)
    Wt = np.array([0.0, 1.0, 3.0, 7.0, 30.0], np.float32)[(i // 3) % 5]
    gv.set_distance_data(D); ov.set_distance_data(D)
    gv.set_weight_data(Wt); ov.set_weight_data(Wt)
    assert gv.weight_storage()[0] == 8
    assert np.array_equal(bits(gv.get_distance_data()), bits(D)), "uploaded distances come back"
    cam = camera_at((320.0, 320.0, -1000.0))             # camz = 10 z + 1005 (exact): depth 1205 is plane 20
    depth = np.full(W * H, 1205, np.uint16)
    step(oracle, gv, ov, depth, cam)
    got, ref = gv.get_distance_data(), ov.dist
    assert_same_floats(got, ref, "distances")
    assert_same_floats(gv.get_weight_data(), ov.weight, "weights")
    not_nan = ~np.isnan(ref)
    assert np.array_equal(bits(got)[not_nan], bits(ref)[not_nan]), "signed zeros and denormals"
    untouched = ov.weight == Wt
    assert np.array_equal(bits(got)[untouched], bits(D)[untouched]), "voxels the frame did not update keep their bits"
    updated = ~untouched
    minus_to_plus = updated & (bits(D) == 0x80000000) & (bits(ref) == 0)
    assert minus_to_plus.sum() > 100, "no -0 blended to +0: the test proves nothing"
    assert (updated & (bits(D) == 0) & (bits(ref) == 0)).sum() > 100, "no +0 stayed +0"
    assert (updated & np.isnan(D)).sum() > 100 and (untouched & np.isnan(D)).sum() > 100


def test_bricks_with_only_skipped_stores_leave_the_incremental_rebuild_exact(oracle):
    """A far wall behind a cleared volume: every voxel in view is free space (tsdf = +trunc) and counts 0 -> 5 leave +trunc as it
    is, so those frames store no distance and mark no brick for the next occupancy rebuild.  Between rounds of them, surface frames;
    after each round the flags of the incremental rebuild equal their definition over ALL distances (= a full scan,
    tests/test_occupancy.py), and the volume is the oracle's."""
    n = 64
    gv, ov = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3), oracle.Volume((n,) * 3, (3000.0,) * 3)
    tau = np.float32(0.01) * np.float32(gv.truncation_distance())
    far_cam = camera_at((1500.0, 1500.0, -2000.0))
    far = np.full(W * H, 9000, np.uint16)
    surface = [synth.depth_frame(i, 200, seed=SEED) for i in range(0, 60, 6)]
    gv.set_counting(True)
    flagged = 0
    rounds = [("far wall", [(far, far_cam)] * 3), ("surface", surface[:4]), ("far wall", [(far, far_cam)] * 2),
              ("surface", surface[4:7]), ("far wall", [(far, far_cam)] * 4), ("surface", surface[7:])]
    for rnd, (what, frames) in enumerate(rounds):
        for d, cam in frames:
            step(oracle, gv, ov, d, cam)
            if rnd == 0:
                assert gv.last_updated_voxels() > 100000 and gv.last_distance_stores() == 0, "free space, counts < 6: nothing stored"
        fine, cell, _ = gv.occupancy_data(force_rebuild=True)
        D = gv.get_distance_data()
        assert_same_floats(D, ov.dist, "round %d (%s): distances" % (rnd, what))
        ef, ec = _expected(D, (n, n, n), tau, trunc=gv.truncation_distance())
        assert np.array_equal(fine, ef), "round %d (%s): fine flags" % (rnd, what)
        assert np.array_equal(cell, ec), "round %d (%s): cell flags" % (rnd, what)
        flagged += int(fine.sum())
    gv.set_counting(False)
    assert flagged > 0, "no surface: the test proves nothing"


_CAST_PROBE = r"""
import sys, numpy as np
import tsdf_amd
from tsdf_amd import synth
n = int(sys.argv[2])
gv = tsdf_amd.TSDFVolume((n, n, n), (3000.0, 3000.0, 3000.0))
for i in range(30):
    d, cam = synth.depth_frame(i, 200, seed=0x5EED0003)
    gv.integrate(d, synth.WIDTH, synth.HEIGHT, cam)
V, N = gv.raycast(synth.WIDTH, synth.HEIGHT, cam)
np.savez(sys.argv[1], D=gv.get_distance_data(), V=V, N=N, cells=np.array(gv.last_raycast_cell_parallel()))
"""


@pytest.mark.parametrize("cells", ["0", "2"])
def test_both_casts_stay_exact_after_a_stream_with_skipped_stores(oracle, tmp_path, cells):
    """30 frames of bench.py's stream at 128^3 (the occupancy flags from the incremental rebuilds of 2, 4, 8, 16 integrations),
    then the march (TSDF_RAY_CELLS=0) or the cell-parallel cast (=2), each in a process of its own: the oracle's picture."""
    n = 128
    out = str(tmp_path / "cast.npz")
    e = dict(os.environ, TSDF_RAY_CELLS=cells)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-c", _CAST_PROBE, out, str(n)], check=True, env=e, cwd=ROOT, timeout=600)
    got = np.load(out)
    ov = oracle.Volume((n,) * 3, (3000.0,) * 3)
    for d, cam in stream(30):
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    assert_same_floats(got["D"], ov.dist, "distances")
    assert bool(got["cells"]) == (cells == "2")
    Vo, No = ov.raycast(W, H, cam.pose(), cam.kinv(), nthreads=oracle.max_threads())
    assert_same_floats(got["V"], Vo, "vertices")
    assert_same_floats(got["N"], No, "normals")
    assert int((~np.isnan(Vo[:, 0])).sum()) > 1000
