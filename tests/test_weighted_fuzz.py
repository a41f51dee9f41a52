"""GPU: weighted integration and its weight models at odd sizes and edges, and weighted frames among the other writers of a volume.

  * one test per seed of tests/weighted_cases.py (aimed first, then drawn): after every frame distances, weights, colour words,
    the counters where counting is on and weight_storage() == (32, pinned) against the composed CPU model (tests/volume_model.py over
    tests/weighted_ref.py); the caller's arrays unchanged; at the end the ray casts of the last two cameras against the oracle on the
    model's arrays, the lazy brick flags at least their definition and the rebuilt ones equal to it, two Z-slabs against the whole
    volume where the case asks for them.  Every fourth seed calls the device variant: depth at an odd uint16 offset into its
    allocation, the weights one float into theirs, guard words round both, every image larger than the one before;
  * the twelve sequences of tests/weighted_sequences.py through tests/test_op_sequences.drive;
  * the weight models at eleven image sizes from 1 x 1 up, four flag values and two kinv;
  * the tracker's weighting mode on a colour volume against the same calls made by hand.

Every comparison is bit for bit.  tests/test_weighted_fuzz_host.py shows, without a GPU, that the cases reach what they are aimed at.

Cost on an MI355X host, oracle work included: the whole file (150 tests) 14.3 s, of which 11.5 s are the first import of torch and the
start of its context in seed 3, the first device variant (a suite that has used torch before does not pay it); every other case 0.01 -
0.25 s, a sequence 0.02 - 0.05 s, a weight-model case under 0.01 s, the tracker 0.39 s.  The parent commit's tests/test_weighted.py on
the same machine: 15.2 s for 25 tests, of which 11.2 s are the same start of torch.
"""
import numpy as np
import pytest

import tsdf_amd
from tests import weighted_cases as WC
from tests import weighted_ref as R
from tests import weighted_sequences as WS
from tests.helpers import H, W, Cam, assert_same_floats
from tests.test_op_sequences import drive
from tsdf_amd import synth

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
_SEEN = {"cases": 0, "worked": 0, "casts": 0, "casts_hit": 0, "device": 0, "grown": 0, "sequences": 0}
GUARD16, GUARD32 = 0xBEEF, F32(-7.0)


def _same_words(got, want, what):
    bad = np.flatnonzero(got != want)
    assert not bad.size, "%s: %d colour words differ, first at %d: %#x vs %#x" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _device_call(gv, op):
    """integrate_weighted_device on arrays inside larger allocations: the depth 5 uint16 in (an odd offset: 2 bytes off a 4-byte
    boundary), the weights one float in, guard words before and behind both.  Returns after the stream has drained, with the
    allocations checked word for word: guards and the caller's arrays alike."""
    import torch
    _, d, p, rgb, cam, w, h = op
    n = w * h
    dbuf = np.full(n + 10, GUARD16, np.uint16)
    dbuf[5:5 + n] = d
    pbuf = np.full(n + 5, GUARD32, F32)
    pbuf[1:1 + n] = p
    td, tp = torch.from_numpy(dbuf.view(np.int16).copy()).cuda(), torch.from_numpy(pbuf.copy()).cuda()
    tc = torch.from_numpy(np.ascontiguousarray(rgb).reshape(-1).copy()).cuda() if rgb is not None else None
    torch.cuda.synchronize()
    assert td.data_ptr() % 4 == 0 and tp.data_ptr() % 4 == 0
    gv.integrate_weighted_device(td.data_ptr() + 10, tp.data_ptr() + 4, w, h, Cam(*cam), rgb_ptr=tc.data_ptr() if tc is not None else None)
    gv.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(td.cpu().numpy().view(np.uint16), dbuf), "the depth allocation was written"
    assert tp.cpu().numpy().tobytes() == pbuf.tobytes(), "the weight allocation was written"


def run_case(oracle, c):
    what = "seed %d" % c["seed"]
    model = WC.CaseModel(oracle, c)
    m = model.m
    gv = tsdf_amd.TSDFVolume(c["dims"], c["phys"])
    slabs = [tsdf_amd.TSDFVolume(c["dims"], c["phys"], slab=s) for s in (c["slabs"] or ())]
    volumes = [gv] + slabs
    kind, dist, weight = c["prior"]
    for v in volumes:
        if c["offset"] is not None:
            v.offset(*c["offset"])
            v.clear()
        if kind == "storage16":
            v.set_weight_storage(16)
        if kind == "pinned":
            assert v.weight_data() and v.weight_storage() == (32, True)
        v.set_weight_cap(c["cap"])
    if c["nodes"] is not None:
        gv.set_deformation(np.concatenate([c["nodes"], np.zeros_like(c["nodes"])], axis=1))
    if dist is not None:
        gv.set_distance_data(dist)
        gv.set_weight_data(weight)
    if kind in ("counts8", "counts16", "storage16", "fp32"):
        assert gv.weight_storage()[0] == {"counts8": 8, "counts16": 16, "storage16": 16, "fp32": 32}[kind], what + ": the storage the prior state asks for"
    if c["colour"]:
        gv.enable_colour()
    gv.set_counting(c["counting"])
    assert F32(gv.truncation_distance()) == m.trunc()
    cams, worked, sizes = [], 0, []
    try:
        for i, op in enumerate(c["ops"]):
            step = "%s, op %d (%s %dx%d)" % (what, i, op[0], op[-2], op[-1])
            cam, (w, h) = Cam(*op[-3]), op[-2:]
            keep = [a.copy() for a in op[1:4] if isinstance(a, np.ndarray)]
            if op[0] == "weighted":
                if c["device"]:
                    _device_call(gv, op)
                    _SEEN["grown"] += int(bool(sizes) and w * h > max(sizes))
                    sizes.append(w * h)
                else:
                    gv.integrate_weighted(op[1], op[2], w, h, cam, rgb=op[3])
                for s in slabs:
                    s.integrate_weighted(op[1], op[2], w, h, cam)
            elif op[0] == "plain":
                for v in volumes:
                    v.integrate(op[1], w, h, cam)
            else:
                for v in volumes:
                    v.deintegrate(op[1], w, h, cam)
            for a, b in zip(keep, [a for a in op[1:4] if isinstance(a, np.ndarray)]):
                assert a.tobytes() == b.tobytes(), step + ": the caller's arrays were written"
            updated, stores = model.apply(op)
            worked += updated
            assert_same_floats(gv.get_weight_data(), m.weight, step + ": weights")
            assert_same_floats(gv.get_distance_data(), m.dist, step + ": distances")
            if c["colour"]:
                _same_words(gv.get_colour_data(), m.colour, step)
            if op[0] == "weighted":
                if c["counting"]:
                    assert gv.last_updated_voxels() == updated, step + ": updated voxels"
                    assert gv.last_distance_stores() == stores, step + ": distance stores"
                assert gv.weight_storage() == (32, kind == "pinned"), step + ": weight storage"
                cams.append((cam, w, h))
        # the pictures of the last two cameras
        for cam, w, h in cams[-2:]:
            V, N = gv.raycast(w, h, cam)
            Vo, No = m.raycast(cam, w, h)
            assert_same_floats(V, Vo, what + ": vertices")
            assert_same_floats(N, No, what + ": normals")
            _SEEN["casts"] += 1
            _SEEN["casts_hit"] += int((~np.isnan(Vo[:, 0])).sum() >= 50)
        # the brick flags: lazy at least their definition, rebuilt equal to it
        fine, cell, reach = m.flags()
        lazy = gv.occupancy_data()
        assert np.all(lazy[0] >= fine) and np.all(lazy[1] >= cell), what + ": lazy flags below their definition"
        rebuilt = gv.occupancy_data(force_rebuild=True)
        assert np.array_equal(rebuilt[0], fine) and np.array_equal(rebuilt[1], cell), what + ": rebuilt flags"
        assert np.array_equal(rebuilt[2], reach), what + ": reach"
        assert np.all(lazy[0] >= rebuilt[0]) and np.all(lazy[1] >= rebuilt[1]), what + ": lazy flags below the rebuilt ones"
        if slabs:
            X, Y, Z = c["dims"]
            parts_d, parts_w = [], []
            for s, (lo, hi) in zip(slabs, c["slabs"]):
                a = s.info().z_store_begin
                planes = s.info().z_store_end - a
                parts_d.append(s.get_distance_data().reshape(planes, -1)[lo - a:hi - a])
                parts_w.append(s.get_weight_data().reshape(planes, -1)[lo - a:hi - a])
            assert_same_floats(np.concatenate(parts_d), m.dist.reshape(Z, -1), what + ": two slabs, distances")
            assert_same_floats(np.concatenate(parts_w), m.weight.reshape(Z, -1), what + ": two slabs, weights")
    finally:
        for v in volumes:
            v.close()
    _SEEN["cases"] += 1
    _SEEN["worked"] += int(worked >= 16)
    _SEEN["device"] += int(c["device"])


@pytest.mark.parametrize("seed", WC.SEEDS)
def test_a_weighted_case_leaves_the_references_state(oracle, seed):
    c = WC.case(seed)
    try:
        run_case(oracle, c)
    except AssertionError as e:
        raise AssertionError("%s\n%s" % (e, WC.describe(c))) from e


def test_the_weighted_cases_were_not_vacuous():
    """The achieved counts of tests/test_weighted_fuzz_host.py, section 4 of its docstring, as the GPU run met them."""
    if _SEEN["cases"] < len(WC.SEEDS):
        pytest.skip("needs the whole sweep")
    print("\nweighted cases: %s" % _SEEN)
    assert _SEEN["worked"] >= 0.9 * _SEEN["cases"], _SEEN
    assert _SEEN["casts_hit"] >= 0.6 * _SEEN["casts"], _SEEN
    assert _SEEN["device"] == len(WC.SEEDS) // 4 and _SEEN["grown"] >= _SEEN["device"], _SEEN


# ---- weighted frames among the other writers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(WS.N))
def test_a_sequence_with_weighted_frames_leaves_the_models_state(oracle, i):
    base, ops = WS.sequence(i)
    drive(oracle, base, ops=ops)
    _SEEN["sequences"] += 1


# ---- the weight models --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("general", [False, True], ids=["standard", "general"])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("width,height", WC.MODEL_SIZES)
def test_depth_weights_at_small_and_odd_sizes(width, height, flags, general):
    """depth_weights_kernel on images narrower than a wave, lower than a workgroup and smaller than 3 x 3, with 65535 and 1 in them."""
    import torch
    d, kinv, z_ref = WC.model_depth(width, height), WC.model_kinv(general), WC.MODEL_Z_REF
    n = width * height
    want = R.depth_weights(d, width, height, kinv, flags, z_ref)
    dd = torch.from_numpy(d.view(np.int16).copy()).cuda()
    out = torch.full((n + 4,), float(GUARD32), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tsdf_amd.depth_weights_device(width, height, dd.data_ptr(), kinv, flags, z_ref, out.data_ptr() + 8)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[:2] == GUARD32) and np.all(got[-2:] == GUARD32), "written outside the image"
    assert_same_floats(got[2:-2], want, "depth_weights_device %dx%d flags %d" % (width, height, flags))
    assert np.array_equal(dd.cpu().numpy().view(np.uint16), d), "the caller's depth image was written"
    keep = d.copy()
    assert_same_floats(tsdf_amd.depth_weights(d, width, height, kinv, flags, z_ref), want, "depth_weights (host) %dx%d flags %d" % (width, height, flags))
    assert np.array_equal(d, keep)


# ---- the tracker on a colour volume ---------------------------------------------------------------------------------------------------------
def test_the_tracker_integrates_rgb_frames_with_the_models_weights():
    """tests/test_weighted.py's tracker test with colour, at 64^3 (its non-vacuity asserts hold there: 262 144 voxels, of which the
    six frames weight far more than 10 000)."""
    import torch
    from tsdf_amd.tracking import FrameToModelTracker
    n, phys, seed, period = (64,) * 3, (3000.0,) * 3, 0x5EED0C02, 200
    flags, z_ref = tsdf_amd.WEIGHTS_INVERSE_SQUARE | tsdf_amd.WEIGHTS_COSINE, 2400.0
    gv, tv = tsdf_amd.TSDFVolume(n, phys), tsdf_amd.TSDFVolume(n, phys)
    gv.enable_colour()
    tv.enable_colour()
    trk = FrameToModelTracker(gv, W, H, weighting=(flags, z_ref))
    weights = torch.empty(W * H, dtype=torch.float32, device="cuda")
    for i in range(6):
        d, cam = synth.depth_frame(i, period, seed=seed, noise=False)
        rgb, _ = synth.colour_frame(i, period, seed=seed)
        trk.process(d, initial_pose=cam.pose().astype(np.float64).reshape(4, 4).T if i == 0 else None, rgb=rgb)
        _, filtered = trk.last_icp_inputs()
        used = Cam(trk.camera.pose(), trk.camera.inverse_pose(), trk.camera.k(), trk.camera.kinv())
        fd = torch.from_numpy(filtered.view(np.int16).copy()).cuda()
        fc = torch.from_numpy(np.ascontiguousarray(rgb, np.uint8).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        tsdf_amd.depth_weights_device(W, H, fd.data_ptr(), used.kinv(), flags, z_ref, weights.data_ptr())
        torch.cuda.synchronize()
        tv.integrate_weighted_device(fd.data_ptr(), weights.data_ptr(), W, H, used, rgb_ptr=fc.data_ptr())
        tv.synchronize()
    trk.synchronize()
    assert gv.weight_storage() == (32, False)
    got = gv.get_weight_data()
    assert (got > 0).sum() > 10000 and np.any((got > 0) & (got != np.round(got)))
    assert_same_floats(got, tv.get_weight_data(), "tracker vs the calls by hand: weights")
    assert_same_floats(gv.get_distance_data(), tv.get_distance_data(), "tracker vs the calls by hand: distances")
    words = gv.get_colour_data()
    assert int((words >> 24).max()) >= 2 and (words != 0).sum() > 1000
    _same_words(words, tv.get_colour_data(), "tracker vs the calls by hand")
    trk.close()
