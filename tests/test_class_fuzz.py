"""GPU: class fusion against its CPU reference where kernels go wrong (include/tsdf_amd.h, "class fusion"; tsdf_amd/csrc/classes.hip).

The class update is band_pass_kernel<STD, ClassVote> (tsdf_amd/csrc/band_pass.hpp), an instantiation of its own of the walk colour
takes: brick walk, camera split, rounding guard band, frustum test, depth read, band test and appended-z-chunk bound, then the vote
of ClassVote.  tests/test_class_fusion.py holds it to the reference at 640 x 480 on
two 3000 mm cubes seen from outside; here it meets what colour (tests/test_colour_parity.py) and weighted integration
(tests/test_weighted_fuzz.py) are held to.

  * one test per seed of tests/class_cases.py (aimed rows first, then 36 drawn): a class volume, a plain twin, the oracle, the
    reference words and, with rgb, a colour twin in lockstep.  After every frame: class words against tests/classes_ref.py word for
    word from the same start words, distances and weights against the twin and the oracle, occupancy against the twin, colour words
    against the colour twin, the caller's arrays unchanged.  At the end: sample_classes at random, off-grid, NaN / inf / 1e30 and
    cell-face points with each face's nextafter neighbours; class_counts at 301 (LDS) and 65535 (global atomics) classes and min_votes 1
    and 3; find_objects at connectivity 6 and 26 against tests/objects_ref.py on the reference words; where the case says so the classed
    ray cast (the twin's cast plus sampling) and the classed surface.  Every fourth drawn seed calls integrate_classes_device on arrays
    inside larger allocations: depth and classes at an odd uint16 offset, confidence and rgb at an odd byte offset, guard words round
    each, every allocation byte-equal afterwards, every image larger than the one before;
  * the twelve sequences of tests/class_sequences.py through tests/test_op_sequences.drive;
  * class_counts (both kernel paths, into a poisoned buffer with a guard word) and sample_classes (offset baked at clear, then moved) on
    the small grids of tests/test_objects.py: one voxel, fewer than 256 voxels, 63 / 64 / 65 voxels modulo 64.

Every comparison is equality of integers or bytes.  tests/test_class_fuzz_host.py shows, without a GPU, that the cases reach what they
are aimed at.

Cost on an MI355X host, oracle work included, each figure from a pytest process of its own: the whole file (74 tests) 5.69 s; the
twelve sequences alone 0.98 s (0.02 - 0.30 s each, the first pays the start of the context); the slowest single test 0.31 s (seeds 28 and
34, the drawn grids of 200 000 voxels and more with start words, where tests/objects_ref.py builds thousands of rows in Python), every
other case 0.02 - 0.27 s.  The parent commit's tests/test_class_fusion.py on the same machine in the same visit: 6.33 s for 29 tests,
its slowest (the 256^3 physical check) 2.63 s.  No torch is imported here: the device variants and the prepared brick list use
tsdf_device_alloc.
"""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import class_cases as CC
from tests import class_sequences as CS
from tests import classes_ref as R
from tests import objects_ref as OR
from tests.helpers import Cam, assert_same_floats
from tests.test_class_fusion import counts_into_poison
from tests.test_colour_parity import set_trunc
from tests.test_objects import GRIDS as SMALL_GRIDS
from tests.test_op_sequences import drive
from tsdf_amd import _capi

pytestmark = pytest.mark.gpu

F32, U16, U32 = np.float32, np.uint16, np.uint32
VOID = tsdf_amd.CLASS_VOID
GUARD16, GUARD8 = 0xBEEF, 0xA5
_SEEN = {"cases": 0, "voted": 0, "general": 0, "device": 0, "grown": 0, "device_rgb": 0, "casts": 0, "casts_hit": 0, "surfaces": 0,
         "objects": 0, "sequences": 0}


class DeviceArray:
    """A device allocation holding a copy of `host` (tests/test_explore.py's helper)."""

    def __init__(self, host):
        self.host = host
        self.p = C.c_void_p()
        _capi.check(_capi.lib.tsdf_device_alloc(max(host.nbytes, 4), C.byref(self.p)))
        _capi.check(_capi.lib.tsdf_device_upload(self.p, host.ctypes.data, host.nbytes))

    def unchanged(self):
        out = np.empty_like(self.host)
        _capi.check(_capi.lib.tsdf_device_download(out.ctypes.data, self.p, out.nbytes))
        return out.tobytes() == self.host.tobytes()

    def free(self):
        _capi.lib.tsdf_device_free(self.p)


def _placed(values, dtype, lead, guard):
    """`values` inside a larger array of guard words, `lead` elements in (and as many behind): -> (DeviceArray, device pointer)."""
    v = np.ascontiguousarray(values, dtype).reshape(-1)
    buf = np.full(v.size + 2 * lead, guard, dtype)
    buf[lead:lead + v.size] = v
    a = DeviceArray(buf)
    assert a.p.value % 4 == 0
    return a, a.p.value + lead * buf.itemsize


def _device_call(gv, f):
    """integrate_classes_device: depth and classes 5 uint16 into their allocations (2 bytes off a 4-byte boundary), confidence and rgb
    7 bytes into theirs.  Returns after the stream has drained, with every allocation checked byte for byte."""
    d, pd = _placed(f["depth"], U16, 5, GUARD16)
    k, pk = _placed(f["classes"], U16, 5, GUARD16)
    held = [d, k]
    ps = pc = None
    if f["confidence"] is not None:
        s, ps = _placed(f["confidence"], np.uint8, 7, GUARD8)
        held.append(s)
    if f["rgb"] is not None:
        c, pc = _placed(f["rgb"], np.uint8, 7, GUARD8)
        held.append(c)
    assert pd % 4 == 2 and pk % 4 == 2 and (ps is None or ps % 2 == 1) and (pc is None or pc % 2 == 1)
    try:
        gv.integrate_classes_device(pd, pk, f["width"], f["height"], Cam(*f["cam"]), confidence_ptr=ps, rgb_ptr=pc)
        gv.synchronize()
        for a, name in zip(held, ("depth", "classes") + (("confidence",) if ps else ()) + (("rgb",) if pc else ())):
            assert a.unchanged(), "the %s allocation was written" % name
    finally:
        for a in held:
            a.free()


def _same_words(got, want, what):
    bad = np.flatnonzero(got != want)
    assert not bad.size, "%s: %d words differ, first at %d: %08x vs %08x" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _volume(c):
    v = tsdf_amd.TSDFVolume(c["dims"], c["phys"])
    if c["bake"] is not None:
        v.offset(*c["bake"])
    if c["trunc"] is not None:
        set_trunc(v, c["trunc"])
    if c["bake"] is not None or c["trunc"] is not None:
        v.clear()
    if c["move"] is not None:
        v.offset(*c["move"])
    return v


def check_queries(gv, words, geom, rng, what, n_points=4000):
    """sample_classes and class_counts of a volume whose words are `words`."""
    pts = CC.sampling_points(rng, geom, n_points)
    got_c, got_n = gv.sample_classes(pts)
    want_c, want_n = R.sample(words, geom, pts)
    bad = np.flatnonzero((got_c != want_c) | (got_n != want_n))
    assert not bad.size, "%s: %d samples differ, first at %r: (%d, %d) vs (%d, %d)" % (what, bad.size, pts[bad[0]], got_c[bad[0]], got_n[bad[0]],
                                                                                     want_c[bad[0]], want_n[bad[0]])
    assert np.all(got_c[-7:] == VOID) and not got_n[-7:].any(), what + ": NaN, inf and 1e30 points"
    for n_classes in (301, 65535):
        for min_votes in (1, 3):
            assert np.array_equal(gv.class_counts(n_classes, min_votes), R.counts(words, n_classes, min_votes)), "%s: counts %d / %d" % (what, n_classes, min_votes)


def check_objects(gv, ob, words, dims, what):
    min_size = 1 if len(words) <= 100000 else 3          # (the reference builds a row per listed object in Python)
    for connectivity in (6, 26):
        ids, L, rows, n_objects = OR.find(words, dims, 1, None, connectivity, min_size)
        gv.find_objects(1, None, connectivity, min_size, into=ob)
        where = "%s: objects at %d" % (what, connectivity)
        i = ob.info
        assert (i.n_labelled, i.n_objects, i.n_listed_objects) == (len(ids), n_objects, len(rows)), where
        assert np.array_equal(ob.voxels, ids) and np.array_equal(ob.labels, L), where
        assert ob.objects.tobytes() == rows.tobytes(), where
        _SEEN["objects"] += int(len(rows) > 0)


def run_case(oracle, c):
    what = "seed %d" % c["seed"]
    ref = CC.Reference(oracle, c)
    gv, tv = _volume(c), _volume(c)
    ctv = _volume(c) if c["colour"] else None
    volumes = [v for v in (gv, tv, ctv) if v is not None]
    ob = tsdf_amd.Objects()
    try:
        gv.enable_classes()
        if c["colour"]:
            gv.enable_colour()
            ctv.enable_colour()
        if c["start"] is not None:
            gv.set_class_data(c["start"])
        geom = R.geometry(gv)
        assert geom[0] == ref.geom[0] and all(np.array_equal(a, b) for a, b in zip(geom[1:], ref.geom[1:])), what + ": geometry"
        if c["bake"] is not None:
            assert np.any(geom[3] != 0) and np.any(geom[2] != geom[3]), what + ": offset != offset_at_clear"
        cast_votes, sizes = 0, []
        for i, f in enumerate(c["frames"]):
            step = "%s, frame %d (%dx%d)" % (what, i, f["width"], f["height"])
            cam, w, h = Cam(*f["cam"]), f["width"], f["height"]
            keep = {k: f[k].copy() for k in ("depth", "classes", "confidence", "rgb") if f[k] is not None}
            if c["device"]:
                _device_call(gv, f)
                _SEEN["grown"] += int(bool(sizes) and w * h > max(sizes))
                _SEEN["device_rgb"] += int(f["rgb"] is not None)
                sizes.append(w * h)
            else:
                gv.integrate_classes(f["depth"], f["classes"], w, h, cam, confidence=f["confidence"], rgb=f["rgb"])
            tv.integrate(f["depth"], w, h, cam)
            if ctv is not None:
                ctv.integrate_colour(f["depth"], f["rgb"], w, h, cam)
            for k, a in keep.items():
                assert a.tobytes() == f[k].tobytes(), step + ": the caller's %s was written" % k
            r = ref.apply(f)
            cast_votes += int((r["outcome"] != 0).sum())
            _same_words(gv.get_class_data(), ref.words, step + ": class words")
            gw, gd = gv.get_weight_data(), gv.get_distance_data()
            assert_same_floats(gw, tv.get_weight_data(), step + ": weights vs twin")
            assert_same_floats(gd, tv.get_distance_data(), step + ": distances vs twin")
            assert_same_floats(gw, ref.ov.weight, step + ": weights vs oracle")
            assert_same_floats(gd, ref.ov.dist, step + ": distances vs oracle")
            for a, b, name in zip(gv.occupancy_data(), tv.occupancy_data(), ("fine", "cell", "reach")):
                assert np.array_equal(a, b), "%s: occupancy %s vs twin" % (step, name)
            if ctv is not None:
                _same_words(gv.get_colour_data(), ctv.get_colour_data(), step + ": colour words vs the colour twin")
                assert_same_floats(gd, ctv.get_distance_data(), step + ": distances vs the colour twin")
        rng = np.random.default_rng(c["seed"])
        check_queries(gv, ref.words, geom, rng, what)
        check_objects(gv, ob, ref.words, c["dims"], what)
        f = c["frames"][-1]
        cam, w, h = Cam(*f["cam"]), f["width"], f["height"]
        if c["cast"]:
            V, N = tv.raycast(w, h, cam)
            Vc, Nc, classes, votes = tsdf_amd.GPURaycaster(w, h).raycast_classes(gv, cam)
            assert_same_floats(Vc, V, what + ": classed cast vertices")
            assert_same_floats(Nc, N, what + ": classed cast normals")
            want_c, want_n = R.sample(ref.words, geom, V)
            assert np.array_equal(classes, want_c) and np.array_equal(votes, want_n), what + ": cast classes vs reference"
            miss = np.isnan(V[:, 0])
            assert np.all(classes[miss] == VOID) and not votes[miss].any(), what + ": misses"
            _SEEN["casts"] += 1
            _SEEN["casts_hit"] += int((~miss).any())
        if c["surface"]:
            S, sc = gv.extract_classed_surface()
            assert_same_floats(S, tv.extract_surface(), what + ": classed surface vertices")
            assert np.array_equal(sc, R.sample(ref.words, geom, S)[0]), what + ": surface classes"
            _SEEN["surfaces"] += int(len(S) > 0)
    finally:
        ob.close()
        for v in volumes:
            v.close()
    _SEEN["cases"] += 1
    if not c["aimed"]:
        _SEEN["voted"] += int(cast_votes > 0)
        _SEEN["general"] += int(cast_votes > 0 and c["kind"] is not None)
        _SEEN["device"] += int(c["device"])


@pytest.mark.parametrize("seed", CC.SEEDS)
def test_a_class_case_leaves_the_references_words(oracle, seed):
    c = CC.case(seed)
    try:
        run_case(oracle, c)
    except AssertionError as e:
        raise AssertionError("%s\n%s" % (e, CC.describe(c))) from e


def test_the_class_cases_were_not_vacuous():
    """The conditions of tests/test_class_fuzz_host.py as the GPU run met them."""
    if _SEEN["cases"] < len(CC.SEEDS):
        pytest.skip("needs the whole sweep")
    print("\nclass cases: %s" % _SEEN)
    assert _SEEN["voted"] >= 30 and _SEEN["general"] >= 4, _SEEN
    assert _SEEN["device"] == CC.N_DRAWN // 4 and _SEEN["grown"] >= _SEEN["device"] and _SEEN["device_rgb"] >= 4, _SEEN
    assert _SEEN["casts_hit"] >= 0.5 * _SEEN["casts"] and _SEEN["surfaces"] >= 3 and _SEEN["objects"] >= len(CC.SEEDS), _SEEN


# ---- class frames among the other writers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(CS.N))
def test_a_sequence_with_class_frames_leaves_the_models_state(oracle, i):
    base, ops = CS.sequence(i)
    drive(oracle, base, ops=ops)
    _SEEN["sequences"] += 1


# ---- counts and sampling on the small grids ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SMALL_GRIDS)
def test_counts_and_sampling_on_a_small_grid(size):
    """The grids of tests/test_objects.py -- one voxel (grid = 1, one lane), 455 voxels (a partial last wave), 384, 780, 1170 and 6633
    voxels (0, 12, 18 and 41 modulo 64, two to 26 workgroups) -- and, beside the one-voxel grid, single rows of 63, 64, 65, 127, 129, 255,
    257, 319 and 321 voxels: 63, 0 and 1 modulo 64 below one workgroup and just above it, where the ballot loop of the path without LDS
    needs every lane of a wave to make the same trips.  Random words with class bits under zero votes; counts on both kernel paths into a
    poisoned buffer with a guard word; sampling with an offset baked at clear and then moved."""
    rng = np.random.default_rng(size[0] * 1000 + size[2])
    grids = [size] + [(x, 1, 1) for x in (63, 64, 65, 127, 129, 255, 257, 319, 321) if size == (1, 1, 1)]
    for dims in grids:
        gv = tsdf_amd.TSDFVolume(dims, (dims[0] * 10.0, dims[1] * 12.5, dims[2] * 9.0))
        gv.offset(100.0, -50.0, 25.0)
        gv.clear()
        gv.offset(-7.5, 3.25, 11.0)
        gv.enable_classes()
        n = gv.resident_voxels()
        words = CC.start_words(rng, n)
        gv.set_class_data(words)
        geom = R.geometry(gv)
        assert np.any(geom[3] != 0) and np.any(geom[2] != geom[3])
        what = "grid %s" % (dims,)
        check_queries(gv, words, geom, rng, what, n_points=800)
        for n_classes in (1, 3, 301, 4096, 4097, 65535):
            for min_votes in (0, 1, 3, 65535):
                want = R.counts(words, n_classes, min_votes)
                assert np.array_equal(counts_into_poison(gv, n_classes, min_votes), want), "%s: counts %d / %d" % (what, n_classes, min_votes)
        assert int(gv.class_counts(65535).sum()) == int(((words >> U32(16)) != 0).sum())
        gv.close()
