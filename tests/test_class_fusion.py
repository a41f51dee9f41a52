"""Class fusion on the GPU (include/tsdf_amd.h, "class fusion"; tsdf_amd/csrc/classes.hip).

  * class integrate leaves distances, weights and occupancy exactly as plain integrate does (twin volume + the CPU oracle), in every
    weight storage, at 64^3 and at an odd grid with partial bricks in x and y and a short last z chunk;
  * the class words are bit-equal to the CPU reference (tests/classes_ref.py: numpy over the oracle's pinned transforms) -- a stream,
    dropouts with random classes, VOID and confidence, off-axis intrinsics (the general-camera instantiation), preset edge words;
  * an image that says nothing (all VOID, all-zero confidence) leaves every word alone; rgb beside classes gives integrate_colour's
    colour words and the same class words;
  * sampling, the classed ray cast, the classed surface and Mesh.sample_classes are the sampling rule applied to their vertices;
  * class_counts is np.bincount over the downloaded words, on both kernel paths;
  * physically: fused classes seen from a new pose are the analytic classes;
  * clear(), enable / disable, and the refusals.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import tsdf_amd
from tests import classes_ref as R
from tests import colour_ref
from tests.helpers import H, W, Cam, assert_same_floats, camera_at
from tsdf_amd import _capi, synth

pytestmark = pytest.mark.gpu
SEED = 0x5EED0003            # bench.py's stream
VOID = tsdf_amd.CLASS_VOID
ODD = (70, 37, 45)           # two bricks in x (64 + 6), ten in y (9 x 4 + 1), a z chunk of 32 and a short one of 13
GRIDS = [(64, 64, 64), ODD]
PHYS = (3000.0,) * 3


@functools.lru_cache(maxsize=None)
def stream(n_frames, period=200):
    """(depth, classes, camera) of the first frames of bench.py's trajectory, with their class frames."""
    out = []
    for i in range(n_frames):
        d, cam = synth.depth_frame(i, period, seed=SEED)
        k, _ = synth.class_frame(i, period, seed=SEED)
        out.append((d, k, cam))
    return tuple(out)


def classed_volume(dims, colour=False):
    gv = tsdf_amd.TSDFVolume(tuple(dims), PHYS)
    gv.enable_classes()
    if colour:
        gv.enable_colour()
    return gv


def set_storage(volumes, mode):
    """The three weight storages, as tests/test_colour_fusion.py reaches them."""
    if mode == 16:
        w = np.zeros(volumes[0].resident_voxels(), np.float32)
        w[0] = 300.0                                        # (the grid's corner voxel: behind the camera of every frame here)
        for v in volumes:
            v.set_weight_data(w)
    elif mode == 32:
        for v in volumes:
            if hasattr(v, "weight_storage"):
                assert v.weight_data()


def off_axis_camera():
    """The skewed, off-centre K of tests/test_colour_fusion.py::test_colour_words_with_off_axis_intrinsics."""
    base = camera_at((1400, 1550, -900), look_at=(1500, 1500, 1500))
    k = np.array([[560.0, 3.0, 300.5], [0.0, 575.0, 251.25], [0.0, 0.0, 1.0]], np.float32)
    kinv = np.linalg.inv(k.astype(np.float64)).astype(np.float32)
    return Cam(base.pose(), base.inverse_pose(), k.T.reshape(-1), kinv.T.reshape(-1))


def noise_frame(seed, ids=5):
    """Random classes from `ids` ids with about 10 % VOID, random confidence 0..255."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, ids, W * H).astype(np.uint16)
    k[rng.random(W * H) < 0.1] = VOID
    return k, rng.integers(0, 256, W * H, dtype=np.uint8)


def check_words(oracle, gv, frames, start=None):
    """frames: (depth, classes, confidence or None, camera).  The GPU's words after all of them against the reference's."""
    want = np.zeros(gv.resident_voxels(), np.uint32) if start is None else start
    geom = R.geometry(gv)
    voted_any = np.zeros(gv.resident_voxels(), bool)
    for d, k, s, cam in frames:
        gv.integrate_classes(d, k, W, H, cam, confidence=s)
        want, _, voted = R.integrate_classes(oracle, want, geom, d, k, s, W, H, cam)
        voted_any |= voted
    got = gv.get_class_data()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%d class words differ, first at %d: %08x vs %08x" % (bad.size, bad[0], got[bad[0]], want[bad[0]])
    assert not np.any(((got >> 16) == 0) & (got != 0))
    return got, voted_any


@pytest.mark.parametrize("mode", [8, 16, 32])
@pytest.mark.parametrize("dims", GRIDS)
def test_class_integrate_leaves_the_distance_update_alone(oracle, dims, mode):
    """6 frames: distances, weights and occupancy flags of integrate_classes are the twin's (plain integrate) and the oracle's."""
    gv, tv = classed_volume(dims), tsdf_amd.TSDFVolume(dims, PHYS)
    ov = oracle.Volume(dims, PHYS)
    set_storage((gv, tv, ov), mode)
    assert gv.weight_storage()[0] == tv.weight_storage()[0] == mode
    for i, (d, k, cam) in enumerate(stream(6)):
        gv.integrate_classes(d, k, W, H, cam, confidence=noise_frame(i)[1] if i % 2 else None)
        tv.integrate(d, W, H, cam)
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    assert gv.weight_storage()[0] == mode
    for got, twin, ref, what in ((gv.get_distance_data(), tv.get_distance_data(), ov.dist, "distances"),
                                 (gv.get_weight_data(), tv.get_weight_data(), ov.weight, "weights")):
        assert_same_floats(got, twin, "%s %d-bit: %s vs twin" % (dims, mode, what))
        assert_same_floats(got, ref, "%s %d-bit: %s vs oracle" % (dims, mode, what))
    for a, b, what in zip(gv.occupancy_data(), tv.occupancy_data(), ("fine", "cell", "reach")):
        assert np.array_equal(a, b), "%s %d-bit: occupancy %s" % (dims, mode, what)
    assert int((gv.get_class_data() != 0).sum()) > 1000


@pytest.mark.parametrize("dims", GRIDS)
def test_class_words_equal_the_cpu_reference_over_a_stream(oracle, dims):
    got, _ = check_words(oracle, classed_volume(dims), [(d, k, None, cam) for d, k, cam in stream(8)])
    assert int(((got >> 16) == 8).sum()) > 100
    assert {1, 2, 3} <= set(np.unique(got[got != 0] & 0xFFFF).tolist())


@pytest.mark.parametrize("dims", GRIDS)
def test_class_words_with_dropouts_void_and_confidence(oracle, dims):
    cam = camera_at((1500, 1500, -1000))
    frames = [(synth.config1_depth(), *noise_frame(1), cam), (synth.config1_depth(2), *noise_frame(2), cam)]
    got, voted = check_words(oracle, classed_volume(dims), frames)
    assert int((got != 0).sum()) > 1000
    assert int((voted & (got == 0)).sum()) > 10            # VOID pixels, zero strengths and ties leave unclassified words in the band


@pytest.mark.parametrize("dims", GRIDS)
def test_class_words_with_off_axis_intrinsics(oracle, dims):
    """A skewed, off-centre K: the general-camera instantiations of integrate and of the class kernel."""
    cam = off_axis_camera()
    frames = [(synth.config1_depth(3), *noise_frame(3), cam), (synth.wall_depth(2300), noise_frame(4)[0], None, cam)]
    got, _ = check_words(oracle, classed_volume(dims), frames)
    assert int((got != 0).sum()) > 1000


@pytest.mark.parametrize("old, k, s, new", [
    (R.word(4, 65535), 4, 255, R.word(4, 65535)),          # saturated, the same class again: stays saturated
    (R.word(4, 65500), 4, 255, R.word(4, 65535)),          # ... and gets there
    (R.word(9, 7), 4, 7, 0),                                # (c, s) against (k, s): the unclassified word
    (R.word(9, 1), 4, 255, R.word(4, 254)),                # (c, 1) against strength 255
    (R.word(9, 300), 4, 255, R.word(9, 45)),               # the candidate survives
    (0, 0, 1, R.word(0, 1)),                                # class 0 on an unclassified word
])
def test_edge_words(oracle, old, k, s, new):
    gv = classed_volume(ODD)
    start = np.full(gv.resident_voxels(), old, np.uint32)
    gv.set_class_data(start)
    d, _, cam = stream(1)[0]
    frame = (d, np.full(W * H, k, np.uint16), np.full(W * H, s, np.uint8), cam)
    got, voted = check_words(oracle, gv, [frame], start=start)
    assert voted.sum() > 500
    assert np.all(got[voted] == np.uint32(new)) and np.all(got[~voted] == np.uint32(old))


def test_an_image_that_says_nothing_leaves_every_word_alone():
    rng = np.random.default_rng(21)
    for dims in GRIDS:
        gv, tv = classed_volume(dims), tsdf_amd.TSDFVolume(dims, PHYS)
        words = rng.integers(0, 5, gv.resident_voxels()).astype(np.uint32) | (rng.integers(1, 9, gv.resident_voxels()).astype(np.uint32) << 16)
        words[rng.random(words.size) < 0.3] = 0
        gv.set_class_data(words)
        (d0, k0, cam0), (d1, _, cam1) = stream(2)
        gv.integrate_classes(d0, np.full(W * H, VOID, np.uint16), W, H, cam0, confidence=np.full(W * H, 200, np.uint8))
        gv.integrate_classes(d1, k0, W, H, cam1, confidence=np.zeros(W * H, np.uint8))
        assert np.array_equal(gv.get_class_data(), words)
        tv.integrate(d0, W, H, cam0)
        tv.integrate(d1, W, H, cam1)
        assert_same_floats(gv.get_distance_data(), tv.get_distance_data(), "distances")
        assert_same_floats(gv.get_weight_data(), tv.get_weight_data(), "weights")
        assert int((gv.get_weight_data() > 0).sum()) > 1000


@pytest.mark.parametrize("mode", [8, 32])
def test_rgb_beside_classes(mode):
    """Colour words are integrate_colour's on a twin (the packed kernel's own colour update at 8 bits, the colour pass at fp32), class
    words those of the call without rgb, distances and weights the twins'."""
    for dims in GRIDS:
        both, ctwin, ktwin = classed_volume(dims, colour=True), tsdf_amd.TSDFVolume(dims, PHYS), classed_volume(dims)
        ctwin.enable_colour()
        set_storage((both, ctwin, ktwin), mode)
        for i, (d, k, cam) in enumerate(stream(4)):
            rgb, _ = synth.colour_frame(i, 200, seed=SEED)
            s = noise_frame(40 + i)[1] if i % 2 else None
            both.integrate_classes(d, k, W, H, cam, confidence=s, rgb=rgb)
            ctwin.integrate_colour(d, rgb, W, H, cam)
            ktwin.integrate_classes(d, k, W, H, cam, confidence=s)
        assert both.weight_storage()[0] == mode
        assert np.array_equal(both.get_colour_data(), ctwin.get_colour_data())
        assert np.array_equal(both.get_class_data(), ktwin.get_class_data())
        assert int((both.get_colour_data() >> 24).astype(bool).sum()) > 1000 and int((both.get_class_data() != 0).sum()) > 1000
        for other in (ctwin, ktwin):
            assert_same_floats(both.get_distance_data(), other.get_distance_data(), "distances")
            assert_same_floats(both.get_weight_data(), other.get_weight_data(), "weights")


def random_words(rng, n, ids=65535, unclassified=0.2):
    words = rng.integers(0, ids, n).astype(np.uint32) | (rng.integers(1, 65536, n).astype(np.uint32) << 16)
    words[rng.random(n) < unclassified] = 0
    return words


@pytest.mark.parametrize("dims", GRIDS)
def test_sample_classes_equals_numpy(dims):
    gv = classed_volume(dims)
    rng = np.random.default_rng(7)
    words = random_words(rng, gv.resident_voxels())
    gv.set_class_data(words)
    geom = R.geometry(gv)
    vs = np.array(gv.voxel_size(), np.float32)
    centres = colour_ref.voxel_centres(*geom[:4])
    faces = (rng.integers(0, np.array(dims) + 1, size=(20000, 3)) * vs).astype(np.float32)      # on voxel faces, grid faces included
    faces[:, 1] += np.float32(0.5) * vs[1]
    pts = rng.uniform(-100.0, 3100.0, size=(50000, 3)).astype(np.float32)
    special = np.array([[np.nan, 5, 5], [5, np.nan, 5], [5, 5, np.nan], [-1e-3, 10, 10], [3000.0, 10, 10], [0, 0, 0],
                        [vs[0], vs[1], vs[2]], [2999.99, 2999.99, 2999.99], [1e30, 0, 0], [-1e30, 0, 0], [np.inf, 1, 1]], np.float32)
    pts = np.concatenate([centres, faces, pts, special])
    for offset in (None, (11.5, -7.25, 3.0)):               # the rule reads offset and offset_at_clear
        if offset:
            gv.offset(*offset)
        got_c, got_n = gv.sample_classes(pts)
        want_c, want_n = R.sample(words, R.geometry(gv), pts)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_n, want_n)
        assert np.all(got_c[-11:-8] == VOID) and np.all(got_n[-11:-8] == 0) and np.all(got_c[-3:] == VOID)
        assert np.all((got_n == 0) == (got_c == VOID))
    got_c, got_n = classed_volume(dims).sample_classes(np.zeros((0, 3), np.float32))
    assert got_c.shape == (0,) and got_n.shape == (0,)


def test_classed_cast_surface_and_mesh_are_sampling_at_their_vertices():
    gv = classed_volume((128,) * 3)
    for i, (d, k, cam) in enumerate(stream(8)):
        gv.integrate_classes(d, k, W, H, cam)
    cam = synth.camera_for_frame(57, 200)
    caster = tsdf_amd.GPURaycaster(W, H)
    V, N = caster.raycast(gv, cam)
    Vc, Nc, classes, votes = caster.raycast_classes(gv, cam)
    assert_same_floats(Vc, V, "vertices")
    assert_same_floats(Nc, N, "normals")
    words = gv.get_class_data()
    want_c, want_n = R.sample(words, R.geometry(gv), V)
    assert np.array_equal(classes, want_c) and np.array_equal(votes, want_n)
    got_c, got_n = gv.sample_classes(V)
    assert np.array_equal(classes, got_c) and np.array_equal(votes, got_n)
    miss = np.isnan(V[:, 0])
    assert miss.any() and (~miss).sum() > 50000
    assert np.all(classes[miss] == VOID) and np.all(votes[miss] == 0)
    assert (classes[~miss] != VOID).mean() > 0.95
    # the surface
    S, sc = gv.extract_classed_surface()
    assert_same_floats(S, gv.extract_surface(), "surface vertices")
    assert np.array_equal(sc, R.sample(words, R.geometry(gv), S)[0])
    assert len(S) > 10000 and (sc != VOID).mean() > 0.9
    # the indexed mesh: device to device on its vertex buffer
    mesh = gv.extract_mesh()
    mc = mesh.sample_classes(gv)
    assert mc.dtype == np.uint16 and mc.shape == (mesh.n_vertices,)
    assert np.array_equal(mc, gv.sample_classes(mesh.vertices)[0])
    assert (mc != VOID).mean() > 0.9 and {1, 2, 3} <= set(np.unique(mc).tolist())


def counts_into_poison(gv, n_classes, min_votes):
    """tsdf_volume_class_counts_device into a buffer of all-ones bytes, with a guard word behind it."""
    lib, out = _capi.lib, np.empty(n_classes + 1, np.uint64)
    poison = np.full(n_classes + 1, 0xFFFFFFFFFFFFFFFF, np.uint64)
    dc = C.c_void_p()
    _capi.check(lib.tsdf_device_alloc(poison.nbytes, C.byref(dc)))
    try:
        _capi.check(lib.tsdf_device_upload(dc, poison.ctypes.data, poison.nbytes))
        _capi.check(lib.tsdf_volume_class_counts_device(gv._h, n_classes, min_votes, dc, C.c_void_p(gv.stream_ptr() or 0)))
        gv.synchronize()
        _capi.check(lib.tsdf_device_download(out.ctypes.data, dc, out.nbytes))
    finally:
        lib.tsdf_device_free(dc)
    assert out[-1] == poison[-1], "the word behind the counts was written"
    return out[:-1]


@pytest.mark.parametrize("dims", [ODD, (128, 96, 80)])      # fewer voxels than one pass of the grid, and several passes
def test_class_counts_equal_bincount(dims):
    gv = classed_volume(dims)
    rng = np.random.default_rng(3)
    n = gv.resident_voxels()
    words = random_words(rng, n)
    few = rng.random(n) < 0.6                               # most voxels in a handful of classes with few votes, as a scene has them
    words[few] = rng.integers(0, 6, few.sum()).astype(np.uint32) | (rng.integers(0, 5, few.sum()).astype(np.uint32) << 16)
    words[(words >> 16) == 0] = 0
    gv.set_class_data(words)
    down = gv.get_class_data()
    for n_classes in (1, 4, 1024, 4096, 4097, 65535):       # (4096 / 4097: either side of the LDS histogram's limit)
        for min_votes in (1, 3):
            c, v = down & 0xFFFF, down >> 16
            sel = (v >= min_votes) & (c < n_classes)
            want = np.bincount(c[sel].astype(np.int64), minlength=n_classes).astype(np.uint64)
            assert np.array_equal(want, R.counts(down, n_classes, min_votes))
            assert np.array_equal(gv.class_counts(n_classes, min_votes), want), (n_classes, min_votes)
            assert np.array_equal(counts_into_poison(gv, n_classes, min_votes), want), (n_classes, min_votes)
    assert np.array_equal(gv.class_counts(8, 0), gv.class_counts(8, 1))      # min_votes 0 counts as 1
    assert int(gv.class_counts(65535).sum()) == int((down != 0).sum())


# The window radius of the test below, chosen on the CPU before any GPU run (tools/class_window_model.py: the oracle's integrate and
# ray cast plus tests/classes_ref.py, which the GPU equals bit for bit): the smallest r whose share of differing pixels is under 1 %.
R_WINDOW = 0


def test_fused_classes_match_the_analytic_classes():
    """40 frames of the synthetic stream at 256^3 with class_frame, then a classed ray cast from a pose not in the stream: on hit pixels
    whose voxel has votes, restricted to pixels whose analytic class is uniform over the (2r + 1)^2 window around them, at most 2 % differ
    from the analytic class of that pose, over at least 100 000 pixels.  r = 0 (every pixel): the CPU model gives 513 of 294 664 pixels
    differing (0.1741 %) there, 70 of 292 093 (0.0240 %) at r = 1 and none from r = 4 on -- the differing pixels sit on the objects'
    silhouettes, where a voxel's band holds votes of both sides."""
    n, F = 256, 40
    gv = classed_volume((n,) * 3)
    for i in range(F):
        d, cam = synth.depth_frame(i, F, seed=SEED)
        k, _ = synth.class_frame(i, F, seed=SEED)
        gv.integrate_classes(d, k, W, H, cam)
    cam = synth.camera_for_frame(0.5, F)                 # halfway between the stream's first two poses
    V, _, classes, votes = tsdf_amd.GPURaycaster(W, H).raycast_classes(gv, cam)
    truth = synth.trace_classes(cam)
    img = truth.reshape(H, W)
    uniform = np.ones((H, W), bool)
    for dy in range(-R_WINDOW, R_WINDOW + 1):
        for dx in range(-R_WINDOW, R_WINDOW + 1):
            y0, y1, x0, x1 = max(0, dy), H + min(0, dy), max(0, dx), W + min(0, dx)
            uniform[y0 - dy:y1 - dy, x0 - dx:x1 - dx] &= img[y0 - dy:y1 - dy, x0 - dx:x1 - dx] == img[y0:y1, x0:x1]
    sel = ~np.isnan(V[:, 0]) & (votes >= 1) & uniform.reshape(-1)
    differ = int((classes[sel] != truth[sel]).sum())
    print("classes: %d pixels compared at r = %d, %d differ (%.4f %%)" % (sel.sum(), R_WINDOW, differ, 100.0 * differ / max(sel.sum(), 1)))
    assert sel.sum() >= 100000
    assert differ <= 0.02 * sel.sum()


def test_clear_disable_and_enable_again():
    gv = classed_volume(ODD)
    d, k, cam = stream(1)[0]
    gv.integrate_classes(d, k, W, H, cam)
    assert gv.get_class_data().any() and gv.class_data()
    gv.clear()
    assert gv.classes_enabled() and not gv.get_class_data().any()
    gv.integrate_classes(d, k, W, H, cam)
    gv.enable_classes()                                  # already enabled: kept
    assert gv.get_class_data().any()
    gv.enable_classes(False)
    assert not gv.classes_enabled()
    with pytest.raises(ValueError, match="not enabled"):
        gv.get_class_data()
    gv.enable_classes()
    assert gv.classes_enabled() and not gv.get_class_data().any()


def test_refusals_explain_themselves_and_write_nothing():
    d, k, cam = stream(1)[0]
    lib, invalid = _capi.lib, _capi.TSDF_ERR_INVALID
    mats = [_capi_fp(m) for m in (cam.pose(), cam.inverse_pose(), cam.k(), cam.kinv())]
    # a slab refuses classes
    slab = tsdf_amd.TSDFVolume((64,) * 3, PHYS, slab=(0, 32))
    with pytest.raises(ValueError, match="tsdf_volume_enable_classes.*slab"):
        slab.enable_classes()
    assert not slab.classes_enabled()
    # every class call on a volume without classes
    plain, twin = tsdf_amd.TSDFVolume((64,) * 3, PHYS), tsdf_amd.TSDFVolume((64,) * 3, PHYS)
    plain.enable_colour()
    calls = {"tsdf_integrate_classes": lambda: plain.integrate_classes(d, k, W, H, cam),
             "tsdf_volume_sample_classes": lambda: plain.sample_classes(np.zeros((4, 3), np.float32)),
             "tsdf_volume_get_class_data": lambda: plain.get_class_data(),
             "tsdf_volume_set_class_data": lambda: plain.set_class_data(np.zeros(64 ** 3, np.uint32)),
             "tsdf_volume_classes": lambda: plain.class_data(),
             "tsdf_volume_class_counts": lambda: plain.class_counts(4),
             "tsdf_raycast_classes": lambda: tsdf_amd.GPURaycaster(W, H).raycast_classes(plain, cam)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match=name + ": classes are not enabled"):
            call()
    with pytest.raises(ValueError, match="not enabled"):
        plain.sample_classes(np.zeros((0, 3), np.float32))
    with pytest.raises(ValueError, match="not enabled"):
        plain.extract_mesh().sample_classes(plain)
    assert_same_floats(plain.get_distance_data(), twin.get_distance_data(), "a refused call wrote distances")
    assert not plain.get_colour_data().any()
    # the rest, on a volume with classes and words to lose
    gv = classed_volume((64,) * 3)
    gv.integrate_classes(d, k, W, H, cam)
    words, dist, weights = gv.get_class_data(), gv.get_distance_data(), gv.get_weight_data()
    rgb, _ = synth.colour_frame(0, 200, seed=SEED)
    with pytest.raises(ValueError, match="tsdf_integrate_classes: rgb given but colour is not enabled"):
        gv.integrate_classes(d, k, W, H, cam, rgb=rgb)
    dd, kk = np.ascontiguousarray(d), np.ascontiguousarray(k)
    for fn in (lib.tsdf_integrate_classes, lib.tsdf_integrate_classes_device):      # (refused before a pointer is looked at)
        assert fn(gv._h, None, None, kk.ctypes.data, None, W, H, *mats) == invalid and "tsdf_integrate_classes: null argument" in _capi.last_error()
        assert fn(gv._h, dd.ctypes.data, None, None, None, W, H, *mats) == invalid and "tsdf_integrate_classes: null argument" in _capi.last_error()
        assert fn(gv._h, dd.ctypes.data, None, kk.ctypes.data, None, 0, H, *mats) == invalid and "tsdf_integrate_classes: empty" in _capi.last_error()
        assert fn(gv._h, dd.ctypes.data, None, kk.ctypes.data, None, W, 0, *mats) == invalid and "tsdf_integrate_classes: empty" in _capi.last_error()
    stand_in = C.create_string_buffer(64)
    p = C.cast(stand_in, C.c_void_p)
    for n_classes in (0, 65536, 1 << 20):
        assert lib.tsdf_volume_class_counts(gv._h, n_classes, 1, p) == invalid and "tsdf_volume_class_counts: n_classes" in _capi.last_error()
        assert lib.tsdf_volume_class_counts_device(gv._h, n_classes, 1, p, None) == invalid and "tsdf_volume_class_counts: n_classes" in _capi.last_error()
        with pytest.raises(ValueError, match="n_classes"):
            gv.class_counts(n_classes)
    # null outputs
    assert lib.tsdf_volume_class_counts(gv._h, 4, 1, None) == invalid and "tsdf_volume_class_counts: null" in _capi.last_error()
    assert lib.tsdf_volume_class_counts_device(gv._h, 4, 1, None, None) == invalid and "tsdf_volume_class_counts: null" in _capi.last_error()
    assert lib.tsdf_volume_sample_classes_device(gv._h, 4, p, None, None, None) == invalid and "tsdf_volume_sample_classes: null" in _capi.last_error()
    assert lib.tsdf_volume_sample_classes_device(gv._h, 4, None, p, None, None) == invalid and "tsdf_volume_sample_classes: null" in _capi.last_error()
    assert lib.tsdf_volume_sample_classes_device(gv._h, 0, None, None, None, None) == _capi.TSDF_OK      # n == 0 launches nothing
    for fn in (lib.tsdf_raycast_classes, lib.tsdf_raycast_classes_device):
        assert fn(gv._h, W, H, mats[0], mats[3], None, None, p, None) == invalid and "tsdf_raycast_classes: null" in _capi.last_error()
        assert fn(gv._h, W, H, mats[0], mats[3], p, None, None, None) == invalid and "tsdf_raycast_classes: null" in _capi.last_error()
    assert lib.tsdf_volume_get_class_data(gv._h, None) == invalid and lib.tsdf_volume_set_class_data(gv._h, None) == invalid
    assert lib.tsdf_volume_classes(gv._h, None) == invalid and lib.tsdf_volume_classes_enabled(gv._h, None) == invalid
    assert stand_in.raw == bytes(64)
    # explicit deformation nodes
    gv.deformation()
    with pytest.raises(ValueError, match="tsdf_integrate_classes.*deformation"):
        gv.integrate_classes(d, k, W, H, cam)
    assert np.array_equal(gv.get_class_data(), words)
    assert_same_floats(gv.get_distance_data(), dist, "a refused call wrote distances")
    assert_same_floats(gv.get_weight_data(), weights, "a refused call wrote weights")


def _capi_fp(a):
    a = np.ascontiguousarray(a, np.float32)
    _capi_fp.keep.append(a)
    return a.ctypes.data_as(C.POINTER(C.c_float))


_capi_fp.keep = []
