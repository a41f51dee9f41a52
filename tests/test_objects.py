"""GPU: the class objects (include/tsdf_amd.h, "class objects") against the CPU reference tests/objects_ref.py.  Every comparison is
equality of integers or bytes.  Random class words (votes from {0, 1, 2, 65535}, class bits under zero votes) on grids whose 64-voxel
chunks straddle rows and planes and end partial, with 1, 3 and 300 classes, both connectivities, four min_size and three min_votes
values, with and without a selection; a checkerboard, two interleaved snakes, a serpentine and a half-filled 32^3 for the class
predicate and deep union-find chains; a fused 48^3 scene; the lookup against the class sampler, with the offset moved after clear; that
the volume is left alone; 16-bit weight storage; a reused handle and a warm run; and the refusals."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import objects_ref as R
from tests.helpers import H, W
from tsdf_amd import _capi, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = tsdf_amd.OBJECT_NONE
SEED = 0x5EED0003
# one voxel; 64-voxel chunks that straddle rows with a partial last chunk; exactly two chunks of one row each plane; a row one longer than a
# chunk; rows of two chunks and two voxels (several chunks a plane); and, because a wave of the flag kernel walks 64 chunks, 104 chunks:
# a full wave and part of a second (the fused 48^3 below: 27 waves, six workgroups and three quarters of one); and 17 391 voxels in 272
# chunks: a second workgroup whose first wave walks 16 chunks while its other three walk none, and a last chunk of 47 voxels
GRIDS = [(1, 1, 1), (13, 7, 5), (64, 3, 2), (65, 4, 3), (130, 3, 3), (67, 9, 11), (33, 31, 17)]
DENSITIES = [0.0, 0.1, 0.5, 0.9, 1.0]
CLASS_COUNTS = [1, 3, 300]
OFFSET = (100.0, -50.0, 25.0)
VS = np.array([10.0, 12.5, 9.0], F32)


def volume_of(size, words=None):
    """Anisotropic voxels (10 x 12.5 x 9 mm) and an offset set after clear, with class words."""
    gv = tsdf_amd.TSDFVolume(size, (size[0] * 10.0, size[1] * 12.5, size[2] * 9.0))
    gv.offset(*OFFSET)
    assert np.array_equal(gv.voxel_size(), VS)
    gv.enable_classes()
    if words is not None:
        gv.set_class_data(words)
    return gv


def select_bytes(classes):
    """What TSDFVolume.find_objects makes of `classes`: the reference's selection."""
    if classes is None:
        return None
    s = np.zeros(max(classes) + 1 if classes else 1, np.uint8)
    s[list(classes)] = 1
    return s


def assert_objects(gv, ob, words, size, min_votes, classes, connectivity, min_sizes, what):
    """find_objects into `ob` at every min_size of min_sizes (and one above the biggest object) equals the reference; returns the last
    (ids, L, rows)."""
    ids = R.labelled(words, min_votes, select_bytes(classes))
    L, every, n_objects = R.objects(words, ids, size, connectivity, 0)
    biggest = int(every["size"].max()) if len(every) else 0
    for min_size in list(min_sizes) + [biggest + 1]:
        rows = every[every["size"] >= min_size]        # (the rule: the rows with size >= min_size, in ascending label)
        assert gv.find_objects(min_votes, classes, connectivity, min_size, into=ob) is ob
        i = ob.info
        where = "%s min_votes %d classes %s connectivity %d min_size %d" % (what, min_votes, classes, connectivity, min_size)
        assert (tuple(i.size), i.connectivity, i.min_votes, i.min_size) == (tuple(size), connectivity, min_votes, min_size), where
        assert (i.n_labelled, i.n_objects, i.n_listed_objects) == (len(ids), n_objects, len(rows)), where
        assert np.array_equal(ob.voxels, ids), where
        assert np.array_equal(ob.labels, L), where
        got = ob.objects
        assert got.dtype == R.OBJECT_DTYPE and got.tobytes() == rows.tobytes(), where
    assert len(rows) == 0
    rows = every[every["size"] >= min_sizes[-1]]
    gv.find_objects(min_votes, classes, connectivity, min_sizes[-1], into=ob)
    return ids, L, rows


@pytest.mark.parametrize("size", GRIDS)
def test_random_words_equal_the_reference(size):
    ob = tsdf_amd.Objects()
    seed = 9000 + size[0] + 3 * size[2]
    gv = volume_of(size)
    k = 0
    for n_classes in CLASS_COUNTS:
        # half of the classes; with 300 classes a selection that ends below the largest class, so n_select cuts too
        chosen = [0] if n_classes == 1 else ([0, 2] if n_classes == 3 else list(range(0, 150, 2)))
        for density in DENSITIES:
            words = R.random_words(size, seed + k, density, n_classes)
            gv.set_class_data(words)
            for min_votes in (0, 1, 2):
                classes = chosen if (k + min_votes) % 2 else None      # every (density, class count) sees both, over its three min_votes
                for connectivity in (6, 26):
                    assert_objects(gv, ob, words, size, min_votes, classes, connectivity, (0, 1, 3),
                                   "grid %s density %s %d classes" % (size, density, n_classes))
            k += 1
    # an empty selection admits nothing, one of every class everything
    assert gv.find_objects(classes=[], into=ob).info.n_labelled == 0
    assert gv.find_objects(classes=range(300), into=ob).info.n_labelled == len(R.labelled(words, 1))
    n = size[0] * size[1] * size[2]
    assert ob.scratch_bytes >= 12 * ((n + 63) // 64)
    gv.close()
    ob.close()


def test_a_two_class_checkerboard():
    size = (13, 7, 5)
    z, y, x = np.meshgrid(np.arange(5), np.arange(7), np.arange(13), indexing="ij")
    words = R.words_of(((x + y + z) % 2).reshape(-1), np.full(13 * 7 * 5, 3))
    gv = volume_of(size, words)
    ob = tsdf_amd.Objects()
    ids, L, rows = assert_objects(gv, ob, words, size, 1, None, 6, (1,), "checkerboard")
    assert len(rows) == 455 and np.array_equal(L, np.arange(455)) and (rows["size"] == 1).all()     # no face neighbour shares the class
    ids, L, rows = assert_objects(gv, ob, words, size, 1, None, 26, (1,), "checkerboard")
    assert rows["size"].tolist() == [228, 227] and rows["class_id"].tolist() == [0, 1] and rows["label"].tolist() == [0, 1]
    assert rows["votes"].tolist() == [3 * 228, 3 * 227]
    gv.close()
    ob.close()


def test_sixty_four_roots_in_a_wave_and_a_one_lane_wave():
    """130 x 1 x 1 with a labelled voxel at every other x: 65 listed voxels, none adjacent to another, so the first wave of the stats
    kernel reduces 64 distinct roots and the second has one lane."""
    size = (130, 1, 1)
    x = np.arange(130)
    words = R.words_of(x % 7, np.where(x % 2 == 0, 1 + x % 5, 0))
    gv = volume_of(size, words)
    ob = tsdf_amd.Objects()
    for connectivity in (6, 26):
        ids, L, rows = assert_objects(gv, ob, words, size, 1, None, connectivity, (1,), "every other voxel at %d" % connectivity)
        assert np.array_equal(ids, x[::2]) and np.array_equal(L, np.arange(65)) and len(rows) == 65 and (rows["size"] == 1).all()
        assert rows["votes"].tolist() == (1 + x[::2] % 5).tolist() and rows["class_id"].tolist() == (x[::2] % 7).tolist()
    gv.close()
    ob.close()


def test_snakes_a_serpentine_and_a_half_filled_cube_give_deep_chains():
    ob = tsdf_amd.Objects()
    # two 200-voxel snakes of different classes next to each other: rows y = 0 and y = 1 of a 200 x 2 grid; then two wound ones
    size = (200, 2, 1)
    words = R.words_of(np.repeat([4, 9], 200), np.full(400, 2))
    gv = volume_of(size, words)
    for connectivity in (6, 26):
        ids, L, rows = assert_objects(gv, ob, words, size, 1, None, connectivity, (1,), "two snakes at %d" % connectivity)
        assert rows["size"].tolist() == [200, 200] and rows["class_id"].tolist() == [4, 9] and rows["label"].tolist() == [0, 200]
        assert rows["sum"].tolist() == [[199 * 100, 0, 0], [199 * 100, 200, 0]] and rows["votes"].tolist() == [400, 400]
    gv.close()
    size = (40, 10, 1)
    cls = np.zeros((10, 40), np.int64)
    votes = np.zeros((10, 40), np.int64)
    # a ribbon two voxels wide, class 1 on one side and class 2 on the other, along rows 0-1, down the right end, back along rows 4-5,
    # down the left end, along rows 8-9: at a turn the outer class goes round the inner one, so each class stays one face-connected path
    cls[0, :], cls[1, :39], cls[4, :39], cls[5, 1:], cls[8, 1:], cls[9, :] = 1, 2, 2, 1, 1, 2
    cls[0:6, 39], cls[1:5, 38], cls[4:10, 0], cls[5:9, 1] = 1, 2, 2, 1
    votes[cls > 0] = 1
    assert (cls == 1).sum() == 124 and (cls == 2).sum() == 124
    words = R.words_of(cls.reshape(-1), votes.reshape(-1))
    gv = volume_of(size, words)
    for connectivity in (6, 26):
        ids, L, rows = assert_objects(gv, ob, words, size, 1, None, connectivity, (1,), "two wound snakes at %d" % connectivity)
        assert rows["class_id"].tolist() == [1, 2] and rows["size"].tolist() == [124, 124] and rows["label"].tolist() == [0, 40]
    gv.close()
    # a serpentine of one class: rows joined at alternating ends, so the object's smallest index is far from most of its voxels
    size = (40, 9, 1)
    votes = np.ones((9, 40), np.int64)
    for y in range(1, 9, 2):
        votes[y, :] = 0
        votes[y, 39 if (y // 2) % 2 == 0 else 0] = 1
    words = R.words_of(np.full(360, 7), votes.reshape(-1))
    gv = volume_of(size, words)
    for connectivity in (6, 26):
        ids, L, rows = assert_objects(gv, ob, words, size, 1, None, connectivity, (1,), "serpentine at %d" % connectivity)
        assert len(rows) == 1 and rows[0]["size"] == 204
    gv.close()
    size = (32, 32, 32)
    words = R.random_words(size, 4242, 0.5, 2)
    gv = volume_of(size, words)
    for connectivity in (6, 26):
        ids, L, rows = assert_objects(gv, ob, words, size, 1, None, connectivity, (2,), "half-filled 32^3 at %d" % connectivity)
        assert len(ids) > 15000 and len(rows) > 2
    gv.close()
    ob.close()


@pytest.fixture(scope="module")
def fused():
    """Three synthetic frames with their class frames on 48^3: (frames, class words) of the device's own integration."""
    frames = []
    for i in range(3):
        d, cam = synth.depth_frame(i * 9, 40, seed=SEED)
        k, _ = synth.class_frame(i * 9, 40, seed=SEED)
        frames.append((d, k, cam))
    gv = fused_volume(frames)
    words = gv.get_class_data()
    gv.close()
    return frames, words


def fused_volume(frames, n=48):
    gv = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    gv.enable_classes()
    for d, k, cam in frames:
        gv.integrate_classes(d, k, W, H, cam)
    return gv


def test_a_fused_scene_a_reused_handle_and_a_warm_run(fused):
    frames, words = fused
    size = (48,) * 3
    ob = tsdf_amd.Objects()
    assert ob.scratch_bytes == 32 and ob.info.n_labelled == 0
    gv = fused_volume(frames)
    assert gv.get_class_data().tobytes() == words.tobytes()
    ids, L, rows = assert_objects(gv, ob, words, size, 1, None, 26, (5,), "fused scene")
    # at the reference's own output every one of the three synthetic classes has a listed object
    want = R.find(words, size, 1, None, 26, 5)[2]
    assert {1, 2, 3} <= set(want["class_id"].tolist()) and len(ids) > 1000
    result = (ob.voxels.tobytes(), ob.labels.tobytes(), ob.objects.tobytes())
    assert result[2] == want.tobytes()
    # the world positions and boxes
    info, vs = ob.info, np.array(gv.voxel_size(), np.float64)
    assert np.array_equal(ob.coordinates, R.coordinates(ids, size).astype(np.uint32))
    assert np.array_equal(ob.centroids, (rows["sum"] / rows["size"][:, None] + 0.5) * vs + np.array(info.offset, np.float64))
    assert np.array_equal(ob.boxes, np.concatenate([rows["lo"], rows["hi"] + 1], axis=1))
    # one run in 16-bit weight storage: weights are not read
    wide = fused_volume(frames)
    wide.set_weight_storage(16)
    assert wide.weight_storage()[0] == 16
    wide.find_objects(1, None, 26, 5, into=ob)
    assert (ob.voxels.tobytes(), ob.labels.tobytes(), ob.objects.tobytes()) == result
    wide.close()
    # the same handle on a small grid and back: the same bytes, and no array grows on the way back or in a warm second run
    gv.find_objects(1, [1, 2, 3], 26, 5, into=ob)
    warm = ob.scratch_bytes
    small_words = R.random_words((13, 7, 5), 77, 0.5, 3)
    small = volume_of((13, 7, 5), small_words)
    assert_objects(small, ob, small_words, (13, 7, 5), 1, [0, 2], 6, (1,), "reused on a small grid")
    small.close()
    for run in range(2):
        gv.find_objects(1, None, 26, 5, into=ob)
        assert (ob.voxels.tobytes(), ob.labels.tobytes(), ob.objects.tobytes()) == result, "run %d" % run
        assert ob.scratch_bytes == warm
    bufs = ob.device_buffers()
    assert all(bufs[k] for k in ("voxels", "masks", "bases", "labels", "objects"))
    host = np.empty(ob.info.n_labelled, np.uint32)
    _capi.check(_capi.lib.tsdf_device_download(host.ctypes.data, C.c_void_p(bufs["voxels"]), host.nbytes))
    assert host.tobytes() == result[0]
    host = np.empty(ob.info.n_listed_objects, R.OBJECT_DTYPE)
    _capi.check(_capi.lib.tsdf_device_download(host.ctypes.data, C.c_void_p(bufs["objects"]), host.nbytes))
    assert host.tobytes() == result[2]
    # an empty result: the buffers are null where they are empty
    gv.find_objects(1, [], 26, 1, into=ob)
    bufs = ob.device_buffers()
    assert (bufs["voxels"], bufs["labels"], bufs["objects"]) == (0, 0, 0) and bufs["masks"] and bufs["bases"]
    assert len(ob.voxels) == 0 and len(ob.labels) == 0 and len(ob.objects) == 0 and ob.scratch_bytes == warm
    assert (ob.lookup(np.full((3, 3), 1500.0, F32)) == NONE).all()
    gv.close()
    ob.close()


def geometry(gv):
    i = gv.info()
    return tuple(int(v) for v in i.size), tuple(i.voxel_size), tuple(i.offset), tuple(i.offset_at_clear)


def assert_lookup(gv, ob, words, points, ids, L, rows, min_votes, classes, what):
    """The lookup of `points` equals the reference, is the sampler's voxel, and the host twin is the device call."""
    size, vs, offset, at_clear = geometry(gv)
    points = np.ascontiguousarray(points, F32).reshape(-1, 3)
    got = ob.lookup(points)
    assert got.dtype == np.uint32 and np.array_equal(got, R.lookup(points, ids, L, rows, size, vs, offset, at_clear)), what
    # the sampler on the same points: a row iff the sampled votes and class are admitted and the object is listed
    sc, sn = gv.sample_classes(points)
    admitted = sn >= max(min_votes, 1)
    if classes is not None:
        admitted &= np.isin(sc, list(classes))
    listed = got != NONE
    assert not (listed & ~admitted).any(), what
    assert np.array_equal(rows["class_id"][got[listed]], sc[listed].astype(np.uint32)), what
    # (admitted and not listed: the voxel's object is below min_size)
    index = {int(v): k for k, v in enumerate(ids)}
    for p in np.flatnonzero(admitted & ~listed):
        v = R.voxel_of(points[p], size, vs, offset, at_clear)
        assert int(L[index[v]]) not in set(rows["label"].tolist()), what
    return got


def device_lookup(ob, points):
    lib = _capi.lib
    points = np.ascontiguousarray(points, F32).reshape(-1, 3)
    n = len(points)
    out = np.full(n, 12345, np.uint32)
    dp, dr = C.c_void_p(), C.c_void_p()
    _capi.check(lib.tsdf_device_alloc(max(points.nbytes, 4), C.byref(dp)))
    _capi.check(lib.tsdf_device_alloc(max(out.nbytes, 4), C.byref(dr)))
    try:
        if n:
            _capi.check(lib.tsdf_device_upload(dp, points.ctypes.data, points.nbytes))
            _capi.check(lib.tsdf_device_upload(dr, out.ctypes.data, out.nbytes))
        ob.lookup_device(n, dp.value, dr.value)
        _capi.check(lib.tsdf_stream_synchronize(None))
        if n:
            _capi.check(lib.tsdf_device_download(out.ctypes.data, dr, out.nbytes))
    finally:
        lib.tsdf_device_free(dp)
        lib.tsdf_device_free(dr)
    return out


def voxel_centres(gv):
    size, vs, offset, at_clear = geometry(gv)
    z, y, x = np.meshgrid(np.arange(size[2]), np.arange(size[1]), np.arange(size[0]), indexing="ij")
    c = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(np.float64)
    return ((c + 0.5) * np.array(vs, np.float64) + np.array(offset, np.float64) + np.array(at_clear, np.float64)).astype(F32)


@pytest.mark.parametrize("moved", ["after clear", "before and after clear"])
def test_lookup_is_the_samplers_voxel(moved):
    size = (13, 7, 5)
    words = R.random_words(size, 31337, 0.6, 3)
    gv = tsdf_amd.TSDFVolume(size, (130.0, 87.5, 45.0))
    if moved == "before and after clear":
        gv.offset(7.0, -3.0, 2.5)
        gv.clear()                        # offset_at_clear = (7, -3, 2.5)
    gv.enable_classes()
    gv.set_class_data(words)
    gv.offset(*OFFSET)                    # the sampler's frame subtracts both; the handle takes both at find_objects
    size_, vs, offset, at_clear = geometry(gv)
    assert offset == OFFSET and at_clear == ((7.0, -3.0, 2.5) if moved == "before and after clear" else (0.0, 0.0, 0.0))
    centres = voxel_centres(gv)
    rng = np.random.default_rng(5)
    lo = np.array(offset) + np.array(at_clear)
    special = np.array([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], lo - 0.01, lo, lo + np.array([130.0, 0, 0]), lo + np.array([0, 87.5, 0]),
                        lo + np.array([0, 0, 45.0]), lo + np.array([129.99, 87.49, 44.99]), [1e30, 0, 0], [-np.inf, 0, 0]], F32)
    scatter = (lo + rng.uniform(-20.0, 150.0, (300, 3))).astype(F32)
    points = np.concatenate([centres, special, scatter])
    ob = tsdf_amd.Objects()
    for min_votes, classes, connectivity, min_size in ((1, None, 26, 1), (2, [0, 2], 6, 2), (0, [1], 26, 3)):
        ids, L, rows = assert_objects(gv, ob, words, size, min_votes, classes, connectivity, (min_size,), "lookup grid, offset moved " + moved)
        got = assert_lookup(gv, ob, words, points, ids, L, rows, min_votes, classes, moved)
        assert (got[len(centres):len(centres) + 4] == NONE).all() and (got[len(centres) + 5:len(centres) + 8] == NONE).all()
        # every voxel centre: listed voxels in listed objects have their row, in list order
        listed_rows = got[:len(centres)][ids.astype(np.int64)]
        keep = np.isin(L, rows["label"])
        assert np.array_equal(listed_rows[keep], np.searchsorted(rows["label"], L[keep]).astype(np.uint32)) and (listed_rows[~keep] == NONE).all()
        assert (listed_rows != NONE).any()
        # the host twin against the device call, at sizes below, at and across a wave and a workgroup
        for n in (0, 1, 64, 257):
            dev = device_lookup(ob, points[:n])
            assert np.array_equal(dev, got[:n]) and np.array_equal(ob.lookup(points[:n]), got[:n]), n
    # the handle remembers the geometry of its find: moving the volume afterwards does not move the lookup
    before = ob.lookup(points)
    gv.offset(0.0, 0.0, 0.0)
    assert np.array_equal(ob.lookup(points), before)
    gv.close()
    assert np.array_equal(ob.lookup(points), before)       # nothing here needs the volume
    ob.close()


def test_the_volume_is_left_alone_and_a_cast_is_an_instance_image(fused):
    frames, words = fused
    gv = fused_volume(frames)
    gv.enable_colour()
    gv.set_colour_data(np.arange(48 ** 3, dtype=np.uint32))
    cam = frames[1][2]
    v0, n0 = gv.raycast(W, H, cam)
    kind0 = gv.last_raycast_cell_parallel()
    state = lambda: (gv.get_distance_data().tobytes(), gv.get_weight_data().tobytes(), gv.get_class_data().tobytes(),
                     gv.get_colour_data().tobytes(), gv.weight_storage())
    before = state()
    ob = gv.find_objects(1, None, 26, 5)
    ids, L, rows = ob.voxels, ob.labels, ob.objects
    # the instance-segmentation image: the lookup on the cast's vertices, misses included
    got = assert_lookup(gv, ob, words, v0, ids, L, rows, 1, None, "a ray cast's vertices")
    miss = np.isnan(v0[:, 0])
    assert miss.any() and (got[miss] == NONE).all() and (got[~miss] != NONE).sum() > 1000
    assert state() == before
    assert gv.last_raycast_cell_parallel() == kind0
    v1, n1 = gv.raycast(W, H, cam)
    assert gv.last_raycast_cell_parallel() == kind0
    assert v1.tobytes() == v0.tobytes() and n1.tobytes() == n0.tobytes()
    ob.close()
    gv.close()


def test_refusals():
    lib, invalid = _capi.lib, _capi.TSDF_ERR_INVALID
    size = (13, 7, 5)
    words = R.random_words(size, 1, 0.5, 3)
    gv = volume_of(size, words)
    plain = tsdf_amd.TSDFVolume(size, (130.0, 87.5, 45.0))           # no classes
    ob = tsdf_amd.Objects()
    sel = (C.c_uint8 * 4)(1, 1, 1, 1)
    info0 = bytes(ob.info)

    def refused(rc, who):
        assert rc == invalid and who in _capi.last_error(), (who, rc, _capi.last_error())

    find = "tsdf_volume_find_objects"
    refused(lib.tsdf_volume_find_objects(None, 1, None, 0, 26, 1, 0, ob._h), find)
    refused(lib.tsdf_volume_find_objects(gv._h, 1, None, 0, 26, 1, 0, None), find)
    refused(lib.tsdf_volume_find_objects(plain._h, 1, None, 0, 26, 1, 0, ob._h), find)
    for connectivity in (0, 7, 18, 27):
        refused(lib.tsdf_volume_find_objects(gv._h, 1, None, 0, connectivity, 1, 0, ob._h), find)
    refused(lib.tsdf_volume_find_objects(gv._h, 1, None, 0, 26, 1, 1, ob._h), find)
    refused(lib.tsdf_volume_find_objects(gv._h, 1, None, 4, 26, 1, 0, ob._h), find)
    refused(lib.tsdf_volume_find_objects(gv._h, 1, sel, 65536, 26, 1, 0, ob._h), find)
    # before any find: buffers, download and lookup are refused, and the refusals above wrote nothing
    assert bytes(ob.info) == info0 and ob.scratch_bytes == 32
    p = C.c_void_p()
    row = np.zeros(4, np.uint32)
    pts = np.zeros((1, 3), F32)
    refused(lib.tsdf_objects_buffers(ob._h, C.byref(p), None, None, None, None), "tsdf_objects_buffers")
    refused(lib.tsdf_objects_download(ob._h, row.ctypes.data, None, None), "tsdf_objects_download")
    refused(lib.tsdf_objects_lookup(ob._h, 1, pts.ctypes.data, row.ctypes.data), "tsdf_objects_lookup")
    refused(lib.tsdf_objects_lookup_device(ob._h, 0, None, None, None), "tsdf_objects_lookup_device")
    with pytest.raises(ValueError, match="tsdf_objects_download"):
        ob.voxels
    with pytest.raises(ValueError, match="tsdf_volume_find_objects"):
        plain.find_objects()
    with pytest.raises(ValueError, match="tsdf_volume_find_objects"):
        gv.find_objects(connectivity=18)
    with pytest.raises(ValueError):
        gv.find_objects(classes=[65535])
    # after a find: null points or rows with n > 0; n == 0 is fine with nulls
    gv.find_objects(into=ob)
    refused(lib.tsdf_objects_lookup(ob._h, 1, None, row.ctypes.data), "tsdf_objects_lookup")
    refused(lib.tsdf_objects_lookup(ob._h, 1, pts.ctypes.data, None), "tsdf_objects_lookup")
    refused(lib.tsdf_objects_lookup_device(ob._h, 1, None, None, None), "tsdf_objects_lookup_device")
    assert lib.tsdf_objects_lookup(ob._h, 0, None, None) == 0 and lib.tsdf_objects_lookup_device(ob._h, 0, None, None, None) == 0
    assert lib.tsdf_objects_buffers(ob._h, None, None, None, None, None) == 0 and lib.tsdf_objects_download(ob._h, None, None, None) == 0
    # a refused find leaves the handle's last result readable
    held = (ob.voxels.tobytes(), ob.labels.tobytes(), ob.objects.tobytes(), bytes(ob.info))
    refused(lib.tsdf_volume_find_objects(gv._h, 1, None, 0, 5, 1, 0, ob._h), find)
    assert (ob.voxels.tobytes(), ob.labels.tobytes(), ob.objects.tobytes(), bytes(ob.info)) == held
    for v in (gv, plain):
        v.close()
    ob.close()
