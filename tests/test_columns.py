"""GPU: the column maps (include/tsdf_amd.h, "column maps") against the CPU reference tests/columns_ref.py.  Every row is compared byte
for byte (tobytes() of the structured array, NaN included), every total integer for integer.  Random state fields with NaN and -0.0
distances (and NaN weights in fp32 storage) on the grids of tests/test_explore.py, all three weight storages, all three axes forward
and reversed, whole and over an inner band with odd ends; planted columns at multiples of 64 along x and at the packed
dwords of the walk; the decreed ends of the height's fraction; the ESDF minimum and its signed zero; the classification through the
device and the host call; a small fused scene, a reused handle and a warm run; that the volume is left alone; and the refusals."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import columns_ref as R
from tests import explore_ref
from tests.helpers import H, W
from tsdf_amd import _capi, synth
from tsdf_amd.api import _DeviceArray

pytestmark = pytest.mark.gpu

F32 = np.float32
GRIDS = [(1, 1, 1), (13, 7, 5), (64, 3, 2), (65, 4, 3), (130, 3, 3), (67, 9, 11), (33, 31, 17)]
DENSITIES = [0.0, 0.1, 0.5, 0.9, 1.0]
OFFSET = (100.0, -50.0, 25.0)
VS = np.array([10.0, 12.5, 9.0], F32)
CLASSIFY = [(0, 0), (1, 2), (2 ** 31 - 1, 0)]


def volume_of(size, D=None, Wt=None):
    """Anisotropic voxels (10 x 12.5 x 9 mm) and an offset, as tests/test_explore.py::volume_of makes them."""
    gv = tsdf_amd.TSDFVolume(size, (size[0] * 10.0, size[1] * 12.5, size[2] * 9.0))
    gv.offset(*OFFSET)
    assert np.array_equal(gv.voxel_size(), VS)
    if D is not None:
        gv.set_distance_data(D)
        gv.set_weight_data(Wt)
    return gv


def widen(gv, bits):
    if gv.weight_storage()[0] != bits:
        gv.set_weight_storage(bits)
    assert gv.weight_storage()[0] == bits


def inner_band(n):
    """lo and hi odd, inside the axis where it is long enough, hi - lo no multiple of 4 (nor of 64); None for an axis shorter than 3."""
    if n < 3:
        return None
    hi = n if n % 2 else n - 1
    if (hi - 1) % 4 == 0 and hi - 2 > 1:
        hi -= 2
    assert hi > 1 and hi % 2 == 1 and ((hi - 1) % 4 != 0 or n < 6)
    return (1, hi)


def assert_map(cmap, want, size, axis, band, reversed_, what, has_esdf=False):
    rows, totals = want
    got = cmap.columns
    assert got.dtype == R.COLUMN_DTYPE and got.shape == rows.shape, what
    if got.tobytes() != rows.tobytes():
        bad = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got.reshape(-1), rows.reshape(-1))])
        assert False, (what, len(bad), int(bad[0]), got.reshape(-1)[bad[0]], rows.reshape(-1)[bad[0]])
    i = cmap.info
    lo, hi = R.band_of(size, axis, band)
    assert {k: int(getattr(i, k)) for k in totals} == totals, what
    assert (tuple(i.size), i.axis, i.lo, i.hi, i.has_esdf) == (tuple(size), axis, lo, hi, int(has_esdf)), what
    assert (tuple(i.map_size), tuple(i.map_axes)) == ((rows.shape[1], rows.shape[0]), R.MAP_AXES[axis]), what
    assert bool(i.flags & _capi.TSDF_COLUMNS_REVERSED) == reversed_, what
    assert i.n_unknown + i.n_free + i.n_occupied == rows.size * (hi - lo), what
    assert (i.n_no_ground, i.n_traversable, i.n_blocked, i.max_step, i.min_headroom) == (0, 0, 0, 0, 0), what
    return got


def cases(size):
    """(axis, band, reversed) of every projection a field is put through: whole and inner band, forward and reversed, on all axes."""
    out = []
    for axis in (0, 1, 2):
        bands = [None] + ([inner_band(size[axis])] if inner_band(size[axis]) else [])
        out += [(axis, band, reversed_) for band in bands for reversed_ in (False, True)]
    return out


@pytest.mark.parametrize("size", GRIDS)
def test_random_state_fields_equal_the_reference(size):
    cmap = tsdf_amd.ColumnMap()
    seed = 9000 + size[0] + 3 * size[2]
    for k, density in enumerate(DENSITIES):
        references = {}   # (the packed storages hold the same field: one reference for both)
        for bits in (8, 16, 32):
            odd = bits == 32   # fp32 storage also gets NaN and fractional weights (a packed count cannot hold them)
            D, Wt = explore_ref.random_state_field(size, seed + k, density, fp32_oddities=odd)
            gv = volume_of(size, D, Wt)
            widen(gv, bits)
            for axis, band, reversed_ in cases(size):
                key = (odd, axis, band, reversed_)
                if key not in references:
                    references[key] = R.project(D, Wt, size, axis, band, reversed_)
                what = "grid %s density %s %d-bit weights axis %d band %s reversed %s" % (size, density, bits, axis, band, reversed_)
                assert gv.column_map(axis, band, reversed_, into=cmap) is cmap
                assert_map(cmap, references[key], size, axis, band, reversed_, what)
            assert gv.weight_storage()[0] == bits
            gv.close()
    cmap.close()


def test_a_third_partial_workgroup():
    # (67, 9, 11) on axis 2 is 603 cells: two workgroups of the walk and 91 lanes of a third
    assert 67 * 9 == 603 and 2 * 256 < 603 < 3 * 256 and (67, 9, 11) in GRIDS


def planted_row_field():
    """(130, 2, 2), columns along x.  (y, z) = (0, 0): occupied at x = 63 alone, free elsewhere, so top and the voxel above lie in
    different chunks; (1, 0): occupied at x = 59, free from 60 to 129, a run across two chunk borders to the end of the column;
    (0, 1): never observed; (1, 1): occupied throughout."""
    size = (130, 2, 2)
    D = np.full((2, 2, 130), 0.5, F32)
    Wt = np.ones((2, 2, 130), F32)
    D[0, 0, 63] = -0.5
    D[0, 0, 64] = 0.25
    D[0, 1, 59] = -0.25
    D[0, 1, :59] = np.where(np.arange(59) % 3 == 0, -0.75, 0.5)
    Wt[0, 1, 10:20] = 0.0
    Wt[1, 0, :] = 0.0
    D[1, 1, :] = -0.125
    return size, D.reshape(-1), Wt.reshape(-1)


def test_planted_columns_at_multiples_of_64_along_x():
    size, D, Wt = planted_row_field()
    whole, _ = R.project(D, Wt, size, 0)
    # what the planting is for, by the reference: (v, u) = (z, y)
    assert (whole[0, 0]["top"], whole[0, 0]["bottom"], whole[0, 0]["headroom"], whole[0, 0]["height"]) == (63, 63, 66, F32(63.5) + F32(-0.5) / F32(-0.75))
    assert (whole[0, 1]["top"], whole[0, 1]["headroom"]) == (59, 70) and whole[0, 1]["n_unknown"] == 10
    assert (whole[1, 0]["n_unknown"], whole[1, 0]["top"]) == (130, -1) and np.isnan(whole[1, 0]["height"])
    assert (whole[1, 1]["n_occupied"], whole[1, 1]["top"], whole[1, 1]["headroom"], whole[1, 1]["height"]) == (130, 129, 0, F32(130.0))
    cmap = tsdf_amd.ColumnMap()
    for bits in (8, 16, 32):
        gv = volume_of(size, D, Wt)
        widen(gv, bits)
        for band in (None, (63, 65), (64, 128), (129, 130), (59, 130), (60, 64), (1, 127)):
            for reversed_ in (False, True):
                want = R.project(D, Wt, size, 0, band, reversed_)
                what = "%d-bit band %s reversed %s" % (bits, band, reversed_)
                assert_map(gv.column_map(0, band, reversed_, into=cmap), want, size, 0, band, reversed_, what)
        gv.close()
    cmap.close()


def test_planted_columns_across_a_packed_dword():
    """(3, 2, 11), columns along z: (x, y) = (0, 0) has its top at z = 3 and free above, across the dword of 8-bit counts (z 0..3 | 4..7)
    and inside one of 16-bit counts' neighbours (z 2, 3 | 4, 5); (1, 0) all free; (2, 0) never observed; (0, 1) all occupied; (1, 1) and
    (2, 1) mixed, with unobserved voxels that end the free run."""
    size = (3, 2, 11)
    D = np.full((11, 2, 3), 0.5, F32)
    Wt = np.ones((11, 2, 3), F32)
    D[3, 0, 0] = -0.5
    D[4, 0, 0] = 0.25
    Wt[:, 0, 2] = 0.0
    D[:, 1, 0] = -1.0
    D[[1, 2, 6], 1, 1] = -0.5
    Wt[9, 1, 1] = 0.0
    D[:5, 1, 2] = -0.5
    Wt[5, 1, 2] = 0.0
    D, Wt = D.reshape(-1), Wt.reshape(-1)
    whole, _ = R.project(D, Wt, size, 2)
    assert (whole[0, 0]["top"], whole[0, 0]["headroom"], whole[0, 0]["height"]) == (3, 7, F32(3.5) + F32(-0.5) / F32(-0.75))
    assert (whole[0, 1]["n_free"], whole[0, 1]["top"]) == (11, -1) and whole[0, 2]["n_unknown"] == 11
    assert (whole[1, 0]["n_occupied"], whole[1, 0]["headroom"], whole[1, 0]["height"]) == (11, 0, F32(11.0))
    assert (whole[1, 1]["top"], whole[1, 1]["headroom"]) == (6, 2) and (whole[1, 2]["top"], whole[1, 2]["headroom"]) == (4, 0)
    cmap = tsdf_amd.ColumnMap()
    for bits in (8, 16, 32):
        gv = volume_of(size, D, Wt)
        widen(gv, bits)
        for band in (None, (3, 5), (1, 10), (3, 4), (4, 5)):   # (the last two: L = 1)
            for reversed_ in (False, True):
                want = R.project(D, Wt, size, 2, band, reversed_)
                assert_map(gv.column_map(2, band, reversed_, into=cmap), want, size, 2, band, reversed_, "%d-bit band %s reversed %s" % (bits, band, reversed_))
        gv.close()
    cmap.close()


def test_the_ends_of_the_heights_fraction():
    """Columns of two voxels, occupied below free, with d1 of NaN, -0.0, +0.0 and +inf and d0 of -inf: the fallback and both ends of f."""
    pairs = [(-1.0, np.nan), (-1.0, -0.0), (-1.0, 0.0), (-1.0, np.inf), (-np.inf, 1.0), (-np.inf, np.inf), (-1.0, 3.0), (-0.5, 0.5)]
    want_height = [1.0, 1.5, 1.5, 0.5, 1.0, 1.0, 0.75, 1.0]
    cmap = tsdf_amd.ColumnMap()
    for axis in (0, 1, 2):
        au, av = R.MAP_AXES[axis]
        size = [0, 0, 0]
        size[axis], size[au], size[av] = 2, len(pairs), 1
        D = np.zeros((size[2], size[1], size[0]), F32)
        for i, (d0, d1) in enumerate(pairs):
            for p, d in ((0, d0), (1, d1)):
                c = [0, 0, 0]
                c[axis], c[au] = p, i
                D[c[2], c[1], c[0]] = d
        D, Wt = D.reshape(-1), np.ones(2 * len(pairs), F32)
        gv = volume_of(tuple(size), D, Wt)
        want = R.project(D, Wt, tuple(size), axis)
        rows = want[0]   # (V, U) = (1, pairs)
        assert rows.shape == (1, len(pairs))
        assert rows[0]["height"].tolist() == want_height and (rows["top"] == 0).all() and (rows["headroom"] == 1).all()
        assert_map(gv.column_map(axis, into=cmap), want, tuple(size), axis, None, False, "axis %d" % axis)
        # reversed the free voxel is below the occupied one: top is the last step, the height its upper face
        want = R.project(D, Wt, tuple(size), axis, None, True)
        assert (want[0]["top"] == 1).all() and (want[0]["height"] == F32(2.0)).all()
        assert_map(gv.column_map(axis, reversed=True, into=cmap), want, tuple(size), axis, None, True, "axis %d reversed" % axis)
        gv.close()
    cmap.close()


def test_the_esdf_minimum():
    size = (33, 31, 17)
    D, Wt = explore_ref.random_state_field(size, 515, 0.5)
    gv = volume_of(size, D, Wt)
    cmap, esdf = tsdf_amd.ColumnMap(), tsdf_amd.ESDF()
    for fill in (False, True):
        gv.compute_esdf(60.0, fill_unknown=fill, into=esdf)
        E = esdf.distances
        assert np.isnan(E).any() != fill
        for axis, band, reversed_ in ((0, None, False), (0, inner_band(33), True), (1, None, True), (1, inner_band(31), False), (2, None, False),
                                      (2, inner_band(17), True)):
            want = R.project(D, Wt, size, axis, band, reversed_, esdf=E)
            what = "fill %s axis %d band %s reversed %s" % (fill, axis, band, reversed_)
            assert_map(gv.column_map(axis, band, reversed_, esdf=esdf, into=cmap), want, size, axis, band, reversed_, what, has_esdf=True)
    gv.close()
    # a plane of sites inside the band: -0.0 behind the surface and +0.0 in front of it, +0.0 in every row whichever is met first
    size = (9, 5, 8)
    D = np.where(np.arange(9 * 5 * 8) // 45 < 4, F32(-0.5), F32(0.5)).astype(F32)
    Wt = np.ones(9 * 5 * 8, F32)
    gv = volume_of(size, D, Wt)
    gv.compute_esdf(into=esdf)
    E = esdf.distances
    zeros = E[E == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    for reversed_ in (False, True):
        # (bands that begin at the plane behind the surface: nothing in them is below zero)
        for band in (None, (3, 5), (3, 8), (3, 4), (4, 6)):
            want = R.project(D, Wt, size, 2, band, reversed_, esdf=E)
            got = assert_map(gv.column_map(2, band, reversed_, esdf=esdf, into=cmap), want, size, 2, band, reversed_, "plane of sites", has_esdf=True)
            if band is not None:
                assert got["min_distance"].view(np.uint32).tolist() == [[0] * 9] * 5
            else:
                assert (got["min_distance"] == F32(-27.0)).all()
    want = R.project(D, Wt, size, 0, None, False, esdf=E)
    got = assert_map(gv.column_map(0, esdf=esdf, into=cmap), want, size, 0, None, False, "plane of sites along x", has_esdf=True)
    assert (got["min_distance"][3:5].view(np.uint32) == 0).all() and (got["min_distance"][:3] < 0).all()
    # refused: an ESDF of another geometry, and one never computed
    other = volume_of((9, 5, 7))
    fresh = tsdf_amd.ESDF()
    for volume, handle, word in ((other, esdf, "another geometry"), (gv, fresh, "never been computed")):
        with pytest.raises(ValueError, match="tsdf_volume_project_columns.*" + word):
            volume.column_map(2, esdf=handle, into=cmap)
    moved = volume_of(size, D, Wt)
    moved.offset(0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="tsdf_volume_project_columns.*another geometry"):
        moved.column_map(2, esdf=esdf, into=cmap)
    for v in (gv, other, moved):
        v.close()
    for h in (cmap, esdf, fresh):
        h.close()


def download(ptr, n):
    host = np.empty(n, np.uint8)
    _capi.check(_capi.lib.tsdf_device_download(host.ctypes.data, C.c_void_p(ptr), n))
    return host


def assert_classes(cmap, rows, what):
    V, U = rows.shape
    for max_step, min_headroom in CLASSIFY:
        want, counts = R.classify(rows, max_step, min_headroom)
        for through in ("host", "device"):
            if through == "host":
                got = cmap.classify(max_step, min_headroom)
            else:
                with _DeviceArray(host=np.full(U * V + 1, 7, np.uint8)) as cells:
                    cmap.classify_device(max_step, min_headroom, cells.ptr.value)
                    got = download(cells.ptr.value, U * V + 1)   # (a blocking copy on the null stream, behind the kernel)
                assert got[-1] == 7
                got = got[:-1].reshape(V, U)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (what, max_step, min_headroom, through)
            i = cmap.info
            assert {k: int(getattr(i, k)) for k in counts} == counts, (what, max_step, min_headroom, through)
            assert (i.max_step, i.min_headroom) == (max_step, min_headroom)
            assert i.n_no_ground + i.n_traversable + i.n_blocked == U * V and i.n_traversable + i.n_blocked == i.n_ground


def test_classification_through_the_device_and_the_host_call():
    cmap = tsdf_amd.ColumnMap()
    for size, axis, reversed_, seed in (((67, 9, 11), 2, False, 31), ((33, 31, 17), 1, True, 32), ((130, 3, 3), 0, False, 33)):
        D, Wt = explore_ref.random_state_field(size, seed, 0.9)
        gv = volume_of(size, D, Wt)
        want = R.project(D, Wt, size, axis, None, reversed_)
        rows = want[0]
        assert_map(gv.column_map(axis, None, reversed_, into=cmap), want, size, axis, None, reversed_, "classify input")
        assert_classes(cmap, rows, "grid %s axis %d" % (size, axis))
        # a new projection forgets the classification
        gv.column_map(axis, None, reversed_, into=cmap)
        i = cmap.info
        assert (i.n_no_ground, i.n_traversable, i.n_blocked, i.max_step, i.min_headroom) == (0, 0, 0, 0, 0)
        gv.close()
    cmap.close()


@pytest.fixture(scope="module")
def fused():
    """Three synthetic frames on 48^3, as tests/test_explore.py::fused makes them: (frames, distances, weights, voxel size, offset)."""
    frames = [synth.depth_frame(i * 9, 40, seed=0x5EEDE5D0) for i in range(3)]
    gv = fused_volume(frames)
    out = frames, gv.get_distance_data(), gv.get_weight_data(), gv.voxel_size(), tuple(gv.offset())
    gv.close()
    return out


def fused_volume(frames, n=48):
    gv = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    for d, cam in frames:
        gv.integrate(d, W, H, cam)
    return gv


def test_a_fused_scene_a_reused_handle_and_a_warm_run(fused):
    frames, D, Wt, vs, offset = fused
    size = (48,) * 3
    cmap = tsdf_amd.ColumnMap()
    assert cmap.scratch_bytes == 64 and tuple(cmap.info.size) == (0, 0, 0)
    gv = fused_volume(frames)
    gv.enable_colour()
    gv.set_colour_data(np.arange(48 ** 3, dtype=np.uint32))
    before = (gv.get_distance_data().tobytes(), gv.get_weight_data().tobytes(), gv.get_colour_data().tobytes(), gv.weight_storage())
    ex = gv.find_frontiers()
    counts = {k: int(getattr(ex.info, k)) for k in ("n_unknown", "n_free", "n_occupied")}
    ex.close()
    results = {}
    for axis in (0, 1, 2):
        want = R.project(D, Wt, size, axis)
        got = assert_map(gv.column_map(axis, into=cmap), want, size, axis, None, False, "fused scene axis %d" % axis)
        results[axis] = got.tobytes()
        i = cmap.info
        assert {k: int(getattr(i, k)) for k in counts} == counts and i.n_ground > 100
        assert np.array_equal(np.array(i.voxel_size, F32), vs) and tuple(i.offset) == offset
        world = cmap.height_world(got)
        assert world.dtype == F32 and world.tobytes() == R.height_world(got, size, axis, None, False, vs, offset).tobytes()
        assert np.isfinite(world).sum() == i.n_ground
    assert cmap.scratch_bytes == 64 + 32 * 48 * 48
    after = (gv.get_distance_data().tobytes(), gv.get_weight_data().tobytes(), gv.get_colour_data().tobytes(), gv.weight_storage())
    assert after == before
    # the same handle on a second, smaller grid and back: the same bytes, and nothing grows on the way back or in a warm second run
    warm, pointer = cmap.scratch_bytes, cmap.device_buffer()
    assert pointer
    field = explore_ref.random_state_field((13, 7, 5), 77, 0.5)
    small = volume_of((13, 7, 5), *field)
    assert_map(small.column_map(1, (1, 6), True, into=cmap), R.project(*field, (13, 7, 5), 1, (1, 6), True), (13, 7, 5), 1, (1, 6), True, "reused on a small grid")
    small.close()
    for run in range(2):
        for axis in (2, 0):
            assert gv.column_map(axis, into=cmap).columns.tobytes() == results[axis], "run %d axis %d" % (run, axis)
            assert (cmap.scratch_bytes, cmap.device_buffer()) == (warm, pointer)
    # the device rows are what the download gives
    host = download(cmap.device_buffer(), 32 * 48 * 48)
    assert host.tobytes() == results[0]
    # the reversed world height of the same surface: hi - height
    rows = gv.column_map(2, (5, 40), True, into=cmap).columns
    assert cmap.height_world(rows).tobytes() == R.height_world(rows, size, 2, (5, 40), True, vs, offset).tobytes()
    gv.close()
    cmap.close()


def test_refusals():
    lib, invalid = _capi.lib, _capi.TSDF_ERR_INVALID
    size = (13, 7, 5)
    gv = volume_of(size, *explore_ref.random_state_field(size, 5, 0.5))
    cmap, empty = tsdf_amd.ColumnMap(), tsdf_amd.ColumnMap()
    cells = np.zeros(13 * 7 + 1, np.uint8)
    rows = np.zeros(13 * 7 + 1, R.COLUMN_DTYPE)

    def refused(rc, name):
        assert rc == invalid, name
        assert name in _capi.last_error(), (name, _capi.last_error())

    project = "tsdf_volume_project_columns"
    # null handle or volume
    refused(lib.tsdf_volume_project_columns(None, 2, 0, 0, None, 0, cmap._h), project)
    refused(lib.tsdf_volume_project_columns(gv._h, 2, 0, 0, None, 0, None), project)
    # the axis and the band: lo >= hi after resolving hi == 0, hi beyond the axis
    for axis, lo, hi in ((3, 0, 0), (0xFFFFFFFF, 0, 0), (2, 5, 0), (2, 3, 3), (2, 4, 3), (2, 0, 6), (0, 13, 0), (0, 0, 14), (1, 7, 8), (1, 0, 0xFFFFFFFF)):
        refused(lib.tsdf_volume_project_columns(gv._h, axis, lo, hi, None, 0, cmap._h), project)
    # unknown flags
    for flags in (2, 4, 8, 0x80000000, 0xFFFFFFFF):
        refused(lib.tsdf_volume_project_columns(gv._h, 2, 0, 0, None, flags, cmap._h), project)
    with pytest.raises(ValueError, match=project):
        gv.column_map(3)
    with pytest.raises(ValueError):
        gv.column_map(2, band=(0, 0))
    # a refusal leaves a fresh handle fresh; classification, buffer and download need a projection
    assert tuple(cmap.info.size) == (0, 0, 0)
    p = C.c_void_p()
    refused(lib.tsdf_columns_classify(empty._h, 0, 0, 0, cells.ctypes.data), "tsdf_columns_classify")
    refused(lib.tsdf_columns_classify_device(empty._h, 0, 0, 0, cells.ctypes.data, None), "tsdf_columns_classify_device")
    refused(lib.tsdf_columns_download(empty._h, rows.ctypes.data), "tsdf_columns_download")
    refused(lib.tsdf_columns_buffer(empty._h, C.byref(p)), "tsdf_columns_buffer")
    # null outputs, unknown classification flags
    gv.column_map(2, into=cmap)
    refused(lib.tsdf_columns_classify(cmap._h, 0, 0, 0, None), "tsdf_columns_classify")
    refused(lib.tsdf_columns_classify_device(cmap._h, 0, 0, 0, None, None), "tsdf_columns_classify_device")
    refused(lib.tsdf_columns_classify(cmap._h, 0, 0, 1, cells.ctypes.data), "tsdf_columns_classify")
    refused(lib.tsdf_columns_classify_device(cmap._h, 0, 0, 1, cells.ctypes.data, None), "tsdf_columns_classify_device")
    refused(lib.tsdf_columns_download(cmap._h, None), "tsdf_columns_download")
    refused(lib.tsdf_columns_buffer(cmap._h, None), "tsdf_columns_buffer")
    refused(lib.tsdf_columns_get_info(cmap._h, None), "tsdf_columns_get_info")
    refused(lib.tsdf_columns_scratch_bytes(cmap._h, None), "tsdf_columns_scratch_bytes")
    # ... and the map is still there
    assert cmap.classify(1, 1).shape == (7, 13)
    # a Z-slab volume and materialised deformation nodes
    slab = tsdf_amd.TSDFVolume((8, 8, 8), (80.0, 80.0, 80.0), slab=(0, 4))
    refused(lib.tsdf_volume_project_columns(slab._h, 2, 0, 0, None, 0, empty._h), project)
    moved = volume_of(size, *explore_ref.random_state_field(size, 5, 0.5))
    nodes = C.c_void_p()
    _capi.check(lib.tsdf_volume_deformation(moved._h, C.byref(nodes)))
    refused(lib.tsdf_volume_project_columns(moved._h, 2, 0, 0, None, 0, empty._h), project)
    assert tuple(empty.info.size) == (0, 0, 0) and empty.scratch_bytes == 64
    for v in (gv, slab, moved):
        v.close()
    cmap.close()
    empty.close()
    lib.tsdf_columns_destroy(None)
