"""GPU: the exploration queries (include/tsdf_amd.h, "exploration") against the CPU reference tests/explore_ref.py.  Every comparison
is equality of integers or bytes.  Random state fields with NaN and -0.0 distances (and NaN weights in fp32 storage) on grids whose
64-voxel chunks straddle rows and planes and end partial, in all three weight storages, both connectivities and four min_size
values; a 200-voxel snake and a half-observed 32^3 for deep union-find chains; a small fused scene, a reused handle and a warm run;
that the volume is left alone; view gain for axis rays, corner ties, rays from outside, inside, faces and corners, every decreed skip,
range limits, duplicates, the keep flag, the host twin against the device call; and the refusals."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import explore_ref as R
from tests.helpers import H, W
from tsdf_amd import _capi, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
# one voxel; 64-voxel chunks that straddle rows with a partial last chunk; exactly two chunks of one row each plane; a row one longer than a
# chunk; rows of two chunks and two voxels (several chunks a plane); and, because a wave of the flag kernel walks 64 chunks, 104 chunks:
# a full wave and part of a second (the fused 48^3 below: 27 waves, six workgroups and three quarters of one); and 17 391 voxels in 272
# chunks: a second workgroup whose first wave walks 16 chunks while its other three walk none, and a last chunk of 47 voxels
GRIDS = [(1, 1, 1), (13, 7, 5), (64, 3, 2), (65, 4, 3), (130, 3, 3), (67, 9, 11), (33, 31, 17)]
DENSITIES = [0.0, 0.1, 0.5, 0.9, 1.0]
OFFSET = (100.0, -50.0, 25.0)
VS = np.array([10.0, 12.5, 9.0], F32)


def volume_of(size, D=None, Wt=None):
    """Anisotropic voxels (10 x 12.5 x 9 mm) and an offset, as tests/test_esdf.py::volume_of makes them."""
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


def assert_frontiers(ex, D, Wt, size, what):
    ids, counts = R.frontiers(D, Wt, size)
    i = ex.info
    got = {k: int(getattr(i, k)) for k in counts}
    assert got == counts, (what, got, counts)
    assert tuple(i.size) == tuple(size) and i.connectivity == 0
    assert np.array_equal(ex.voxels, ids), what
    return ids


def assert_clusters(ex, ids, size, connectivity, min_size, what):
    labels, rows, n_clusters = R.clusters(ids, size, connectivity, min_size)
    assert ex.cluster(connectivity, min_size) is ex
    i = ex.info
    assert (i.connectivity, i.n_clusters, i.n_listed_clusters) == (connectivity, n_clusters, len(rows)), what
    assert np.array_equal(ex.labels, labels), what
    got = ex.clusters
    assert got.dtype == R.CLUSTER_DTYPE and got.tobytes() == rows.tobytes(), what
    return rows


@pytest.mark.parametrize("size", GRIDS)
def test_random_state_fields_equal_the_reference(size):
    ex = tsdf_amd.Explorer()
    seed = 7000 + size[0] + 3 * size[2]
    for k, density in enumerate(DENSITIES):
        for bits in (8, 16, 32):
            # fp32 storage also gets NaN and fractional weights (a packed count cannot hold them)
            D, Wt = R.random_state_field(size, seed + k, density, fp32_oddities=bits == 32)
            gv = volume_of(size, D, Wt)
            widen(gv, bits)
            what = "grid %s density %s %d-bit weights" % (size, density, bits)
            assert gv.find_frontiers(into=ex) is ex
            ids = assert_frontiers(ex, D, Wt, size, what)
            assert gv.weight_storage()[0] == bits
            for connectivity in (6, 26):
                biggest = 0
                for min_size in (0, 1, 3):
                    rows = assert_clusters(ex, ids, size, connectivity, min_size, "%s connectivity %d min_size %d" % (what, connectivity, min_size))
                    biggest = max([biggest] + rows["size"].tolist())
                assert len(assert_clusters(ex, ids, size, connectivity, biggest + 1, what + " min_size above every cluster")) == 0
            gv.close()
    n = size[0] * size[1] * size[2]
    assert ex.scratch_bytes >= 12 * ((n + 63) // 64)
    ex.close()


def test_sixty_four_roots_in_a_wave_and_a_one_lane_wave():
    """130 x 1 x 1, free at even x and unknown at odd x: 65 frontiers, none adjacent to another, so the first wave of the stats kernel
    reduces 64 distinct roots and the second has one lane."""
    size = (130, 1, 1)
    D = np.full(130, 0.5, F32)
    Wt = (np.arange(130) % 2 == 0).astype(F32)
    gv = volume_of(size, D, Wt)
    ex = gv.find_frontiers()
    ids = assert_frontiers(ex, D, Wt, size, "every other voxel")
    assert ids.tolist() == list(range(0, 130, 2))
    for connectivity in (6, 26):
        rows = assert_clusters(ex, ids, size, connectivity, 1, "every other voxel at %d" % connectivity)
        assert len(rows) == 65 and (rows["size"] == 1).all() and rows["sum"][:, 0].tolist() == list(range(0, 130, 2))
    gv.close()
    ex.close()


def test_a_snake_and_a_half_observed_cube_give_deep_chains():
    # one row of 200 free voxels under a row of unknown ones: a single cluster, 200 long, whatever the order the hooks land in
    size = (200, 2, 1)
    D = np.full(400, 0.5, F32)
    Wt = np.concatenate([np.ones(200, F32), np.zeros(200, F32)])
    gv = volume_of(size, D, Wt)
    ex = gv.find_frontiers()
    ids = assert_frontiers(ex, D, Wt, size, "snake")
    assert ids.tolist() == list(range(200))
    for connectivity in (6, 26):
        rows = assert_clusters(ex, ids, size, connectivity, 1, "snake at %d" % connectivity)
        assert len(rows) == 1 and rows[0]["size"] == 200 and rows[0]["sum"].tolist() == [199 * 100, 0, 0]
    gv.close()
    # a serpentine: rows of frontiers joined at alternating ends, so the one cluster's smallest index is far from most of its voxels
    size = (40, 9, 1)
    Wt = np.ones((9, 40), F32)
    for y in range(1, 9, 2):
        Wt[y, :] = 0.0
        Wt[y, 39 if (y // 2) % 2 == 0 else 0] = 1.0
    D = np.full(360, 0.25, F32)
    gv = volume_of(size, D, Wt.reshape(-1))
    ids = assert_frontiers(gv.find_frontiers(into=ex), D, Wt.reshape(-1), size, "serpentine")
    for connectivity in (6, 26):
        assert_clusters(ex, ids, size, connectivity, 1, "serpentine at %d" % connectivity)
    gv.close()
    size = (32, 32, 32)
    D, Wt = R.random_state_field(size, 4242, 0.5)
    gv = volume_of(size, D, Wt)
    ids = assert_frontiers(gv.find_frontiers(into=ex), D, Wt, size, "half-observed 32^3")
    assert len(ids) > 5000
    for connectivity in (6, 26):
        rows = assert_clusters(ex, ids, size, connectivity, 2, "half-observed 32^3 at %d" % connectivity)
        # (by the CPU reference: face neighbours alone do not percolate at this density, with edges and corners nearly all join up)
        assert rows["size"].max() > (100 if connectivity == 6 else 5000)
    gv.close()
    ex.close()


@pytest.fixture(scope="module")
def fused():
    """Three synthetic frames on 48^3: (frames, distances, weights, voxel size) of the device's own integration."""
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
    ex = tsdf_amd.Explorer()
    assert ex.scratch_bytes == 64 and ex.info.n_frontiers == 0
    results = {}
    for bits in (8, 16, 32):
        gv = fused_volume(frames)
        widen(gv, bits)
        ids = assert_frontiers(gv.find_frontiers(into=ex), D, Wt, size, "fused scene, %d-bit weights" % bits)
        assert len(ids) > 1000 and ex.info.n_occupied > 100 and ex.info.n_unknown > 1000
        rows = assert_clusters(ex, ids, size, 26, 5, "fused scene, %d-bit weights" % bits)
        results[bits] = (ex.voxels.tobytes(), ex.labels.tobytes(), rows.tobytes())
        assert results[bits] == results[8]
        # the world positions: voxel centres, and the centroid from the exact sums
        c = R.coordinates(ids, size)
        assert np.array_equal(ex.coordinates, c.astype(np.uint32))
        assert np.array_equal(ex.points, ((c.astype(F32) + F32(0.5)) * vs + np.array(offset, F32)).astype(F32))
        assert np.array_equal(ex.centroids, (rows["sum"] / rows["size"][:, None] + 0.5) * vs.astype(np.float64) + np.array(offset, np.float64))
        gv.close()
    # the same handle on a small grid and back: the same bytes, and no array grows on the way back or in a warm second run
    gv = fused_volume(frames)
    warm = ex.scratch_bytes
    small = volume_of((13, 7, 5), *R.random_state_field((13, 7, 5), 77, 0.5))
    ids_small = assert_frontiers(small.find_frontiers(into=ex), *R.random_state_field((13, 7, 5), 77, 0.5), (13, 7, 5), "reused on a small grid")
    assert_clusters(ex, ids_small, (13, 7, 5), 6, 1, "reused on a small grid")
    small.close()
    for run in range(2):
        gv.find_frontiers(into=ex).cluster(26, 5)
        assert (ex.voxels.tobytes(), ex.labels.tobytes(), ex.clusters.tobytes()) == results[8], "run %d" % run
        assert ex.scratch_bytes == warm
    bufs = ex.device_buffers()
    assert all(bufs[k] for k in ("voxels", "masks", "bases", "labels", "clusters"))
    host = np.empty(ex.info.n_frontiers, np.uint32)
    _capi.check(_capi.lib.tsdf_device_download(host.ctypes.data, C.c_void_p(bufs["voxels"]), host.nbytes))
    assert host.tobytes() == results[8][0]
    gv.close()
    ex.close()


def test_the_volume_is_left_alone(fused):
    frames = fused[0]
    gv = fused_volume(frames)
    gv.enable_colour()
    gv.set_colour_data(np.arange(48 ** 3, dtype=np.uint32))
    cam = frames[1][1]
    v0, n0 = gv.raycast(W, H, cam)
    kind0 = gv.last_raycast_cell_parallel()
    before = (gv.get_distance_data().tobytes(), gv.get_weight_data().tobytes(), gv.get_colour_data().tobytes(), gv.weight_storage())
    ex = gv.find_frontiers().cluster(26, 1)
    o, d = tsdf_amd.pixel_rays(cam, W, H, 16)
    assert len(o) == (W // 16) * (H // 16)
    gain = gv.view_gain(o, d, explorer=ex)[0]
    assert gain > 0 and ex.info.n_frontiers > 0
    after = (gv.get_distance_data().tobytes(), gv.get_weight_data().tobytes(), gv.get_colour_data().tobytes(), gv.weight_storage())
    assert after == before
    assert gv.last_raycast_cell_parallel() == kind0
    v1, n1 = gv.raycast(W, H, cam)
    assert gv.last_raycast_cell_parallel() == kind0
    assert v1.tobytes() == v0.tobytes() and n1.tobytes() == n0.tobytes()
    assert (~np.isnan(v0[:, 0])).sum() > 1000
    ex.close()
    gv.close()


# ---- view gain ---------------------------------------------------------------------------------------------------------------------
GAIN_GRID = (13, 7, 5)


def gain_rays():
    """Rays in the frame of volume_of(GAIN_GRID): (origins, directions), float32."""
    off, vs, N = np.array(OFFSET, np.float64), VS.astype(np.float64), np.array(GAIN_GRID)
    at = lambda *voxel: off + np.array(voxel, np.float64) * vs            # a point given in voxel units
    rays = []
    # axis rays through voxel centres, both ways, from outside and from inside (two s_k are 0)
    for axis in range(3):
        for sign in (1.0, -1.0):
            dirn = np.zeros(3)
            dirn[axis] = sign
            start = np.array([6.5, 3.5, 2.5])
            rays.append((at(*start), dirn))
            start[axis] = -2.25 if sign > 0 else N[axis] + 2.25
            rays.append((at(*start), 3.0 * dirn))
    # axis rays that miss (a_k outside with s_k == 0), and one exactly on the upper face (a_k == N_k: outside)
    rays += [(at(-3.0, 9.0, 2.5), (1.0, 0.0, 0.0)), (at(6.5, 3.5, 5.0), (1.0, 0.0, 0.0)), (at(6.5, 0.0, 2.5), (1.0, 0.0, 0.0))]
    # corner-tie diagonals: from a lattice corner inside, from the grid's own corner, from outside through corners, and backwards
    cube = np.array([1.0, 1.0, 1.0]) * vs
    rays += [(at(2, 1, 1), cube), (at(0, 0, 0), cube), (at(-2, -2, -2), cube), (at(5, 5, 5), -cube), (at(13, 7, 5), -cube),
             (at(3, 2, 0), cube * np.array([1.0, -1.0, 1.0])), (at(0, 3, 2), cube * np.array([1.0, 1.0, 0.0]))]
    # starts on a face and on an edge, inwards and outwards; non-unit and tiny directions
    rays += [(at(0, 3.5, 2.5), (1.0, 0.2, 0.1)), (at(0, 3.5, 2.5), (-1.0, 0.2, 0.1)), (at(13, 7, 2.5), (-1.0, -1.0, 0.01)),
             (at(6.5, 3.5, 2.5), (250.0, -120.0, 33.0)), (at(6.5, 3.5, 2.5), (1e-3, 2e-3, -1e-3)), (at(6.5, 3.5, 2.5), (1e-30, 0.0, 0.0))]
    # rays that miss the grid altogether, and one that points away from it
    rays += [(at(-5, -5, -5), (1.0, -1.0, 0.0)), (at(20, 3, 2), (0.0, 1.0, 0.0)), (at(-1, 3, 2), (-1.0, 0.1, 0.0))]
    # every decreed skip
    nan, inf = np.nan, np.inf
    rays += [((nan, 0, 0), (1, 0, 0)), ((0, inf, 0), (1, 0, 0)), ((0, 0, -inf), (1, 0, 0)), (at(6.5, 3.5, 2.5), (nan, 1, 0)),
             (at(6.5, 3.5, 2.5), (1, inf, 0)), (at(6.5, 3.5, 2.5), (0.0, 0.0, 0.0)), (at(6.5, 3.5, 2.5), (-0.0, 0.0, -0.0)),
             ((3e38, 0, 0), (1, 0, 0)), (at(6.5, 3.5, 2.5), (3e38, 3e38, 0.0))]
    rng = np.random.default_rng(99)
    for _ in range(40):      # from in and around the grid towards a point inside it, at three scales of the direction
        start, target = rng.uniform(-2.0, N + 2.0), rng.uniform(0.0, N)
        rays.append((at(*start), (target - start) * vs * rng.choice([0.01, 1.0, 40.0])))
    o = np.array([r[0] for r in rays], F32)
    d = np.array([r[1] for r in rays], F32)
    return o, d


@pytest.fixture(scope="module")
def gain_field():
    D, Wt = R.random_state_field(GAIN_GRID, 31337, 0.45)
    D[D < 0] = np.where(np.random.default_rng(5).random((D < 0).sum()) < 0.75, F32(0.3), D[D < 0])   # fewer walls: longer walks
    centre = (2 * GAIN_GRID[1] + 3) * GAIN_GRID[0] + 6                 # voxel (6, 3, 2), where the axis rays start: observed and free
    D[centre], Wt[centre] = F32(0.5), F32(2.0)
    return D, Wt, R.states(D, Wt)


def ref_gain(state, o, d, t=None, mask=None):
    return R.view_gain(state, GAIN_GRID, VS, OFFSET, o, d, t, mask)


def assert_gain(got, ref, what):
    assert got[0] == ref[0], (what, got[0], ref[0])
    for k, name in ((1, "unknown"), (2, "free"), (3, "stop")):
        assert np.array_equal(got[k], ref[k]), (what, name, np.flatnonzero(got[k] != ref[k])[:8])


def test_view_gain_equals_the_reference_ray_for_ray(gain_field):
    D, Wt, state = gain_field
    o, d = gain_rays()
    n = len(o)
    ref = ref_gain(state, o, d)
    assert (ref[3] == 0).sum() >= 9 and (ref[3] == 1).sum() > 10 and (ref[3] == 2).sum() > 5 and ref[0] > 20
    rng = np.random.default_rng(3)
    limits = {"none": None, "tiny": np.full(n, 1e-6, F32), "mid-voxel": rng.uniform(0.2, 60.0, n).astype(F32), "inf": np.full(n, np.inf, F32),
              "mixed": rng.choice(np.array([np.nan, 0.0, -1.0, 5.0, 1e9, np.inf], F32), n)}
    for bits in (8, 16, 32):
        gv = volume_of(GAIN_GRID, D, Wt)
        widen(gv, bits)
        fresh = tsdf_amd.Explorer()
        after = gv.find_frontiers()
        for name, t in limits.items():
            want = ref_gain(state, o, d, t)
            for ex, which in ((fresh, "a fresh handle"), (after, "a handle after find_frontiers")):
                assert_gain(gv.view_gain(o, d, t, explorer=ex), want, "%d-bit weights, t_max %s, %s" % (bits, name, which))
        assert_gain(gv.view_gain(o, d), ref, "a private handle")
        assert after.info.n_frontiers == len(R.frontiers(D, Wt, GAIN_GRID)[0])     # the list is still the handle's
        fresh.close()
        after.close()
        gv.close()


def test_view_gain_counts_duplicates_once_keeps_its_mask_and_takes_any_n(gain_field):
    D, Wt, state = gain_field
    o, d = gain_rays()
    gv = volume_of(GAIN_GRID, D, Wt)
    ex = tsdf_amd.Explorer()
    # n in {0, 1, 64, 257}: tiled rays, more than one workgroup
    for n in (0, 1, 64, 257):
        idx = np.arange(n) % len(o)
        assert_gain(gv.view_gain(o[idx], d[idx], explorer=ex), ref_gain(state, o[idx], d[idx]), "n = %d" % n)
    assert gv.view_gain(o[:0], d[:0], explorer=ex)[0] == 0
    # duplicates of one ray: the gain is that ray's count
    k = int(np.argmax(ref_gain(state, o, d)[1]))
    one = gv.view_gain(o[k:k + 1], d[k:k + 1], explorer=ex)
    many = gv.view_gain(np.repeat(o[k:k + 1], 70, axis=0), np.repeat(d[k:k + 1], 70, axis=0), explorer=ex)
    assert one[0] == many[0] == int(one[1][0]) > 1 and (many[1] == one[1][0]).all()
    # keep: the union over two calls; without it the mask restarts; n == 0 with keep counts what is there
    half = len(o) // 2
    a = ref_gain(state, o[:half], d[:half])
    b = ref_gain(state, o[half:], d[half:])
    union = ref_gain(state, o[half:], d[half:], mask=a[4])
    assert union[0] == len(a[4] | b[4]) > max(a[0], b[0])
    assert_gain(gv.view_gain(o[:half], d[:half], explorer=ex), a, "first half")
    assert_gain(gv.view_gain(o[half:], d[half:], explorer=ex, keep=True), union, "second half, kept")
    assert gv.view_gain(o[:0], d[:0], explorer=ex, keep=True)[0] == union[0]
    assert_gain(gv.view_gain(o[half:], d[half:], explorer=ex), b, "second half, restarted")
    assert gv.view_gain(o[:0], d[:0], explorer=ex)[0] == 0
    # a find_frontiers of the same grid between two kept calls leaves the mask alone
    gv.view_gain(o[:half], d[:half], explorer=ex)
    gv.find_frontiers(into=ex)
    assert_gain(gv.view_gain(o[half:], d[half:], explorer=ex, keep=True), union, "kept across find_frontiers")
    ex.close()
    gv.close()


class DeviceArray:
    def __init__(self, host=None, nbytes=0):
        self.p = C.c_void_p()
        self.nbytes = host.nbytes if host is not None else nbytes
        _capi.check(_capi.lib.tsdf_device_alloc(max(self.nbytes, 4), C.byref(self.p)))
        if host is not None and host.nbytes:
            _capi.check(_capi.lib.tsdf_device_upload(self.p, host.ctypes.data, host.nbytes))

    def get(self, dtype):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype)
        if out.nbytes:
            _capi.check(_capi.lib.tsdf_device_download(out.ctypes.data, self.p, out.nbytes))
        return out

    def free(self):
        _capi.lib.tsdf_device_free(self.p)


def test_the_host_twin_equals_the_device_call(gain_field):
    D, Wt, state = gain_field
    o, d = gain_rays()
    n = len(o)
    t = np.random.default_rng(8).uniform(0.5, 90.0, n).astype(F32)
    gv = volume_of(GAIN_GRID, D, Wt)
    ex = tsdf_amd.Explorer()
    host = gv.view_gain(o, d, t, explorer=ex)
    assert_gain(host, ref_gain(state, o, d, t), "host twin")
    do, dd, dt = DeviceArray(o), DeviceArray(d), DeviceArray(t)
    du, df, ds = DeviceArray(nbytes=4 * n), DeviceArray(nbytes=4 * n), DeviceArray(nbytes=n)
    gain = gv.view_gain_device(ex, n, do.p.value, dd.p.value, dt.p.value, du.p.value, df.p.value, ds.p.value)
    assert_gain((gain, du.get(np.uint32), df.get(np.uint32), ds.get(np.uint8)), host, "device call")
    # any output may be NULL: the gain alone, and one array alone without the count (asynchronous: the next blocking call orders it)
    assert gv.view_gain_device(ex, n, do.p.value, dd.p.value, dt.p.value) == host[0]
    du2 = DeviceArray(nbytes=4 * n)
    assert gv.view_gain_device(ex, n, do.p.value, dd.p.value, None, unknown_ptr=du2.p.value, gain=False) is None
    gv.synchronize()
    assert np.array_equal(du2.get(np.uint32), ref_gain(state, o, d)[1])
    for a in (do, dd, dt, du, df, ds, du2):
        a.free()
    ex.close()
    gv.close()


def test_refusals(gain_field):
    D, Wt, _ = gain_field
    lib, invalid = _capi.lib, _capi.TSDF_ERR_INVALID
    gv = volume_of(GAIN_GRID, D, Wt)
    ex = tsdf_amd.Explorer()
    o, d = gain_rays()
    u = np.zeros(len(o) + 1, np.uint32)
    g = C.c_uint64(0)

    def refused(rc, name):
        assert rc == invalid, name
        assert name in _capi.last_error(), (name, _capi.last_error())

    gain = lambda v, e, n, op, dp, flags, up, gp: lib.tsdf_volume_view_gain(v, e, n, op, dp, None, flags, up, None, None, gp)
    gain_device = lambda v, e, n, op, dp, flags, up, gp: lib.tsdf_volume_view_gain_device(v, e, n, op, dp, None, flags, up, None, None, gp)
    # null handles and volumes
    refused(lib.tsdf_volume_find_frontiers(None, 0, ex._h), "tsdf_volume_find_frontiers")
    refused(lib.tsdf_volume_find_frontiers(gv._h, 0, None), "tsdf_volume_find_frontiers")
    for call, name in ((gain, "tsdf_volume_view_gain"), (gain_device, "tsdf_volume_view_gain_device")):
        refused(call(None, ex._h, 1, o.ctypes.data, d.ctypes.data, 0, u.ctypes.data, C.byref(g)), name)
        refused(call(gv._h, None, 1, o.ctypes.data, d.ctypes.data, 0, u.ctypes.data, C.byref(g)), name)
        # unknown flags, null rays with n > 0, no output at all, more rays than a launch holds
        refused(call(gv._h, ex._h, 1, o.ctypes.data, d.ctypes.data, 2, u.ctypes.data, C.byref(g)), name)
        refused(call(gv._h, ex._h, 1, None, d.ctypes.data, 0, u.ctypes.data, C.byref(g)), name)
        refused(call(gv._h, ex._h, 1, o.ctypes.data, None, 0, u.ctypes.data, C.byref(g)), name)
        refused(call(gv._h, ex._h, 1, o.ctypes.data, d.ctypes.data, 0, None, None), name)
        refused(call(gv._h, ex._h, (2 ** 31 - 1) * 256 + 1, o.ctypes.data, d.ctypes.data, 0, u.ctypes.data, C.byref(g)), name)
        # n == 0 is fine, with null rays too
        assert call(gv._h, ex._h, 0, None, None, 0, None, C.byref(g)) == _capi.TSDF_OK and g.value == 0
    refused(lib.tsdf_volume_find_frontiers(gv._h, 1, ex._h), "tsdf_volume_find_frontiers")
    # a handle that holds nothing yet / is not clustered
    empty = tsdf_amd.Explorer()
    refused(lib.tsdf_explorer_cluster_frontiers(empty._h, 26, 1, None), "tsdf_explorer_cluster_frontiers")
    refused(lib.tsdf_explorer_frontier_download(empty._h, u.ctypes.data), "tsdf_explorer_frontier_download")
    refused(lib.tsdf_explorer_frontier_buffers(empty._h, None, None, None), "tsdf_explorer_frontier_buffers")
    gv.find_frontiers(into=ex)
    refused(lib.tsdf_explorer_cluster_buffers(ex._h, None, None), "tsdf_explorer_cluster_buffers")
    refused(lib.tsdf_explorer_cluster_download(ex._h, u.ctypes.data, None), "tsdf_explorer_cluster_download")
    for connectivity in (0, 4, 8, 18, 27):
        refused(lib.tsdf_explorer_cluster_frontiers(ex._h, connectivity, 1, None), "tsdf_explorer_cluster_frontiers")
    ex.cluster(6, 1)
    gv.find_frontiers(into=ex)          # ... and the labels are stale again
    refused(lib.tsdf_explorer_cluster_download(ex._h, u.ctypes.data, None), "tsdf_explorer_cluster_download")
    # a handle of another geometry: another size, another offset; a fresh handle adopts the volume's
    other = volume_of((12, 7, 5), *R.random_state_field((12, 7, 5), 1, 0.5))
    for call, name in ((gain, "tsdf_volume_view_gain"), (gain_device, "tsdf_volume_view_gain_device")):
        refused(call(other._h, ex._h, 0, None, None, 0, None, C.byref(g)), name)
    moved = volume_of(GAIN_GRID, D, Wt)
    moved.offset(0.0, 0.0, 0.0)
    refused(gain(moved._h, ex._h, 0, None, None, 0, None, C.byref(g)), "tsdf_volume_view_gain")
    assert gain(other._h, empty._h, 0, None, None, 0, None, C.byref(g)) == _capi.TSDF_OK
    assert tuple(empty.info.size) == (12, 7, 5)
    refused(gain(gv._h, empty._h, 0, None, None, 0, None, C.byref(g)), "tsdf_volume_view_gain")
    other.find_frontiers(into=ex)       # find_frontiers re-targets a handle
    assert tuple(ex.info.size) == (12, 7, 5)
    # a Z-slab volume and materialised deformation nodes
    slab = tsdf_amd.TSDFVolume((8, 8, 8), (80.0, 80.0, 80.0), slab=(0, 4))
    refused(lib.tsdf_volume_find_frontiers(slab._h, 0, empty._h), "tsdf_volume_find_frontiers")
    spare = tsdf_amd.Explorer()         # (a refusal leaves a fresh handle fresh)
    refused(gain(slab._h, spare._h, 0, None, None, 0, None, C.byref(g)), "tsdf_volume_view_gain")
    nodes = C.c_void_p()
    _capi.check(lib.tsdf_volume_deformation(moved._h, C.byref(nodes)))
    refused(lib.tsdf_volume_find_frontiers(moved._h, 0, spare._h), "tsdf_volume_find_frontiers")
    refused(gain(moved._h, spare._h, 0, None, None, 0, None, C.byref(g)), "tsdf_volume_view_gain")
    assert tuple(spare.info.size) == (0, 0, 0)
    spare.close()
    with pytest.raises(ValueError, match="tsdf_explorer_cluster_frontiers"):
        ex.cluster(7)
    for v in (gv, other, moved, slab):
        v.close()
    ex.close()
    empty.close()
