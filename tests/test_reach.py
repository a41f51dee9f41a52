"""GPU: the reachability group (include/tsdf_amd.h, "reachability") against the CPU reference tests/reach_ref.py.  Every comparison is
equality of integers or bytes.  Random state fields with NaN and -0.0 distances (NaN and fractional weights in fp32 storage) on grids
of one voxel, exactly one brick of 8^3, a second brick one voxel thick, partial bricks on every axis and 27 bricks, at three densities
in the three weight storages, both connectivities, 1, 3 and 64 seeds with NaN, off-grid and blocked ones, with and without
TSDF_REACH_THROUGH_UNKNOWN and three caps; a serpentine whose one corridor crosses brick borders dozens of times; corner steps whose
2 x 2 x 2 block spans eight bricks; clearance from an ESDF of a fused scene; lookup, paths and ranking; that nothing read is written;
a warm and a reused handle; two runs; and the refusals."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import explore_ref as E
from tests import reach_ref as R
from tests.helpers import H, W
from tsdf_amd import _capi, synth
from tsdf_amd.api import _DeviceArray

pytestmark = pytest.mark.gpu

F32 = np.float32
U = R.UNREACHED
# (the last: 17 391 voxels in 272 chunks of 64 ids, so the flag walk has a second workgroup whose first wave walks 16 chunks while its
# other three walk none, and a last chunk of 47 voxels; 5 x 4 x 3 bricks, partial on every axis)
GRIDS = [(1, 1, 1), (8, 8, 8), (9, 8, 8), (8, 8, 9), (13, 7, 5), (17, 9, 10), (65, 4, 3), (24, 24, 24), (33, 31, 17)]
DENSITIES = [0.1, 0.5, 0.9]
CAPS = [0, 35, 400]
OFFSET = (100.0, -50.0, 25.0)
VS = np.array([10.0, 12.5, 9.0], F32)


def volume_of(size, D=None, Wt=None, offset=OFFSET):
    """Anisotropic voxels (10 x 12.5 x 9 mm) and an offset, as tests/test_explore.py::volume_of makes them."""
    gv = tsdf_amd.TSDFVolume(size, (size[0] * 10.0, size[1] * 12.5, size[2] * 9.0))
    gv.offset(*offset)
    assert np.array_equal(gv.voxel_size(), VS)
    if D is not None:
        gv.set_distance_data(D)
        gv.set_weight_data(Wt)
    return gv


def widen(gv, bits):
    if gv.weight_storage()[0] != bits:
        gv.set_weight_storage(bits)
    assert gv.weight_storage()[0] == bits


def centres(ids, size, vs=VS, offset=OFFSET):
    return R.centres(np.asarray(ids, np.int64), size, vs, offset)


def seeds_for(trav, size, n, rng):
    """n seed points: 1 -- the centre of a traversable voxel where there is one; 3 -- that, a NaN and a point off the grid; 64 -- points
    anywhere in and just outside the grid (so some fall into blocked voxels and some off it), voxel corners among them, and a NaN."""
    N = np.array(size, np.float64)
    open_ids = np.flatnonzero(trav)
    first = centres([rng.choice(open_ids) if len(open_ids) else 0], size)[0]
    if n == 1:
        return first[None, :]
    lo, vs = np.array(OFFSET, np.float64), VS.astype(np.float64)
    if n == 3:
        return np.array([first, (np.nan, 0.0, 0.0), lo + (N + 0.5) * vs], F32)
    p = lo + rng.uniform(-0.5, N + 0.5, (n, 3)) * vs
    p[:8] = lo + np.floor(rng.uniform(0.0, N, (8, 3))) * vs        # on the lower corner of a voxel: the floor decides
    p[8] = (np.inf, p[8][1], p[8][2])
    p[9] = (p[9][0], np.nan, p[9][2])
    return p.astype(F32)


def assert_reach(gv, reach, trav, size, seeds, connectivity, max_cost, what, **kw):
    want, seed_ids = R.cost_field(trav, size, VS, OFFSET, seeds, connectivity, max_cost)
    assert gv.reach(seeds, connectivity, max_cost=max_cost, into=reach, **kw) is reach
    got = reach.costs
    assert got.dtype == np.uint32 and np.array_equal(got, want), (what, np.flatnonzero(got != want)[:10], got[got != want][:10], want[got != want][:10])
    i = reach.info
    counts = R.info(trav, want)
    assert {k: int(getattr(i, k)) for k in counts} == counts, what
    assert tuple(i.size) == tuple(size) and i.connectivity == connectivity and i.max_cost == max_cost, what
    assert np.array_equal(np.array(i.voxel_size, F32), VS) and tuple(i.offset) == OFFSET, what
    assert 1 <= i.rounds <= counts["n_traversable"] + 1, what
    return want, seed_ids


@pytest.mark.parametrize("size", GRIDS)
def test_random_state_fields_equal_the_reference(size):
    reach = tsdf_amd.Reach()
    n = size[0] * size[1] * size[2]
    rng = np.random.default_rng(500 + n)
    # 18 fields: every density in every storage twice, while connectivity, seed count, the flag and the cap rotate through all their
    # values beside them.  The two largest grids, whose references take longest, take six of them: every value of every factor.  (Every
    # combination of the six factors meets in test_every_combination_on_one_grid below.)
    seen = set()
    for c in (range(18) if n <= 2000 else (0, 1, 4, 7, 11, 14)):
        d, bits, connectivity = (c // 3) % 3, (8, 16, 32)[c % 3], (6, 26)[c % 2]
        n_seeds, through, cap = (1, 3, 64)[(c + c // 3) % 3], bool((c // 2) % 2), CAPS[(c // 6 + c) % 3]
        seen |= {("d", d), ("b", bits), ("c", connectivity), ("s", n_seeds), ("t", through), ("m", cap)}
        D, Wt = E.random_state_field(size, 9000 + 31 * c + n, DENSITIES[d], fp32_oddities=bits == 32)
        gv = volume_of(size, D, Wt)
        widen(gv, bits)
        trav = R.traversable(D, Wt, through)
        seeds = seeds_for(trav, size, n_seeds, rng)
        what = "grid %s density %s %d-bit weights connectivity %d %d seeds through %s cap %d" % (size, DENSITIES[d], bits, connectivity, n_seeds, through, cap)
        assert_reach(gv, reach, trav, size, seeds, connectivity, cap, what, through_unknown=through)
        assert reach.info.flags == (1 if through else 0) and gv.weight_storage()[0] == bits
        gv.close()
    assert len(seen) == 16
    reach.close()


@pytest.mark.parametrize("density", DENSITIES)
def test_every_combination_on_one_grid(density):
    """13 x 7 x 5 (two bricks along x, partial on every axis): the three storages x both connectivities x 1, 3 and 64 seeds x the flag x
    the three caps, 108 fields a density, one volume per storage."""
    size = (13, 7, 5)
    reach = tsdf_amd.Reach()
    rng = np.random.default_rng(int(density * 100))
    count = 0
    for bits in (8, 16, 32):
        D, Wt = E.random_state_field(size, 600 + bits + int(density * 10), density, fp32_oddities=bits == 32)
        gv = volume_of(size, D, Wt)
        widen(gv, bits)
        for through in (False, True):
            trav = R.traversable(D, Wt, through)
            for n_seeds in (1, 3, 64):
                seeds = seeds_for(trav, size, n_seeds, rng)
                for connectivity in (6, 26):
                    for cap in CAPS:
                        what = "density %s %d-bit weights connectivity %d %d seeds through %s cap %d" % (density, bits, connectivity, n_seeds, through, cap)
                        assert_reach(gv, reach, trav, size, seeds, connectivity, cap, what, through_unknown=through)
                        count += 1
        assert gv.weight_storage()[0] == bits
        gv.close()
    assert count == 108
    reach.close()


def test_no_seeds_and_a_grid_without_a_traversable_voxel():
    size = (13, 7, 5)
    D, Wt = E.random_state_field(size, 11, 0.5)
    gv = volume_of(size, D, Wt)
    reach = gv.reach(np.zeros((0, 3), F32))
    i = reach.info
    assert np.all(reach.costs == U) and (i.n_reached, i.n_seed_voxels, i.max_cost_reached, i.rounds) == (0, 0, 0, 1)
    assert i.n_traversable == int(R.traversable(D, Wt).sum())
    gv.set_distance_data(np.full(13 * 7 * 5, -1.0, F32))
    gv.set_weight_data(np.ones(13 * 7 * 5, F32))
    gv.reach(centres([0, 100], size), into=reach)
    assert np.all(reach.costs == U) and reach.info.n_traversable == 0 and reach.info.rounds == 1
    reach.close()
    gv.close()


def serpentine():
    """24^3: free slabs x = 0, 2, ..., 22 between occupied walls x = 1, 3, ..., 23, each wall with one free voxel -- at (y, z) = (23, 23) and
    (0, 0) in turn -- so the one corridor crosses every slab from corner to corner."""
    size = (24, 24, 24)
    D = np.full((24, 24, 24), 0.5, F32)   # [z][y][x]
    for k, x in enumerate(range(1, 24, 2)):
        D[:, :, x] = -0.5
        gap = 23 if k % 2 == 0 else 0
        D[gap, gap, x] = 0.5
    return size, D.reshape(-1), np.ones(24 ** 3, F32)


def test_a_serpentine_takes_many_rounds():
    size, D, Wt = serpentine()
    gv = volume_of(size, D, Wt)
    reach = tsdf_amd.Reach()
    trav = R.traversable(D, Wt)
    for connectivity in (26, 6):
        want, _ = assert_reach(gv, reach, trav, size, centres([0], size), connectivity, 0, "serpentine at %d" % connectivity)
        # every free voxel is reached, the far slab last: 11 slabs crossed corner to corner and 22 steps through walls
        assert np.all(want[trav] != U) and int(want.max()) >= 11 * 23 * 14 + 22 * 10
        # the corridor crosses brick borders dozens of times, and a round carries the field across one border at the most
        # (12 slabs, each two bricks across on the diagonal: the field is 24 bricks from the seed's at the far end)
        assert reach.info.rounds >= 24, reach.info.rounds
    # a cap in the middle of the corridor
    assert_reach(gv, reach, trav, size, centres([0], size), 26, 2000, "serpentine capped")
    reach.close()
    gv.close()


def test_corner_steps_across_eight_bricks():
    # all occupied but the 2 x 2 x 2 block round the brick corner (8, 8, 8): its eight voxels lie in eight different bricks
    size = (16, 16, 16)
    block = [(x, y, z) for z in (7, 8) for y in (7, 8) for x in (7, 8)]
    vid = lambda x, y, z: (z * 16 + y) * 16 + x
    reach = tsdf_amd.Reach()
    for blocked in [None] + block[1:7]:
        D = np.full(16 ** 3, -0.5, F32)
        for v in block:
            if v != blocked:
                D[vid(*v)] = 0.5
        gv = volume_of(size, D, np.ones(16 ** 3, F32))
        trav = R.traversable(D, np.ones(16 ** 3, F32))
        for connectivity in (26, 6):
            want, _ = assert_reach(gv, reach, trav, size, centres([vid(7, 7, 7)], size), connectivity, 0, "block without %s at %d" % (blocked, connectivity))
            assert want[vid(8, 8, 8)] == (30 if connectivity == 6 else 17 if blocked is None else 24)
        gv.close()
    # a diagonal staircase of such blocks from (1, 1, 1) to (14, 14, 14): corner steps only pay, across every brick corner on the way
    D = np.full((16, 16, 16), -0.5, F32)
    for k in range(1, 14):
        D[k:k + 2, k:k + 2, k:k + 2] = 0.5
    D = D.reshape(-1)
    gv = volume_of(size, D, np.ones(16 ** 3, F32))
    trav = R.traversable(D, np.ones(16 ** 3, F32))
    want, _ = assert_reach(gv, reach, trav, size, centres([vid(1, 1, 1)], size), 26, 0, "staircase")
    assert want[vid(14, 14, 14)] == 13 * 17
    gv.close()
    reach.close()


# ---- a fused scene: clearance, ranking, and what is left alone --------------------------------------------------------------------
def fused_volume(frames, n=48):
    gv = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    for d, cam in frames:
        gv.integrate(d, W, H, cam)
    return gv


@pytest.fixture(scope="module")
def fused():
    """Three synthetic frames on 48^3: (frames, distances, weights, voxel size, offset) of the device's own integration."""
    frames = [synth.depth_frame(i * 9, 40, seed=0x5EEDE5D0) for i in range(3)]
    gv = fused_volume(frames)
    out = frames, gv.get_distance_data(), gv.get_weight_data(), gv.voxel_size(), tuple(gv.offset())
    gv.close()
    return out


def assert_fused(gv, reach, trav, vs, offset, seeds, connectivity, max_cost, what, **kw):
    size = (48,) * 3
    want, _ = R.cost_field(trav, size, vs, offset, seeds, connectivity, max_cost)
    gv.reach(seeds, connectivity, max_cost=max_cost, into=reach, **kw)
    assert np.array_equal(reach.costs, want), what
    counts = R.info(trav, want)
    assert {k: int(getattr(reach.info, k)) for k in counts} == counts, what
    return want


def test_clearance_from_an_esdf(fused):
    frames, D, Wt, vs, offset = fused
    size = (48,) * 3
    gv = fused_volume(frames)
    reach, esdf = tsdf_amd.Reach(), tsdf_amd.ESDF()
    for fill in (False, True):
        gv.compute_esdf(500.0, fill_unknown=fill, into=esdf)
        e = esdf.distances.copy()          # the reference takes the device's own ESDF: only this group is under test
        for clearance in (70.0, 190.0):
            trav = R.traversable(D, Wt, fill, e, clearance)
            assert 100 < trav.sum() < R.traversable(D, Wt, fill).sum()
            open_ids = np.flatnonzero(trav)
            seeds = R.centres(open_ids[[0, len(open_ids) // 2]], size, vs, offset)
            want = assert_fused(gv, reach, trav, vs, offset, seeds, 26, 0, "clearance %s fill %s" % (clearance, fill), esdf=esdf,
                                clearance=clearance, through_unknown=fill)
            assert (want != U).sum() > 100 and reach.info.clearance == F32(clearance)
        assert np.array_equal(esdf.distances.view(np.uint32), e.view(np.uint32))
    # a clearance of 0 with an ESDF still drops the voxels whose ESDF value is NaN or negative
    trav = R.traversable(D, Wt, True, e, 0.0)
    assert_fused(gv, reach, trav, vs, offset, seeds, 6, 0, "clearance 0", esdf=esdf, clearance=0.0, through_unknown=True)
    for h in (reach, esdf, gv):
        h.close()


def test_ranking_frontier_clusters(fused):
    frames, D, Wt, vs, offset = fused
    size = (48,) * 3
    gv = fused_volume(frames)
    ex = gv.find_frontiers().cluster(6, 1)
    ids, labels, table = ex.voxels, ex.labels, ex.clusters
    assert len(table) >= 2
    trav = R.traversable(D, Wt)
    seeds = R.centres(ids[:1], size, vs, offset)      # a frontier voxel is free: a seed
    reach = tsdf_amd.Reach()
    for connectivity, cap in ((26, 0), (6, 0), (26, 150)):
        want = assert_fused(gv, reach, trav, vs, offset, seeds, connectivity, cap, "rank at %d cap %d" % (connectivity, cap))
        got = reach.rank(ex)
        ref = R.rank(want, ids, labels, table)
        assert got.dtype == R.CLUSTER_DTYPE and got.tobytes() == ref.tobytes(), (connectivity, cap)
        assert (got["cost"] != U).any()
        if cap:   # most clusters lie beyond the cap: no member reached
            none = got[got["cost"] == U]
            assert len(none) and np.all(none["voxel"] == 0xFFFFFFFF)
        # the device variant, and the routes to every cluster's best voxel
        with _DeviceArray(nbytes=16 * len(table)) as rows:
            reach.rank_device(ex, rows.ptr.value)
            host = np.zeros(len(table), R.CLUSTER_DTYPE)
            _capi.check(_capi.lib.tsdf_device_download(host.ctypes.data, rows.ptr, host.nbytes))   # (a blocking copy on the null stream)
        assert host.tobytes() == ref.tobytes()
        best = got[got["cost"] != U]["voxel"]
        routes = reach.paths(reach.voxel_centres(best))
        for v, route in zip(best, routes):
            assert route.tolist() == R.path(want, trav, size, connectivity, int(v))
    # a clustering with min_size above every cluster: an empty table ranks to nothing
    ex.cluster(6, 10 ** 6)
    assert len(reach.rank(ex)) == 0
    assert (ex.voxels.tobytes(), ex.labels.tobytes()) == (ids.tobytes(), labels.tobytes())
    for h in (reach, ex, gv):
        h.close()


def test_nothing_that_is_read_is_written(fused):
    frames = fused[0]
    gv = fused_volume(frames)
    cam = frames[1][1]
    v0, n0 = gv.raycast(W, H, cam)
    kind0 = gv.last_raycast_cell_parallel()
    esdf = gv.compute_esdf(300.0)
    ex = gv.find_frontiers().cluster(26, 1)
    state = lambda: (gv.get_distance_data().tobytes(), gv.get_weight_data().tobytes(), gv.weight_storage(), esdf.distances.tobytes(),
                     ex.voxels.tobytes(), ex.labels.tobytes(), ex.clusters.tobytes())
    before = state()
    reach = gv.reach(ex.points, 26, esdf=esdf, clearance=70.0)
    assert reach.info.n_reached > 0
    ranked = reach.rank(ex)
    reach.paths(reach.voxel_centres(ranked[ranked["cost"] != U]["voxel"]), 8)
    reach.lookup(ex.points)
    assert state() == before
    assert gv.last_raycast_cell_parallel() == kind0
    v1, n1 = gv.raycast(W, H, cam)
    assert v1.tobytes() == v0.tobytes() and n1.tobytes() == n0.tobytes() and (~np.isnan(v0[:, 0])).sum() > 1000
    for h in (reach, ex, esdf, gv):
        h.close()


# ---- lookup and paths on 13 x 7 x 5 ---------------------------------------------------------------------------------------------------
SMALL = (13, 7, 5)


@pytest.fixture(scope="module")
def small():
    """(distances, weights, traversable, seeds): a half-observed 13 x 7 x 5 crossed through unknown space from two seeds."""
    D, Wt = E.random_state_field(SMALL, 4321, 0.5)
    trav = R.traversable(D, Wt, True)
    seeds = centres(np.flatnonzero(trav)[[3, 200]], SMALL)
    return D, Wt, trav, seeds


@pytest.mark.parametrize("connectivity", [26, 6])
def test_lookup_and_paths(small, connectivity):
    D, Wt, trav, seeds = small
    gv = volume_of(SMALL, D, Wt)
    reach = tsdf_amd.Reach()
    want, seed_ids = assert_reach(gv, reach, trav, SMALL, seeds, connectivity, 0, "small", through_unknown=True)
    gv.close()          # the handle remembers the geometry: nothing below needs the volume
    assert len(seed_ids) == 2 and (want != U).sum() > 100 and (want == U).sum() > 10
    # lookup: voxel centres, points on voxel faces and corners (the floor decides), just off every side, NaN and infinities
    lo, vs, N = np.array(OFFSET, np.float64), VS.astype(np.float64), np.array(SMALL, np.float64)
    rng = np.random.default_rng(5)
    pts = [centres(np.arange(13 * 7 * 5), SMALL).astype(np.float64), lo + np.floor(rng.uniform(0, N, (64, 3))) * vs,
           lo + rng.uniform(-1.0, N + 1.0, (150, 3)) * vs, lo + N * vs, lo + np.array([[0.0, 0.0, 0.0], [-1e-3, 1.0, 1.0], [13.0, 1.0, 1.0]]) * vs,
           np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, -3e38, 0]])]
    pts = np.concatenate([np.atleast_2d(p) for p in pts]).astype(F32)
    for n in (0, 1, 64, 257, len(pts)):
        got = reach.lookup(pts[:n])
        assert got.dtype == np.uint32 and np.array_equal(got, R.lookup(want, SMALL, VS, OFFSET, pts[:n])), n
    with _DeviceArray(host=pts) as dp, _DeviceArray(nbytes=4 * len(pts)) as dc:
        reach.lookup_device(len(pts), dp.ptr.value, dc.ptr.value)
        host = np.zeros(len(pts), np.uint32)
        _capi.check(_capi.lib.tsdf_device_download(host.ctypes.data, dc.ptr, host.nbytes))
    assert np.array_equal(host, R.lookup(want, SMALL, VS, OFFSET, pts))
    # paths: every reached voxel as a goal, then unreached goals, one off the grid and a NaN
    reached = np.flatnonzero(want != U)
    goals = np.concatenate([centres(reached, SMALL), centres(np.flatnonzero(want == U)[:5], SMALL), pts[-4:]])
    routes = reach.paths(goals)
    longest = 0
    for k, route in enumerate(routes):
        ref = R.path(want, trav, SMALL, connectivity, R.point_voxel(goals[k], SMALL, VS, OFFSET))
        assert route.dtype == np.uint32 and route.tolist() == ref, (k, route, ref)
        longest = max(longest, len(ref))
    assert longest > 5 and all(len(routes[np.flatnonzero(reached == s)[0]]) == 1 for s in seed_ids)   # a goal on a seed: itself
    assert all(len(r) == 0 for r in routes[len(reached):])
    # rows that fit exactly, rows of one, and a row longer than any path: the length is the whole path's, the rest is left as it was
    for max_len in (longest, 1, 3, longest + 2):
        keep = np.full((len(goals), max_len), 0xABCD0000, np.uint32) + np.arange(max_len, dtype=np.uint32)
        lengths, rows = reach.paths(goals, max_len, rows=keep.copy())
        ref_lengths, ref_rows = R.paths(want, trav, SMALL, VS, OFFSET, connectivity, goals, max_len, rows=keep)
        assert np.array_equal(lengths, ref_lengths) and np.array_equal(rows, ref_rows), max_len
        assert lengths.max() == longest
    assert reach.paths(np.zeros((0, 3), F32)) == []
    reach.close()


def test_a_warm_handle_a_reused_handle_and_two_runs(small):
    D, Wt, trav, seeds = small
    reach = tsdf_amd.Reach()
    assert reach.scratch_bytes == 160 and reach.device_buffer() == 0
    big_size = (24, 24, 24)
    Db, Wb = E.random_state_field(big_size, 77, 0.9)
    big, little = volume_of(big_size, Db, Wb), volume_of(SMALL, D, Wt)
    big_trav = R.traversable(Db, Wb)
    big_seeds = centres(np.flatnonzero(big_trav)[[0, 5000]], big_size)
    first, _ = assert_reach(big, reach, big_trav, big_size, big_seeds, 26, 0, "cold")
    warm, pointer = reach.scratch_bytes, reach.device_buffer()
    # 1 bit a voxel, two words a brick and the counters
    assert warm == 8 * ((24 ** 3 + 63) // 64) + 8 * 27 + 160 and pointer
    # the same handle on a small grid and back: the same bytes, no array grows or moves
    assert_reach(little, reach, trav, SMALL, seeds, 6, 400, "reused on a small grid", through_unknown=True)
    assert reach.scratch_bytes == warm
    for run in range(2):
        big.reach(big_seeds, 26, into=reach)
        assert reach.costs.tobytes() == first.tobytes(), "run %d" % run
        assert reach.scratch_bytes == warm and reach.device_buffer() == pointer
    host = np.empty(24 ** 3, np.uint32)
    _capi.check(_capi.lib.tsdf_device_download(host.ctypes.data, C.c_void_p(pointer), host.nbytes))
    assert host.tobytes() == first.tobytes()
    # seeds that are already on the device
    with _DeviceArray(host=big_seeds) as ds:
        _capi.check(_capi.lib.tsdf_volume_compute_reach_device(big._h, len(big_seeds), ds.ptr, 26, None, 0.0, 0, 0, reach._h))
    assert reach.costs.tobytes() == first.tobytes()
    for h in (reach, big, little):
        h.close()


def test_refusals(small):
    D, Wt, trav, seeds = small
    lib, invalid = _capi.lib, _capi.TSDF_ERR_INVALID
    gv = volume_of(SMALL, D, Wt)
    reach, empty = tsdf_amd.Reach(), tsdf_amd.Reach()
    esdf, fresh_esdf = gv.compute_esdf(100.0), tsdf_amd.ESDF()
    out = np.zeros(64, np.uint32)
    sp, op = seeds.ctypes.data, out.ctypes.data

    def refused(rc, name):
        assert rc == invalid, name
        assert name in _capi.last_error(), (name, _capi.last_error())

    slab = tsdf_amd.TSDFVolume((16, 16, 16), (160.0,) * 3, slab=(0, 8))
    nodes = volume_of(SMALL, D, Wt)
    nodes.deformation()
    other = volume_of((12, 7, 5), *E.random_state_field((12, 7, 5), 1, 0.5))
    moved = volume_of(SMALL, D, Wt, offset=(0.0, 0.0, 0.0))
    scaled = tsdf_amd.TSDFVolume(SMALL, (SMALL[0] * 10.0, SMALL[1] * 12.5, SMALL[2] * 18.0))    # the grid and the offset of gv, z voxels twice as long
    scaled.offset(*OFFSET)
    assert np.array_equal(scaled.voxel_size(), np.array([10.0, 12.5, 18.0], F32)) and tuple(scaled.offset()) == OFFSET
    for fn, name in ((lib.tsdf_volume_compute_reach, "tsdf_volume_compute_reach"), (lib.tsdf_volume_compute_reach_device, "tsdf_volume_compute_reach_device")):
        refused(fn(None, 2, sp, 26, None, 0.0, 0, 0, reach._h), name)
        refused(fn(gv._h, 2, sp, 26, None, 0.0, 0, 0, None), name)
        refused(fn(gv._h, 2, None, 26, None, 0.0, 0, 0, reach._h), name)
        refused(fn(slab._h, 2, sp, 26, None, 0.0, 0, 0, reach._h), name)
        refused(fn(nodes._h, 2, sp, 26, None, 0.0, 0, 0, reach._h), name)
        for connectivity in (0, 4, 8, 18, 27):
            refused(fn(gv._h, 2, sp, connectivity, None, 0.0, 0, 0, reach._h), name)
        refused(fn(gv._h, 2, sp, 26, None, 0.0, 0, 2, reach._h), name)
        for clearance in (-1.0, float("nan"), float("inf")):
            refused(fn(gv._h, 2, sp, 26, esdf._h, clearance, 0, 0, reach._h), name)
        refused(fn(gv._h, 2, sp, 26, None, 10.0, 0, 0, reach._h), name)                 # a clearance without an ESDF
        refused(fn(gv._h, 2, sp, 26, fresh_esdf._h, 10.0, 0, 0, reach._h), name)        # an ESDF never computed
        refused(fn(other._h, 2, sp, 26, esdf._h, 10.0, 0, 0, reach._h), name)           # ... of another size
        refused(fn(moved._h, 2, sp, 26, esdf._h, 10.0, 0, 0, reach._h), name)           # ... of another offset
        refused(fn(scaled._h, 2, sp, 26, esdf._h, 10.0, 0, 0, reach._h), name)          # ... of other voxel sizes, all else equal
        assert "ESDF was computed for another geometry" in _capi.last_error()
    assert reach.info.n_reached == 0 and reach.device_buffer() == 0
    # a handle never computed
    ex = gv.find_frontiers().cluster(26, 1)
    rows = np.zeros(int(ex.info.n_listed_clusters) + 1, R.CLUSTER_DTYPE)
    refused(lib.tsdf_reach_download(empty._h, op), "tsdf_reach_download")
    refused(lib.tsdf_reach_lookup(empty._h, 2, sp, op), "tsdf_reach_lookup")
    refused(lib.tsdf_reach_lookup_device(empty._h, 2, sp, op, None), "tsdf_reach_lookup_device")
    refused(lib.tsdf_reach_paths(empty._h, 2, sp, 4, op, op), "tsdf_reach_paths")
    refused(lib.tsdf_reach_paths_device(empty._h, 2, sp, 4, op, op, None), "tsdf_reach_paths_device")
    refused(lib.tsdf_reach_rank_frontiers(empty._h, ex._h, rows.ctypes.data), "tsdf_reach_rank_frontiers")
    refused(lib.tsdf_reach_rank_frontiers_device(empty._h, ex._h, rows.ctypes.data, None), "tsdf_reach_rank_frontiers_device")
    # null arrays, max_len == 0
    gv.reach(seeds, into=reach, through_unknown=True)
    refused(lib.tsdf_reach_download(reach._h, None), "tsdf_reach_download")
    refused(lib.tsdf_reach_buffer(reach._h, None), "tsdf_reach_buffer")
    refused(lib.tsdf_reach_get_info(reach._h, None), "tsdf_reach_get_info")
    refused(lib.tsdf_reach_scratch_bytes(reach._h, None), "tsdf_reach_scratch_bytes")
    for fn, name, tail in ((lib.tsdf_reach_lookup, "tsdf_reach_lookup", ()), (lib.tsdf_reach_lookup_device, "tsdf_reach_lookup_device", (None,))):
        refused(fn(reach._h, 2, None, op, *tail), name)
        refused(fn(reach._h, 2, sp, None, *tail), name)
        assert fn(reach._h, 0, None, None, *tail) == _capi.TSDF_OK
    for fn, name, tail in ((lib.tsdf_reach_paths, "tsdf_reach_paths", ()), (lib.tsdf_reach_paths_device, "tsdf_reach_paths_device", (None,))):
        refused(fn(reach._h, 2, None, 4, op, op, *tail), name)
        refused(fn(reach._h, 2, sp, 0, op, op, *tail), name)
        refused(fn(reach._h, 2, sp, 4, None, op, *tail), name)
        refused(fn(reach._h, 2, sp, 4, op, None, *tail), name)
        assert fn(reach._h, 0, None, 0, None, None, *tail) == _capi.TSDF_OK
    # ranking: a null explorer, null rows, one that is not clustered, one of another geometry
    rank, rank_device = lib.tsdf_reach_rank_frontiers, lambda r, e, p: lib.tsdf_reach_rank_frontiers_device(r, e, p, None)
    unclustered, elsewhere = gv.find_frontiers(), moved.find_frontiers().cluster(26, 1)
    for fn, name in ((rank, "tsdf_reach_rank_frontiers"), (rank_device, "tsdf_reach_rank_frontiers_device")):
        refused(fn(None, ex._h, rows.ctypes.data), name)
        refused(fn(reach._h, None, rows.ctypes.data), name)
        refused(fn(reach._h, ex._h, None), name)
        refused(fn(reach._h, unclustered._h, rows.ctypes.data), name)
        refused(fn(reach._h, elsewhere._h, rows.ctypes.data), name)
    with pytest.raises(ValueError, match="tsdf_volume_compute_reach: connectivity must be 6 or 26"):
        gv.reach(seeds, 18)
    lib.tsdf_reach_destroy(None)
    for h in (reach, empty, esdf, fresh_esdf, ex, unclustered, elsewhere, slab, nodes, other, moved, scaled, gv):
        h.close()
