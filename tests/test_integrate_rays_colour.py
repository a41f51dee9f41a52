"""Coloured ray integration and the colour at ray-query hits on the GPU (include/tsdf_amd.h, "ray integration" rules 9 - 12 and "ray
queries"; tsdf_amd/csrc/integrate_rays.hip, raycast_rays.hpp) against the CPU reference (tests/rays_colour_ref.py), bit for bit in
distances, weights and colour words: every set of tests/rays_colour_cases.py through both entry points, with one origin and with one
per ray, in all three weight storages, beside a plain twin volume, between coloured depth frames, call after call, with the scratch
released, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import colour_ref
from tests import ray_ref
from tests import rays_colour_cases as CC
from tests import rays_colour_ref as cref
from tests import rays_integrate_ref as ref
from tests.helpers import H, W, assert_same_floats
from tsdf_amd import _capi, synth
from tsdf_amd.api import _DeviceArray, _fp, unit_directions

F = np.float32
SEED, PERIOD = 0x5EEDF05E, 40
GUARD_WORD, GUARD = 0x7FC0BEEF7FC0BEEF, 256            # guard regions of 256 bytes


def set_trunc(vol, trunc):
    i = vol.info()
    _capi.check(_capi.lib.tsdf_volume_set_header(vol._h, _fp(np.array(i.offset, F)), float(trunc), float(i.max_weight),
                                                 _fp(np.array(i.global_translation, F)), _fp(np.array(i.global_rotation, F))))


def gpu_volume(c, bits=8, colour=True, words=True):
    """The case's grid with its start state (tests/rays_colour_cases.start_state)."""
    dims, phys, offset = c.grid
    v = tsdf_amd.TSDFVolume(dims, phys)
    v.offset(*offset)
    if bits != 8:
        v.set_weight_storage(bits)
    if c.trunc is not None:
        set_trunc(v, c.trunc)
        v.set_distance_data(np.full(v.resident_voxels(), c.trunc, F))      # the cleared field of that truncation distance
    if colour:
        v.enable_colour(True)
        if words:
            geom = ref.geometry(v)
            v.set_colour_data(CC.start_state(geom)[2])
    return v


def assert_state(vol, dist, weight, words, what):
    assert_same_floats(vol.get_distance_data(), dist, what + ": distances")
    assert_same_floats(vol.get_weight_data(), weight, what + ": weights")
    if words is not None:
        got = np.asarray(vol.get_colour_data()).reshape(-1)
        bad = np.nonzero(got != words)[0]
        assert bad.size == 0, "%s: %d colour words differ, first at %d: %08x, expected %08x" % (what, bad.size, bad[0], got[bad[0]],
                                                                                               words[bad[0]])


def call_host(vol, o, p, rgb, lo, hi, flags):
    return vol.integrate_rays(o[0] if len(o) == 1 else o, p, band_only=bool(flags & ref.BAND_ONLY), min_range=lo, max_range=hi, rgb=rgb)


def call_device(vol, o, p, rgb, lo, hi, flags, count=True):
    """Through tsdf_integrate_rays_colour_device, origins, points and colours between guard regions on the device; -> updated voxels."""
    guard = np.full(GUARD, 0xA5, np.uint8)
    parts = [guard, o.reshape(-1).view(np.uint8), guard, p.reshape(-1).view(np.uint8), guard, rgb.reshape(-1), guard]
    host = np.concatenate(parts)
    at_o, at_p, at_c = GUARD, 2 * GUARD + o.nbytes, 3 * GUARD + o.nbytes + p.nbytes
    box = (C.c_uint64 * 3)(GUARD_WORD, GUARD_WORD, GUARD_WORD)
    with _DeviceArray(host) as dev:
        base = dev.ptr.value
        out = C.cast(C.byref(box, 8), C.POINTER(C.c_uint64)) if count else None
        _capi.check(_capi.lib.tsdf_integrate_rays_colour_device(vol._h, len(p), C.c_void_p(base + at_o), len(o), C.c_void_p(base + at_p),
                                                                C.c_void_p(base + at_c), lo, hi, flags, out))
        vol.synchronize()
        back = np.empty_like(host)
        _capi.check(_capi.lib.tsdf_device_download(back.ctypes.data, dev.ptr, host.nbytes))
    assert np.array_equal(back, host), "the rays, their colours or the guard regions around them were written"
    assert box[0] == GUARD_WORD and box[2] == GUARD_WORD
    return int(box[1]) if count else None


def run(vol, c, entry=call_host, expand=False):
    counts = []
    for o, p, rgb, lo, hi, flags in c.calls:
        if expand and len(o) == 1:
            o = np.ascontiguousarray(np.repeat(o, len(p), 0))
        counts.append(entry(vol, o, p, rgb, lo, hi, flags))
    return counts


def expected(name):
    d, w, words, masks, _, _ = CC.reference(name)
    return d, w, words, [int(m.sum()) for m in masks]


@pytest.mark.gpu
@pytest.mark.parametrize("bits", (8, 16, 32))
@pytest.mark.parametrize("name", CC.NAMES)
def test_bit_parity_in_every_weight_storage(oracle, name, bits):
    c = CC.case(name)
    d, w, words, counts = expected(name)
    vol = gpu_volume(c, bits)
    assert run(vol, c) == counts                                           # several calls in a row: the scratch is zero again each time
    assert_state(vol, d, w, words, "%s, %d-bit weights" % (name, bits))
    assert vol.weight_storage() == (bits, False)
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CC.NAMES)
def test_the_device_entry_point_and_its_guards(oracle, name):
    c = CC.case(name)
    d, w, words, counts = expected(name)
    vol = gpu_volume(c)
    assert run(vol, c, call_device) == counts
    assert_state(vol, d, w, words, name + ", device pointers")
    vol.close()
    if name in ("outside", "g2_scan"):                                     # updated_voxels == NULL: asynchronous, the same bits
        vol = gpu_volume(c)
        run(vol, c, lambda *a: call_device(*a, count=False))
        assert_state(vol, d, w, words, name + ", device pointers, no count")
        vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CC.NAMES)
def test_one_origin_per_ray_gives_the_bits_of_one_origin(oracle, name):
    c = CC.case(name)
    d, w, words, counts = expected(name)
    vol = gpu_volume(c)
    assert run(vol, c, expand=True) == counts
    assert_state(vol, d, w, words, name + ", n origins")
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("inside", "trunc_edges", "g2_scan"))
def test_offset_at_clear_plays_no_part(oracle, name):
    """The colour word has the index of the distance: a volume cleared at another offset gives the same words."""
    c = CC.case(name)
    d, w, words, counts = expected(name)
    dims, phys, offset = c.grid
    vol = tsdf_amd.TSDFVolume(dims, phys)
    vol.offset(81.0, -88.0, 67.0)
    vol.clear()                                                            # bakes that offset in as offset_at_clear
    vol.offset(*offset)
    assert tuple(vol.info().offset_at_clear) == (81.0, -88.0, 67.0)
    if c.trunc is not None:
        set_trunc(vol, c.trunc)
        vol.set_distance_data(np.full(vol.resident_voxels(), c.trunc, F))
    vol.enable_colour(True)
    vol.set_colour_data(CC.start_state(ref.geometry(vol))[2])
    assert run(vol, c) == counts
    assert_state(vol, d, w, words, name + ", offset_at_clear set")
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("inside", "per_ray_origins", "contention", "g2_scan"))
def test_a_plain_twin_has_the_same_distances_under_a_cap_and_across_the_widening(oracle, name):
    c = CC.case(name)
    n = int(np.prod(c.grid[0]))
    rng = np.random.RandomState(4)
    for cap, start_w in ((4, rng.randint(0, 9, n).astype(F)), (0, rng.randint(250, 256, n).astype(F))):
        twins = []
        for coloured in (True, False):
            vol = gpu_volume(c, colour=coloured)
            vol.set_weight_data(start_w)
            if cap:
                vol.set_weight_cap(cap)
            assert vol.weight_storage() == (8, False)
            if coloured:
                counts = run(vol, c)
            else:
                counts = [vol.integrate_rays(o[0] if len(o) == 1 else o, p, band_only=bool(fl & ref.BAND_ONLY), min_range=lo, max_range=hi)
                          for o, p, _, lo, hi, fl in c.calls]
            twins.append((counts, vol.get_distance_data(), vol.get_weight_data(), vol.weight_storage()))
            vol.close()
        assert twins[0][0] == twins[1][0] and twins[0][3] == twins[1][3]
        assert_same_floats(twins[0][1], twins[1][1], "%s: distances beside the plain twin (cap %d)" % (name, cap))
        assert_same_floats(twins[0][2], twins[1][2], "%s: weights beside the plain twin (cap %d)" % (name, cap))
        if cap:
            assert twins[0][2].max() <= max(cap, start_w.max()) and (twins[0][2] == cap).sum() >= 10     # the cap bites
        else:
            assert twins[0][3][0] == 16 and twins[0][2].max() >= 256       # widened on the way


@pytest.mark.gpu
def test_between_two_coloured_depth_frames(oracle):
    """A coloured depth frame, the coloured rays, another coloured depth frame: the depth path and the ray path share the words."""
    c = CC.case("outside")
    ov, geom = CC.make_geometry(oracle, c)
    frames = [(synth.depth_frame(i, PERIOD, seed=SEED), synth.colour_frame(i, PERIOD, seed=SEED)[0]) for i in (3, 12)]
    vol = gpu_volume(c, words=False)
    cgeom = colour_ref.geometry(vol)
    words = np.zeros(vol.resident_voxels(), np.uint32)

    def depth_step(frame):
        nonlocal words
        (depth, cam), rgb = frame
        vol.integrate_colour(depth, rgb, W, H, cam)
        ov.integrate(depth, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
        words = colour_ref.integrate_colour(oracle, words, cgeom, depth, rgb, W, H, cam)[0]

    depth_step(frames[0])
    assert ((words >> 24) > 0).sum() >= 300
    d, w = ov.dist.copy(), ov.weight.copy()
    blended = 0
    for o, p, rgb, lo, hi, flags in c.calls:
        before = words
        d, w, _, words, _, col = cref.integrate(geom, d, w, words, o, p, rgb, lo, hi, flags)
        blended += int((((before >> 24) > 0) & cref.mask(geom, col)).sum())
    assert blended >= 20                                                   # ray colours blended into depth-frame colours
    run(vol, c)
    assert_state(vol, d, w, words, "rays after a coloured depth frame")
    ov.set_distance_data(d)
    ov.set_weight_data(w)
    depth_step(frames[1])
    assert_state(vol, ov.dist, ov.weight, words, "then another coloured depth frame")
    vol.close()


@pytest.mark.gpu
def test_five_permutations_give_identical_bits(oracle):
    sets = CC.permutation_sets()
    _, geom = CC.RC.make_geometry(oracle, CC.G1)
    d0, w0, words0 = CC.start_state(geom)
    rd, rw, upd, rwords, _, _ = cref.integrate(geom, d0, w0, words0, *sets[0])
    c = CC.case("inside")
    for i, (o, p, rgb) in enumerate(sets):
        vol = gpu_volume(c)
        assert vol.integrate_rays(o, p, rgb=rgb) == int(upd.sum())
        assert_state(vol, rd, rw, rwords, "permutation %d" % i)
        vol.close()


@pytest.mark.gpu
def test_the_scratch_is_reported_released_and_left_zero(oracle):
    c = CC.case("outside")
    d, w, words, counts = expected("outside")
    voxels = int(np.prod(c.grid[0]))
    vol = gpu_volume(c)
    assert vol.ray_scratch_bytes() == 0
    vol.release_ray_scratch()                                              # nothing to release yet
    o, p, rgb, lo, hi, flags = c.calls[0]
    # a plain call holds the plain scratch only, however often it is made
    plain = gpu_volume(c)
    plain.integrate_rays(o[0], p)
    held = plain.ray_scratch_bytes()
    assert 8 * voxels <= held < 8 * voxels + 4096
    plain.integrate_rays(o[0], p)
    assert plain.ray_scratch_bytes() == held
    # a coloured call adds 16 bytes per voxel, on a volume that has made plain calls too
    plain.integrate_rays(o[0], p, rgb=rgb)
    assert plain.ray_scratch_bytes() >= held + 16 * voxels
    plain.integrate_rays(o[0], p)
    assert plain.ray_scratch_bytes() >= held + 16 * voxels
    plain.release_ray_scratch()
    assert plain.ray_scratch_bytes() == 0
    plain.close()
    # released between the calls: the same bits
    for i, (o, p, rgb, lo, hi, flags) in enumerate(c.calls):
        assert call_host(vol, o, p, rgb, lo, hi, flags) == counts[i]
        assert vol.ray_scratch_bytes() >= 24 * voxels
        vol.release_ray_scratch()
        assert vol.ray_scratch_bytes() == 0
    assert_state(vol, d, w, words, "released between the calls")
    vol.close()


@pytest.mark.gpu
def test_a_plain_call_between_coloured_ones_leaves_the_colours_and_the_scratch_alone(oracle):
    """coloured, plain, coloured on one volume: were either scratch left dirty, the next call of the other kind would show it."""
    c = CC.case("outside")
    _, geom = CC.make_geometry(oracle, c)
    d, w, words = CC.start_state(geom)
    vol = gpu_volume(c)
    for i, (o, p, rgb, lo, hi, flags) in enumerate(c.calls + c.calls[:1]):
        if i == 1:
            acc = ref.accumulate(geom, o, p, lo, hi, flags)
            d, w, _ = ref.apply(geom, d, w, acc)
            vol.integrate_rays(o[0], p)
        else:
            d, w, _, words, _, _ = cref.integrate(geom, d, w, words, o, p, rgb, lo, hi, flags)
            call_host(vol, o, p, rgb, lo, hi, flags)
    assert_state(vol, d, w, words, "coloured, plain, coloured, coloured")
    vol.close()


@pytest.mark.gpu
def test_refusals_change_nothing(oracle):
    lib = _capi.lib
    c = CC.case("inside")
    d, w, words, _ = expected("inside")
    o, p, rgb = c.calls[0][:3]
    vol = gpu_volume(c)
    run(vol, c)
    uncoloured = gpu_volume(c, colour=False)
    slab = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3, slab=(0, 8))
    nodes = tsdf_amd.TSDFVolume((16, 16, 16), (1000.0,) * 3)
    nodes.enable_colour(True)
    nodes.deformation()                                                    # materialises the node array
    scratch = vol.ray_scratch_bytes()

    def snapshot(v):
        return (v.get_distance_data(), v.get_weight_data(), v.weight_storage(), v.ray_scratch_bytes(),
                np.asarray(v.get_colour_data()).copy() if v.colour_enabled() else None)

    before = {id(v): snapshot(v) for v in (vol, uncoloured, slab, nodes)}

    def untouched(v, what):
        """distances, weights, their storage, the scratch held and the colour words of v are what they were before the refusals"""
        if v is None:
            return
        was, now = before[id(v)], snapshot(v)
        assert_same_floats(now[0], was[0], what + ": distances")
        assert_same_floats(now[1], was[1], what + ": weights")
        assert now[2] == was[2] and now[3] == was[3], what
        assert (was[4] is None and now[4] is None) or np.array_equal(now[4], was[4]), what + ": colour words"

    def refused(what, v, n, op, n_origins, pp, cp, flags=0):
        for fn in (lib.tsdf_integrate_rays_colour, lib.tsdf_integrate_rays_colour_device):
            count = C.c_uint64(GUARD_WORD)
            rc = fn(v._h if v else None, n, op, n_origins, pp, cp, 0.0, float("inf"), flags, C.byref(count))
            assert rc == _capi.TSDF_ERR_INVALID, what
            assert len(_capi.last_error()) > 0
            assert count.value == GUARD_WORD, "updated_voxels was written by a refused call: " + what
            untouched(v, what)

    op, pp, cp = C.c_void_p(o.ctypes.data), C.c_void_p(p.ctypes.data), C.c_void_p(rgb.ctypes.data)
    n = len(p)
    refused("null volume", None, n, op, 1, pp, cp)
    refused("null origins", vol, n, None, 1, pp, cp)
    refused("null points", vol, n, op, 1, None, cp)
    refused("null rgb", vol, n, op, 1, pp, None)
    refused("two origins", vol, n, op, 2, pp, cp)
    refused("no origins", vol, n, op, 0, pp, cp)
    refused("too many rays", vol, (1 << 23) + 1, op, 1, pp, cp)
    refused("unknown flag", vol, n, op, 1, pp, cp, flags=2)
    refused("no colour", uncoloured, n, op, 1, pp, cp)
    refused("slab", slab, n, op, 1, pp, cp)
    refused("nodes", nodes, n, op, 1, pp, cp)
    with pytest.raises(ValueError):
        vol.integrate_rays(o[0], p, rgb=rgb[:-1])
    untouched(vol, "one colour short")
    with pytest.raises(ValueError):
        uncoloured.cast_rays(o, p[:1] - o, colours=True)
    # the refused casts write none of their outputs (host arrays: the device entry point refuses before it would read a pointer)
    dirs = np.ascontiguousarray(p[:1] - o, F)
    dp = C.c_void_p(dirs.ctypes.data)
    for fn in (lib.tsdf_volume_cast_rays_colour, lib.tsdf_volume_cast_rays_colour_device):
        for what, v, points, colours in (("null rgb", vol, True, False), ("null points", vol, False, True), ("no colour", uncoloured, True, True),
                                         ("slab", slab, True, True), ("null volume", None, True, True)):
            out_p, out_t, out_n = np.full((2, 3), 7.5, F), np.full(2, 7.5, F), np.full((2, 3), 7.5, F)
            out_c = np.full((2, 3), 0xA5, np.uint8)
            rc = fn(v._h if v else None, 1, op, dp, None, C.c_void_p(out_p.ctypes.data) if points else None, C.c_void_p(out_t.ctypes.data),
                    C.c_void_p(out_n.ctypes.data), C.c_void_p(out_c.ctypes.data) if colours else None)
            assert rc == _capi.TSDF_ERR_INVALID and len(_capi.last_error()) > 0, what
            assert (out_p == 7.5).all() and (out_t == 7.5).all() and (out_n == 7.5).all() and (out_c == 0xA5).all(), what
            untouched(v, "cast, " + what)
    assert uncoloured.ray_scratch_bytes() == 0
    # n == 0 succeeds and changes nothing
    assert vol.integrate_rays(o[0], np.empty((0, 3), F), rgb=np.empty((0, 3), np.uint8)) == 0
    assert vol.ray_scratch_bytes() == scratch
    assert_state(vol, d, w, words, "after the refusals")
    for v in (vol, uncoloured, slab, nodes):
        v.close()


@pytest.mark.gpu
def test_cast_rays_with_colours(oracle):
    """Points, t and normals are those of cast_rays; the colours are the reference's sampling of the reference's own hit points."""
    c = CC.case("outside")
    d, w, words, _ = expected("outside")
    vol = gpu_volume(c)
    run(vol, c)
    ov, geom = CC.make_geometry(oracle, c)
    ov.set_distance_data(d)
    ov.set_weight_data(w)
    origins = np.concatenate([np.repeat(o, len(p), 0)[::3] for o, p, _, _, _, _ in c.calls])
    points = np.concatenate([p[::3] for _, p, _, _, _, _ in c.calls])
    dirs = unit_directions(points - origins)
    # rays that miss, a non-finite one and one from outside the box looking away
    origins = np.concatenate([origins, origins[:3]]).astype(F)
    dirs = np.concatenate([dirs, -dirs[:1], [[np.nan, 0, 1]], [[0, 0, 0]]]).astype(F)
    rp, rt, rn = ray_ref.cast(oracle, ov, origins, dirs, normals=True)
    want = cref.sample(geom, words, rp)
    gp, gt, gn, gc = vol.cast_rays(origins, dirs, normals=True, colours=True)
    pp, pt, pn = vol.cast_rays(origins, dirs, normals=True)
    for got, plain, reference, what in ((gp, pp, rp, "points"), (gt, pt, rt, "t"), (gn, pn, rn, "normals")):
        assert_same_floats(got, plain, what + " with and without colours")
        assert_same_floats(got, reference, what + " against the reference")
    assert gc.dtype == np.uint8 and gc.shape == (len(origins), 3)
    assert np.array_equal(gc, want)
    miss = np.isnan(rt)
    assert miss.sum() >= 3 and (~miss).sum() >= 200 and (gc[miss] == 0).all() and (gc[~miss] != 0).any(axis=1).sum() >= 150
    # the device entry point between guards, without t and normals
    n = len(origins)
    host = np.concatenate([origins.reshape(-1), dirs.reshape(-1)]).astype(F)
    with _DeviceArray(host) as rays, _DeviceArray(nbytes=12 * n) as dp, _DeviceArray(np.full(3 * n + 2 * 256, 0xA5, np.uint8)) as dc:
        vol.cast_rays_device(n, rays.ptr.value, rays.ptr.value + 12 * n, None, dp.ptr.value, None, None, colours_ptr=dc.ptr.value + 256)
        vol.synchronize()
        back = np.empty(3 * n + 512, np.uint8)
        _capi.check(_capi.lib.tsdf_device_download(back.ctypes.data, dc.ptr, back.nbytes))
    assert (back[:256] == 0xA5).all() and (back[-256:] == 0xA5).all() and np.array_equal(back[256:-256].reshape(-1, 3), want)
    vol.close()


@pytest.mark.gpu
def test_round_trip_a_uniform_scan_comes_back_in_its_colour(oracle):
    c = CC.case("uniform")
    _, geom = CC.make_geometry(oracle, c)
    o, p, rgb, lo, hi, flags = c.calls[0]
    vol = gpu_volume(c, words=False)
    vol.integrate_rays(o[0], p, rgb=rgb)
    _, col = cref.accumulate(geom, o, p, rgb, lo, hi, flags)
    dirs = unit_directions(p - o)
    hits, t, colours = vol.cast_rays(np.repeat(o, len(p), 0), dirs, colours=True)
    cells = cref.sample_cells(geom, hits)
    in_set = np.array([cell is not None and cell in col for cell in cells])
    assert (~np.isnan(t)).sum() >= 200 and in_set.sum() >= 200             # (the coverage test_integrate_rays.py asks of its cast)
    assert (colours[in_set] == np.array(CC.UNIFORM, np.uint8)).all()
    assert (colours[np.isnan(t)] == 0).all()
    vol.close()
