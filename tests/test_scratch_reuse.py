"""One handle, several shapes: the scratch arrays a handle keeps between calls (tsdf_amd/csrc/device_buffer.hpp) only go
wrong when a handle meets a second, different shape, and most tests make a handle per shape.  Every case here runs small, large, small
on ONE handle and compares every result, bit for bit, with the same call on a FRESH handle that was given the same state.

Shapes: depth frames of 32 x 24, 80 x 56 and 32 x 24 pixels; a volume of 40 x 24 x 36 voxels, no multiple of the integrate brick
(64 x 4 x 32) on any axis, once with the packed weights a volume starts with and once with the fp32 array.  The environment's
TSDF_WEIGHT_PACK is read once per process, so the fp32 run is chosen per volume with set_weight_storage(32) on the empty volume,
which leaves the array TSDF_WEIGHT_PACK=0 starts with."""
import numpy as np
import pytest

import tsdf_amd
from tsdf_amd import _capi, synth
from tsdf_amd.api import _DeviceArray

from tests.helpers import assert_same_floats

pytestmark = pytest.mark.gpu

GRID = (40, 24, 36)
PHYSICAL = (3000.0, 3000.0, 3000.0)
FRAMES = ((32, 24), (80, 56), (32, 24))   # small, large, small
COUNTS = (1, 1000, 1)
STORAGE = ("packed", "fp32")
MESH_TABLE_BYTES = 256 * 32 + 256


def camera(width, height, frame):
    cam = tsdf_amd.Camera(0.82 * width, 0.82 * width, width / 2.0, height / 2.0)
    return synth.camera_for_frame(frame, 8, camera=cam)


def depth_and_camera(step):
    width, height = FRAMES[step]
    depth, cam = synth.depth_frame(step, 8, 0x5C4A7C00 + step, width, height, camera=camera(width, height, step))
    return depth, cam, width, height


def colour_of(step, cam):
    width, height = FRAMES[step]
    return synth.trace_colour(cam, width, height)


def new_volume(storage, colour=False):
    v = tsdf_amd.TSDFVolume(GRID, PHYSICAL)
    if storage == "fp32":
        v.set_weight_storage(32)
    if colour:
        v.enable_colour()
    return v


def state_of(v, colour=False):
    return (v.get_distance_data(), v.get_weight_data(), v.get_colour_data() if colour else None)


def fresh_with(state, storage, grid=GRID, physical=PHYSICAL):
    """A new volume holding `state`: no scratch array of it has seen a call yet."""
    v = tsdf_amd.TSDFVolume(grid, physical)
    v.set_distance_data(state[0])
    v.set_weight_data(state[1])
    if storage == "fp32":
        v.set_weight_storage(32)
    if state[2] is not None:
        v.enable_colour()
        v.set_colour_data(state[2])
    return v


def assert_same_state(a, b, what, colour=False):
    assert_same_floats(a.get_distance_data(), b.get_distance_data(), what + ": distances")
    assert_same_floats(a.get_weight_data(), b.get_weight_data(), what + ": weights")
    if colour:
        assert np.array_equal(a.get_colour_data(), b.get_colour_data()), what + ": colours"


def sphere_state(grid=GRID, trunc=None):
    """An analytic field: a sphere of 8 voxels radius (in index space) about the grid's centre, every voxel observed once."""
    X, Y, Z = grid
    z, y, x = np.meshgrid(np.arange(Z, dtype=np.float32), np.arange(Y, dtype=np.float32), np.arange(X, dtype=np.float32), indexing="ij")
    r = min(8.0, min(grid) / 3.0)
    d = (np.sqrt((x - X / 2.0) ** 2 + (y - Y / 2.0) ** 2 + (z - Z / 2.0) ** 2) - np.float32(r)) * np.float32(50.0)
    if trunc is not None:
        d = np.clip(d, -trunc, trunc)
    return d.astype(np.float32).reshape(-1), np.ones(X * Y * Z, np.float32), None


def sphere_volume(grid=GRID, physical=PHYSICAL):
    v = tsdf_amd.TSDFVolume(grid, physical)
    state = sphere_state(grid, np.float32(v.truncation_distance()))
    v.set_distance_data(state[0])
    v.set_weight_data(state[1])
    return v, state


# ---- integrate and ray cast --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGE)
def test_integrate_and_raycast_host_variants(storage):
    subject = new_volume(storage)
    hits = 0
    for step in range(3):
        depth, cam, width, height = depth_and_camera(step)
        what = "%s, step %d (%d x %d)" % (storage, step, width, height)
        fresh = fresh_with(state_of(subject), storage)
        subject.integrate(depth, width, height, cam)
        fresh.integrate(depth, width, height, cam)
        assert_same_state(subject, fresh, what)
        caster = tsdf_amd.GPURaycaster(width, height)
        V, N = caster.raycast(subject, cam)
        Vf, Nf = caster.raycast(fresh, cam)
        assert_same_floats(V, Vf, what + ": vertices")
        assert_same_floats(N, Nf, what + ": normals")
        hits += int((~np.isnan(V[:, 0])).sum())
        fresh.close()
    assert (subject.get_weight_data() > 0).any() and hits > 0
    subject.close()


def integrate_and_cast_on_device(v, depth, cam, width, height, casts):
    """-> [(vertices, normals)] of `casts` device ray casts behind one device integrate"""
    n = width * height
    out = []
    with _DeviceArray(depth) as dd, _DeviceArray(nbytes=12 * n) as dv, _DeviceArray(nbytes=12 * n) as dn:
        v.integrate_device(dd.ptr.value, width, height, cam)
        for _ in range(casts):
            tsdf_amd.GPURaycaster(width, height).raycast_device(v, cam, dv.ptr.value, dn.ptr.value)
            v.synchronize()
            V, N = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
            _capi.check(_capi.lib.tsdf_device_download(V.ctypes.data, dv.ptr, V.nbytes))
            _capi.check(_capi.lib.tsdf_device_download(N.ctypes.data, dn.ptr, N.nbytes))
            out.append((V, N))
        v.synchronize()
    return out


@pytest.mark.parametrize("storage", STORAGE)
def test_integrate_and_raycast_device_variants(storage):
    # (two casts a step: the per-pixel hit words have two sides, used alternately, and the second cast takes the order the first learnt)
    subject = new_volume(storage)
    hits = 0
    for step in range(3):
        depth, cam, width, height = depth_and_camera(step)
        what = "%s, step %d (%d x %d)" % (storage, step, width, height)
        fresh = fresh_with(state_of(subject), storage)
        got = integrate_and_cast_on_device(subject, depth, cam, width, height, 2)
        want = integrate_and_cast_on_device(fresh, depth, cam, width, height, 1)[0]
        assert_same_state(subject, fresh, what)
        for i, (V, N) in enumerate(got):
            assert_same_floats(V, want[0], what + ": vertices of cast %d" % i)
            assert_same_floats(N, want[1], what + ": normals of cast %d" % i)
        hits += int((~np.isnan(want[0][:, 0])).sum())
        fresh.close()
    assert hits > 0
    subject.close()


@pytest.mark.parametrize("storage", STORAGE)
def test_colour_integrate_and_raycast(storage):
    subject = new_volume(storage, colour=True)
    coloured = 0
    for step in range(3):
        depth, cam, width, height = depth_and_camera(step)
        rgb = colour_of(step, cam)
        what = "%s, step %d (%d x %d)" % (storage, step, width, height)
        fresh = fresh_with(state_of(subject, colour=True), storage)
        subject.integrate_colour(depth, rgb, width, height, cam)
        fresh.integrate_colour(depth, rgb, width, height, cam)
        assert_same_state(subject, fresh, what, colour=True)
        caster = tsdf_amd.GPURaycaster(width, height)
        V, N, c = caster.raycast_colour(subject, cam)
        Vf, Nf, cf = caster.raycast_colour(fresh, cam)
        assert_same_floats(V, Vf, what + ": vertices")
        assert_same_floats(N, Nf, what + ": normals")
        assert np.array_equal(c, cf), what + ": colours of the hits"
        coloured += int(c.any(axis=1).sum())
        fresh.close()
    assert coloured > 0
    subject.close()


def test_bilateral_host_variant():
    subject = tsdf_amd.BilateralFilter(30.0, 4.5)
    for step in range(3):
        depth, _, width, height = depth_and_camera(step)
        got, want = depth.copy(), depth.copy()
        subject.filter(got, width, height)
        fresh = tsdf_amd.BilateralFilter(30.0, 4.5)
        fresh.filter(want, width, height)
        fresh.close()
        assert np.array_equal(got, want), "step %d (%d x %d)" % (step, width, height)
        assert not np.array_equal(got, depth)
    subject.close()


# ---- the one-shot host variants ----------------------------------------------------------------------------------------------------
def query_points(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * np.array(PHYSICAL) * 1.1 - 150.0).astype(np.float32)   # (some outside the grid)


def test_sample_field_host_variant():
    subject, state = sphere_volume()
    for i, n in enumerate(COUNTS):
        P = query_points(n, 100 + i)
        fresh = fresh_with(state, "packed")
        for got, want, name in zip(subject.sample_field(P), fresh.sample_field(P), ("distance", "gradient", "weight")):
            assert_same_floats(got, want, "n = %d: %s" % (n, name))
        fresh.close()
    subject.close()


def test_cast_rays_host_variant():
    subject, state = sphere_volume()
    centre = np.array(PHYSICAL, np.float32) / 2
    hits = 0
    for i, n in enumerate(COUNTS):
        O = query_points(n, 200 + i)
        D = (centre - O) + query_points(n, 300 + i) * np.float32(0.05)   # towards the sphere, give or take
        fresh = fresh_with(state, "packed")
        got, want = subject.cast_rays(O, D, normals=True, normalise=True), fresh.cast_rays(O, D, normals=True, normalise=True)
        for g, w, name in zip(got, want, ("points", "t", "normals")):
            assert_same_floats(g, w, "n = %d: %s" % (n, name))
        hits += int((~np.isnan(got[1])).sum())
        fresh.close()
    assert hits > 0
    subject.close()


@pytest.mark.parametrize("storage", STORAGE)
def test_integrate_rays_host_variant(storage):
    subject = new_volume(storage)
    origin = np.array([1500.0, 1400.0, -500.0], np.float32)
    total = 0
    for i, n in enumerate(COUNTS):
        P = (query_points(n, 400 + i) * np.float32(0.5) + np.float32(750.0)).astype(np.float32)
        fresh = fresh_with(state_of(subject), storage)
        got, want = subject.integrate_rays(origin, P), fresh.integrate_rays(origin, P)
        assert got == want, "n = %d: updated voxels" % n
        assert_same_state(subject, fresh, "%s, n = %d" % (storage, n))
        assert subject.ray_scratch_bytes() == fresh.ray_scratch_bytes()
        total += got
        fresh.close()
    assert total > 0
    subject.close()


# ---- mesh and distance-field handles -----------------------------------------------------------------------------------------------
def mesh_scratch_after(chunks):
    """include/tsdf_amd.h, "indexed mesh": 32 bytes per 64 voxels of the marched range, 16 per 65536 (and 16 for the totals' slot of the
    scan), the table, the two pinned totals -- for the largest range the handle has marched, since its arrays only grow."""
    return 32 * chunks + 16 * ((chunks + 1023) // 1024 + 1) + MESH_TABLE_BYTES + 16


def test_mesh_handle_box_whole_box():
    volume, _ = sphere_volume()
    box = (16, 10, 9, 23, 13, 12)                    # 8 x 4 x 4 voxels: 2 chunks of 64, across the sphere's near pole
    whole_chunks = (GRID[0] * GRID[1] * GRID[2] + 63) // 64
    subject = tsdf_amd.Mesh()
    for which, chunks_so_far in ((box, 2), (None, whole_chunks), (box, whole_chunks)):
        what = "box %r" % (which,)
        volume.extract_mesh(box=which, normals=True, into=subject)
        fresh = volume.extract_mesh(box=which, normals=True)
        assert subject.n_vertices == fresh.n_vertices > 0 and subject.n_indices == fresh.n_indices > 0, what
        assert_same_floats(subject.vertices, fresh.vertices, what + ": vertices")
        assert np.array_equal(subject.indices, fresh.indices), what + ": indices"
        assert_same_floats(subject.normals, fresh.normals, what + ": normals")
        assert subject.scratch_bytes == mesh_scratch_after(chunks_so_far), what
        assert fresh.scratch_bytes == mesh_scratch_after(2 if which else whole_chunks), what
        fresh.close()
    subject.close()
    volume.close()


def test_esdf_handle_small_large_small():
    grids = ((16, 10, 12), GRID, (16, 10, 12))
    subject = tsdf_amd.ESDF()
    empty = subject.scratch_bytes                    # the flags and the count: what a handle holds before any computation
    largest = 0
    for i, grid in enumerate(grids):
        volume, _ = sphere_volume(grid, tuple(75.0 * g for g in grid))
        n = grid[0] * grid[1] * grid[2]
        largest = max(largest, n)
        volume.compute_esdf(max_distance=600.0, into=subject)
        fresh = volume.compute_esdf(max_distance=600.0)
        what = "grid %r" % (grid,)
        assert subject.n_sites == fresh.n_sites > 0, what
        assert_same_floats(subject.distances, fresh.distances, what + ": distances")
        # the one-shot host variant, n = 1, 1000, 1
        P = (query_points(COUNTS[i], 500 + i) / np.array(PHYSICAL) * np.array([75.0 * g for g in grid])).astype(np.float32)
        for got, want, name in zip(subject.sample(P, gradient=True), fresh.sample(P, gradient=True), ("distance", "gradient")):
            assert_same_floats(got, want, what + ": sampled " + name)
        assert subject.scratch_bytes == empty + 4 * largest <= 4 * largest + 65536, what
        assert fresh.scratch_bytes == empty + 4 * n, what
        fresh.close()
        volume.close()
    subject.close()


# ---- volume fusion: the scratch holds the source's summary, so it grows with the source ----------------------------------------------
@pytest.mark.parametrize("storage", STORAGE)
def test_fuse_small_then_larger_source(storage):
    subject = new_volume(storage)
    total = 0
    for grid in ((16, 10, 12), (48, 40, 44), (16, 10, 12)):
        source, _ = sphere_volume(grid, PHYSICAL)
        fresh = fresh_with(state_of(subject), storage)
        got, want = subject.fuse(source), fresh.fuse(source)
        what = "%s, source %r" % (storage, grid)
        assert got == want, what + ": fused voxels"
        assert subject.last_fuse_bricks() == fresh.last_fuse_bricks(), what
        assert_same_state(subject, fresh, what)
        total += got
        fresh.close()
        source.close()
    assert total > 0
    subject.close()
