"""GPU: the mesh smoothing (include/tsdf_amd.h, "mesh smoothing") against the CPU reference tests/smooth_ref.py, bit for bit: the
hand-made cases through tsdf_smooth_mesh_device (the smallest meshes at which the rows, the scans, the edge table and the sums can go
wrong) with and without each flag, every one run twice; tsdf_vertex_normals_device on the same cases; the refusals; then meshes of
random fields, of the sphere scene and of a fused scene through Mesh.smooth, a box mesh with its border pinned, Mesh.compute_normals
after a simplification, a chain with the simplification and the components filter, a reused handle with its scratch formula, and
two handles that serve every operation in turn."""
import collections

import numpy as np
import pytest

import tsdf_amd
from tests import components_ref
from tests import simplify_ref
from tests import smooth_ref as ref
from tests.helpers import assert_same_floats
from tests.test_components_ref_host import MESH_GRIDS, mesh_seed
from tests.test_mesh_indexed import fused_scene, volume_of
from tests.test_smooth_ref_host import large_sphere
from tests.test_simplify import FRESH_HANDLE, Device, assert_simplified, mesh_arrays, same_bytes
from tsdf_amd import _capi

pytestmark = pytest.mark.gpu

CASES = ref.hand_made_cases()
lib = _capi.lib
INVALID = _capi.TSDF_ERR_INVALID
PIN, NORMALS = ref.PIN_BOUNDARY, ref.NORMALS
TAUBIN = (10, 0.5, -0.53)
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def scratch_formula(n_vertices, n_triples, passes, flags):
    """The header's formula for a smoothing into a fresh handle."""
    v_chunks = (n_vertices + 63) // 64
    total = FRESH_HANDLE + 16 * ((v_chunks + 1023) // 1024 + 1) + 8
    if n_triples == 0:
        passes = 0
    if passes > 0:
        total += 8 * n_vertices + 8 * 3 * n_triples + 4 * v_chunks
    if passes > 1:
        total += 12 * n_vertices
    if passes > 0 and flags & PIN:
        E = 2
        while E < 2 * 3 * n_triples:
            E *= 2
        total += n_vertices + 12 * E
    if flags & NORMALS:
        total += 24 * n_vertices
    return total


def assert_smoothed(got, src, args, flags, what):
    """`got` (V, I, N or None, RGB or None) is the reference's smoothing of `src` with args = (iterations, lambda, mu); returns the
    reference's positions."""
    V, I, N, RGB = src
    rV = ref.smooth(V, I, *args, flags)
    assert got[0].shape == rV.shape and got[0].dtype == np.float32, (what, got[0].shape, rV.shape)
    assert np.array_equal(bits(got[0]), bits(rV)), what + ": vertices"     # no position is computed to NaN: the very bits
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], I), what + ": indices"
    assert (got[2] is None) == (N is None and not flags & NORMALS) and (got[3] is None) == (RGB is None), what
    if flags & NORMALS:
        assert_same_floats(got[2], ref.vertex_normals(rV, I), what + ": face normals")
    elif N is not None:
        assert got[2].tobytes() == N.tobytes(), what + ": normals"
    if RGB is not None:
        assert got[3].dtype == np.uint8 and got[3].tobytes() == RGB.tobytes(), what + ": colours"
    return rV


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made_cases_equal_the_reference_twice(name):
    V, I, it, lam, mu = CASES[name]
    rng = np.random.default_rng(len(V))
    N, RGB = simplify_ref.unit(rng, len(V)), rng.integers(0, 256, (len(V), 3)).astype(np.uint8)
    for flags in (0, PIN, NORMALS, PIN | NORMALS):
        runs = [tsdf_amd.smooth_mesh(V, I, it, lam, mu, bool(flags & PIN), bool(flags & NORMALS), N, RGB) for _ in range(2)]
        for got in runs:
            rV = assert_smoothed(got, (V, I, N, RGB), (it, lam, mu), flags, "%s flags %d" % (name, flags))
        assert same_bytes(runs[0], runs[1]), name
        if name in ("no iterations", "minus zero factors", "empty", "no triple") or (flags & PIN and name in ("one triangle", "two triangles")):
            assert runs[0][0].tobytes() == V.tobytes(), name           # the identity
        if name == "guard":
            assert np.isfinite(rV).all() and runs[0][0].tobytes() != V.tobytes()
    # without normals or colours given: none come back
    got = tsdf_amd.smooth_mesh(V, I, it, lam, mu)
    assert_smoothed(got, (V, I, None, None), (it, lam, mu), 0, name + " bare")


@pytest.mark.parametrize("name", sorted(CASES))
def test_vertex_normals_of_the_hand_made_cases(name):
    V, I = CASES[name][:2]
    runs = [tsdf_amd.vertex_normals(V, I) for _ in range(2)]
    assert runs[0].shape == V.shape and runs[0].dtype == np.float32
    assert_same_floats(runs[0], ref.vertex_normals(V, I), name)
    assert runs[0].tobytes() == runs[1].tobytes()
    if name == "tetrahedron":                                           # wired like extract_surface's triangles: outwards
        assert ((runs[0].astype(np.float64) * (V - V.mean(axis=0))).sum(axis=1) > 0).all()


@pytest.fixture
def device():
    d = Device()
    yield d
    d.close()


def test_refusals_touch_nothing_and_a_good_call_follows(device):
    V, I, it, lam, mu = CASES["strip 129"]
    rng = np.random.default_rng(7)
    N, RGB = simplify_ref.unit(rng, len(V)), rng.integers(0, 256, (len(V), 3)).astype(np.uint8)
    n, ni = len(V), len(I)
    held = [device.put(a) for a in (V, I, N, RGB)]
    (dV, _), (dI, _), (dN, _), (dC, _) = held
    dO, out_padded = device.put(np.zeros((n, 3), np.float32))
    dst = tsdf_amd.Mesh()
    big = tsdf_amd.smooth_mesh_device(n, ni, dV.value, dI.value, dst, it, lam, mu, normals_ptr=dN.value, colours_ptr=dC.value)   # dst holds something to lose
    assert big is dst and dst.n_vertices == n
    call = lambda nv, ni_, v, i, its, l, m, flags, d: lib.tsdf_smooth_mesh_device(nv, ni_, v, i, dN, dC, its, l, m, flags, d, None)

    def refused(rc, words):
        assert rc == INVALID and words in _capi.last_error(), (rc, words, _capi.last_error())
    refused(call(n, ni, dV, dI, it, lam, mu, 0, None), "null dst")
    refused(call(n, ni, None, dI, it, lam, mu, 0, dst._h), "null device_vertices")
    refused(call(n, ni, dV, None, it, lam, mu, 0, dst._h), "null device_indices")
    refused(call(n, ni - 1, dV, dI, it, lam, mu, 0, dst._h), "multiple of 3")
    refused(call(2 ** 32, ni, dV, dI, it, lam, mu, 0, dst._h), "32-bit")
    refused(call(n, 3 * 2 ** 31, dV, dI, it, lam, mu, 0, dst._h), "32-bit")
    for bad in (float("inf"), float("-inf"), float("nan")):
        refused(call(n, ni, dV, dI, it, bad, mu, 0, dst._h), "finite")
        refused(call(n, ni, dV, dI, it, lam, bad, 0, dst._h), "finite")
    refused(call(n, ni, dV, dI, 1025, lam, mu, 0, dst._h), "iterations")
    refused(call(n, ni, dV, dI, it, lam, mu, 4, dst._h), "unknown flags")
    refused(call(0, 3, None, dI, it, lam, mu, 0, dst._h), "not below n_vertices")
    # an index equal to n_vertices, in each of the three places: found on the device, dst left empty, nothing past the arrays touched;
    # with and without passes, pins and normals
    for place, (its, flags) in zip((0, 1, 2), ((it, 0), (0, NORMALS), (it, PIN | NORMALS))):
        bad = I.copy()
        bad[3 * 40 + place] = n
        dB, padded = device.put(bad)
        refused(call(n, ni, dV, dB, its, lam, mu, flags, dst._h), "not below n_vertices")
        assert (dst.n_vertices, dst.n_indices) == (0, 0) and dst.vertices.shape == (0, 3)
        assert device.unchanged(dB, padded)
        refused(lib.tsdf_vertex_normals_device(n, ni, dV, dB, dO, None), "not below n_vertices")
        got = np.empty_like(out_padded)                               # (its n_vertices triples are unspecified; nothing behind them is touched)
        _capi.check(lib.tsdf_device_download(got.ctypes.data, dO, got.nbytes))
        assert device.unchanged(dB, padded) and (got[-8:] == out_padded[-8:]).all()
    assert all(device.unchanged(p, padded) for p, padded in held)
    # the same dst serves a good call afterwards, exactly
    tsdf_amd.smooth_mesh_device(n, ni, dV.value, dI.value, dst, it, lam, mu, True, False, dN.value, dC.value)
    assert_smoothed(mesh_arrays(dst), (V, I, N, RGB), (it, lam, mu), PIN, "after the refusals")
    assert list(dst.info().box) == [0] * 6 and dst.info().flags == 3
    assert all(device.unchanged(p, padded) for p, padded in held)
    # the normals call writes its n_vertices triples and nothing behind them
    _capi.check(lib.tsdf_vertex_normals_device(n, ni, dV, dI, dO, None))
    got = np.empty_like(out_padded)
    _capi.check(lib.tsdf_device_download(got.ctypes.data, dO, got.nbytes))
    assert_same_floats(got[:-8].view(np.float32), ref.vertex_normals(V, I), "normals on the device")
    assert (got[-8:] == out_padded[-8:]).all()
    # the handle calls
    other = tsdf_amd.Mesh()
    refused(lib.tsdf_mesh_smooth(None, it, lam, mu, 0, dst._h, None), "null src")
    refused(lib.tsdf_mesh_smooth(dst._h, it, lam, mu, 0, None, None), "null dst")
    with pytest.raises(ValueError, match="dst is src"):
        dst.smooth(into=dst)
    refused(lib.tsdf_mesh_smooth(dst._h, it, lam, mu, 8, other._h, None), "unknown flags")
    with pytest.raises(ValueError, match="finite"):
        dst.smooth(lam=float("nan"), into=other)
    with pytest.raises(ValueError, match="iterations"):
        dst.smooth(iterations=2000, into=other)
    refused(lib.tsdf_mesh_compute_normals(None, None), "null mesh")
    with pytest.raises(ValueError, match="not been labelled"):       # a smoothed mesh is not labelled
        dst.labels


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def test_random_field_meshes_equal_the_reference(oracle):
    moved = 0
    dst = tsdf_amd.Mesh()
    for size in MESH_GRIDS:
        gv, _ = volume_of(size, mesh_seed(size))
        mesh = gv.extract_mesh()
        src = mesh_arrays(mesh)
        before = [a.tobytes() for a in src[:2]]
        assert ref.loose_vertices(src[0]).any() and ref.pinned(src[0], src[1]).any()     # the NaN crossings; the grid's faces
        for flags in (0, PIN | NORMALS):
            runs = []
            for _ in range(2):
                assert mesh.smooth(*TAUBIN, pin_boundary=bool(flags & PIN), normals=bool(flags & NORMALS), into=dst) is dst
                runs.append(mesh_arrays(dst))
            rV = assert_smoothed(runs[0], src, TAUBIN, flags, "grid %s flags %d" % (size, flags))
            assert same_bytes(runs[0], runs[1])
            assert dst.box == mesh.box and dst.info().flags == (1 if flags & NORMALS else 0)
            moved += int((bits(rV) != bits(src[0])).any(axis=1).sum())
        assert [a.tobytes() for a in mesh_arrays(mesh)[:2]] == before   # src is unchanged
    assert moved > 10000


@pytest.fixture(scope="module")
def sphere():
    gv = tsdf_amd.TSDFVolume(components_ref.SCENE_SIZE, (640.0,) * 3)
    gv.set_distance_data(components_ref.sphere_scene())
    return gv


def test_the_sphere_scene_equals_the_reference(sphere):
    mesh = sphere.extract_mesh(normals=True)
    src = mesh_arrays(mesh)
    before = [a.tobytes() for a in src[:3]]
    assert (len(src[0]), len(src[1]) // 3) == (4422, 8824)
    kept = mesh.smooth(*TAUBIN)                                       # the field's normals are carried along
    assert_smoothed(mesh_arrays(kept), src, TAUBIN, 0, "sphere scene")
    faced = mesh.smooth(*TAUBIN, normals=True)
    assert_smoothed(mesh_arrays(faced), src, TAUBIN, NORMALS, "sphere scene, face normals")
    assert kept.info().flags == 1 and faced.info().flags == 1 and faced.box == mesh.box
    # the face normals of the untouched surface point out of it, like the field's gradient
    own = tsdf_amd.vertex_normals(src[0], src[1]).astype(np.float64)
    near, _, outward = large_sphere(src[0])
    assert near.sum() > 3000 and ((own[near] * outward).sum(axis=1) > 0.99).all()
    assert ((src[2][near].astype(np.float64) * outward).sum(axis=1) > 0.99).all()
    # the plain Laplacian, and Mesh.compute_normals on the result
    plain = mesh.smooth(10, 0.5, 0.0)
    assert_smoothed(mesh_arrays(plain), src, (10, 0.5, 0.0), 0, "sphere scene, Laplacian")
    assert plain.compute_normals() is plain
    assert_same_floats(plain.normals, ref.vertex_normals(plain.vertices, src[1]), "compute_normals")
    assert [a.tobytes() for a in mesh_arrays(mesh)[:3]] == before


@pytest.fixture(scope="module")
def scene():
    return fused_scene(True)


def test_a_fused_scene_with_normals_and_colours(scene):
    mesh = scene.extract_mesh(normals=True, colours=True)
    src = mesh_arrays(mesh)
    before = [a.tobytes() for a in src]
    dst = tsdf_amd.Mesh()
    for flags in (PIN, NORMALS):
        runs = []
        for _ in range(2):
            mesh.smooth(*TAUBIN, pin_boundary=bool(flags & PIN), normals=bool(flags & NORMALS), into=dst)
            runs.append(mesh_arrays(dst))
        rV = assert_smoothed(runs[0], src, TAUBIN, flags, "fused scene flags %d" % flags)
        assert same_bytes(runs[0], runs[1])
        assert dst.info().flags == 3 and dst.box == mesh.box
        assert (bits(rV) != bits(src[0])).any(axis=1).sum() > mesh.n_vertices // 2
    assert [a.tobytes() for a in mesh_arrays(mesh)] == before        # src's four arrays are unchanged


def test_a_box_mesh_with_pins_keeps_its_border_and_neighbouring_boxes_still_agree(sphere):
    left, right = sphere.extract_mesh(box=(0, 0, 0, 24, 64, 64)), sphere.extract_mesh(box=(24, 0, 0, 64, 64, 64))
    out = []
    for mesh in (left, right):
        V, I = mesh.vertices, mesh.indices
        pins = ref.pinned(V, I)
        got = mesh.smooth(*TAUBIN, pin_boundary=True)
        assert_smoothed(mesh_arrays(got), (V, I, None, None), TAUBIN, PIN, "box %s" % (mesh.box,))
        moved = (bits(got.vertices) != bits(V)).any(axis=1)
        assert pins.any() and not moved[pins].any() and moved.any()
        out.append((V, got.vertices, pins))
    assert len(out[0][0]) == 1960 and out[0][2].sum() == 108
    # the vertices the two boxes share (the same lattice edge has the same bytes in both) have the same bytes after smoothing too
    def once(V):                                                      # (positions that several lattice edges share are left out)
        keys = [v.tobytes() for v in V]
        count = collections.Counter(keys)
        return {k: i for i, k in enumerate(keys) if count[k] == 1}
    a, b = once(out[0][0]), once(out[1][0])
    shared = [(a[k], b[k]) for k in a if k in b]
    assert len(shared) == 108
    for i, j in shared:
        assert out[0][2][i] and out[1][2][j] and out[0][1][i].tobytes() == out[1][1][j].tobytes()
    # ... which smoothing without the flag breaks
    loose = [mesh.smooth(*TAUBIN).vertices for mesh in (left, right)]
    assert any(loose[0][i].tobytes() != loose[1][j].tobytes() for i, j in shared)


def test_compute_normals_after_a_simplification(sphere):
    mesh = sphere.extract_mesh()
    small = mesh.simplify(20.0)
    assert small.info().flags == 0
    with pytest.raises(ValueError):
        small.normals
    V, I = small.vertices, small.indices
    for _ in range(2):                                                # creates the array, then replaces it
        small.compute_normals()
        assert small.info().flags == 1
        assert_same_floats(small.normals, ref.vertex_normals(V, I), "normals of the level of detail")
    assert small.vertices.tobytes() == V.tobytes() and small.indices.tobytes() == I.tobytes()
    N = small.normals.astype(np.float64)
    finite = np.isfinite(N).all(axis=1)
    assert finite.sum() > 800 and np.abs(np.linalg.norm(N[finite], axis=1) - 1.0).max() < 1e-6
    # a labelled mesh stays labelled; an empty one gains the flag and nothing else
    info = mesh.label_components()
    mesh.compute_normals()
    assert mesh.info().flags == 1 and len(mesh.labels) == mesh.n_vertices and info["n_components"] == 5
    assert_same_floats(mesh.normals, ref.vertex_normals(mesh.vertices, mesh.indices), "normals of the extraction")
    empty = tsdf_amd.TSDFVolume((16, 16, 16), (160.0,) * 3).extract_mesh()
    assert empty.compute_normals().info().flags == 1 and empty.normals.shape == (0, 3)


def test_a_chain_simplify_smooth_filter(sphere):
    mesh = sphere.extract_mesh(normals=True)
    V, I, N, _ = mesh_arrays(mesh)
    small = mesh.simplify(20.0)
    smooth = small.smooth(5, 0.5, -0.53, normals=True)
    final = smooth.filter_components(components_ref.SCENE_MIN_TRIANGLES)
    sV, sI, sN, _, _ = simplify_ref.simplify(V, I, 20.0, N)
    rV = assert_smoothed(mesh_arrays(smooth), (sV, sI, sN, None), (5, 0.5, -0.53), NORMALS, "simplified, then smoothed")
    rN = ref.vertex_normals(rV, sI)
    L, T, info = components_ref.label(len(rV), sI)
    (fV, fN), fI, keep = components_ref.filter_mesh(L, T, info, sI, [rV, rN], components_ref.SCENE_MIN_TRIANGLES)
    got = mesh_arrays(final)
    assert np.array_equal(bits(got[0]), bits(fV)) and np.array_equal(got[1], fI) and len(fI) > 300 and len(fV) < len(rV)
    assert_same_floats(got[2], fN, "final normals")
    assert final.box == mesh.box and final.info().flags == 1


def test_a_reused_handle_is_exact_and_its_scratch_follows_the_formula(scene, sphere):
    dst = tsdf_amd.Mesh()
    assert dst.scratch_bytes == FRESH_HANDLE
    big = scene.extract_mesh(normals=True, colours=True)
    nv, nt = big.n_vertices, big.n_indices // 3
    big.smooth(*TAUBIN, pin_boundary=True, normals=True, into=dst)
    first = mesh_arrays(dst)
    assert_smoothed(first, mesh_arrays(big), TAUBIN, PIN | NORMALS, "big")
    held = dst.scratch_bytes
    assert held == scratch_formula(nv, nt, 20, PIN | NORMALS)
    # what each part of the formula is for, each into a fresh handle
    for args, flags, passes in (((0, 0.5, -0.53), 0, 0), ((1, 0.5, 0.0), 0, 1), (TAUBIN, 0, 20), (TAUBIN, PIN, 20), ((0, 0.5, -0.53), NORMALS, 0)):
        fresh = big.smooth(*args, pin_boundary=bool(flags & PIN), normals=bool(flags & NORMALS))
        assert fresh.scratch_bytes == scratch_formula(nv, nt, passes, flags), (args, flags)
    # small ones into the same handle: nothing of the big one shows, nothing grows
    for name in ("tetrahedron", "fan hub first", "strip 129", "empty", "no triple"):
        V, I, it, lam, mu = CASES[name]
        with tsdf_amd.api._DeviceArray(V) as dv, tsdf_amd.api._DeviceArray(I) as di:
            tsdf_amd.smooth_mesh_device(len(V), len(I), dv.ptr.value, di.ptr.value, dst, it, lam, mu, True, True)
            assert_smoothed(mesh_arrays(dst), (V, I, None, None), (it, lam, mu), PIN | NORMALS, "small: " + name)
        assert dst.scratch_bytes == held
    small = sphere.extract_mesh()
    small.smooth(*TAUBIN, into=dst)
    assert_smoothed(mesh_arrays(dst), mesh_arrays(small), TAUBIN, 0, "small")
    assert dst.scratch_bytes == held and small.n_vertices < big.n_vertices
    # ... and the big one again, warm: the same bytes, no growth
    big.smooth(*TAUBIN, pin_boundary=True, normals=True, into=dst)
    assert same_bytes(mesh_arrays(dst), first) and dst.scratch_bytes == held


def test_two_handles_serve_every_operation_in_turn(sphere):
    """Each handle is in turn the output of an extraction, a filter, a simplification and a smoothing, so every operation finds the
    scratch (parts, keep masks and bases, the table) as another one sized and left it."""
    a, b = tsdf_amd.Mesh(), tsdf_amd.Mesh()
    taubin = (5, 0.5, -0.53)

    def assert_filtered(got, src, min_triangles, what):
        V, I, N, _ = src
        L, T, info = components_ref.label(len(V), I)
        (fV, fN), fI, _ = components_ref.filter_mesh(L, T, info, I, [V, N], min_triangles)
        assert np.array_equal(bits(got[0]), bits(fV)) and np.array_equal(got[1], fI) and got[1].dtype == np.uint32, what
        assert_same_floats(got[2], fN, what + ": normals")
        assert got[3] is None and 0 < len(fV) <= len(V), what

    def chain(verify):
        steps = []
        assert sphere.extract_mesh(normals=True, into=a) is a
        steps.append(mesh_arrays(a))
        assert a.filter_components(components_ref.SCENE_MIN_TRIANGLES, into=b) is b
        steps.append(mesh_arrays(b))
        assert b.simplify(20.0, into=a) is a
        steps.append(mesh_arrays(a))
        assert a.smooth(*taubin, pin_boundary=True, normals=True, into=b) is b
        steps.append(mesh_arrays(b))
        assert b.compute_normals() is b
        steps.append(mesh_arrays(b))
        assert b.simplify(40.0, into=a) is a
        steps.append(mesh_arrays(a))
        assert a.filter_components(1, into=b) is b
        steps.append(mesh_arrays(b))
        assert a.box == b.box == (0, 0, 0, 63, 63, 63) and a.info().flags == b.info().flags == 1
        if verify:
            assert (len(steps[0][0]), len(steps[0][1]) // 3) == (4422, 8824)
            assert_filtered(steps[1], steps[0], components_ref.SCENE_MIN_TRIANGLES, "filtered")
            assert_simplified(steps[2], steps[1], 20.0, "simplified")
            rV = assert_smoothed(steps[3], steps[2], taubin, PIN | NORMALS, "smoothed")
            assert (bits(rV) != bits(steps[2][0])).any()                    # (the kept spheres are closed: the pins find no border)
            assert same_bytes(steps[4][:2], steps[3][:2])
            assert_same_floats(steps[4][2], ref.vertex_normals(steps[3][0], steps[3][1]), "compute_normals")
            assert_simplified(steps[5], steps[4], 40.0, "simplified again")
            assert_filtered(steps[6], steps[5], 1, "filtered again")
        return steps

    first = chain(True)
    held = (a.scratch_bytes, b.scratch_bytes)
    again = chain(False)
    assert all(same_bytes(x, y) for x, y in zip(first, again))         # warm scratch of other operations: the same bytes
    assert (a.scratch_bytes, b.scratch_bytes) == held


def test_an_empty_mesh():
    plain = tsdf_amd.TSDFVolume((16, 16, 16), (160.0,) * 3)
    mesh = plain.extract_mesh(normals=True)
    dst = tsdf_amd.Mesh()
    V, I, it, lam, mu = CASES["tetrahedron"]
    for _ in range(2):                                                # into a fresh handle, then into one that held something
        mesh.smooth(into=dst)
        assert (dst.n_vertices, dst.n_indices) == (0, 0) and dst.vertices.shape == (0, 3) and dst.normals.shape == (0, 3)
        assert dst.box == mesh.box and dst.info().flags == 1 and dst.device_buffers() == (0, 0, 0, 0)
        assert dst.smooth(pin_boundary=True, normals=True).n_vertices == 0
        with tsdf_amd.api._DeviceArray(V) as dv, tsdf_amd.api._DeviceArray(I) as di:
            tsdf_amd.smooth_mesh_device(len(V), len(I), dv.ptr.value, di.ptr.value, dst, it, lam, mu)
            assert dst.n_vertices == 4
    assert tsdf_amd.vertex_normals(np.zeros((0, 3), np.float32), []).shape == (0, 3)
