"""GPU: the mesh simplification (include/tsdf_amd.h, "mesh simplification") against the CPU reference tests/simplify_ref.py, bit for bit:
the hand-made cases through tsdf_simplify_mesh_device (the smallest meshes at which the cell table, the scans, the order by
representative and the integer sums can go wrong), every one run twice; the refusals; then meshes of random fields, of the sphere scene
and of a fused scene through Mesh.simplify, what it must leave alone, a reused handle with its scratch bound, and a chain with the
components filter."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import components_ref
from tests import simplify_ref as ref
from tests.helpers import H, W, assert_same_floats
from tests.test_components_ref_host import MESH_GRIDS, mesh_seed
from tests.test_mesh_indexed import fused_scene, volume_of
from tsdf_amd import _capi, synth

pytestmark = pytest.mark.gpu

CASES = ref.hand_made_cases()
lib = _capi.lib
INVALID = _capi.TSDF_ERR_INVALID
SENTINEL = 0xA5
FRESH_HANDLE = 256 * 32 + 256 + 16                                    # the marching cubes table and the two pinned totals
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def scratch_bound(n_vertices, n_triples, n_clusters):
    """The header's formula for a simplification into a fresh handle."""
    P = 2
    while P < 2 * n_vertices:
        P *= 2
    v_chunks, t_chunks = (n_vertices + 63) // 64, (n_triples + 63) // 64
    return FRESH_HANDLE + 12 * P + 4 * n_vertices + 80 * n_clusters + 12 * (v_chunks + t_chunks) + 16 * ((max(v_chunks, t_chunks) + 1023) // 1024 + 1) + 8


def mesh_arrays(mesh):
    f = mesh.info().flags
    return (mesh.vertices, mesh.indices, mesh.normals if f & 1 else None, mesh.colours if f & 2 else None)


def assert_simplified(got, src, h, what):
    """`got` (V, I, N or None, RGB or None) is the reference's simplification of `src` at h; returns the reference's clusters."""
    V, I, N, RGB = src
    rV, rI, rN, rC, cluster = ref.simplify(V, I, h, N, RGB)
    assert got[0].shape == rV.shape and got[0].dtype == np.float32, (what, got[0].shape, rV.shape)
    assert np.array_equal(bits(got[0]), bits(rV)), what + ": vertices"              # no position is computed to NaN: the very bits
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], rI), what + ": indices"
    assert (got[2] is None) == (N is None) and (got[3] is None) == (RGB is None), what
    if N is not None:
        assert_same_floats(got[2], rN, what + ": normals")
    if RGB is not None:
        assert got[3].dtype == np.uint8 and np.array_equal(got[3], rC), what + ": colours"
    return cluster


def same_bytes(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made_cases_equal_the_reference_twice(name):
    V, I, h, N, RGB = CASES[name]
    runs = [tsdf_amd.simplify_mesh(V, I, h, N, RGB) for _ in range(2)]
    for got in runs:
        assert_simplified(got, (V, I, N, RGB), h, name)
    assert same_bytes(runs[0], runs[1]), name
    if name == "one cell":
        assert runs[0][0].shape == (1, 3) and runs[0][1].shape == (0,)
    if name == "own cells":                                           # the identity
        assert same_bytes(runs[0], (V, I, N, RGB))


class Device:
    """Device copies of host arrays for one test, each with a sentinel word behind it."""

    def __init__(self):
        self.held = []

    def put(self, host):
        raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        padded = np.concatenate([raw, np.full(8, SENTINEL, np.uint8)])
        p = C.c_void_p()
        _capi.check(lib.tsdf_device_alloc(padded.nbytes, C.byref(p)))
        self.held.append(p)
        _capi.check(lib.tsdf_device_upload(p, padded.ctypes.data, padded.nbytes))
        return p, padded

    def unchanged(self, p, padded):
        out = np.empty_like(padded)
        _capi.check(lib.tsdf_device_download(out.ctypes.data, p, out.nbytes))
        return np.array_equal(out, padded)

    def close(self):
        for p in self.held:
            lib.tsdf_device_free(p)
        self.held = []


@pytest.fixture
def device():
    d = Device()
    yield d
    d.close()


def test_refusals_touch_nothing_and_a_good_call_follows(device):
    V, I, h, N, RGB = CASES["paired 65"]
    n, ni = len(V), len(I)
    held = [device.put(a) for a in (V, I, N, RGB)]
    (dV, _), (dI, _), (dN, _), (dC, _) = held
    dst = tsdf_amd.Mesh()
    big = tsdf_amd.simplify_mesh_device(n, ni, dV.value, dI.value, h, dst, dN.value, dC.value)      # dst holds something to lose
    assert big is dst and dst.n_vertices > 0
    call = lambda nv, ni_, v, i, cell, flags, d: lib.tsdf_simplify_mesh_device(nv, ni_, v, i, dN, dC, cell, flags, d, None)

    def refused(rc, words):
        assert rc == INVALID and words in _capi.last_error(), (rc, words, _capi.last_error())
    refused(call(n, ni, dV, dI, h, 0, None), "null dst")
    refused(call(n, ni, None, dI, h, 0, dst._h), "null device_vertices")
    refused(call(n, ni, dV, None, h, 0, dst._h), "null device_indices")
    refused(call(n, ni - 1, dV, dI, h, 0, dst._h), "multiple of 3")
    refused(call(2 ** 32, ni, dV, dI, h, 0, dst._h), "32-bit")
    refused(call(n, 3 * 2 ** 31, dV, dI, h, 0, dst._h), "32-bit")
    refused(call(2 ** 30 + 1, ni, dV, dI, h, 0, dst._h), "2^30")
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        refused(call(n, ni, dV, dI, bad, 0, dst._h), "cell_size")
    refused(call(n, ni, dV, dI, h, 1, dst._h), "unknown flags")
    refused(call(0, 3, None, dI, h, 0, dst._h), "not below n_vertices")
    # an index equal to n_vertices, in each of the three places: found on the device, dst left empty, nothing past the arrays touched
    for place in (0, 1, 2):
        bad = I.copy()
        bad[3 * 40 + place] = n
        dB, padded = device.put(bad)
        refused(call(n, ni, dV, dB, h, 0, dst._h), "not below n_vertices")
        assert (dst.n_vertices, dst.n_indices) == (0, 0) and dst.vertices.shape == (0, 3)
        assert device.unchanged(dB, padded)
    assert all(device.unchanged(p, padded) for p, padded in held)
    # the same dst serves a good call afterwards, exactly
    tsdf_amd.simplify_mesh_device(n, ni, dV.value, dI.value, h, dst, dN.value, dC.value)
    assert_simplified(mesh_arrays(dst), (V, I, N, RGB), h, "after the refusals")
    assert list(dst.info().box) == [0] * 6 and dst.info().flags == 3
    assert all(device.unchanged(p, padded) for p, padded in held)
    # the handle calls
    other = tsdf_amd.Mesh()
    refused(lib.tsdf_mesh_simplify(None, h, 0, dst._h, None), "null src")
    refused(lib.tsdf_mesh_simplify(dst._h, h, 0, None, None), "null dst")
    with pytest.raises(ValueError, match="dst is src"):
        dst.simplify(h, into=dst)
    refused(lib.tsdf_mesh_simplify(dst._h, h, 2, other._h, None), "unknown flags")
    for bad in (0.0, -5.0, float("nan")):
        with pytest.raises(ValueError, match="cell_size"):
            dst.simplify(bad, into=other)
    with pytest.raises(ValueError, match="not been labelled"):      # a simplified mesh is not labelled
        dst.labels


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def multi_member(cluster):
    return int((np.bincount(cluster) > 1).sum()) if len(cluster) else 0


def test_random_field_meshes_equal_the_reference(oracle):
    clusters = triples = 0
    dst = tsdf_amd.Mesh()
    for size in MESH_GRIDS:
        gv, _ = volume_of(size, mesh_seed(size))
        mesh = gv.extract_mesh()
        src = mesh_arrays(mesh)
        assert ref.cells(src[0], 25.0)[0].any()                      # loose vertices: the NaN crossings
        runs = []
        for _ in range(2):
            assert mesh.simplify(25.0, into=dst) is dst
            runs.append(mesh_arrays(dst))
        cluster = assert_simplified(runs[0], src, 25.0, "grid %s" % (size,))
        assert same_bytes(runs[0], runs[1])
        assert dst.box == mesh.box and dst.info().flags == 0
        clusters += multi_member(cluster)
        triples += dst.n_indices // 3
        if size == (40, 33, 21):
            assert multi_member(cluster) > 100 and dst.n_indices // 3 > 100 and 0 < dst.n_indices < mesh.n_indices
    assert clusters > 100 and triples > 100


@pytest.fixture(scope="module")
def sphere():
    gv = tsdf_amd.TSDFVolume(components_ref.SCENE_SIZE, (640.0,) * 3)
    gv.set_distance_data(components_ref.sphere_scene())
    return gv


@pytest.mark.parametrize("cell,counts", [(20.0, (871, 1728)), (40.0, (247, 480)), (2.0 ** -8, (4410, 8800))])
def test_the_sphere_scene_equals_the_reference(sphere, cell, counts):
    mesh = sphere.extract_mesh(normals=True)
    src = mesh_arrays(mesh)
    assert (len(src[0]), len(src[1]) // 3) == (4422, 8824)
    src = (src[0], src[1], ref.sphere_normals(src[0], components_ref.SCENE_SPHERES, 10.0), None)
    runs = [tsdf_amd.simplify_mesh(*src[:2], cell, normals=src[2]) for _ in range(2)]
    cluster = assert_simplified(runs[0], src, cell, "sphere scene at %g" % cell)
    assert same_bytes(runs[0], runs[1])
    assert (len(runs[0][0]), len(runs[0][1]) // 3) == counts
    if cell >= 20.0:
        assert multi_member(cluster) > 100 and len(runs[0][1]) // 3 > 100
        assert np.abs(np.linalg.norm(runs[0][2].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    # ... and handle to handle, with the normals the extraction gave
    dst = mesh.simplify(cell)
    assert_simplified(mesh_arrays(dst), mesh_arrays(mesh), cell, "sphere scene handle at %g" % cell)
    assert (dst.n_vertices, dst.n_indices // 3) == counts and dst.info().flags == 1 and dst.box == mesh.box


@pytest.fixture(scope="module")
def scene():
    return fused_scene(True)


def test_a_fused_scene_with_normals_and_colours(scene):
    cell = 2 * 3000.0 / 64
    mesh = scene.extract_mesh(normals=True, colours=True)
    src = mesh_arrays(mesh)
    before = [a.tobytes() for a in src]
    dst = tsdf_amd.Mesh()
    runs = []
    for _ in range(2):
        mesh.simplify(cell, into=dst)
        runs.append(mesh_arrays(dst))
    cluster = assert_simplified(runs[0], src, cell, "fused scene")
    assert same_bytes(runs[0], runs[1])
    assert multi_member(cluster) > 100 and dst.n_indices // 3 > 100 and dst.n_vertices < mesh.n_vertices / 3
    assert dst.info().flags == 3 and dst.box == mesh.box
    assert np.isfinite(runs[0][2]).all(axis=1).sum() > dst.n_vertices // 2 and len(np.unique(runs[0][3], axis=0)) > 10
    assert [a.tobytes() for a in mesh_arrays(mesh)] == before        # src's four arrays are unchanged
    assert dst.scratch_bytes <= scratch_bound(mesh.n_vertices, mesh.n_indices // 3, dst.n_vertices)


def test_simplification_leaves_the_source_the_volume_the_soup_and_the_ray_cast_alone(sphere):
    gv = sphere
    cam = synth.camera_for_frame(4, 40)
    caster = tsdf_amd.GPURaycaster(W, H)
    S0 = gv.extract_surface()
    V0, N0 = caster.raycast(gv, cam)
    D0, W0 = gv.get_distance_data(), gv.get_weight_data()
    mesh = gv.extract_mesh(normals=True)
    mesh.label_components()
    before = [a.tobytes() for a in mesh_arrays(mesh)[:3]] + [mesh.labels.tobytes(), mesh.component_triangles.tobytes()]
    small = mesh.simplify(20.0)
    assert mesh.n_vertices > small.n_vertices > 0
    assert [a.tobytes() for a in mesh_arrays(mesh)[:3]] + [mesh.labels.tobytes(), mesh.component_triangles.tobytes()] == before
    V1, N1 = caster.raycast(gv, cam)
    assert_same_floats(V1, V0, "ray cast vertices")
    assert_same_floats(N1, N0, "ray cast normals")
    assert_same_floats(gv.extract_surface(), S0, "soup")
    assert_same_floats(gv.get_distance_data(), D0, "distances")
    assert_same_floats(gv.get_weight_data(), W0, "weights")


def test_a_reused_handle_is_exact_and_its_scratch_stays_within_the_bound(scene, sphere):
    dst = tsdf_amd.Mesh()
    assert dst.scratch_bytes == FRESH_HANDLE
    big = scene.extract_mesh(normals=True, colours=True)
    big.simplify(30.0, into=dst)
    assert_simplified(mesh_arrays(dst), mesh_arrays(big), 30.0, "big")
    bound = scratch_bound(big.n_vertices, big.n_indices // 3, dst.n_vertices)
    assert FRESH_HANDLE < dst.scratch_bytes <= bound
    held = dst.scratch_bytes
    # a small one into the same handle: nothing of the big one shows, nothing grows
    for name in ("interleaved", "loose", "triples", "colours", "empty", "no indices"):
        V, I, h, N, RGB = CASES[name]
        with tsdf_amd.api._DeviceArray(V) as dv, tsdf_amd.api._DeviceArray(I) as di, tsdf_amd.api._DeviceArray(N, 0) as dn, \
                tsdf_amd.api._DeviceArray(RGB, 0) as dc:
            tsdf_amd.simplify_mesh_device(len(V), len(I), dv.ptr.value, di.ptr.value, h, dst, dn.ptr.value if N is not None else 0,
                                          dc.ptr.value if RGB is not None else 0)
            assert_simplified(mesh_arrays(dst), (V, I, N, RGB), h, "small: " + name)
        assert dst.scratch_bytes == held
    small = sphere.extract_mesh()
    small.simplify(40.0, into=dst)
    assert_simplified(mesh_arrays(dst), mesh_arrays(small), 40.0, "small")
    assert dst.scratch_bytes == held and small.n_vertices < big.n_vertices
    # ... and the big one again, warm: the same bytes, no growth
    first = big.simplify(30.0)
    big.simplify(30.0, into=dst)
    assert same_bytes(mesh_arrays(dst), mesh_arrays(first)) and dst.scratch_bytes == held
    assert first.scratch_bytes <= bound


def test_a_chain_with_the_components_filter(sphere):
    mesh = sphere.extract_mesh(normals=True)
    V, I, N, _ = mesh_arrays(mesh)
    kept = mesh.filter_components(components_ref.SCENE_MIN_TRIANGLES)
    small = kept.simplify(40.0)
    info = small.label_components()
    final = small.filter_components(1)
    # the reference chain
    L, T, rinfo = components_ref.label(len(V), I)
    (kV, kN), kI, _ = components_ref.filter_mesh(L, T, rinfo, I, [V, N], components_ref.SCENE_MIN_TRIANGLES)
    assert_same_floats(kept.vertices, kV, "filtered")
    sV, sI, sN, _, _ = ref.simplify(kV, kI, 40.0, kN)
    assert_simplified(mesh_arrays(small), (kV, kI, kN, None), 40.0, "simplified")
    L2, T2, info2 = components_ref.label(len(sV), sI)
    assert info == info2 and np.array_equal(small.labels, L2) and np.array_equal(small.component_triangles, T2)
    (fV, fN), fI, keep = components_ref.filter_mesh(L2, T2, info2, sI, [sV, sN], 1)
    got = mesh_arrays(final)
    assert np.array_equal(bits(got[0]), bits(fV)) and np.array_equal(got[1], fI)
    assert_same_floats(got[2], fN, "final normals")
    assert len(fI) > 300 and np.array_equal(np.unique(got[1]), np.arange(final.n_vertices))      # no unreferenced vertex is left
    assert final.box == mesh.box and final.info().flags == 1


def test_an_empty_mesh():
    plain = tsdf_amd.TSDFVolume((16, 16, 16), (160.0,) * 3)
    mesh = plain.extract_mesh(normals=True)
    dst = tsdf_amd.Mesh()
    V, I, h, N, RGB = CASES["triples"]
    for _ in range(2):                                                # into a fresh handle, then into one that held something
        mesh.simplify(10.0, into=dst)
        assert (dst.n_vertices, dst.n_indices) == (0, 0) and dst.vertices.shape == (0, 3) and dst.normals.shape == (0, 3)
        assert dst.box == mesh.box and dst.info().flags == 1 and dst.device_buffers() == (0, 0, 0, 0)
        assert dst.simplify(10.0).n_vertices == 0
        with tsdf_amd.api._DeviceArray(V) as dv, tsdf_amd.api._DeviceArray(I) as di:
            tsdf_amd.simplify_mesh_device(len(V), len(I), dv.ptr.value, di.ptr.value, h, dst)
            assert dst.n_vertices == 4
