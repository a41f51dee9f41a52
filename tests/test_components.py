"""GPU: the mesh components (include/tsdf_amd.h, "mesh components") against the CPU reference tests/components_ref.py, bit for bit:
hand-made index buffers through tsdf_label_components_device (the smallest graphs at which a lock-free union-find can go wrong: deep
chains, one contended word, the take-over of one component, degenerate and repeated triples), every one run twice; the refusals; then
meshes of random fields and of a sphere scene through Mesh.label_components / Mesh.filter_components, with what they must leave alone."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import components_ref as ref
from tests import mesh_ref
from tests.helpers import H, W, assert_same_floats
from tests.test_components_ref_host import MESH_GRIDS, mesh_seed
from tests.test_mesh_indexed import reference, volume_of, within_bound
from tsdf_amd import _capi, synth

pytestmark = pytest.mark.gpu

CASES = ref.hand_made_cases()
lib = _capi.lib
INVALID = _capi.TSDF_ERR_INVALID
SENTINEL = 0xA5A5A5A5


class Device:
    """Device copies of host uint32 arrays for one test."""

    def __init__(self):
        self.held = []

    def put(self, host):
        host = np.ascontiguousarray(host, np.uint32)
        p = C.c_void_p()
        _capi.check(lib.tsdf_device_alloc(max(host.nbytes, 4), C.byref(p)))
        self.held.append(p)
        if host.nbytes:
            _capi.check(lib.tsdf_device_upload(p, host.ctypes.data, host.nbytes))
        return p

    def get(self, p, n):
        out = np.empty(n, np.uint32)
        if n:
            _capi.check(lib.tsdf_device_download(out.ctypes.data, p, out.nbytes))
        return out

    def close(self):
        for p in self.held:
            lib.tsdf_device_free(p)
        self.held = []


@pytest.fixture
def device():
    d = Device()
    yield d
    d.close()


def assert_info(info, rinfo, what=""):
    assert info == rinfo, (what, info, rinfo)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made_index_buffers_equal_the_reference_twice(name, device):
    n, I = CASES[name]
    rL, rT, rinfo = ref.label(n, I)
    runs = [tsdf_amd.label_components(n, I) for _ in range(2)]
    for L, T, info in runs:
        assert L.dtype == np.uint32 and T.dtype == np.uint32
        assert np.array_equal(L, rL), name
        assert np.array_equal(T, rT), name
        assert_info(info, rinfo, name)
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    # without the counter array: the same labels; the largest component is not looked for
    dI, dL = device.put(I), device.put(np.full(n, SENTINEL))
    info = tsdf_amd.label_components_device(n, len(I), dI.value if len(I) else 0, dL.value)
    assert np.array_equal(device.get(dL, n), rL)
    assert (info["n_components"], info["n_triangles"]) == (rinfo["n_components"], rinfo["n_triangles"])
    assert (info["largest_triangles"], info["largest_label"]) == (0, ref.NO_LABEL)


def test_refusals_touch_nothing(device):
    n, I = CASES["random 2000"]
    dI, dL, dT = device.put(I), device.put(np.full(n + 1, SENTINEL)), device.put(np.full(n + 1, SENTINEL))
    info = _capi.ComponentsInfo()
    call = lambda nv, ni, i, l, t: lib.tsdf_label_components_device(nv, ni, i, l, t, C.byref(info), None)
    untouched = lambda: (device.get(dL, n + 1) == SENTINEL).all() and (device.get(dT, n + 1) == SENTINEL).all()
    assert call(n, len(I), dI, None, dT) == INVALID and "device_labels" in _capi.last_error()
    assert call(n, len(I), None, dL, dT) == INVALID and "device_indices" in _capi.last_error()
    assert call(n, len(I) - 1, dI, dL, dT) == INVALID and "multiple of 3" in _capi.last_error()
    assert call(2 ** 32, len(I), dI, dL, dT) == INVALID and "32-bit" in _capi.last_error()
    assert call(n, 3 * 2 ** 31, dI, dL, dT) == INVALID and "32-bit" in _capi.last_error()
    assert call(0, 3, dI, dL, dT) == INVALID
    assert untouched()
    assert lib.tsdf_label_components_device(0, 0, None, dL, None, C.byref(info), None) == 0      # nothing to label is not an error
    assert (info.n_components, info.n_triangles, info.largest_triangles, info.largest_label) == (0, 0, 0, ref.NO_LABEL)
    assert untouched()
    # an index equal to n_vertices: found on the device, an error return, and the element past the arrays' ends survives
    bad = I.copy()
    bad[3 * 700 + 1] = n
    dB = device.put(bad)
    assert call(n, len(bad), dB, dL, dT) == INVALID
    assert "not below n_vertices" in _capi.last_error()
    assert device.get(dL, n + 1)[n] == SENTINEL and device.get(dT, n + 1)[n] == SENTINEL
    first = I.copy()
    first[3 * 1500] = n                                               # ... as the index the counts are taken by
    dF = device.put(first)
    assert call(n, len(first), dF, dL, dT) == INVALID
    assert device.get(dL, n + 1)[n] == SENTINEL and device.get(dT, n + 1)[n] == SENTINEL
    # and the same arrays serve a good call afterwards
    assert call(n, len(I), dI, dL, dT) == 0
    rL, rT, rinfo = ref.label(n, I)
    assert np.array_equal(device.get(dL, n), rL) and np.array_equal(device.get(dT, n), rT)
    assert device.get(dL, n + 1)[n] == SENTINEL and device.get(dT, n + 1)[n] == SENTINEL
    assert info.n_components == rinfo["n_components"] and info.largest_label == rinfo["largest_label"]
    # the mesh calls
    a = tsdf_amd.Mesh()
    assert lib.tsdf_mesh_label_components(None, None, None) == INVALID
    assert lib.tsdf_mesh_component_buffers(None, None, None) == INVALID
    assert lib.tsdf_mesh_component_download(None, None, None) == INVALID
    assert lib.tsdf_mesh_filter_components(None, 0, 0, a._h, None) == INVALID and lib.tsdf_mesh_filter_components(a._h, 0, 0, None, None) == INVALID
    with pytest.raises(ValueError, match="dst is src"):
        a.filter_components(into=a)
    assert lib.tsdf_mesh_filter_components(a._h, 0, 2, tsdf_amd.Mesh()._h, None) == INVALID and "unknown flags" in _capi.last_error()
    with pytest.raises(ValueError, match="not been labelled"):
        a.labels
    with pytest.raises(ValueError, match="not been labelled"):
        a.component_buffers()


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def mesh_arrays(mesh):
    f = mesh.info().flags
    return (mesh.vertices, mesh.indices, mesh.normals if f & 1 else None, mesh.colours if f & 2 else None)


def assert_labelled(mesh, what):
    """Labels, sizes and info of `mesh` are the reference's for its own arrays; returns them."""
    V, I = mesh.vertices, mesh.indices
    rL, rT, rinfo = ref.label(len(V), I)
    info = mesh.label_components()
    assert_info(info, rinfo, what)
    assert np.array_equal(mesh.labels, rL), what
    assert np.array_equal(mesh.component_triangles, rT), what
    assert all(mesh.component_buffers()) == (len(V) > 0)
    return rL, rT, rinfo


def assert_filtered(dst, src_arrays, labelling, min_triangles, keep_largest, src_info, what):
    rL, rT, rinfo = labelling
    V, I, N, RGB = src_arrays
    (kV, kN, kC), kI, keep = ref.filter_mesh(rL, rT, rinfo, I, [V, N, RGB], min_triangles, keep_largest)
    assert (dst.n_vertices, dst.n_indices) == (len(kV), len(kI)), what
    assert_same_floats(dst.vertices, kV, what + ": vertices")
    assert np.array_equal(dst.indices, kI), what + ": indices"
    if N is not None:
        assert_same_floats(dst.normals, kN, what + ": normals")
    if RGB is not None:
        assert np.array_equal(dst.colours, kC), what + ": colours"
    assert dst.info().flags == src_info.flags and list(dst.info().box) == list(src_info.box)
    return keep


@pytest.fixture(scope="module")
def grids():
    """size -> (volume, distances), made once."""
    out = {}
    for size in MESH_GRIDS:
        gv, D = volume_of(size, mesh_seed(size))
        out[size] = (gv, D)
    return out


@pytest.mark.parametrize("size", MESH_GRIDS)
def test_random_field_meshes_label_and_filter_like_the_reference(oracle, grids, size):
    gv, D = grids[size]
    mesh = gv.extract_mesh()
    assert within_bound(mesh, size)                                   # the extraction alone allocates nothing for components
    V, I = mesh.vertices, mesh.indices
    rV, rI = reference(oracle, gv, D, size)[:2]
    assert_same_floats(V, rV, "vertices")
    assert np.array_equal(I, rI)
    labelling = assert_labelled(mesh, "grid %s" % (size,))
    assert labelling[2]["n_components"] >= 3
    assert mesh.scratch_bytes <= size[0] * size[1] * size[2] + 65536 + 8 * len(V) + 32           # the documented bound
    again = gv.extract_mesh()
    again.label_components()
    assert again.labels.tobytes() == mesh.labels.tobytes() and again.component_triangles.tobytes() == mesh.component_triangles.tobytes()
    before = [a.tobytes() for a in mesh_arrays(mesh)[:2]]
    src_info = mesh.info()
    dst = tsdf_amd.Mesh()
    for min_triangles, largest in [(0, False), (1, False), (2, False), (5, False), (2 ** 40, False), (0, True), (5, True), (2 ** 40, True)]:
        what = "grid %s min %d largest %d" % (size, min_triangles, largest)
        assert mesh.filter_components(min_triangles, largest, into=dst) is dst
        keep = assert_filtered(dst, (V, I, None, None), labelling, min_triangles, largest, src_info, what)
        if min_triangles == 0 and not largest:
            assert dst.vertices.tobytes() == before[0] and dst.indices.tobytes() == before[1]      # the identity
        # labelling dst gives exactly the kept components
        dL, dT, dinfo = assert_labelled(dst, what + ": dst")
        kept_roots = np.unique(labelling[0][keep])
        assert dinfo["n_components"] == len(kept_roots)
        assert sorted(dT[np.unique(dL)].tolist()) == sorted(labelling[1][kept_roots].tolist())
        assert dst.scratch_bytes <= 65536 + 8 * len(V) + 32 + 12 * (len(V) // 64 + len(I) // 192 + 2)   # (dst's arrays only grow)
    assert [a.tobytes() for a in mesh_arrays(mesh)[:2]] == before     # src's arrays are unchanged
    assert np.array_equal(mesh.labels, labelling[0])                  # ... and its labels still there


def test_normals_colours_boxes_and_a_reused_dst(oracle):
    size = (40, 33, 21)
    gv, D = volume_of(size, mesh_seed(size))
    gv.enable_colour()
    rng = np.random.default_rng(77)
    gv.set_colour_data(rng.integers(0, 2 ** 32, size[0] * size[1] * size[2], dtype=np.uint64).astype(np.uint32))
    dst = tsdf_amd.Mesh()
    small_box, big_box = (38, 31, 19, 39, 32, 20), (5, 3, 2, 38, 30, 20)
    seen = []
    for box, normals, colours, min_triangles, largest in [(None, True, True, 2, False), (small_box, True, False, 0, False),
                                                           (big_box, False, True, 5, False), (None, True, True, 2 ** 40, False),
                                                           (None, False, False, 0, True), (big_box, True, True, 3, True)]:
        what = "box %s normals %d colours %d min %d largest %d" % (box, normals, colours, min_triangles, largest)
        mesh = gv.extract_mesh(box=box, normals=normals, colours=colours)
        arrays = mesh_arrays(mesh)
        rV, rI = reference(oracle, gv, D, size, box)[:2]
        assert_same_floats(arrays[0], rV, what)
        assert np.array_equal(arrays[1], rI)
        before = [None if a is None else a.tobytes() for a in arrays]
        mesh.filter_components(min_triangles, largest, into=dst)      # (labels the source itself)
        labelling = ref.label(len(rV), rI)
        assert np.array_equal(mesh.labels, labelling[0]) and np.array_equal(mesh.component_triangles, labelling[1])
        assert_filtered(dst, arrays, labelling, min_triangles, largest, mesh.info(), what)
        assert [None if a is None else a.tobytes() for a in mesh_arrays(mesh)] == before          # src's four arrays are unchanged
        if not normals:
            with pytest.raises(ValueError, match="TSDF_MESH_NORMALS"):
                dst.normals
        seen.append(dst.n_vertices)
    assert seen[0] > seen[1] > 0 and seen[2] > seen[1] and seen[3] == 0 and seen[4] > 0              # dst shrank and grew
    # a new extraction forgets the labels
    mesh = gv.extract_mesh(into=mesh)
    with pytest.raises(ValueError, match="not been labelled"):
        mesh.labels


def test_an_empty_mesh(device):
    plain = tsdf_amd.TSDFVolume((16, 16, 16), (160.0,) * 3)
    mesh = plain.extract_mesh(normals=True)
    assert mesh.label_components() == {"n_components": 0, "n_triangles": 0, "largest_triangles": 0, "largest_label": ref.NO_LABEL}
    assert mesh.labels.shape == (0,) and mesh.component_triangles.shape == (0,) and mesh.component_buffers() == (0, 0)
    for largest in (False, True):
        dst = mesh.filter_components(0, largest)
        assert (dst.n_vertices, dst.n_indices) == (0, 0) and dst.vertices.shape == (0, 3) and dst.normals.shape == (0, 3)
        assert dst.label_components()["n_components"] == 0
    # an unlabelled empty mesh filters too, into a handle that held something
    n, I = CASES["tie"]
    assert tsdf_amd.label_components(n, I)[2]["largest_label"] == 3
    assert plain.extract_mesh().filter_components(5).n_vertices == 0


# ---- the scene -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    gv = tsdf_amd.TSDFVolume(ref.SCENE_SIZE, (640.0,) * 3)
    D = ref.sphere_scene()
    gv.set_distance_data(D)
    return gv, D


def test_the_filter_leaves_the_two_spheres_and_keep_largest_the_larger(oracle, scene):
    gv, D = scene
    rV, rI = reference(oracle, gv, D, ref.SCENE_SIZE)[:2]
    labelling = ref.label(len(rV), rI)
    assert labelling[2]["n_components"] == 5
    mesh = gv.extract_mesh(normals=True)
    arrays = mesh_arrays(mesh)
    assert_same_floats(arrays[0], rV, "scene")
    info = mesh.label_components()
    assert_info(info, labelling[2], "scene")
    assert np.array_equal(mesh.labels, labelling[0]) and np.array_equal(mesh.component_triangles, labelling[1])
    two = mesh.filter_components(ref.SCENE_MIN_TRIANGLES)
    assert_filtered(two, arrays, labelling, ref.SCENE_MIN_TRIANGLES, False, mesh.info(), "two spheres")
    assert two.label_components()["n_components"] == 2
    one = mesh.filter_components(ref.SCENE_MIN_TRIANGLES, keep_largest=True)
    assert_filtered(one, arrays, labelling, ref.SCENE_MIN_TRIANGLES, True, mesh.info(), "the larger sphere")
    oinfo = one.label_components()
    assert oinfo["n_components"] == 1 and oinfo["n_triangles"] == info["largest_triangles"] == oinfo["largest_triangles"]
    # every kept soup vertex is the soup's, bit for bit: the larger sphere's vertices lie round its centre
    kept = one.vertices[one.indices]
    centre = (np.array(ref.SCENE_SPHERES[0][0]) + 0.5) * 10.0
    assert np.abs(np.linalg.norm(kept - centre, axis=1) - ref.SCENE_SPHERES[0][1] * 10.0).max() < 10.0


def test_components_leave_the_volume_the_soup_and_the_ray_cast_alone(scene):
    gv, _ = scene
    cam = synth.camera_for_frame(4, 40)
    caster = tsdf_amd.GPURaycaster(W, H)
    S0 = gv.extract_surface()
    V0, N0 = caster.raycast(gv, cam)
    D0, W0 = gv.get_distance_data(), gv.get_weight_data()
    mesh = gv.extract_mesh(normals=True)
    mesh.label_components()
    kept = mesh.filter_components(ref.SCENE_MIN_TRIANGLES)
    assert mesh.n_vertices > kept.n_vertices > 0
    V1, N1 = caster.raycast(gv, cam)
    assert_same_floats(V1, V0, "ray cast vertices")
    assert_same_floats(N1, N0, "ray cast normals")
    assert_same_floats(gv.extract_surface(), S0, "soup")
    assert_same_floats(gv.get_distance_data(), D0, "distances")
    assert_same_floats(gv.get_weight_data(), W0, "weights")
    again = gv.extract_mesh(normals=True).filter_components(ref.SCENE_MIN_TRIANGLES)     # and the same arrays on every run
    assert again.vertices.tobytes() == kept.vertices.tobytes() and again.indices.tobytes() == kept.indices.tobytes()
    assert again.normals.tobytes() == kept.normals.tobytes()
