"""GPU: the indexed mesh (tsdf_volume_extract_mesh; include/tsdf_amd.h, "indexed mesh") against the CPU reference tests/mesh_ref.py,
which is built from the oracle's soup: V and I bit for bit, V[I] the device's own extract_surface(), boxes, normals and colours per
shared vertex, a reused handle, the refusals, the scratch bound, and that an extraction leaves the volume's other results alone.
Grids are the smallest at which the 64-voxel chunking can go wrong: rows shorter than, equal to and longer than a chunk, chunks that
span several rows and planes, more than one workgroup."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import mesh_ref
from tests.helpers import H, W, assert_same_floats
from tests.test_mesh_ref_host import octants
from tsdf_amd import _capi, synth

pytestmark = pytest.mark.gpu

GRIDS = [(2, 2, 2), (3, 2, 5), (64, 2, 2), (65, 3, 2), (129, 7, 3), (130, 5, 4), (40, 33, 21)]
OFFSET = (100.0, -50.0, 25.0)


def volume_of(size, seed):
    gv = tsdf_amd.TSDFVolume(size, (size[0] * 10.0, size[1] * 12.5, size[2] * 9.0))
    gv.offset(*OFFSET)
    D = mesh_ref.random_field(size, seed)
    gv.set_distance_data(D)
    return gv, D


def reference(oracle, gv, D, size, box=None):
    return mesh_ref.indexed(oracle, D, size, gv.voxel_size(), gv.offset(), box)


def assert_mesh(mesh, ref, what):
    V, I = ref[0], ref[1]
    assert (mesh.n_vertices, mesh.n_indices) == (len(V), len(I)), what
    assert_same_floats(mesh.vertices, V, what + ": vertices")
    assert np.array_equal(mesh.indices, I), what + ": indices"
    return mesh.vertices, mesh.indices


def within_bound(mesh, size):
    return mesh.scratch_bytes <= size[0] * size[1] * size[2] + 65536


@pytest.mark.parametrize("size", GRIDS)
def test_random_fields_equal_the_reference_bit_for_bit(oracle, size):
    gv, D = volume_of(size, 3000 + size[0] + size[2])
    ref = reference(oracle, gv, D, size)
    mesh = gv.extract_mesh()
    V, I = assert_mesh(mesh, ref, "grid %s" % (size,))
    assert len(V) > 0 and int(I.max()) == len(V) - 1 and len(I) % 3 == 0
    S = gv.extract_surface()
    assert S.shape == (len(I), 3)
    assert_same_floats(V[I], S, "expansion %s" % (size,))               # the device's own soup, NaN vertices included
    assert mesh.box == (0, 0, 0, size[0] - 1, size[1] - 1, size[2] - 1)
    assert np.array_equal(mesh.triangles(), mesh_ref.triangles(I))
    assert within_bound(mesh, size)
    v, i, nrm, rgb = mesh.device_buffers()
    assert v and i and not nrm and not rgb


BOXES = {
    (130, 5, 4): [(60, 0, 0, 70, 4, 3), (120, 1, 1, 130, 4, 3), (1, 0, 1, 129, 2, 2),            # straddling x = 64 and x = 128
                  (63, 0, 0, 64, 1, 1), (64, 2, 1, 65, 3, 2), (128, 3, 2, 129, 4, 3), (0, 0, 0, 1, 1, 1),   # one cube each
                  (100, 0, 0, 1000, 1000, 1000)],                                                  # past the grid: clipped
    (40, 33, 21): [(5, 3, 2, 38, 30, 20), (38, 31, 19, 39, 32, 20), (20, 16, 10, 400, 330, 210), (0, 0, 0, 39, 1, 20)],
}


@pytest.mark.parametrize("size", sorted(BOXES))
def test_boxes_equal_the_reference_and_share_their_edges(oracle, size):
    gv, D = volume_of(size, 4000 + size[0])
    mesh = tsdf_amd.Mesh()
    whole = reference(oracle, gv, D, size)
    Vw, _ = assert_mesh(gv.extract_mesh(into=mesh), whole, "grid %s" % (size,))
    whole_bits = dict(zip(whole[3].tolist(), map(tuple, Vw.view(np.uint32).tolist())))
    some = 0
    for box in BOXES[size] + octants(size):
        ref = reference(oracle, gv, D, size, box)
        assert gv.extract_mesh(box=box, into=mesh) is mesh
        V, I = assert_mesh(mesh, ref, "grid %s box %s" % (size, box))
        assert list(mesh.box) == mesh_ref.clip_box(size, box)
        some += len(V) > 0
        # the same edge has the same bytes in every box that holds it: the whole grid's
        for k, v in zip(ref[3].tolist(), map(tuple, V.view(np.uint32).tolist())):
            assert whole_bits[k] == v, (box, k)
        assert within_bound(mesh, size)
    assert some == len(BOXES[size] + octants(size))                # (every one of them holds surface, by the CPU reference)
    assert list(gv.extract_mesh(box=(100, 0, 0, 1000, 1000, 1000), into=mesh).box) == mesh_ref.clip_box(size, (100, 0, 0, 1000, 1000, 1000))
    # a box that clips to nothing is an empty mesh; a begin that is not below its end is refused, with a message
    empty = gv.extract_mesh(box=(size[0] - 1, 0, 0, size[0] + 5, 2, 2), into=mesh)
    assert (empty.n_vertices, empty.n_indices) == (0, 0) and empty.vertices.shape == (0, 3) and empty.indices.shape == (0,)
    for bad in ((5, 0, 0, 5, 2, 2), (0, 3, 0, 4, 2, 2), (0, 0, 2, 4, 4, 1)):
        with pytest.raises(ValueError, match="not below its end"):
            gv.extract_mesh(box=bad, into=mesh)
        assert "tsdf_volume_extract_mesh" in _capi.last_error()


def fused_scene(colour):
    """The three frames of tests/test_cpp_field.py on a 64^3 volume."""
    gv = tsdf_amd.TSDFVolume((64,) * 3, (3000.0,) * 3)
    if colour:
        gv.enable_colour()
    for i in range(3):
        d, cam = synth.depth_frame(i * 9, 40, seed=0x5EEDF1E2)
        if colour:
            rgb, _ = synth.colour_frame(i * 9, 40, seed=0x5EEDF1E2)
            gv.integrate_colour(d, rgb, W, H, cam)
        else:
            gv.integrate(d, W, H, cam)
    return gv


@pytest.fixture(scope="module")
def scene():
    return fused_scene(True)


def test_fused_volume_normals_and_colours_are_the_queries_at_the_shared_vertices(oracle, scene):
    gv, size = scene, (64,) * 3
    ref = reference(oracle, gv, gv.get_distance_data(), size)
    mesh = gv.extract_mesh(normals=True, colours=True)
    V, I = assert_mesh(mesh, ref, "fused 64^3")
    N, rgb = mesh.normals, mesh.colours
    assert N.shape == V.shape and rgb.shape == V.shape and rgb.dtype == np.uint8
    assert_same_floats(N, gv.sample_field(V, weight=False, unit_gradient=True)[1], "normals")
    assert np.array_equal(rgb, gv.sample_colours(V))
    # so that none of this passes on an empty mesh (the scene's soup has >= 3000 vertices, at most six copies of each; the CPU
    # reference has 8334 unique vertices for a soup of 49134, 8104 finite normals and 8334 coloured vertices on this scene)
    assert len(V) >= 500 and np.isfinite(N).all(axis=1).sum() >= 200 and rgb.any(axis=1).sum() >= 100
    assert_same_floats(V[I], gv.extract_surface(), "expansion")
    assert all(mesh.device_buffers())
    # one array at a time
    only_n = gv.extract_mesh(normals=True)
    assert_same_floats(only_n.normals, N, "normals alone")
    with pytest.raises(ValueError, match="TSDF_MESH_COLOURS"):
        only_n.colours
    only_c = gv.extract_mesh(colours=True)
    assert np.array_equal(only_c.colours, rgb)
    with pytest.raises(ValueError, match="TSDF_MESH_NORMALS"):
        only_c.normals
    assert within_bound(mesh, size)


def test_a_reused_handle_is_exact_every_time(oracle):
    size = (130, 5, 4)
    gv, D = volume_of(size, 5000)
    mesh = tsdf_amd.Mesh()
    whole = reference(oracle, gv, D, size)
    V1, I1 = (a.copy() for a in assert_mesh(gv.extract_mesh(into=mesh), whole, "first"))
    scratch = mesh.scratch_bytes
    one = (64, 2, 1, 65, 3, 2)
    assert_mesh(gv.extract_mesh(box=one, into=mesh), reference(oracle, gv, D, size, one), "one cube")
    V2, I2 = assert_mesh(gv.extract_mesh(into=mesh), whole, "again")
    assert V1.tobytes() == V2.tobytes() and I1.tobytes() == I2.tobytes()
    assert mesh.scratch_bytes == scratch and within_bound(mesh, size)      # nothing grew


def test_refusals_and_edge_cases(scene):
    plain = tsdf_amd.TSDFVolume((16, 16, 16), (160.0,) * 3)
    cleared = plain.extract_mesh(normals=True)                     # +trunc everywhere: no surface
    assert (cleared.n_vertices, cleared.n_indices) == (0, 0)
    assert cleared.vertices.shape == (0, 3) and cleared.normals.shape == (0, 3) and cleared.device_buffers() == (0, 0, 0, 0)
    with pytest.raises(ValueError, match="without colour"):
        plain.extract_mesh(colours=True)
    slab = tsdf_amd.TSDFVolume((16, 16, 16), (160.0,) * 3, slab=(0, 8))
    with pytest.raises(ValueError, match="Z-slab"):
        slab.extract_mesh()
    assert slab.extract_surface().shape == (0, 3)                  # the soup path still serves slabs
    mesh = scene.extract_mesh()
    for which in (2, 3):                                           # downloading an array the mesh lacks
        args = [None] * 4
        args[which] = np.zeros(3 * mesh.n_vertices + 3, np.float32).ctypes.data
        assert _capi.lib.tsdf_mesh_download(mesh._h, *args) == _capi.TSDF_ERR_INVALID
    table = tsdf_amd.marching_cubes_table()
    for bad in ((1, 0, 12), (1, 3, 0)):                            # no such edge; four vertices
        t = table.copy()
        t[bad[0], bad[1]] = bad[2]
        assert _capi.lib.tsdf_volume_extract_mesh(scene._h, t.ctypes.data, None, 0, mesh._h) == _capi.TSDF_ERR_INVALID
    assert _capi.lib.tsdf_volume_extract_mesh(scene._h, table.ctypes.data, None, 4, mesh._h) == _capi.TSDF_ERR_INVALID   # unknown flag
    thin = tsdf_amd.TSDFVolume((1, 8, 8), (10.0, 80.0, 80.0))
    thin.set_distance_data(np.where(np.arange(64) % 2, -1.0, 1.0).astype(np.float32))
    assert thin.extract_mesh().n_vertices == 0                     # an axis shorter than 2: no cube
    n = C.c_uint64(0)
    assert _capi.lib.tsdf_mesh_scratch_bytes(mesh._h, C.byref(n)) == 0 and n.value == mesh.scratch_bytes
    assert within_bound(mesh, (64,) * 3)


def test_an_extraction_leaves_the_soup_and_the_ray_cast_alone(scene):
    cam = synth.camera_for_frame(4, 40)
    caster = tsdf_amd.GPURaycaster(W, H)
    S0 = scene.extract_surface()
    V0, N0 = caster.raycast(scene, cam)
    D0, W0 = scene.get_distance_data(), scene.get_weight_data()
    a = scene.extract_mesh(normals=True, colours=True)
    b = scene.extract_mesh(box=(3, 5, 7, 40, 41, 42), normals=True)
    assert a.n_vertices > b.n_vertices > 0
    V1, N1 = caster.raycast(scene, cam)
    assert_same_floats(V1, V0, "ray cast vertices")
    assert_same_floats(N1, N0, "ray cast normals")
    assert_same_floats(scene.extract_surface(), S0, "soup")
    assert_same_floats(scene.get_distance_data(), D0, "distances")
    assert_same_floats(scene.get_weight_data(), W0, "weights")
    c = scene.extract_mesh(normals=True, colours=True)             # and the same arrays on every run
    assert a.vertices.tobytes() == c.vertices.tobytes() and a.indices.tobytes() == c.indices.tobytes()
    assert a.normals.tobytes() == c.normals.tobytes() and a.colours.tobytes() == c.colours.tobytes()
