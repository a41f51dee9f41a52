"""GPU: the scene-flow step (tsdf_volume_apply_scene_flow; include/tsdf_amd.h, "scene flow") against the CPU reference
tests/scene_flow_ref.py: the whole node array bit for bit, the info counts, and distances, weights and colours untouched.  Scenes are a
sphere and a tilted plane that leaves the grid, fused (by the oracle) from three depth frames of a 40 x 30 camera into grids with a non-zero offset:
24 x 20 x 17, 70 x 9 x 9 (chunks wrap rows, the x neighbour crosses a chunk), 65 x 2 x 2 and 33^3 (no plane of 128).  Every case
asserts on the reference's own numbers that it is not vacuous."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import tsdf_amd
from tests import mesh_ref, scene_flow_cases as cases, scene_flow_ref as ref
from tsdf_amd import _capi
from tsdf_amd.api import _DeviceArray

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
VOXEL = 10.0
GRIDS = [(24, 20, 17), (70, 9, 9), (65, 2, 2), (33, 33, 33)]
SCENES = [(g, "plane") for g in GRIDS] + [((24, 20, 17), "sphere"), ((33, 33, 33), "sphere")]
POSITIONS = [(0.0, 0.0, 0.0), (15.0, -10.0, 5.0), (-20.0, 8.0, -10.0)]


def new_volume(size, offset):
    gv = tsdf_amd.TSDFVolume(size, tuple(s * VOXEL for s in size))
    gv.offset(*offset)
    return gv


@functools.lru_cache(maxsize=None)
def _scene(size, kind):
    import oracle
    oracle.build()
    X, Y, Z = size
    front = float(np.ceil(1.15 * max(X * VOXEL / 2 * cases.FOCAL / cases.CX, Y * VOXEL / 2 * cases.FOCAL / cases.CY)))
    offset = (-X * VOXEL / 2 + 3.0, -Y * VOXEL / 2 - 2.0, front)
    centre = np.array([offset[a] + size[a] * VOXEL / 2 for a in range(3)]) + np.array([1.5, -2.5, 0.75])
    if kind == "sphere":
        depth_of = lambda p: cases.sphere_depth(p, centre, 0.33 * min(size) * VOXEL)
    else:
        normal = (0.9 * Z / X, 0.5 * Z / Y, -1.0)     # across the grid it moves by 0.7 of the grid's depth: it leaves through two faces
        depth_of = lambda p: cases.plane_depth(p, centre, normal)
    ov = oracle.Volume(size, tuple(s * VOXEL for s in size))
    ov.offset(*offset)
    for p in POSITIONS:                            # (the oracle's integrate: what the device's is pinned to, bit for bit)
        cam = cases.camera(p)
        ov.integrate(depth_of(p).reshape(-1), cases.WIDTH, cases.HEIGHT, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    D, Wt = ov.dist.copy(), ov.weight.copy()
    V, I, _, keys = mesh_ref.indexed(oracle, D, size, ov.voxel_size(), ov.offset())
    assert len(V) >= 40 and len(I) >= 60, (size, kind, len(V))
    return types.SimpleNamespace(size=size, offset=offset, D=D, Wt=Wt, V=V, I=I, keys=keys, depth_of=depth_of, vs=ov.voxel_size(),
                                 n=X * Y * Z)


def fresh(sc, colour=False):
    gv = new_volume(sc.size, sc.offset)
    gv.set_distance_data(sc.D)
    gv.set_weight_data(sc.Wt)
    if colour:
        gv.enable_colour()
        gv.set_colour_data(np.random.default_rng(3).integers(0, 2 ** 32, sc.n, dtype=np.uint64).astype(U32))
    return gv


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(U32), np.ascontiguousarray(b, F32).view(U32))


def expected(oracle, gv, sc, depth, flow, cam, threshold, deformed=False):
    """(nodes after, info, pixel per vertex, seen mask) by the CPU reference, from the volume's nodes now."""
    nodes = gv.get_deformation()
    P = sc.V
    if deformed:
        P = oracle.deform_points(sc.size, sc.vs, sc.offset, (0.0, 0.0, 0.0), nodes, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), sc.V)
    pix, seen = ref.correspond(oracle, P, depth, flow, cases.WIDTH, cases.HEIGHT, cam.pose(), cam.inverse_pose(), cam.k(), cam.kinv(), threshold)
    after, moved = ref.apply(nodes, sc.keys, sc.I, pix, flow, sc.size)
    info = {"n_vertices": len(sc.V), "n_correspondences": int((pix != ref.NONE).sum()), "n_nodes_moved": moved}
    return after, info, pix, seen


def check(oracle, gv, sc, depth, flow, cam, threshold=10.0, deformed=False, mesh=None, least=5, least_excluded=0):
    d0, w0 = gv.get_distance_data(), gv.get_weight_data()
    c0 = gv.get_colour_data() if gv.colour_enabled() else None
    after, info, pix, seen = expected(oracle, gv, sc, depth, flow, cam, threshold, deformed)
    assert info["n_correspondences"] >= least and info["n_nodes_moved"] >= least, info       # the reference itself: not vacuous
    assert len(sc.V) - info["n_correspondences"] >= least_excluded, info
    got_info = gv.apply_scene_flow(depth, flow, cam, threshold, deformed, mesh)
    assert got_info == info
    got = gv.get_deformation()
    assert same_bits(got, after), "%d of %d nodes differ" % ((got.view(U32) != after.view(U32)).any(axis=1).sum(), len(got))
    assert same_bits(gv.get_distance_data(), d0) and same_bits(gv.get_weight_data(), w0)
    if c0 is not None:
        assert np.array_equal(gv.get_colour_data(), c0)
    assert gv.info().deformation_materialised == 1
    return pix, seen, got


@pytest.mark.parametrize("size,kind", SCENES)
def test_a_constant_and_a_random_flow_equal_the_reference_bit_for_bit(oracle, size, kind):
    sc = _scene(size, kind)
    cam, depth = cases.camera(POSITIONS[0]), sc.depth_of(POSITIONS[0])
    gv = fresh(sc, colour=size == (24, 20, 17))
    before = gv.get_deformation()
    mesh = gv.extract_mesh()
    _, _, got = check(oracle, gv, sc, depth, cases.constant_flow((2.0, -1.0, 3.5)), cam, mesh=mesh)
    assert same_bits(got[:, 3:], before[:, 3:])                                   # rotations are untouched
    count = ref.counts(sc.keys, sc.I, sc.size)
    assert (count == 0).any() and same_bits(got[count == 0], before[count == 0])
    assert mesh.scratch_bytes >= 8 * mesh.n_vertices
    # a second frame with a flow per pixel, into the same handle: it accumulates on the first
    check(oracle, gv, sc, depth, cases.random_flow(size[0] + len(kind)), cam, mesh=mesh)
    # the same two frames on a fresh volume with a private mesh each: the same bytes
    again = fresh(sc)
    again.apply_scene_flow(depth, cases.constant_flow((2.0, -1.0, 3.5)), cam)
    again.apply_scene_flow(depth, cases.random_flow(size[0] + len(kind)), cam)
    assert same_bits(again.get_deformation(), gv.get_deformation())


@pytest.mark.parametrize("size,kind", [((70, 9, 9), "plane"), ((33, 33, 33), "sphere")])
def test_pixels_without_flow_or_depth_are_left_out(oracle, size, kind):
    sc = _scene(size, kind)
    cam, depth = cases.camera(POSITIONS[1]), sc.depth_of(POSITIONS[1])
    rng = np.random.default_rng(9)
    flow = cases.random_flow(21)
    holes = rng.random((cases.HEIGHT, cases.WIDTH)) < 0.3
    flow[holes, rng.integers(0, 3, holes.sum())] = np.array([np.nan, np.inf, -np.inf], F32)[rng.integers(0, 3, holes.sum())]
    pix, seen, _ = check(oracle, fresh(sc), sc, depth, flow, cam)
    assert (seen & (pix == ref.NONE)).sum() >= 3                                  # seen, but the flow there is not finite
    # zero-depth pixels
    gaps = depth.copy()
    gaps[rng.random(gaps.shape) < 0.3] = 0
    full, _, _, _ = expected(oracle, fresh(sc), sc, depth, cases.random_flow(22), cam, 10.0)
    _, _, got = check(oracle, fresh(sc), sc, gaps, cases.random_flow(22), cam)
    assert not same_bits(got, full)                                               # (the gaps did take vertices away)


def test_a_camera_that_sees_half_the_mesh_and_a_tight_threshold(oracle):
    sc = _scene((24, 20, 17), "sphere")
    # shifted sideways until the image's edge runs through the sphere: the rest of it projects off the image
    position = (-180.0, 0.0, 0.0)
    cam, depth = cases.camera(position), sc.depth_of(position)
    inside = mesh_pixels_inside(oracle, sc, cam)
    assert 0.2 < inside.mean() < 0.8
    check(oracle, fresh(sc), sc, depth, cases.random_flow(31), cam, least_excluded=int((~inside).sum()))
    # a threshold that excludes most of what the default keeps
    cam, depth = cases.camera(POSITIONS[0]), sc.depth_of(POSITIONS[0])
    _, wide, _, _ = expected(oracle, fresh(sc), sc, depth, cases.random_flow(32), cam, 10.0)
    pix, _, _ = check(oracle, fresh(sc), sc, depth, cases.random_flow(32), cam, threshold=0.75, least=3)
    assert 3 <= (pix != ref.NONE).sum() < wide["n_correspondences"] // 2


def mesh_pixels_inside(oracle, sc, cam):
    p = oracle.world_to_pixel_n(sc.V, cam.inverse_pose(), cam.k())
    return (p[:, 0] >= 0) & (p[:, 0] < cases.WIDTH) & (p[:, 1] >= 0) & (p[:, 1] < cases.HEIGHT)


@pytest.mark.parametrize("size,kind", [((24, 20, 17), "sphere"), ((70, 9, 9), "plane")])
def test_deformed_vertices_after_a_first_frame(oracle, size, kind):
    sc = _scene(size, kind)
    gv = fresh(sc)
    mesh = gv.extract_mesh()
    cam, depth = cases.camera(POSITIONS[0]), sc.depth_of(POSITIONS[0])
    check(oracle, gv, sc, depth, cases.constant_flow((3.0, -2.0, 4.0)), cam, mesh=mesh)
    # deform_mesh places a point relative to the grid's corner (it takes the offset off and the nodes carry the offset at clear, 0
    # here): seen from a camera moved by -offset the deformed mesh is where the canonical one was, plus the flow
    moved_cam = cases.camera(tuple(np.asarray(POSITIONS[0]) - np.asarray(sc.offset)))
    canonical, _, _, _ = expected(oracle, gv, sc, depth, cases.random_flow(41), moved_cam, 10.0, deformed=False)
    V0 = mesh.vertices
    pix, _, got = check(oracle, gv, sc, depth, cases.random_flow(41), moved_cam, deformed=True, mesh=mesh)
    assert not same_bits(got, canonical)                                          # the flag changed which vertices correspond
    assert same_bits(mesh.vertices, V0)                                           # the handle's vertices are not changed
    assert mesh.scratch_bytes >= 20 * mesh.n_vertices


def test_a_constant_flow_moves_every_vertex_of_a_fully_seen_sphere_along_it(oracle):
    sc = _scene((33, 33, 33), "sphere")
    gv = fresh(sc)
    f = np.array([3.0, -4.0, 12.0], F32)
    depth = np.full((cases.HEIGHT, cases.WIDTH), 500, np.uint16)
    before = gv.deform_mesh(sc.V)
    info = gv.apply_scene_flow(depth, cases.constant_flow(f), cases.camera(POSITIONS[0]), threshold=1.0e9)
    assert info["n_correspondences"] == info["n_vertices"] == len(sc.V)          # fully seen
    move = (gv.deform_mesh(sc.V) - before).astype(np.float64)
    length = float(np.sqrt((f.astype(np.float64) ** 2).sum()))
    along = move @ (f.astype(np.float64) / length)
    # eight products and seven sums of coordinates below 1024, twice: 32 roundings of at most 2^-24 * 1024 each
    tol = 32 * 2.0 ** -24 * 1024.0
    assert (along > 0).all() and (along <= length + tol).all()
    assert (np.abs(move - along[:, None] * (f / length)[None, :]) <= tol).all()


def test_an_empty_mesh_is_a_no_op(oracle):
    gv = new_volume((24, 20, 17), (5.0, 6.0, 300.0))
    info = gv.apply_scene_flow(np.full((cases.HEIGHT, cases.WIDTH), 400, np.uint16), cases.constant_flow((1.0, 1.0, 1.0)), cases.camera(POSITIONS[0]))
    assert info == {"n_vertices": 0, "n_correspondences": 0, "n_nodes_moved": 0}
    assert gv.info().deformation_materialised == 0
    thin = tsdf_amd.TSDFVolume((9, 1, 9), (90.0, 10.0, 90.0))                      # an axis shorter than 2: no cube, no mesh
    assert thin.apply_scene_flow(np.zeros((cases.HEIGHT, cases.WIDTH), np.uint16), cases.constant_flow((1.0, 1.0, 1.0)),
                                 cases.camera(POSITIONS[0]))["n_vertices"] == 0


def test_the_device_variant_gives_the_same_bytes(oracle):
    sc = _scene((70, 9, 9), "plane")
    cam, depth, flow = cases.camera(POSITIONS[2]), sc.depth_of(POSITIONS[2]), cases.random_flow(51)
    host = fresh(sc)
    host_info = host.apply_scene_flow(depth, flow, cam)
    dev = fresh(sc)
    with _DeviceArray(depth) as d, _DeviceArray(flow) as f:
        info = dev.apply_scene_flow_device(d.ptr.value, f.ptr.value, cases.WIDTH, cases.HEIGHT, cam)
    assert info == host_info and info["n_correspondences"] >= 5
    assert same_bits(dev.get_deformation(), host.get_deformation())


def test_refusals(oracle):
    sc = _scene((24, 20, 17), "sphere")
    gv = fresh(sc)
    cam, depth, flow = cases.camera(POSITIONS[0]), sc.depth_of(POSITIONS[0]), cases.constant_flow((1.0, 2.0, 3.0))
    mesh = gv.extract_mesh()
    nodes = gv.get_deformation()

    def refused(match, volume=gv, mesh=mesh, cam=cam, threshold=10.0):
        with pytest.raises(ValueError, match=match):
            volume.apply_scene_flow(depth, flow, cam, threshold, False, mesh)
        assert "tsdf_volume_apply_scene_flow" in _capi.last_error()

    for t in (0.0, -1.0, float("nan")):
        refused("threshold", threshold=t)
    for which in range(4):
        m = [np.array(a, F32) for a in (cam.pose(), cam.inverse_pose(), cam.k(), cam.kinv())]
        m[which][3] = np.inf if which % 2 else np.nan
        refused("non-finite", cam=cases.Cam(*m))
    refused("whole grid", mesh=gv.extract_mesh(box=(0, 0, 0, 10, 10, 10)))
    refused("whole grid", mesh=tsdf_amd.Mesh())                                   # never extracted into
    refused("whole grid", mesh=mesh.filter_components(1))
    refused("whole grid", mesh=mesh.simplify(25.0))
    other = new_volume((24, 20, 16), sc.offset)
    refused("whole grid", mesh=other.extract_mesh())
    refused("whole grid", volume=other)
    slab = tsdf_amd.TSDFVolume(sc.size, tuple(s * VOXEL for s in sc.size), slab=(0, 8))
    refused("slab", volume=slab)
    # through the C ABI: each null argument, unknown flags, an image of no pixels
    p, ip, k, kinv = (np.array(a, F32) for a in (cam.pose(), cam.inverse_pose(), cam.k(), cam.kinv()))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    args = [gv._h, mesh._h, depth.ctypes.data, flow.ctypes.data, cases.WIDTH, cases.HEIGHT, fp(p), fp(ip), fp(k), fp(kinv), 10.0, 0, None]
    for i in (0, 1, 2, 3, 6, 7, 8, 9):
        bad = list(args)
        bad[i] = None
        assert _capi.lib.tsdf_volume_apply_scene_flow(*bad) == _capi.TSDF_ERR_INVALID and "null" in _capi.last_error()
        assert _capi.lib.tsdf_volume_apply_scene_flow_device(*(bad + [None])) == _capi.TSDF_ERR_INVALID
    bad = list(args)
    bad[11] = 2
    assert _capi.lib.tsdf_volume_apply_scene_flow(*bad) == _capi.TSDF_ERR_INVALID and "flags" in _capi.last_error()
    bad = list(args)
    bad[4] = 0
    assert _capi.lib.tsdf_volume_apply_scene_flow(*bad) == _capi.TSDF_ERR_INVALID and "image" in _capi.last_error()
    # nothing was written by any of them, and the accepted call (info may be NULL) still works afterwards
    assert same_bits(gv.get_deformation(), nodes) and gv.info().deformation_materialised == 0
    assert _capi.lib.tsdf_volume_apply_scene_flow(*args) == _capi.TSDF_OK
    after, _, _, _ = expected(oracle, fresh(sc), sc, depth, flow, cam, 10.0)
    assert same_bits(gv.get_deformation(), after)
