"""GPU: the mesh renderer (include/tsdf_amd.h, "mesh rendering") against the CPU reference tests/render_ref.py, every target byte for
byte and every count: planted triangles on exact screen coordinates (ties on edges and vertices, the dropped and the dead, the large
path and its threshold, the ends of the screen range), a random soup on the 1/256 grid, then the mesh of a fused 32^3 sphere with
normals and colours from three poses, simplified (the large path), smoothed, with and without vertex normals, every subset of
targets, a warm handle at another size, two runs, the ray cast's normals, the depth map fed back to integrate, the refusals, a bad
index and the empty mesh.  Images are 64 x 48 and 37 x 29: the last wave of the pixel kernel is partial."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tsdf_amd
from tests import render_ref as ref
from tests.helpers import H, W, camera_at
from tsdf_amd import _capi

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(64, 48), (37, 29)]
FX, CX, CY = 64.0, 32.0, 24.0
IDENTITY = np.eye(4, dtype=F).reshape(-1)
K = np.array([FX, 0, 0, 0, FX, 0, CX, CY, 1], F)
ALL = ("triangle", "z", "depth", "vertices", "normals", "rgb")
BARE = ALL[:5]
LARGE = _capi.TSDF_RENDER_LARGE_BOX


def vertex(sx, sy, z):
    """The world point (identity pose) with the screen point (sx, sy) at depth z; exact for the dyadic values used here."""
    return [(sx - CX) * z / FX, (sy - CY) * z / FX, z]


def mesh_of(corners):
    """corners: per triangle three (sx, sy, z) in the wired order -> V, I."""
    V = np.array([vertex(*c) for tri in corners for c in tri], F).reshape(-1, 3)
    I = np.arange(len(V), dtype=np.uint32).reshape(-1, 3)[:, [0, 2, 1]].reshape(-1)
    return V, I


def check(got, want, targets, what):
    """Every requested target byte for byte, and the counts."""
    for name in targets:
        assert ref.same_bytes(got[name], want[name]), "%s: %s differs in %d places" % (
            what, name, int((np.ascontiguousarray(got[name]).view(np.uint8) != np.ascontiguousarray(want[name]).view(np.uint8)).sum()))
    info = {k: v for k, v in want["info"].items() if k != "bad_index"}
    assert got["info"] == info, (what, got["info"], info)


def both(V, I, size, near, far, cull=False, normals=None, colours=None, inv_pose=IDENTITY, k=K, into=None):
    targets = ALL if colours is not None else BARE
    got = tsdf_amd.render_mesh(V, I, inv_pose, k, size, near, far, cull, targets, normals, colours, into=into)
    want = ref.render(V, I, size[0], size[1], inv_pose, k, near, far, ref.CULL_BACK if cull else 0, normals, colours)
    return got, want, targets


S20 = 1048576.0
PLANTED = {
    # name: (triangles in wired order, near, far)
    "shared edge": ([((2, 2, 64), (30, 2, 64), (30, 30, 64)), ((2, 2, 64), (30, 30, 64), (2, 30, 64))], 1, 4096),
    "shared edge, sloped": ([((2, 2, 64), (30, 2, 128), (30, 30, 256)), ((2, 2, 64), (30, 30, 256), (2, 30, 32))], 1, 4096),
    "vertex on a centre": ([((10, 10, 64), (20.5, 3.25, 64), (25.75, 18.5, 128)), ((10, 10, 64), (25.75, 18.5, 128), (4.5, 22.25, 64)),
                            ((10, 10, 64), (4.5, 22.25, 64), (20.5, 3.25, 64))], 1, 4096),
    "zero area": ([((5, 5, 64), (9, 5, 64), (13, 5, 64)), ((5, 5, 64), (5, 5, 64), (13, 9, 64)), ((3, 3, 64), (12, 3, 64), (3, 12, 64))], 1, 4096),
    "behind near and beyond far": ([((3, 3, 0.5), (20, 3, 64), (3, 20, 64)), ((3, 3, 64), (20, 3, 8192), (3, 20, 64)),
                                    ((5, 5, 1), (30, 5, 4096), (5, 30, 64))], 1, 4096),
    "off every side": ([((-20, -10, 64), (90, 20, 64), (30, 70, 128))], 1, 4096),
    "whole image": ([((-1, -1, 64), (130, -1, 64), (-1, 100, 64))], 1, 4096),
    "ten times larger": ([((-640, -480, 64), (1300, -480, 128), (-640, 1000, 64))], 1, 4096),
    "at the large threshold": ([((2, 2, 64), (17.5, 2, 64), (2, 17.5, 64)), ((20, 2, 64), (51.5, 2, 64), (20, 9.5, 64))], 1, 4096),          # 16 x 16 and 32 x 8
    "one over the threshold": ([((2, 2, 64), (17.5, 2, 64), (2, 18, 64)), ((20, 2, 64), (51.5, 2, 64), (20, 10, 64))], 1, 4096),            # 16 x 17 and 32 x 9
    "identical": ([((4, 4, 64), (40, 8, 128), (10, 40, 64))] * 2 + [((4, 4, 32), (8, 4, 32), (4, 8, 32))], 1, 4096),
    "both windings": ([((2, 2, 64), (30, 2, 64), (2, 30, 64)), ((34, 2, 64), (34, 30, 64), (62, 2, 64))], 1, 4096),
    "screen range": ([((S20, 10, 64), (10, 10, 64), (10, 40, 64)), ((S20 + 0.125, 20, 64), (12, 12, 64), (12, 42, 64)),
                      ((-S20, -S20, 64), (50, 5, 64), (5, 40, 64)), ((20, -S20 - 0.125, 64), (50, 5, 64), (5, 40, 64))], 1, 4096),
}


@pytest.mark.parametrize("size", SIZES)
def test_planted_triangles_equal_the_reference(size):
    renderer = tsdf_amd.Renderer()
    for name, (corners, near, far) in sorted(PLANTED.items()):
        V, I = mesh_of(corners)
        wants = {}
        for cull in (False, True):
            got, wants[cull], targets = both(V, I, size, near, far, cull, into=renderer)
            check(got, wants[cull], targets, "%s cull %d" % (name, cull))
        info, culled = wants[False]["info"], wants[True]["info"]
        # what each case is there for, by the reference alone
        if name == "behind near and beyond far":
            assert info["n_dropped"] == 2 and info["n_live"] == 1
        if name == "zero area":
            assert info["n_live"] == 1 and info["n_dropped"] == 0
        if name in ("whole image", "ten times larger"):
            assert info["n_pixels_hit"] == size[0] * size[1] and info["n_large"] == 1
        if name == "at the large threshold" and size == (64, 48):
            assert info["n_large"] == 0 and info["n_live"] == 2
        if name == "one over the threshold" and size == (64, 48):
            assert info["n_large"] == 2
        if name == "identical":
            assert (wants[False]["triangle"] == 0).any() and not (wants[False]["triangle"] == 1).any()
        if name == "both windings":
            assert info["n_live"] == 2 and culled["n_live"] == 1 and 0 < culled["n_pixels_hit"] < info["n_pixels_hit"]
        if name == "screen range":
            assert info["n_dropped"] == 2 and info["n_live"] == 2
    renderer.close()


def test_a_nan_vertex_and_an_infinite_one_drop_their_triangles():
    V, I = mesh_of([((3, 3, 64), (20, 3, 64), (3, 20, 64)), ((30, 3, 64), (50, 3, 64), (30, 20, 64)), ((30, 25, 64), (50, 25, 64), (30, 40, 64))])
    V[1, 0] = np.nan
    V[5, 2] = np.inf
    got, want, targets = both(V, I, (64, 48), 1, 4096)
    check(got, want, targets, "NaN vertex")
    assert want["info"]["n_dropped"] == 2 and want["info"]["n_live"] == 1 and want["info"]["n_pixels_hit"] > 50


@pytest.mark.parametrize("size", SIZES)
def test_a_soup_on_the_fixed_point_grid_equals_the_reference(size):
    rng = np.random.default_rng(500 + size[0])
    n = 500
    sx = rng.integers(-16 * 256, (size[0] + 16) * 256, (n, 3)) / 256.0
    sy = rng.integers(-16 * 256, (size[1] + 16) * 256, (n, 3)) / 256.0
    whole = rng.random((n, 3)) < 0.4                                         # whole and half pixels: centres on edges and vertices
    sx[whole] = np.round(sx[whole] * 2) / 2
    sy[whole] = np.round(sy[whole] * 2) / 2
    z = 2.0 ** rng.integers(4, 9, (n, 3))
    small = rng.random(n) < 0.7                                              # most of them a few pixels, like marching-cubes triangles
    sx[small] = sx[small, :1] + (sx[small] - sx[small, :1]) / 16
    sy[small] = sy[small, :1] + (sy[small] - sy[small, :1]) / 16
    sx, sy = np.round(sx * 256) / 256, np.round(sy * 256) / 256
    V = np.array([vertex(sx[t, c], sy[t, c], z[t, c]) for t in range(n) for c in range(3)], F)
    I = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)[:, [0, 2, 1]].reshape(-1)
    N = rng.normal(size=(3 * n, 3)).astype(F)
    N[7] = 0.0
    N[11, 1] = np.nan
    RGB = rng.integers(0, 256, (3 * n, 3)).astype(np.uint8)
    X, Y, _, usable = ref.project(V, IDENTITY, K, 1, 4096)
    assert usable.all() and np.array_equal(X, np.round(sx.reshape(-1) * 256).astype(np.int64)) and np.array_equal(Y, np.round(sy.reshape(-1) * 256).astype(np.int64))
    for cull in (False, True):
        got, want, targets = both(V, I, size, 1, 4096, cull, N, RGB)
        check(got, want, targets, "soup %s cull %d" % (size, cull))
        assert want["info"]["n_pixels_hit"] > size[0] * size[1] // 2
    assert want["coverage"].max() > 1


# ---- the fused sphere -------------------------------------------------------------------------------------------------------------------
RK = np.array([52.5, 0, 0, 0, 52.5, 0, 31.5, 23.5, 1], F)                    # the depth camera's view at a tenth of its resolution
CENTRE, RADIUS, DISTANCE = np.array([1500.0, 1500.0, 1500.0]), 600.0, 2000.0
POSES = {"front": ((1500, 1500, -500), tuple(CENTRE), 100.0, 8000.0),
         "oblique": ((600, 1100, -300), tuple(CENTRE), 100.0, 8000.0),
         "close": ((1500, 1400, 300), tuple(CENTRE), 700.0, 8000.0)}         # the nearest surface is 600 mm away: triangles cross near


def on_orbit(yaw, pitch):
    """A camera DISTANCE from the sphere's centre, looking at it; (0, 0) is the front view."""
    y, p = np.radians(yaw), np.radians(pitch)
    return camera_at(tuple(CENTRE + DISTANCE * np.array([np.sin(y) * np.cos(p), np.sin(p), -np.cos(y) * np.cos(p)])), look_at=tuple(CENTRE))


def sphere_frame(cam):
    """The exact depth image (uint16 mm, 0: no hit) of the sphere alone -- no background, so its outline has no neighbours behind it --
    and a colour image that varies over the surface."""
    o, d = tsdf_amd.pixel_rays(cam, W, H)
    o, d = o.astype(np.float64), d.astype(np.float64)                        # d has camera depth 1: t is the depth
    a, b, c = (d * d).sum(axis=1), (d * (o - CENTRE)).sum(axis=1), ((o - CENTRE) ** 2).sum(axis=1) - RADIUS ** 2
    disc = b * b - a * c
    t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, 0.0)
    p = o + t[:, None] * d
    rgb = np.where(disc[:, None] > 0, np.clip((p - CENTRE) / RADIUS * 127 + 128, 0, 255), 0).astype(np.uint8)
    return np.round(t).astype(np.uint16), rgb.reshape(-1)


def fused_sphere():
    """Seven views round the front of the sphere, so that the outline of the front view is seen from the side as well."""
    gv = tsdf_amd.TSDFVolume((32,) * 3, (3000.0,) * 3)
    gv.enable_colour()
    for yaw, pitch in ((0, 0), (-20, 0), (20, 0), (-40, 0), (40, 0), (0, -30), (0, 30)):
        cam = on_orbit(yaw, pitch)
        depth, rgb = sphere_frame(cam)
        gv.integrate_colour(depth, rgb, W, H, cam)
    return gv


@pytest.fixture(scope="module")
def sphere():
    gv = fused_sphere()
    mesh = gv.extract_mesh(normals=True, colours=True)
    arrays = (mesh.vertices, mesh.indices, mesh.normals, mesh.colours)
    assert len(arrays[0]) > 300
    views = {name: (np.asarray(camera_at(p, look_at=at).inverse_pose(), F).reshape(-1).copy(), near, far) for name, (p, at, near, far) in POSES.items()}
    wants = {name: ref.render(arrays[0], arrays[1], 64, 48, ip, RK, near, far, 0, arrays[2], arrays[3]) for name, (ip, near, far) in views.items()}
    yield gv, mesh, arrays, views, wants
    mesh.close()
    gv.close()


def test_the_fused_sphere_from_three_poses(sphere):
    _, mesh, _, views, wants = sphere
    renderer = tsdf_amd.Renderer()
    for name, (ip, near, far) in views.items():
        got = mesh.render(ip, RK, (64, 48), near, far, targets=ALL, into=renderer)
        check(got, wants[name], ALL, name)
        assert wants[name]["info"]["n_pixels_hit"] > 200, name
    assert wants["close"]["info"]["n_dropped"] > 0 and wants["front"]["info"]["n_dropped"] == 0
    # two runs give the same bytes
    again = mesh.render(*views["oblique"][:1], RK, (64, 48), *views["oblique"][1:], targets=ALL, into=renderer)
    check(again, wants["oblique"], ALL, "oblique again")
    # a warm handle at the other image size: nothing grows, and the small image is the reference's
    warm = renderer.scratch_bytes
    V, I, N, RGB = sphere[2]
    ip, near, far = views["front"]
    small = mesh.render(ip, RK, (37, 29), near, far, targets=ALL, into=renderer)
    check(small, ref.render(V, I, 37, 29, ip, RK, near, far, 0, N, RGB), ALL, "37 x 29")
    assert renderer.scratch_bytes == warm == 8 * 64 * 48 + 16 * len(V) + 4 * (len(I) // 3 + 1) + 40
    renderer.close()


def test_back_face_culling_leaves_the_view_from_outside_alone(sphere):
    _, mesh, _, views, wants = sphere
    ip, near, far = views["front"]
    got = mesh.render(ip, RK, (64, 48), near, far, cull_back=True, targets=ALL)
    for name in ALL:
        assert ref.same_bytes(got[name], wants["front"][name]), name
    assert 0 < got["info"]["n_live"] <= wants["front"]["info"]["n_live"]


def test_simplified_and_smoothed_meshes(sphere):
    _, mesh, _, views, _ = sphere
    ip, near, far = views["front"]
    nearer = np.asarray(camera_at((1500, 1500, -100), look_at=tuple(CENTRE)).inverse_pose(), F).reshape(-1).copy()
    for what, other in (("simplified", mesh.simplify(500.0)), ("smoothed", mesh.smooth(5, normals=True))):
        V, I, N, RGB = other.vertices, other.indices, other.normals, other.colours
        if what == "simplified":
            ip = nearer                                                               # so that its triangles' boxes pass the threshold
        want = ref.render(V, I, 64, 48, ip, RK, near, far, 0, N, RGB)
        got = other.render(ip, RK, (64, 48), near, far, targets=ALL)
        check(got, want, ALL, what)
        assert want["info"]["n_pixels_hit"] > 200
        if what == "simplified":
            assert want["info"]["n_large"] > 0 and got["info"]["n_large"] == want["info"]["n_large"]     # the large path was taken
        other.close()


def test_vertex_normals_against_the_face_normal_fallback(sphere):
    _, mesh, (V, I, N, RGB), views, wants = sphere
    ip, near, far = views["oblique"]
    got, want, targets = both(V, I, (64, 48), near, far, inv_pose=ip, k=RK)           # no normals given: the faces'
    check(got, want, targets, "face normals")
    hit = want["triangle"] != ref.MISS
    smooth = wants["oblique"]["normals"]
    # the same winners and depths, another normal map: a face normal is one direction per triangle, finite wherever the triangle has an area
    # in space; the field's gradient is NaN at vertices next to unobserved voxels.  (No sign is asserted between the two: at the rim of
    # what one frame observed the projective field's gradient and the faces that close the surface need not agree.)
    assert ref.same_bytes(want["z"], wants["oblique"]["z"]) and ref.same_bytes(want["triangle"], wants["oblique"]["triangle"])
    assert not ref.same_bytes(want["normals"], smooth)
    assert hit.sum() > 200 and np.isfinite(want["normals"][hit]).all() and np.isfinite(smooth[hit]).all(axis=1).any()


def test_every_subset_of_targets(sphere):
    _, mesh, _, views, wants = sphere
    ip, near, far = views["front"]
    renderer = tsdf_amd.Renderer()
    for r in range(len(ALL) + 1):
        for subset in itertools.combinations(ALL, r):
            got = renderer.render(mesh, ip, RK, (64, 48), near, far, targets=subset)
            assert set(got) == set(subset) | {"info"}
            check(got, wants["front"], subset, "targets %s" % (subset,))
    renderer.close()


def test_normals_agree_in_sign_with_the_ray_cast_and_the_depth_map_integrates(sphere):
    gv, mesh, _, _, _ = sphere
    cam = on_orbit(0, 0)
    Vr, Nr = gv.raycast(W, H, cam)
    got = mesh.render(cam.inverse_pose(), cam.k(), (W, H), 100.0, 8000.0, targets=("vertices", "normals", "depth", "z"))
    Nm = got["normals"]
    hit = np.isfinite(Vr).all(axis=1) & np.isfinite(Nr).all(axis=1) & np.isfinite(Nm).all(axis=1)
    assert hit.sum() > 10000
    assert ((Nm[hit].astype(np.float64) * Nr[hit].astype(np.float64)).sum(axis=1) > 0).all()
    # the depth map has the format integrate takes
    depth = got["depth"]
    assert depth.dtype == np.uint16 and depth.shape == (W * H,) and (depth > 0).sum() == got["info"]["n_pixels_hit"]
    fresh = tsdf_amd.TSDFVolume((32,) * 3, (3000.0,) * 3)
    fresh.integrate(depth, W, H, cam)
    assert (fresh.get_weight_data() > 0).sum() > 0                                    # observes voxels: the format is the one integrate takes
    fresh.close()


# ---- refusals and bad input -------------------------------------------------------------------------------------------------------------
def test_refusals_a_bad_index_and_the_empty_mesh(sphere):
    _, mesh, (V, I, N, RGB), views, wants = sphere
    ip, near, far = views["front"]
    renderer = tsdf_amd.Renderer()
    good = dict(inv_pose=ip, k=RK, size=(64, 48), near=near, far=far)

    def refused(words, **change):
        args = dict(good, **change)
        with pytest.raises(ValueError, match=words):
            renderer.render(mesh, args["inv_pose"], args["k"], args["size"], args["near"], args["far"], targets=args.get("targets", ("depth",)))
    refused("pixels", size=(0, 48))
    refused("pixels", size=(64, 0))
    bad = ip.copy()
    bad[13] = np.inf
    refused("finite", inv_pose=bad)
    for at, value in ((1, 0.25), (3, 0.25), (8, 1.5), (0, np.nan)):
        kk = RK.copy()
        kk[at] = value
        refused("non-standard k|finite", k=kk)
    refused("near", near=0.0)
    refused("near", near=-5.0)
    refused("near", near=10.0, far=5.0)
    refused("near", far=np.inf)
    refused("near", near=np.nan)
    refused("unknown render targets", targets=("depth", "stencil"))
    with pytest.raises(ValueError, match="unknown flags"):
        t = _capi.RenderTargets()
        _capi.check(_capi.lib.tsdf_mesh_render(renderer._h, mesh._h, 64, 48, ip.ctypes.data_as(_capi._fp), RK.ctypes.data_as(_capi._fp), near, far, 6, C.byref(t), None))
    with pytest.raises(ValueError, match="multiple of 3"):
        tsdf_amd.render_mesh(V, I[:-1], ip, RK, (64, 48), near, far, into=renderer)
    with pytest.raises(ValueError, match="no colours"):
        tsdf_amd.render_mesh(V, I, ip, RK, (64, 48), near, far, targets=("rgb",), into=renderer)
    plain = sphere[0].extract_mesh()                                                  # a handle without colours
    with pytest.raises(ValueError, match="no colours"):
        plain.render(ip, RK, (64, 48), near, far, targets=("rgb",), into=renderer)
    plain.close()
    # the handle still renders
    check(mesh.render(ip, RK, (64, 48), near, far, targets=ALL, into=renderer), wants["front"], ALL, "after the refusals")

    # an index that is not below n_vertices: found on the device, reported by the call that waits
    broken = I.copy()
    broken[len(I) // 2] = len(V)
    with pytest.raises(ValueError, match="not below n_vertices"):
        tsdf_amd.render_mesh(V, broken, ip, RK, (64, 48), near, far, into=renderer)
    with pytest.raises(ValueError, match="not below n_vertices"):
        tsdf_amd.render_mesh(V[:0], I[:3], ip, RK, (64, 48), near, far, into=renderer)
    check(mesh.render(ip, RK, (64, 48), near, far, targets=ALL, into=renderer), wants["front"], ALL, "after the bad index")

    # the empty mesh: a successful render of all misses
    got = tsdf_amd.render_mesh(V[:0], I[:0], ip, RK, (37, 29), near, far, targets=BARE, into=renderer)
    check(got, ref.render(V[:0], I[:0], 37, 29, ip, RK, near, far), BARE, "empty")
    assert (got["triangle"] == ref.MISS).all() and np.isnan(got["z"]).all() and (got["depth"] == 0).all() and got["info"]["n_pixels_hit"] == 0
    empty = tsdf_amd.Mesh()
    got = empty.render(ip, RK, (37, 29), near, far, targets=BARE, into=renderer)
    assert (got["triangle"] == ref.MISS).all() and got["info"] == {"n_triangles": 0, "n_live": 0, "n_dropped": 0, "n_large": 0, "n_pixels_hit": 0}
    empty.close()
    renderer.close()


def test_a_render_without_info_reports_the_bad_index_when_somebody_waits():
    V, I = mesh_of([((3, 3, 64), (20, 3, 64), (3, 20, 64)), ((30, 3, 64), (50, 3, 64), (30, 20, 64))])
    I = I.copy()
    I[4] = 77
    renderer = tsdf_amd.Renderer()
    from tsdf_amd.api import _DeviceArray
    with _DeviceArray(V) as dv, _DeviceArray(I) as di, _DeviceArray(nbytes=4 * 64 * 48) as dt:
        assert renderer.render_arrays_device(len(V), I.size, dv.ptr.value, di.ptr.value, IDENTITY, K, (64, 48), 1, 4096,
                                             targets={"triangle": dt.ptr.value}) is None
        with pytest.raises(ValueError, match="not below n_vertices"):
            renderer.info()
        tri = np.empty(64 * 48, np.uint32)
        _capi.check(_capi.lib.tsdf_device_download(tri.ctypes.data, dt.ptr, tri.nbytes))
        assert set(tri.tolist()) == {0, ref.MISS}                                    # the other triangle was rendered
        I[4] = 5
        _capi.check(_capi.lib.tsdf_device_upload(di.ptr, I.ctypes.data, I.nbytes))
        renderer.render_arrays_device(len(V), I.size, dv.ptr.value, di.ptr.value, IDENTITY, K, (64, 48), 1, 4096, targets={"triangle": dt.ptr.value})
        assert renderer.info()["n_live"] == 2
    renderer.close()
