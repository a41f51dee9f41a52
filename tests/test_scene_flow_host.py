"""Scene flow without a GPU (include/tsdf_amd.h, "scene flow"): the two CPU reference updates of tests/scene_flow_ref.py agree
within a derived tolerance, the per-voxel count is bounded below 255 by the triangle table, the header declares the entry points, the
built library exports them, the Python binding carries the same argument lists and null arguments are refused before a device is
touched."""
import ctypes as C
import os
import re

import numpy as np

from tests import mesh_ref, scene_flow_cases as cases, scene_flow_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
MATRICES = ["const float [16]", "const float [16]", "const float [9]", "const float [9]"]
EXPECTED = {
    "tsdf_volume_apply_scene_flow": ("int", ["tsdf_volume *", "tsdf_mesh *", "const uint16_t *", "const float *", "uint32_t", "uint32_t"] + MATRICES +
                                     ["float", "uint32_t", "tsdf_scene_flow_info *"]),
    "tsdf_volume_apply_scene_flow_device": ("int", ["tsdf_volume *", "tsdf_mesh *", "const uint16_t *", "const float *", "uint32_t", "uint32_t"] +
                                            MATRICES + ["float", "uint32_t", "tsdf_scene_flow_info *", "void *"]),
}


def sphere_scene(oracle):
    """A 14 x 12 x 11 grid of 10 mm voxels with a sphere in it, 350 mm in front of the 40 x 30 camera; the mesh by the CPU reference."""
    size, voxel = (14, 12, 11), 10.0
    offset = (-70.0, -60.0, 300.0)
    centre, radius = (2.0, -3.0, 356.0), 38.0
    D = cases.sphere_field(size, voxel, offset, centre, radius, 19.0)
    V, I, _, keys = mesh_ref.indexed(oracle, D, size, (voxel,) * 3, offset)
    cam = cases.camera((0.0, 0.0, 0.0))
    depth = cases.sphere_depth((0.0, 0.0, 0.0), centre, radius)
    return size, V, I, keys, cam, depth


def test_the_gather_equals_the_serial_scatter_within_rounding(oracle):
    size, V, I, keys, cam, depth = sphere_scene(oracle)
    assert len(V) > 200
    flow = cases.random_flow(11)
    flow[12:14, 14:22] = np.nan
    pix, seen = ref.correspond(oracle, V, depth, flow, cases.WIDTH, cases.HEIGHT, cam.pose(), cam.inverse_pose(), cam.k(), cam.kinv(), 10.0)
    corr = pix != ref.NONE
    assert corr.sum() > 40 and (~seen).sum() > 50 and (seen & ~corr).sum() > 0       # the far side is not seen; NaN pixels are dropped
    n = size[0] * size[1] * size[2]
    nodes = np.zeros((n, 6), F32)
    nodes[:, :3] = np.random.default_rng(5).uniform(-400.0, 400.0, (n, 3)).astype(F32)
    nodes[:, 3:] = 7.0
    gathered, moved = ref.apply(nodes, keys, I, pix, flow, size)
    scattered, magnitude = ref.scatter_serial(nodes, keys, I, pix, flow, size)
    count = ref.counts(keys, I, size)
    changed = (gathered != nodes).any(axis=1)
    assert moved > 40 and changed.sum() > 40 and changed.sum() <= moved
    assert np.array_equal(gathered[:, 3:], nodes[:, 3:]) and np.array_equal(scattered[:, 3:], nodes[:, 3:])
    assert np.array_equal(gathered[count == 0], nodes[count == 0])
    # Both are fp32 sums of the same terms -- the node's translation and scale * flow once per corresponding soup vertex -- added in
    # different orders: the scatter adds them one at a time, the gather adds m equal terms as one product.  Each of the at most
    # n_adds = count[v] roundings of either is at most 2^-24 of a partial sum, itself at most the sum of |terms|: the two differ by
    # at most n_adds * 2^-23 * sum |terms| per component.
    bound = count[:, None] * 2.0 ** -23 * magnitude
    err = np.abs(gathered[:, :3].astype(np.float64) - scattered[:, :3].astype(np.float64))
    assert (err <= bound).all(), float((err - bound).max())
    assert (err > 0).any()                                                          # (the two orders do round differently somewhere)


def test_the_count_of_a_voxel_stays_below_255(oracle):
    """count[v] sums, over the eight cubes round v, the entries of each cube's table row that lie on the three cube edges ending in
    v's corner of that cube.  v is a different corner of each of the eight: the bound is the sum over the corners of the largest such
    number any configuration has."""
    table, n = oracle.mc_tables()
    touching = [np.array([c in mesh_ref.EDGE[e] for e in range(12)]) for c in range(8)]
    bound = 0
    for c in range(8):
        worst = 0
        for kind in range(256):
            row = table[kind][:n[kind]].astype(np.int64)
            worst = max(worst, int(touching[c][row].sum()))
        bound += worst
    assert 6 <= bound < 255, bound


def declarations():
    text = open(os.path.join(ROOT, "include", "tsdf_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(tsdf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        if name not in EXPECTED:
            continue
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)(\[\d+\])?$", a)
            types.append((m.group(1).strip() + (" " + m.group(3) if m.group(3) else "")).strip())
        out[name] = (ret, types)
    return text, out


def test_the_header_declares_the_signatures():
    text, decl = declarations()
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    assert re.search(r"#define\s+TSDF_SCENE_FLOW_DEFORMED\s+1u\b", text)
    info = re.search(r"typedef\s+struct\s+tsdf_scene_flow_info\s*\{(.*?)\}\s*tsdf_scene_flow_info\s*;", text, flags=re.S)
    assert info and " ".join(info.group(1).split()) == "uint64_t n_vertices, n_correspondences, n_nodes_moved;"
    host = open(os.path.join(ROOT, "tsdf_amd", "host", "include", "SceneFusion_krnl.hpp")).read()
    assert re.search(r"void\s+process_frames\(TSDFVolume \*volume, const Camera \*const camera, const uint16_t width, const uint16_t height,\s*"
                     r"const uint16_t \*const h_depth_data, const float3 \*const h_scene_flow\);", host)


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments():
    from tsdf_amd import _capi
    vp, u32, u64, fp = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_float)
    lib = _capi.lib
    assert _capi.TSDF_SCENE_FLOW_DEFORMED == 1
    common = [vp, vp, vp, vp, u32, u32, fp, fp, fp, fp, C.c_float, u32, C.POINTER(_capi.SceneFlowInfo)]
    assert lib.tsdf_volume_apply_scene_flow.argtypes == common and lib.tsdf_volume_apply_scene_flow.restype == C.c_int
    assert lib.tsdf_volume_apply_scene_flow_device.argtypes == common + [vp]
    assert [(n, t) for n, t in _capi.SceneFlowInfo._fields_] == [("n_vertices", u64), ("n_correspondences", u64), ("n_nodes_moved", u64)]
    assert C.sizeof(_capi.SceneFlowInfo) == 24
    assert {"tsdf_volume_apply_scene_flow", "tsdf_volume_apply_scene_flow_device"} <= set(_capi.EXPORTS)
    # null arguments are refused before anything touches a device, and leave a message
    invalid = _capi.TSDF_ERR_INVALID
    assert lib.tsdf_volume_apply_scene_flow(None, None, None, None, 40, 30, None, None, None, None, 10.0, 0, None) == invalid
    assert "tsdf_volume_apply_scene_flow" in _capi.last_error() and "null" in _capi.last_error()
    assert lib.tsdf_volume_apply_scene_flow_device(None, None, None, None, 40, 30, None, None, None, None, 10.0, 0, None, None) == invalid
    import tsdf_amd
    for name in ("apply_scene_flow", "apply_scene_flow_device", "get_deformation"):
        assert callable(getattr(tsdf_amd.TSDFVolume, name)), name
