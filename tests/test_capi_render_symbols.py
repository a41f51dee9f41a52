"""The C ABI of the mesh renderer (include/tsdf_amd.h, "mesh rendering"): the header declares the eight entry points, the flag, the
large-box constant and the two structs with the signatures the issue gives, the built library exports them, the Python binding carries
the same argument lists and struct layouts, and null and malformed arguments are refused, with a message, before a device or a handle
is touched (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW = ["uint32_t", "uint32_t", "const float", "const float", "float", "float", "uint32_t", "const tsdf_render_targets *", "tsdf_render_info *"]
EXPECTED = {
    "tsdf_render_create": ("int", ["tsdf_render **"]),
    "tsdf_render_destroy": ("void", ["tsdf_render *"]),
    "tsdf_render_scratch_bytes": ("int", ["const tsdf_render *", "uint64_t *"]),
    "tsdf_render_get_info": ("int", ["const tsdf_render *", "tsdf_render_info *"]),
    "tsdf_render_set_large_box": ("int", ["tsdf_render *", "uint32_t"]),
    "tsdf_render_mesh_device": ("int", ["tsdf_render *", "uint64_t", "uint64_t", "const float *", "const uint32_t *", "const float *", "const uint8_t *"]
                                + VIEW + ["void *"]),
    "tsdf_mesh_render_device": ("int", ["tsdf_render *", "tsdf_mesh *"] + VIEW + ["void *"]),
    "tsdf_mesh_render": ("int", ["tsdf_render *", "tsdf_mesh *"] + VIEW),
}


def declarations():
    """(the header, name -> (return type, argument types with the parameter names and array bounds taken out))."""
    whole = open(os.path.join(ROOT, "include", "tsdf_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(tsdf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        if name not in EXPECTED:
            continue
        types = []
        for a in args.split(","):
            a = re.sub(r"\[\d+\]$", "", " ".join(a.split()))
            m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a)
            types.append(m.group(1).strip())
        out[name] = (ret, types)
    return whole, out


def test_the_header_declares_the_signatures_the_flag_and_the_contract():
    whole, decl = declarations()
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    assert re.search(r"#define\s+TSDF_RENDER_CULL_BACK\s+1u\b", whole) and re.search(r"#define\s+TSDF_RENDER_LARGE_BOX\s+256u\b", whole)
    assert whole.index("/* ---- mesh smoothing") < whole.index("/* ---- mesh rendering") < whole.index("/* ---- scene flow")
    group = whole[whole.index("/* ---- mesh rendering"):whole.index("/* ---- scene flow")]
    for words in ("(I[3t], I[3t+2], I[3t+1])", "world_to_camera", "r = 1.0f / c.z", "sx = fx * (c.x / c.z) + cx", "rintf(sx * 256.0f)", "2^20", "USABLE", "LIVE",
                  "A2 = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0)", "FRONT-FACING", "A2 < 0", "TOP-LEFT", "a_k > 0, or", "a_k == 0 and b_k > 0", "2^58",
                  "b1 = (float)E_1 / (float)|A2|", "rr = r0 + (b1 * (r1 - r0) + b2 * (r2 - r0))", "z = 1.0f / rr", "((uint64)bits(z) << 32) | t",
                  "0xFFFFFFFF", "q1 = (b1 * r1) * z", "a0 + (q1 * (a1 - a0) + q2 * (a2 - a0))", "sqrtf((n.x n.x + n.y n.y) + n.z n.z)", "+ 0.5f",
                  "tsdf_vertices_to_depth_device", "n_dropped", "n_large", "pinned", "8 bytes per pixel", "16", "atomicMin", "DESIGN.md 34",
                  "near-plane clipping", "2^32 - 1", "different devices"):
        assert words in group, words
    for field in ("uint32_t *triangle;", "float *z;", "uint16_t *depth;", "float *vertices;", "float *normals;", "uint8_t *rgb;",
                  "uint64_t n_triangles, n_live, n_dropped, n_large, n_pixels_hit;"):
        assert field in group, field


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments_and_the_host_refuses():
    from tsdf_amd import _capi
    vp, u32, u64, f32, fp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float, C.POINTER(C.c_float)
    lib = _capi.lib
    for name in EXPECTED:
        assert name in _capi.EXPORTS
    assert (_capi.TSDF_RENDER_CULL_BACK, _capi.TSDF_RENDER_LARGE_BOX, _capi.TSDF_RENDER_MISS) == (1, 256, 0xFFFFFFFF)
    T, I = _capi.RenderTargets, _capi.RenderInfo
    assert C.sizeof(T) == 48 and [f[0] for f in T._fields_] == ["triangle", "z", "depth", "vertices", "normals", "rgb"]
    assert C.sizeof(I) == 40 and [f[0] for f in I._fields_] == ["n_triangles", "n_live", "n_dropped", "n_large", "n_pixels_hit"]
    view = [u32, u32, fp, fp, f32, f32, u32, C.POINTER(T), C.POINTER(I)]
    assert lib.tsdf_render_create.argtypes == [C.POINTER(vp)] and lib.tsdf_render_create.restype == C.c_int
    assert lib.tsdf_render_destroy.argtypes == [vp] and lib.tsdf_render_destroy.restype is None
    assert lib.tsdf_render_scratch_bytes.argtypes == [vp, C.POINTER(u64)]
    assert lib.tsdf_render_get_info.argtypes == [vp, C.POINTER(I)]
    assert lib.tsdf_render_set_large_box.argtypes == [vp, u32] and lib.tsdf_render_set_large_box.restype == C.c_int
    assert lib.tsdf_render_mesh_device.argtypes == [vp, u64, u64, vp, vp, vp, vp] + view + [vp] and lib.tsdf_render_mesh_device.restype == C.c_int
    assert lib.tsdf_mesh_render_device.argtypes == [vp, vp] + view + [vp] and lib.tsdf_mesh_render_device.restype == C.c_int
    assert lib.tsdf_mesh_render.argtypes == [vp, vp] + view and lib.tsdf_mesh_render.restype == C.c_int

    # refused before anything touches a device or reads a handle (the pointers below are never followed), with a message
    invalid, p = _capi.TSDF_ERR_INVALID, vp(64)
    raw = lib.tsdf_render_mesh_device
    ident = np.eye(4, dtype=np.float32).reshape(-1)
    k0 = np.array([64, 0, 0, 0, 64, 0, 32, 24, 1], np.float32)
    as_fp = lambda a: a.ctypes.data_as(fp)
    depth_only, with_rgb = T(depth=64), T(depth=64, rgb=64)

    def call(r=p, nv=6, ni=3, v=p, i=p, n=None, rgb=None, w=64, h=48, ip=ident, k=k0, near=1.0, far=100.0, flags=0, t=depth_only):
        return raw(r, nv, ni, v, i, n, rgb, w, h, None if ip is None else as_fp(ip), None if k is None else as_fp(k), near, far, flags,
                   None if t is None else C.byref(t), None, None)

    def refused(rc, *words):
        assert rc == invalid
        for w in words:
            assert w in _capi.last_error(), (w, _capi.last_error())
    refused(call(r=None), "tsdf_render_mesh_device", "null render handle")
    refused(call(ip=None), "null inv_pose or k")
    refused(call(k=None), "null inv_pose or k")
    refused(call(t=None), "null targets")
    refused(call(v=None), "null device_vertices")
    refused(call(i=None), "null device_indices")
    refused(call(ni=4), "multiple of 3")
    refused(call(nv=2 ** 32), "32-bit")
    refused(call(w=0), "pixels")
    refused(call(h=0), "pixels")
    refused(call(w=65537, h=65535), "pixels")                 # 2^32 - 1 exactly
    refused(call(w=65536, h=65536), "pixels")
    for bad in (float("inf"), float("nan")):
        m = ident.copy()
        m[7] = bad
        refused(call(ip=m), "inv_pose[7]", "finite")
        kk = k0.copy()
        kk[6] = bad
        refused(call(k=kk), "k[6]", "finite")
        refused(call(near=bad), "near")
        refused(call(far=bad), "far")
    for at, value in ((1, 0.5), (2, 0.5), (3, -1.0), (5, 1e-3), (8, 2.0)):
        kk = k0.copy()
        kk[at] = value
        refused(call(k=kk), "non-standard k")
    refused(call(near=0.0), "near")
    refused(call(near=-1.0), "near")
    refused(call(near=2.0, far=1.0), "near")
    refused(call(flags=2), "unknown flags")
    refused(call(t=with_rgb), "rgb target", "no colours")
    for fn in (lib.tsdf_mesh_render_device, lib.tsdf_mesh_render):
        tail = [None] if fn is lib.tsdf_mesh_render_device else []
        refused(fn(None, p, 64, 48, as_fp(ident), as_fp(k0), 1.0, 100.0, 0, C.byref(depth_only), None, *tail), "null render handle")
        refused(fn(p, None, 64, 48, as_fp(ident), as_fp(k0), 1.0, 100.0, 0, C.byref(depth_only), None, *tail), "null mesh")
        refused(fn(p, p, 64, 48, None, as_fp(k0), 1.0, 100.0, 0, C.byref(depth_only), None, *tail), "null inv_pose or k")
        refused(fn(p, p, 64, 48, as_fp(ident), as_fp(k0), 1.0, 100.0, 0, None, None, *tail), "null targets")
    refused(lib.tsdf_render_create(None), "tsdf_render_create")
    refused(lib.tsdf_render_scratch_bytes(None, None), "tsdf_render_scratch_bytes")
    refused(lib.tsdf_render_get_info(None, None), "tsdf_render_get_info")
    refused(lib.tsdf_render_set_large_box(None, 256), "tsdf_render_set_large_box")
    lib.tsdf_render_destroy(None)                              # (a null handle is fine)
    import tsdf_amd
    assert hasattr(tsdf_amd.Mesh, "render") and hasattr(tsdf_amd.Renderer, "render") and hasattr(tsdf_amd.Renderer, "render_device")
    assert callable(tsdf_amd.render_mesh) and callable(tsdf_amd.render_mesh_device)
    assert list(tsdf_amd.RENDER_TARGETS) == ["triangle", "z", "depth", "vertices", "normals", "rgb"]
