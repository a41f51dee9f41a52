"""The C ABI of the mesh smoothing (include/tsdf_amd.h, "mesh smoothing"): the header declares the four entry points and the two flags
with the signatures the issue gives, the built library exports them, the Python binding carries the same argument lists, and null and
malformed arguments are refused, with a message, before a device or a handle is touched (no GPU needed)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {
    "tsdf_smooth_mesh_device": ("int", ["uint64_t", "uint64_t", "const float *", "const uint32_t *", "const float *", "const uint8_t *", "uint32_t",
                                        "float", "float", "uint32_t", "tsdf_mesh *", "void *"]),
    "tsdf_mesh_smooth": ("int", ["tsdf_mesh *", "uint32_t", "float", "float", "uint32_t", "tsdf_mesh *", "void *"]),
    "tsdf_vertex_normals_device": ("int", ["uint64_t", "uint64_t", "const float *", "const uint32_t *", "float *", "void *"]),
    "tsdf_mesh_compute_normals": ("int", ["tsdf_mesh *", "void *"]),
}


def declarations():
    """(the header, name -> (return type, argument types with the parameter names taken out) of the four declarations)."""
    whole = open(os.path.join(ROOT, "include", "tsdf_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(tsdf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        if name not in EXPECTED:
            continue
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a)
            types.append(m.group(1).strip())
        out[name] = (ret, types)
    return whole, out


def test_the_header_declares_the_signatures_the_flags_and_the_contract():
    whole, decl = declarations()
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    assert re.search(r"#define\s+TSDF_SMOOTH_PIN_BOUNDARY\s+1u\b", whole) and re.search(r"#define\s+TSDF_SMOOTH_NORMALS\s+2u\b", whole)
    assert whole.index("/* ---- mesh simplification") < whole.index("/* ---- mesh smoothing") < whole.index("/* ---- scene flow")
    group = whole[whole.index("/* ---- mesh smoothing"):whole.index("/* ---- scene flow")]
    for words in ("LOOSE", "LIVE", "2^21", "llrintf(P_a(u) * 1024.0f)", "((double)S / (double)deg)", "(double)f * (d - (double)p)", "Guard", "m == 1",
                  "m >= 3", "llrint(c_a * 65536.0)", "I[3t+2]", "(min << 32) | max", "DESIGN.md 21", "8 n_indices", "12 E", "24 n_vertices",
                  "iterations above 1024", "dst == src"):
        assert words in group, words
    # the group that listed smoothing as out of scope points here instead
    assert 'Smoothing is the group "mesh smoothing"' in whole


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments_and_the_host_refuses():
    from tsdf_amd import _capi
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    lib = _capi.lib
    for name in EXPECTED:
        assert name in _capi.EXPORTS
    assert (_capi.TSDF_SMOOTH_PIN_BOUNDARY, _capi.TSDF_SMOOTH_NORMALS) == (1, 2)
    assert lib.tsdf_smooth_mesh_device.argtypes == [u64, u64, vp, vp, vp, vp, u32, f32, f32, u32, vp, vp] and lib.tsdf_smooth_mesh_device.restype == C.c_int
    assert lib.tsdf_mesh_smooth.argtypes == [vp, u32, f32, f32, u32, vp, vp] and lib.tsdf_mesh_smooth.restype == C.c_int
    assert lib.tsdf_vertex_normals_device.argtypes == [u64, u64, vp, vp, vp, vp] and lib.tsdf_vertex_normals_device.restype == C.c_int
    assert lib.tsdf_mesh_compute_normals.argtypes == [vp, vp] and lib.tsdf_mesh_compute_normals.restype == C.c_int
    # refused before anything touches a device or reads a handle (the pointers below are never followed), with a message
    invalid, p = _capi.TSDF_ERR_INVALID, vp(64)
    raw = lib.tsdf_smooth_mesh_device

    def refused(rc, *words):
        assert rc == invalid
        for w in words:
            assert w in _capi.last_error(), (w, _capi.last_error())
    refused(raw(6, 3, p, p, None, None, 1, 0.5, -0.53, 0, None, None), "tsdf_smooth_mesh_device", "null dst")
    refused(raw(6, 3, None, p, None, None, 1, 0.5, -0.53, 0, p, None), "null device_vertices")
    refused(raw(6, 3, p, None, None, None, 1, 0.5, -0.53, 0, p, None), "null device_indices")
    refused(raw(6, 4, p, p, None, None, 1, 0.5, -0.53, 0, p, None), "multiple of 3")
    refused(raw(2 ** 32, 3, p, p, None, None, 1, 0.5, -0.53, 0, p, None), "32-bit")
    refused(raw(6, 3 * 2 ** 31, p, p, None, None, 1, 0.5, -0.53, 0, p, None), "32-bit")
    for bad in (float("inf"), float("-inf"), float("nan")):
        refused(raw(6, 3, p, p, None, None, 1, bad, -0.53, 0, p, None), "finite")
        refused(raw(6, 3, p, p, None, None, 1, 0.5, bad, 0, p, None), "finite")
    refused(raw(6, 3, p, p, None, None, 1025, 0.5, -0.53, 0, p, None), "iterations")
    refused(raw(6, 3, p, p, None, None, 1, 0.5, -0.53, 4, p, None), "unknown flags")
    refused(lib.tsdf_mesh_smooth(None, 1, 0.5, -0.53, 0, p, None), "tsdf_mesh_smooth", "null src")
    refused(lib.tsdf_mesh_smooth(p, 1, 0.5, -0.53, 0, None, None), "null dst")
    refused(lib.tsdf_mesh_smooth(p, 1, 0.5, -0.53, 0, p, None), "dst is src")
    normals = lib.tsdf_vertex_normals_device
    refused(normals(6, 3, None, p, p, None), "tsdf_vertex_normals_device", "null device_vertices")
    refused(normals(6, 3, p, None, p, None), "null device_indices")
    refused(normals(6, 3, p, p, None, None), "null device_normals_out")
    refused(normals(6, 5, p, p, p, None), "multiple of 3")
    refused(normals(2 ** 32, 3, p, p, p, None), "32-bit")
    refused(normals(0, 3, None, p, None, None), "not below n_vertices")
    refused(lib.tsdf_mesh_compute_normals(None, None), "tsdf_mesh_compute_normals", "null mesh")
    import tsdf_amd
    assert hasattr(tsdf_amd.Mesh, "smooth") and hasattr(tsdf_amd.Mesh, "compute_normals")
    assert callable(tsdf_amd.smooth_mesh) and callable(tsdf_amd.smooth_mesh_device) and callable(tsdf_amd.vertex_normals)
