"""The C ABI of the mesh simplification (include/tsdf_amd.h, "mesh simplification"): the header declares the two entry points with the
signatures the issue gives, the built library exports them, the Python binding carries the same argument lists, and null and malformed
arguments are refused, with a message, before a device or a handle is touched (no GPU needed)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {
    "tsdf_simplify_mesh_device": ("int", ["uint64_t", "uint64_t", "const float *", "const uint32_t *", "const float *", "const uint8_t *", "float",
                                          "uint32_t", "tsdf_mesh *", "void *"]),
    "tsdf_mesh_simplify": ("int", ["tsdf_mesh *", "float", "uint32_t", "tsdf_mesh *", "void *"]),
}


def declarations():
    """(the header, name -> (return type, argument types with the parameter names taken out) of the two declarations)."""
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


def test_the_header_declares_the_signatures_and_the_contract():
    whole, decl = declarations()
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    group = whole[whole.index("/* ---- mesh simplification"):whole.index("/* ---- distance field")]
    assert whole.index("/* ---- mesh components") < whole.index("/* ---- mesh simplification")
    for words in ("floorf(V_a / h)", "2^20", "2^21", "<< 42", "smallest source index", "llrintf(V_a * 1024.0f)", "llrintf(N_a * 1048576.0f)",
                  "(2 S + n) / (2 n)", "position weld", "tsdf_mesh_filter_components(dst, 1, 0", "80 n_clusters", "12 P"):
        assert words in group, words
    # the two groups that listed simplification as out of scope point here instead
    assert len(re.findall(r'simplification are the group "mesh simplification" below', whole)) == 2


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
    assert lib.tsdf_simplify_mesh_device.argtypes == [u64, u64, vp, vp, vp, vp, f32, u32, vp, vp] and lib.tsdf_simplify_mesh_device.restype == C.c_int
    assert lib.tsdf_mesh_simplify.argtypes == [vp, f32, u32, vp, vp] and lib.tsdf_mesh_simplify.restype == C.c_int
    # refused before anything touches a device or reads a handle (the pointers below are never followed), with a message
    invalid, p = _capi.TSDF_ERR_INVALID, vp(64)
    raw = lib.tsdf_simplify_mesh_device

    def refused(rc, *words):
        assert rc == invalid
        for w in words:
            assert w in _capi.last_error(), (w, _capi.last_error())
    refused(raw(6, 3, p, p, None, None, 1.0, 0, None, None), "tsdf_simplify_mesh_device", "null dst")
    refused(raw(6, 3, None, p, None, None, 1.0, 0, p, None), "null device_vertices")
    refused(raw(6, 3, p, None, None, None, 1.0, 0, p, None), "null device_indices")
    refused(raw(6, 4, p, p, None, None, 1.0, 0, p, None), "multiple of 3")
    refused(raw(2 ** 32, 3, p, p, None, None, 1.0, 0, p, None), "32-bit")
    refused(raw(6, 3 * 2 ** 31, p, p, None, None, 1.0, 0, p, None), "32-bit")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(raw(6, 3, p, p, None, None, bad, 0, p, None), "cell_size")
    refused(raw(6, 3, p, p, None, None, 1.0, 1, p, None), "unknown flags")
    refused(raw(2 ** 30 + 1, 3, p, p, None, None, 1.0, 0, p, None), "2^30")
    refused(lib.tsdf_mesh_simplify(None, 1.0, 0, p, None), "tsdf_mesh_simplify", "null src")
    refused(lib.tsdf_mesh_simplify(p, 1.0, 0, None, None), "null dst")
    refused(lib.tsdf_mesh_simplify(p, 1.0, 0, p, None), "dst is src")
    import tsdf_amd
    assert hasattr(tsdf_amd.Mesh, "simplify")
    assert callable(tsdf_amd.simplify_mesh) and callable(tsdf_amd.simplify_mesh_device)
