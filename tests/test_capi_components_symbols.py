"""The C ABI of the mesh components (include/tsdf_amd.h, "mesh components"): the header declares the five entry points with the
signatures the issue gives, the built library exports them, the Python binding carries the same argument lists, and null arguments are
refused before a device is touched (no GPU needed)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {
    "tsdf_label_components_device": ("int", ["uint64_t", "uint64_t", "const uint32_t *", "uint32_t *", "uint32_t *", "tsdf_components_info *", "void *"]),
    "tsdf_mesh_label_components": ("int", ["tsdf_mesh *", "tsdf_components_info *", "void *"]),
    "tsdf_mesh_component_buffers": ("int", ["const tsdf_mesh *", "const uint32_t **", "const uint32_t **"]),
    "tsdf_mesh_component_download": ("int", ["const tsdf_mesh *", "uint32_t *", "uint32_t *"]),
    "tsdf_mesh_filter_components": ("int", ["tsdf_mesh *", "uint64_t", "uint32_t", "tsdf_mesh *", "void *"]),
}


def declarations():
    """name -> (return type, argument types with the parameter names taken out) of the five declarations."""
    text = open(os.path.join(ROOT, "include", "tsdf_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
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
    return text, out


def test_the_header_declares_the_signatures():
    text, decl = declarations()
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    assert re.search(r"#define\s+TSDF_MESH_KEEP_LARGEST\s+1u\b", text)
    info = re.search(r"typedef\s+struct\s+tsdf_components_info\s*\{(.*?)\}\s*tsdf_components_info\s*;", text, flags=re.S)
    assert info and " ".join(info.group(1).split()) == "uint64_t n_components, n_triangles, largest_triangles; uint32_t largest_label;"


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments():
    from tsdf_amd import _capi
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib = _capi.lib
    assert _capi.TSDF_MESH_KEEP_LARGEST == 1
    info = C.POINTER(_capi.ComponentsInfo)
    assert lib.tsdf_label_components_device.argtypes == [u64, u64, vp, vp, vp, info, vp] and lib.tsdf_label_components_device.restype == C.c_int
    assert lib.tsdf_mesh_label_components.argtypes == [vp, info, vp]
    assert lib.tsdf_mesh_component_buffers.argtypes == [vp, C.POINTER(vp), C.POINTER(vp)]
    assert lib.tsdf_mesh_component_download.argtypes == [vp, vp, vp]
    assert lib.tsdf_mesh_filter_components.argtypes == [vp, u64, u32, vp, vp]
    assert [(n, t) for n, t in _capi.ComponentsInfo._fields_] == [("n_components", u64), ("n_triangles", u64), ("largest_triangles", u64),
                                                                   ("largest_label", u32)]
    assert C.sizeof(_capi.ComponentsInfo) == 32
    # null and malformed arguments are refused before anything touches a device, and leave a message
    invalid = _capi.TSDF_ERR_INVALID
    assert lib.tsdf_label_components_device(5, 0, None, None, None, None, None) == invalid
    assert "tsdf_label_components_device" in _capi.last_error()
    assert lib.tsdf_label_components_device(5, 3, None, vp(64), None, None, None) == invalid
    assert lib.tsdf_label_components_device(5, 4, vp(64), vp(64), None, None, None) == invalid and "multiple of 3" in _capi.last_error()
    assert lib.tsdf_label_components_device(2 ** 32, 3, vp(64), vp(64), None, None, None) == invalid
    assert lib.tsdf_label_components_device(5, 3 * 2 ** 31, vp(64), vp(64), None, None, None) == invalid
    assert lib.tsdf_mesh_label_components(None, None, None) == invalid
    assert lib.tsdf_mesh_component_buffers(None, None, None) == invalid
    assert lib.tsdf_mesh_component_download(None, None, None) == invalid
    assert lib.tsdf_mesh_filter_components(None, 0, 0, None, None) == invalid
    import tsdf_amd
    for name in ("label_components", "labels", "component_triangles", "component_buffers", "filter_components"):
        assert hasattr(tsdf_amd.Mesh, name), name
    assert callable(tsdf_amd.label_components) and callable(tsdf_amd.label_components_device)
