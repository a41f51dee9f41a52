"""The C ABI of the class objects (include/tsdf_amd.h, "class objects"): the header declares the nine entry points with the signatures
the group gives, the built library exports them, the Python binding carries the same argument lists and struct layouts (the 72-byte info
and the 72-byte row), and null arguments are refused before a device is touched (no GPU needed)."""
import ctypes as C
import os
import re

from tests.capi_header import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {
    "tsdf_objects_create": ("int", ["tsdf_objects **"]),
    "tsdf_objects_destroy": ("void", ["tsdf_objects *"]),
    "tsdf_volume_find_objects": ("int", ["const tsdf_volume *", "uint32_t", "const uint8_t *", "uint32_t", "uint32_t", "uint32_t", "uint32_t",
                                         "tsdf_objects *"]),
    "tsdf_objects_get_info": ("int", ["const tsdf_objects *", "tsdf_objects_info *"]),
    "tsdf_objects_buffers": ("int", ["const tsdf_objects *", "const uint32_t **", "const uint64_t **", "const uint32_t **", "const uint32_t **",
                                     "const tsdf_class_object **"]),
    "tsdf_objects_download": ("int", ["const tsdf_objects *", "uint32_t *", "uint32_t *", "tsdf_class_object *"]),
    "tsdf_objects_lookup_device": ("int", ["const tsdf_objects *", "uint64_t", "const float *", "uint32_t *", "void *"]),
    "tsdf_objects_lookup": ("int", ["const tsdf_objects *", "uint64_t", "const float *", "uint32_t *"]),
    "tsdf_objects_scratch_bytes": ("int", ["const tsdf_objects *", "uint64_t *"]),
}


def test_the_header_declares_the_signatures():
    text, decl = declarations(EXPECTED)
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    assert re.search(r"typedef\s+struct\s+tsdf_objects\s+tsdf_objects\s*;", text)
    assert re.search(r"#define\s+TSDF_OBJECT_NONE\s+0xFFFFFFFFu\b", text)
    info = re.search(r"typedef\s+struct\s+tsdf_objects_info\s*\{(.*?)\}\s*tsdf_objects_info\s*;", text, flags=re.S)
    assert info and " ".join(info.group(1).split()) == ("uint32_t size[3]; uint32_t connectivity; float voxel_size[3]; float offset[3]; "
                                                        "uint32_t min_votes, min_size; uint64_t n_labelled, n_objects, n_listed_objects;")
    row = re.search(r"typedef\s+struct\s+tsdf_class_object\s*\{(.*?)\}\s*tsdf_class_object\s*;", text, flags=re.S)
    assert row and " ".join(row.group(1).split()) == ("uint32_t label, size; uint32_t lo[3], hi[3]; uint64_t sum[3]; uint64_t votes; "
                                                      "uint32_t class_id, reserved;")


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments():
    from tsdf_amd import _capi
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    lib = _capi.lib
    assert _capi.TSDF_OBJECT_NONE == 0xFFFFFFFF
    for name in EXPECTED:
        assert name in _capi.EXPORTS, name
    assert lib.tsdf_objects_create.argtypes == [C.POINTER(vp)] and lib.tsdf_objects_create.restype == C.c_int
    assert lib.tsdf_objects_destroy.argtypes == [vp] and lib.tsdf_objects_destroy.restype is None
    assert lib.tsdf_volume_find_objects.argtypes == [vp, u32, vp, u32, u32, u32, u32, vp]
    assert lib.tsdf_objects_get_info.argtypes == [vp, C.POINTER(_capi.ObjectsInfo)]
    assert lib.tsdf_objects_buffers.argtypes == [vp] + [C.POINTER(vp)] * 5
    assert lib.tsdf_objects_download.argtypes == [vp, vp, vp, vp]
    assert lib.tsdf_objects_lookup_device.argtypes == [vp, u64, vp, vp, vp]
    assert lib.tsdf_objects_lookup.argtypes == [vp, u64, vp, vp]
    assert lib.tsdf_objects_scratch_bytes.argtypes == [vp, C.POINTER(u64)]
    I, O = _capi.ObjectsInfo, _capi.ClassObject
    assert [(n, t) for n, t in I._fields_] == [
        ("size", u32 * 3), ("connectivity", u32), ("voxel_size", f32 * 3), ("offset", f32 * 3), ("min_votes", u32), ("min_size", u32),
        ("n_labelled", u64), ("n_objects", u64), ("n_listed_objects", u64)]
    assert C.sizeof(I) == 72
    assert [getattr(I, n).offset for n, _ in I._fields_] == [0, 12, 16, 28, 40, 44, 48, 56, 64]
    assert [(n, t) for n, t in O._fields_] == [("label", u32), ("size", u32), ("lo", u32 * 3), ("hi", u32 * 3), ("sum", u64 * 3),
                                               ("votes", u64), ("class_id", u32), ("reserved", u32)]
    assert C.sizeof(O) == 72
    assert [getattr(O, n).offset for n, _ in O._fields_] == [0, 4, 8, 20, 32, 56, 64, 68]
    import tsdf_amd
    from tsdf_amd import api
    D = api.OBJECT_DTYPE
    assert D.itemsize == 72 and [D.fields[n][1] for n in D.names] == [0, 4, 8, 20, 32, 56, 64, 68]
    assert D.names == tuple(n for n, _ in O._fields_)
    assert tsdf_amd.OBJECT_DTYPE is D and tsdf_amd.OBJECT_NONE == 0xFFFFFFFF
    # null arguments are refused before anything touches a device, and leave a message naming the entry point
    invalid = _capi.TSDF_ERR_INVALID
    calls = {
        "tsdf_objects_create": lambda: lib.tsdf_objects_create(None),
        "tsdf_volume_find_objects": lambda: lib.tsdf_volume_find_objects(None, 1, None, 0, 26, 1, 0, None),
        "tsdf_objects_get_info": lambda: lib.tsdf_objects_get_info(None, None),
        "tsdf_objects_buffers": lambda: lib.tsdf_objects_buffers(None, None, None, None, None, None),
        "tsdf_objects_download": lambda: lib.tsdf_objects_download(None, None, None, None),
        "tsdf_objects_lookup_device": lambda: lib.tsdf_objects_lookup_device(None, 0, None, None, None),
        "tsdf_objects_lookup": lambda: lib.tsdf_objects_lookup(None, 0, None, None),
        "tsdf_objects_scratch_bytes": lambda: lib.tsdf_objects_scratch_bytes(None, None),
    }
    for name, call in calls.items():
        assert call() == invalid, name
        assert name in _capi.last_error(), (name, _capi.last_error())
    lib.tsdf_objects_destroy(None)   # a null handle is ignored
    assert callable(tsdf_amd.TSDFVolume.find_objects)
    for name in ("info", "voxels", "coordinates", "labels", "objects", "centroids", "boxes", "lookup", "lookup_device", "device_buffers",
                 "scratch_bytes", "close"):
        assert hasattr(tsdf_amd.Objects, name), name
