"""The C ABI of the column maps (include/tsdf_amd.h, "column maps"): the header declares the nine entry points with the signatures the
group gives, the built library exports them, the Python binding carries the same argument lists and struct layouts (the 32-byte row,
the 136-byte info), the flag and cell constants agree, and null arguments are refused before a device is touched (no GPU needed)."""
import ctypes as C
import os
import re

from tests.capi_header import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {
    "tsdf_columns_create": ("int", ["tsdf_columns **"]),
    "tsdf_columns_destroy": ("void", ["tsdf_columns *"]),
    "tsdf_volume_project_columns": ("int", ["const tsdf_volume *", "uint32_t", "uint32_t", "uint32_t", "const tsdf_esdf *", "uint32_t", "tsdf_columns *"]),
    "tsdf_columns_get_info": ("int", ["const tsdf_columns *", "tsdf_columns_info *"]),
    "tsdf_columns_buffer": ("int", ["const tsdf_columns *", "const tsdf_column **"]),
    "tsdf_columns_download": ("int", ["const tsdf_columns *", "tsdf_column *"]),
    "tsdf_columns_scratch_bytes": ("int", ["const tsdf_columns *", "uint64_t *"]),
    "tsdf_columns_classify_device": ("int", ["tsdf_columns *", "uint32_t", "uint32_t", "uint32_t", "uint8_t *", "void *"]),
    "tsdf_columns_classify": ("int", ["tsdf_columns *", "uint32_t", "uint32_t", "uint32_t", "uint8_t *"]),
}


def test_the_header_declares_the_signatures():
    text, decl = declarations(EXPECTED)
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    assert re.search(r"typedef\s+struct\s+tsdf_columns\s+tsdf_columns\s*;", text)
    for name, value in (("TSDF_COLUMNS_REVERSED", "1u"), ("TSDF_CELL_NO_GROUND", "0u"),
                        ("TSDF_CELL_TRAVERSABLE", "1u"), ("TSDF_CELL_BLOCKED", "2u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), text), name
    row = re.search(r"typedef\s+struct\s+tsdf_column\s*\{(.*?)\}\s*tsdf_column\s*;", text, flags=re.S)
    assert row and " ".join(row.group(1).split()) == ("uint32_t n_unknown, n_free, n_occupied; int32_t top, bottom; uint32_t headroom; "
                                                      "float height; float min_distance;")
    info = re.search(r"typedef\s+struct\s+tsdf_columns_info\s*\{(.*?)\}\s*tsdf_columns_info\s*;", text, flags=re.S)
    assert info and " ".join(info.group(1).split()) == (
        "uint32_t size[3]; uint32_t axis; float voxel_size[3]; float offset[3]; uint32_t lo, hi; uint32_t flags; uint32_t has_esdf; "
        "uint32_t map_size[2]; uint32_t map_axes[2]; uint64_t n_unknown, n_free, n_occupied, n_ground; "
        "uint64_t n_no_ground, n_traversable, n_blocked; uint32_t max_step, min_headroom;")
    whole = open(os.path.join(ROOT, "include", "tsdf_amd.h")).read()
    assert whole.index("/* ---- rolling volume") < whole.index("/* ---- column maps") < whole.index("/* ---- slab exchange")
    group = whole[whole.index("/* ---- column maps"):whole.index("typedef struct tsdf_columns tsdf_columns;")]
    for word in ("Out of scope", "multi-level", "0x7FC00000", "+0.0f", "TSDF_ERR_INVALID", "does not synchronise"):
        assert word in group, word


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments():
    from tsdf_amd import _capi
    vp, u32, i32, u64, f32 = C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64, C.c_float
    lib = _capi.lib
    assert _capi.TSDF_COLUMNS_REVERSED == 1
    assert (_capi.TSDF_CELL_NO_GROUND, _capi.TSDF_CELL_TRAVERSABLE, _capi.TSDF_CELL_BLOCKED) == (0, 1, 2)
    for name in EXPECTED:
        assert name in _capi.EXPORTS, name
    assert lib.tsdf_columns_create.argtypes == [C.POINTER(vp)] and lib.tsdf_columns_create.restype == C.c_int
    assert lib.tsdf_columns_destroy.argtypes == [vp] and lib.tsdf_columns_destroy.restype is None
    assert lib.tsdf_volume_project_columns.argtypes == [vp, u32, u32, u32, vp, u32, vp]
    assert lib.tsdf_columns_get_info.argtypes == [vp, C.POINTER(_capi.ColumnsInfo)]
    assert lib.tsdf_columns_buffer.argtypes == [vp, C.POINTER(vp)]
    assert lib.tsdf_columns_download.argtypes == [vp, vp]
    assert lib.tsdf_columns_scratch_bytes.argtypes == [vp, C.POINTER(u64)]
    assert lib.tsdf_columns_classify_device.argtypes == [vp, u32, u32, u32, vp, vp]
    assert lib.tsdf_columns_classify.argtypes == [vp, u32, u32, u32, vp]
    assert [(n, t) for n, t in _capi.Column._fields_] == [("n_unknown", u32), ("n_free", u32), ("n_occupied", u32), ("top", i32), ("bottom", i32),
                                                           ("headroom", u32), ("height", f32), ("min_distance", f32)]
    assert C.sizeof(_capi.Column) == 32 and _capi.Column.top.offset == 12 and _capi.Column.height.offset == 24
    assert [(n, t) for n, t in _capi.ColumnsInfo._fields_] == [
        ("size", u32 * 3), ("axis", u32), ("voxel_size", f32 * 3), ("offset", f32 * 3), ("lo", u32), ("hi", u32), ("flags", u32), ("has_esdf", u32),
        ("map_size", u32 * 2), ("map_axes", u32 * 2), ("n_unknown", u64), ("n_free", u64), ("n_occupied", u64), ("n_ground", u64),
        ("n_no_ground", u64), ("n_traversable", u64), ("n_blocked", u64), ("max_step", u32), ("min_headroom", u32)]
    assert C.sizeof(_capi.ColumnsInfo) == 136 and _capi.ColumnsInfo.lo.offset == 40 and _capi.ColumnsInfo.n_unknown.offset == 72
    assert _capi.ColumnsInfo.max_step.offset == 128
    import tsdf_amd
    from tsdf_amd import api
    assert api.COLUMN_DTYPE.itemsize == 32 and api.COLUMN_DTYPE.fields["top"][1] == 12 and api.COLUMN_DTYPE.fields["min_distance"][1] == 28
    assert tsdf_amd.COLUMN_DTYPE is api.COLUMN_DTYPE
    assert (tsdf_amd.CELL_NO_GROUND, tsdf_amd.CELL_TRAVERSABLE, tsdf_amd.CELL_BLOCKED) == (0, 1, 2)
    from tests import columns_ref
    assert columns_ref.COLUMN_DTYPE == api.COLUMN_DTYPE
    # null arguments are refused before anything touches a device, and leave a message naming the entry point
    invalid = _capi.TSDF_ERR_INVALID
    calls = {
        "tsdf_columns_create": lambda: lib.tsdf_columns_create(None),
        "tsdf_volume_project_columns": lambda: lib.tsdf_volume_project_columns(None, 2, 0, 0, None, 0, None),
        "tsdf_columns_get_info": lambda: lib.tsdf_columns_get_info(None, None),
        "tsdf_columns_buffer": lambda: lib.tsdf_columns_buffer(None, None),
        "tsdf_columns_download": lambda: lib.tsdf_columns_download(None, None),
        "tsdf_columns_scratch_bytes": lambda: lib.tsdf_columns_scratch_bytes(None, None),
        "tsdf_columns_classify_device": lambda: lib.tsdf_columns_classify_device(None, 0, 0, 0, None, None),
        "tsdf_columns_classify": lambda: lib.tsdf_columns_classify(None, 0, 0, 0, None),
    }
    for name, call in calls.items():
        assert call() == invalid, name
        message = _capi.last_error()
        assert re.search(r"\b%s\b" % name, message), (name, message)
    lib.tsdf_columns_destroy(None)   # a null handle is ignored
    assert callable(tsdf_amd.TSDFVolume.column_map)
    for name in ("columns", "info", "classify", "classify_device", "device_buffer", "scratch_bytes", "close", "height_world"):
        assert hasattr(tsdf_amd.ColumnMap, name), name
