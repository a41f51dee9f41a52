"""The rolling-volume group of include/tsdf_amd.h (no GPU needed): its three functions are declared with the documented signatures,
exported by the library and bound in Python, and its two flags have the documented values."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "tsdf_volume_restore_shifted": "int tsdf_volume_restore_shifted(tsdf_volume *volume, const tsdf_snapshot *snapshot, const int32_t brick_shift[3], uint32_t flags);",
    "tsdf_snapshot_select": "int tsdf_snapshot_select(const tsdf_snapshot *src, const int32_t lo[3], const int32_t hi[3], uint32_t flags, tsdf_snapshot *dst);",
    "tsdf_volume_shift": "int tsdf_volume_shift(tsdf_volume *volume, const int32_t box_shift[3], tsdf_snapshot *work, tsdf_snapshot *leaving);",
}


def header():
    text = open(os.path.join(ROOT, "include", "tsdf_amd.h")).read()
    return text, re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_header_declares_the_group():
    text, code = header()
    assert text.index("---- sparse snapshot") < text.index("---- rolling volume") < text.index("int tsdf_volume_restore_shifted(")
    for name, signature in SIGNATURES.items():
        assert signature in code, name
    assert re.search(r"#define TSDF_RESTORE_KEEP_OTHERS 1u\b", code) and re.search(r"#define TSDF_SELECT_OUTSIDE 1u\b", code)


def test_the_library_exports_and_python_binds_the_group():
    lib = ctypes.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    from tsdf_amd import _capi
    i32p = ctypes.POINTER(ctypes.c_int32)
    expected = {
        "tsdf_volume_restore_shifted": [ctypes.c_void_p, ctypes.c_void_p, i32p, ctypes.c_uint32],
        "tsdf_snapshot_select": [ctypes.c_void_p, i32p, i32p, ctypes.c_uint32, ctypes.c_void_p],
        "tsdf_volume_shift": [ctypes.c_void_p, i32p, ctypes.c_void_p, ctypes.c_void_p],
    }
    for name, argtypes in expected.items():
        assert hasattr(lib, name), name
        assert name in _capi.EXPORTS, name
        bound = getattr(_capi.lib, name)
        assert bound.restype is ctypes.c_int and list(bound.argtypes) == argtypes, name
    assert _capi.TSDF_RESTORE_KEEP_OTHERS == 1 and _capi.TSDF_SELECT_OUTSIDE == 1


def test_null_arguments_are_refused_before_a_device_is_touched():
    from tsdf_amd import _capi
    lib = _capi.lib
    three = (ctypes.c_int32 * 3)(0, 0, 0)
    assert lib.tsdf_volume_restore_shifted(None, None, three, 0) != 0
    assert b"tsdf_volume_restore_shifted" in _capi.lib.tsdf_last_error()
    assert lib.tsdf_snapshot_select(None, three, three, 0, None) != 0
    assert b"tsdf_snapshot_select" in _capi.lib.tsdf_last_error()
    assert lib.tsdf_volume_shift(None, three, None, None) != 0
    assert b"tsdf_volume_shift" in _capi.lib.tsdf_last_error()
