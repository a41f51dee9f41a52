"""The C ABI of the frame differences (include/tsdf_amd.h, "frame differences", and the tracker's dynamic rejection): the header declares
the entry points with the signatures the group gives, the built library exports them, the Python binding carries the same argument lists
and struct layouts (the 56-byte blob row), and everything that can be refused without a device is refused with a message naming the
entry point (no GPU needed)."""
import ctypes as C
import os
import re

from tests.capi_header import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {
    "tsdf_frame_diff_create": ("int", ["tsdf_frame_diff **"]),
    "tsdf_frame_diff_destroy": ("void", ["tsdf_frame_diff *"]),
    "tsdf_frame_diff_get_info": ("int", ["const tsdf_frame_diff *", "tsdf_frame_diff_info *"]),
    "tsdf_frame_diff_scratch_bytes": ("int", ["const tsdf_frame_diff *", "uint64_t *"]),
    "tsdf_frame_diff_compare_device": ("int", ["tsdf_frame_diff *", "const uint16_t *", "const uint16_t *", "uint32_t", "uint32_t",
                                               "const tsdf_diff_params *", "uint8_t *", "void *"]),
    "tsdf_frame_diff_cluster": ("int", ["tsdf_frame_diff *", "uint32_t", "uint32_t", "uint32_t", "void *"]),
    "tsdf_frame_diff_buffers": ("int", ["const tsdf_frame_diff *", "const uint32_t **", "const uint64_t **", "const uint32_t **", "const uint32_t **",
                                        "const tsdf_diff_blob **"]),
    "tsdf_frame_diff_download": ("int", ["const tsdf_frame_diff *", "uint32_t *", "uint32_t *", "tsdf_diff_blob *"]),
    "tsdf_frame_diff_mask_device": ("int", ["tsdf_frame_diff *", "uint32_t", "uint8_t *", "uint32_t *", "const uint16_t *", "uint16_t *", "void *"]),
    "tsdf_tracker_set_dynamic_rejection": ("int", ["tsdf_tracker *", "const tsdf_diff_rejection *"]),
    "tsdf_tracker_dynamic_rejection": ("int", ["const tsdf_tracker *", "int *", "tsdf_diff_rejection *"]),
    "tsdf_tracker_last_rejection": ("int", ["const tsdf_tracker *", "uint64_t [5]", "uint64_t *", "const uint8_t **"]),
}


def struct_body(text, name):
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S)
    return " ".join(m.group(1).split()) if m else None


def test_the_header_declares_the_signatures():
    text, decl = declarations(EXPECTED)
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    assert re.search(r"typedef\s+struct\s+tsdf_frame_diff\s+tsdf_frame_diff\s*;", text)
    for name, value in (("NO_FRAME", "0u"), ("NO_MODEL", "1u"), ("SAME", "2u"), ("FARTHER", "3u"), ("NEARER", "4u"), ("NO_BLOB", "0xffffffffu")):
        assert re.search(r"#define\s+TSDF_DIFF_%s\s+%s\b" % (name, value), text), name
    assert struct_body(text, "tsdf_diff_params") == "uint32_t tolerance; uint32_t quadratic;"
    assert struct_body(text, "tsdf_diff_blob") == ("uint32_t label, size; uint32_t lo[2], hi[2]; uint32_t min_depth, max_depth; "
                                                   "uint64_t sum_x, sum_y, sum_depth;")
    assert struct_body(text, "tsdf_frame_diff_info") == ("uint32_t width, height; uint32_t tolerance, quadratic; uint32_t connectivity; "
                                                         "uint32_t depth_step, min_pixels; uint32_t reserved; uint64_t counts[5]; "
                                                         "uint64_t n_blobs, n_kept_blobs;")
    assert struct_body(text, "tsdf_diff_rejection") == ("uint32_t tolerance, quadratic; uint32_t connectivity; uint32_t depth_step, min_pixels; "
                                                        "uint32_t dilate;")


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments():
    from tsdf_amd import _capi
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib = _capi.lib
    for name in EXPECTED:
        assert name in _capi.EXPORTS, name
    assert lib.tsdf_frame_diff_create.argtypes == [C.POINTER(vp)] and lib.tsdf_frame_diff_create.restype == C.c_int
    assert lib.tsdf_frame_diff_destroy.argtypes == [vp] and lib.tsdf_frame_diff_destroy.restype is None
    assert lib.tsdf_frame_diff_get_info.argtypes == [vp, C.POINTER(_capi.FrameDiffInfo)]
    assert lib.tsdf_frame_diff_scratch_bytes.argtypes == [vp, C.POINTER(u64)]
    assert lib.tsdf_frame_diff_compare_device.argtypes == [vp, vp, vp, u32, u32, C.POINTER(_capi.DiffParams), vp, vp]
    assert lib.tsdf_frame_diff_cluster.argtypes == [vp, u32, u32, u32, vp]
    assert lib.tsdf_frame_diff_buffers.argtypes == [vp] + [C.POINTER(vp)] * 5
    assert lib.tsdf_frame_diff_download.argtypes == [vp, vp, vp, vp]
    assert lib.tsdf_frame_diff_mask_device.argtypes == [vp, u32, vp, vp, vp, vp, vp]
    assert lib.tsdf_tracker_set_dynamic_rejection.argtypes == [vp, C.POINTER(_capi.DiffRejection)]
    assert lib.tsdf_tracker_dynamic_rejection.argtypes == [vp, C.POINTER(C.c_int), C.POINTER(_capi.DiffRejection)]
    assert lib.tsdf_tracker_last_rejection.argtypes == [vp, C.POINTER(u64 * 5), C.POINTER(u64), C.POINTER(vp)]
    assert [(n, t) for n, t in _capi.DiffBlob._fields_] == [("label", u32), ("size", u32), ("lo", u32 * 2), ("hi", u32 * 2), ("min_depth", u32),
                                                           ("max_depth", u32), ("sum_x", u64), ("sum_y", u64), ("sum_depth", u64)]
    assert C.sizeof(_capi.DiffBlob) == 56 and _capi.DiffBlob.sum_x.offset == 32 and _capi.DiffBlob.min_depth.offset == 24
    assert C.sizeof(_capi.FrameDiffInfo) == 88 and _capi.FrameDiffInfo.counts.offset == 32 and _capi.FrameDiffInfo.n_blobs.offset == 72
    assert C.sizeof(_capi.DiffParams) == 8 and C.sizeof(_capi.DiffRejection) == 24
    import tsdf_amd
    from tsdf_amd import api
    d = api.DIFF_BLOB_DTYPE
    assert d.itemsize == 56 and d.fields["lo"][1] == 8 and d.fields["hi"][1] == 16 and d.fields["min_depth"][1] == 24 and d.fields["sum_x"][1] == 32
    assert (api.DIFF_NO_FRAME, api.DIFF_NO_MODEL, api.DIFF_SAME, api.DIFF_FARTHER, api.DIFF_NEARER, api.DIFF_NO_BLOB) == (0, 1, 2, 3, 4, 0xFFFFFFFF)
    assert api.DIFF_DEFAULTS == dict(tolerance=50, quadratic=0, connectivity=8, depth_step=50, min_pixels=64, dilate=4)
    for name in ("compare", "compare_device", "counts", "states", "cluster", "blobs", "pixels", "labels", "mask", "mask_device", "info", "scratch_bytes"):
        assert hasattr(tsdf_amd.FrameDiff, name), name
    from tsdf_amd import synth, tracking
    assert callable(synth.moving_disc_frame)
    for name in ("set_dynamic_rejection", "dynamic_rejection", "last_rejection"):
        assert callable(getattr(tracking.FrameToModelTracker, name)), name


def test_what_needs_no_device_is_refused():
    """Null handles everywhere; the argument checks that come before the handle is touched are reached with a pointer that is never
    read (the checks of the handle's state come after them)."""
    from tsdf_amd import _capi
    lib, invalid = _capi.lib, _capi.TSDF_ERR_INVALID
    n, on, p, r = C.c_uint64(0), C.c_int(0), _capi.DiffParams(50, 0), _capi.DiffRejection(50, 0, 8, 50, 64, 4)
    calls = {
        "tsdf_frame_diff_create": lambda: lib.tsdf_frame_diff_create(None),
        "tsdf_frame_diff_get_info": lambda: lib.tsdf_frame_diff_get_info(None, None),
        "tsdf_frame_diff_scratch_bytes": lambda: lib.tsdf_frame_diff_scratch_bytes(None, C.byref(n)),
        "tsdf_frame_diff_compare_device": lambda: lib.tsdf_frame_diff_compare_device(None, None, None, 4, 4, C.byref(p), None, None),
        "tsdf_frame_diff_cluster": lambda: lib.tsdf_frame_diff_cluster(None, 8, 50, 1, None),
        "tsdf_frame_diff_buffers": lambda: lib.tsdf_frame_diff_buffers(None, None, None, None, None, None),
        "tsdf_frame_diff_download": lambda: lib.tsdf_frame_diff_download(None, None, None, None),
        "tsdf_frame_diff_mask_device": lambda: lib.tsdf_frame_diff_mask_device(None, 0, None, None, None, None, None),
        "tsdf_tracker_set_dynamic_rejection": lambda: lib.tsdf_tracker_set_dynamic_rejection(None, C.byref(r)),
        "tsdf_tracker_dynamic_rejection": lambda: lib.tsdf_tracker_dynamic_rejection(None, C.byref(on), None),
        "tsdf_tracker_last_rejection": lambda: lib.tsdf_tracker_last_rejection(None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == invalid, name
        assert name in _capi.last_error(), (name, _capi.last_error())
    lib.tsdf_frame_diff_destroy(None)   # a null handle is ignored
    # the arguments alone: refused in front of the handle check
    dummy = C.c_void_p(64)   # (never read)
    compare = lambda f, m, w, h, prm: lib.tsdf_frame_diff_compare_device(None, f, m, w, h, prm, None, None)
    refused = {
        "null frame or model": [lambda: compare(None, dummy, 4, 4, C.byref(p)), lambda: compare(dummy, None, 4, 4, C.byref(p))],
        "null params": [lambda: compare(dummy, dummy, 4, 4, None)],
        "a side is above 65535": [lambda: compare(dummy, dummy, 65536, 1, C.byref(p)), lambda: compare(dummy, dummy, 1, 65536, C.byref(p)),
                                  lambda: compare(dummy, dummy, 65535, 65537, C.byref(p)),       # 2^32 - 1 pixels
                                  lambda: compare(dummy, dummy, 0xFFFFFFFF, 0xFFFFFFFF, C.byref(p))],
        "width * height must be in": [lambda: compare(dummy, dummy, 0, 4, C.byref(p)), lambda: compare(dummy, dummy, 4, 0, C.byref(p))],
        "connectivity must be 4 or 8": [lambda c=c: lib.tsdf_frame_diff_cluster(None, c, 50, 1, None) for c in (0, 6, 26, 5)] +
                                       [lambda: lib.tsdf_tracker_set_dynamic_rejection(None, C.byref(_capi.DiffRejection(50, 0, 6, 50, 64, 4)))],
        "is above 32": [lambda: lib.tsdf_frame_diff_mask_device(None, 33, None, None, None, None, None),
                        lambda: lib.tsdf_tracker_set_dynamic_rejection(None, C.byref(_capi.DiffRejection(50, 0, 8, 50, 64, 33)))],
        "given together or not at all": [lambda: lib.tsdf_frame_diff_mask_device(None, 0, None, None, dummy, None, None),
                                         lambda: lib.tsdf_frame_diff_mask_device(None, 0, None, None, None, dummy, None)],
    }
    for text, some in refused.items():
        for call in some:
            assert call() == invalid, text
            assert text in _capi.last_error(), (text, _capi.last_error())
    assert compare(dummy, dummy, 65535, 65535, C.byref(p)) == invalid and "null handle" in _capi.last_error()   # the largest image passes the size checks
