"""The C ABI of colour alignment (include/tsdf_amd.h, "colour alignment"): the header declares the six entry points with the shapes the
group states, the built library exports them, the Python binding carries the same argument lists, and NULL arguments are refused with
the function's name in the message before anything touches a device (no GPU needed)."""
import ctypes as C
import os
import re

from tests.test_capi_rays_integrate_symbols import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {
    "tsdf_volume_sample_intensity_device": ["const tsdf_volume *", "uint64_t", "const float *", "float *", "float *", "void *"],
    "tsdf_volume_sample_intensity": ["const tsdf_volume *", "uint64_t", "const float *", "float *", "float *"],
    "tsdf_rgb_to_intensity_device": ["uint32_t", "uint32_t", "const uint8_t *", "uint32_t", "float *", "void *"],
    # (an array parameter keeps its name and extent: they are part of the shape)
    "tsdf_aligner_step_colour": ["tsdf_aligner *", "const tsdf_volume *", "uint32_t", "const float *", "const float *", "const double T[16]",
                                 "float", "float", "float", "float A[36]", "float b[6]", "float residual_inliers[4]", "float *"],
    "tsdf_aligner_run_colour": ["tsdf_aligner *", "const tsdf_volume *", "uint32_t", "const tsdf_align_colour_stage *", "float", "float", "float",
                                "double T[16]", "float residual[2]", "float inliers[2]"],
    "tsdf_tracker_align_field_colour": ["tsdf_tracker *", "const float kinv[9]", "const uint8_t *", "float", "float", "double T_world_cam[16]",
                                        "float residual[2]", "float inliers[2]"],
}


def test_the_header_declares_the_signatures():
    text, decl = declarations()
    for name, args in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    stage = re.search(r"typedef struct tsdf_align_colour_stage \{(.*?)\} tsdf_align_colour_stage;", text, re.S)
    assert stage, "tsdf_align_colour_stage"
    fields = [" ".join(f.split()) for f in stage.group(1).split(";") if f.strip()]
    assert fields == ["const float *device_points", "const float *device_intensity", "uint32_t n", "uint32_t iterations"], fields


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments_and_null_is_refused_by_name():
    from tsdf_amd import _capi
    vp, u32, u64, f = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    lib = _capi.lib
    assert lib.tsdf_volume_sample_intensity_device.argtypes == [vp, u64, vp, vp, vp, vp]
    assert lib.tsdf_volume_sample_intensity.argtypes == [vp, u64, vp, vp, vp]
    assert lib.tsdf_rgb_to_intensity_device.argtypes == [u32, u32, vp, u32, vp, vp]
    assert lib.tsdf_aligner_step_colour.argtypes == [vp, vp, u32, vp, vp, vp, f, f, f, vp, vp, vp, vp]
    assert lib.tsdf_aligner_run_colour.argtypes == [vp, vp, u32, vp, f, f, f, vp, vp, vp]
    assert lib.tsdf_tracker_align_field_colour.argtypes == [vp, vp, vp, f, f, vp, vp, vp]
    assert [n for n, _ in _capi.AlignColourStage._fields_] == ["device_points", "device_intensity", "n", "iterations"]
    assert C.sizeof(_capi.AlignColourStage) == 24

    def refused(rc, name):
        assert rc == _capi.TSDF_ERR_INVALID, name
        assert name in _capi.last_error(), (name, _capi.last_error())

    refused(lib.tsdf_volume_sample_intensity_device(None, 0, None, None, None, None), "tsdf_volume_sample_intensity")
    refused(lib.tsdf_volume_sample_intensity(None, 0, None, None, None), "tsdf_volume_sample_intensity")
    refused(lib.tsdf_rgb_to_intensity_device(4, 4, None, 1, None, None), "tsdf_rgb_to_intensity")
    refused(lib.tsdf_aligner_step_colour(None, None, 0, None, None, None, 1.0, 1.0, 0.0, None, None, None, None), "tsdf_aligner_step_colour")
    refused(lib.tsdf_aligner_run_colour(None, None, 0, None, 1.0, 1.0, 0.0, None, None, None), "tsdf_aligner_run_colour")
    refused(lib.tsdf_aligner_run_colour(None, None, 1, None, 1.0, 1.0, 0.0, None, None, None), "tsdf_aligner_run_colour")
    refused(lib.tsdf_tracker_align_field_colour(None, None, None, 1.0, 0.0, None, None, None), "tsdf_tracker_align_field_colour")
    import tsdf_amd
    assert callable(tsdf_amd.TSDFVolume.sample_intensity) and callable(tsdf_amd.TSDFVolume.sample_intensity_device)
    assert callable(tsdf_amd.rgb_to_intensity) and callable(tsdf_amd.rgb_to_intensity_device)
