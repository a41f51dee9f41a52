"""The C ABI of coloured ray integration and of the colour at ray-query hits (include/tsdf_amd.h, "ray integration" rules 9 - 12, "ray
queries"): the header declares the five entry points with the signatures the issue gives, the built library exports them, and the
Python binding carries the same argument lists (no GPU needed)."""
import ctypes as C
import os

from tests.test_capi_rays_integrate_symbols import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYS_ARGS = ["tsdf_volume *", "uint64_t", "const float *", "uint64_t", "const float *", "const uint8_t *", "float", "float", "int", "uint64_t *"]
CAST_ARGS = ["const tsdf_volume *", "uint64_t", "const float *", "const float *", "const float *", "float *", "float *", "float *", "uint8_t *"]
EXPECTED = {"tsdf_integrate_rays_colour_device": RAYS_ARGS, "tsdf_integrate_rays_colour": RAYS_ARGS,
            "tsdf_volume_ray_scratch_bytes": ["const tsdf_volume *", "uint64_t *"],
            "tsdf_volume_cast_rays_colour_device": CAST_ARGS, "tsdf_volume_cast_rays_colour": CAST_ARGS}


def test_the_header_declares_the_signatures():
    text, decl = declarations()
    for name, args in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments():
    from tsdf_amd import _capi
    vp, u64, f, i = C.c_void_p, C.c_uint64, C.c_float, C.c_int
    rays = [vp, u64, vp, u64, vp, vp, f, f, i, C.POINTER(u64)]
    cast = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
    lib = _capi.lib
    assert lib.tsdf_integrate_rays_colour_device.argtypes == rays and lib.tsdf_integrate_rays_colour.argtypes == rays
    assert lib.tsdf_volume_cast_rays_colour_device.argtypes == cast and lib.tsdf_volume_cast_rays_colour.argtypes == cast
    assert lib.tsdf_volume_ray_scratch_bytes.argtypes == [vp, C.POINTER(u64)]
    # a null volume is refused before anything touches a device
    assert lib.tsdf_integrate_rays_colour(None, 0, None, 0, None, None, 0.0, 1.0, 0, None) == _capi.TSDF_ERR_INVALID
    assert lib.tsdf_volume_cast_rays_colour(None, 0, None, None, None, None, None, None, None) == _capi.TSDF_ERR_INVALID
    assert lib.tsdf_volume_ray_scratch_bytes(None, None) == _capi.TSDF_ERR_INVALID
    import tsdf_amd
    assert callable(tsdf_amd.TSDFVolume.ray_scratch_bytes)
