"""Ray integration's C ABI (include/tsdf_amd.h, "ray integration"): the header declares the three entry points with the signatures the
issue gives, the built library exports them, and the Python binding carries the same argument lists (no GPU needed)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYS_ARGS = ["tsdf_volume *", "uint64_t", "const float *", "uint64_t", "const float *", "float", "float", "int", "uint64_t *"]
EXPECTED = {"tsdf_integrate_rays_device": RAYS_ARGS, "tsdf_integrate_rays": RAYS_ARGS, "tsdf_volume_release_ray_scratch": ["tsdf_volume *"]}


def declarations():
    text = open(os.path.join(ROOT, "include", "tsdf_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(tsdf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            types.append(re.sub(r"\s*[A-Za-z_][A-Za-z0-9_]*$", "", a) if not a.endswith("*") else a)
        out[name] = [t.replace(" *", " *").strip() for t in types]
    return text, out


def test_the_header_declares_the_signatures():
    text, decl = declarations()
    for name, args in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    assert re.search(r"#define\s+TSDF_RAYS_BAND_ONLY\s+1\b", text)


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments():
    from tsdf_amd import _capi
    vp, u64, f, i = C.c_void_p, C.c_uint64, C.c_float, C.c_int
    rays = [vp, u64, vp, u64, vp, f, f, i, C.POINTER(u64)]
    assert _capi.TSDF_RAYS_BAND_ONLY == 1
    assert _capi.lib.tsdf_integrate_rays_device.argtypes == rays and _capi.lib.tsdf_integrate_rays.argtypes == rays
    assert _capi.lib.tsdf_volume_release_ray_scratch.argtypes == [vp]
    # a null volume is refused before anything touches a device
    assert _capi.lib.tsdf_integrate_rays(None, 0, None, 0, None, 0.0, 1.0, 0, None) == _capi.TSDF_ERR_INVALID
    assert _capi.lib.tsdf_volume_release_ray_scratch(None) == _capi.TSDF_ERR_INVALID
    import tsdf_amd
    for method in ("integrate_rays", "integrate_rays_device", "release_ray_scratch"):
        assert callable(getattr(tsdf_amd.TSDFVolume, method))
