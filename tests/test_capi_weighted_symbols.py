"""The C ABI of weighted integration (include/tsdf_amd.h, "weighted integration"): the header declares the six entry points and the two
flags, the built library exports them, the Python binding carries the same argument lists, the header states the rule, and null or bad
arguments are refused before a device is touched (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tsdf_amd.h")
MATS = ["const float [16]", "const float [16]", "const float [9]", "const float [9]"]
EXPECTED = {
    "tsdf_integrate_weighted": ("int", ["tsdf_volume *", "const uint16_t *", "const float *", "const uint8_t *", "uint32_t", "uint32_t"] + MATS),
    "tsdf_integrate_weighted_device": ("int", ["tsdf_volume *", "const uint16_t *", "const float *", "const uint8_t *", "uint32_t", "uint32_t"] + MATS),
    "tsdf_depth_weights_device": ("int", ["uint32_t", "uint32_t", "const uint16_t *", "const float [9]", "uint32_t", "float", "float *", "void *"]),
    "tsdf_depth_weights": ("int", ["uint32_t", "uint32_t", "const uint16_t *", "const float [9]", "uint32_t", "float", "float *"]),
    "tsdf_tracker_set_weighting": ("int", ["tsdf_tracker *", "uint32_t", "float"]),
    "tsdf_tracker_weighting": ("int", ["const tsdf_tracker *", "uint32_t *", "float *"]),
}


def declarations():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(tsdf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        if name not in EXPECTED:
            continue
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)(\[\d+\])?$", a)
            types.append((m.group(1).strip() + (" " + m.group(3) if m.group(3) else "")).strip())
        out[name] = (ret, types)
    return text, out


def test_the_header_declares_the_signatures():
    text, decl = declarations()
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    assert re.search(r"#define\s+TSDF_WEIGHTS_INVERSE_SQUARE\s+1u\b", text)
    assert re.search(r"#define\s+TSDF_WEIGHTS_COSINE\s+2u\b", text)


def test_the_library_exports_them_and_the_binding_carries_the_same_arguments():
    lib_path = os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    from tsdf_amd import _capi, api, tracking
    vp, u32, f32, fp = C.c_void_p, C.c_uint32, C.c_float, C.POINTER(C.c_float)
    for name in EXPECTED:
        assert name in exported, name + " is not exported by libtsdf_hip.so"
        assert name in _capi.EXPORTS, name
    lib = _capi.lib
    for name in ("tsdf_integrate_weighted", "tsdf_integrate_weighted_device"):
        assert getattr(lib, name).argtypes == [vp, vp, vp, vp, u32, u32, fp, fp, fp, fp] and getattr(lib, name).restype == C.c_int
    assert lib.tsdf_depth_weights_device.argtypes == [u32, u32, vp, fp, u32, f32, vp, vp]
    assert lib.tsdf_depth_weights.argtypes == [u32, u32, vp, fp, u32, f32, vp]
    assert lib.tsdf_tracker_set_weighting.argtypes == [vp, u32, f32]
    assert lib.tsdf_tracker_weighting.argtypes == [vp, C.POINTER(u32), C.POINTER(f32)]
    assert (_capi.TSDF_WEIGHTS_INVERSE_SQUARE, _capi.TSDF_WEIGHTS_COSINE) == (1, 2) == (api.WEIGHTS_INVERSE_SQUARE, api.WEIGHTS_COSINE)
    assert callable(api.TSDFVolume.integrate_weighted) and callable(api.TSDFVolume.integrate_weighted_device)
    assert callable(api.depth_weights) and callable(api.depth_weights_device)
    assert callable(tracking.FrameToModelTracker.set_weighting) and callable(tracking.FrameToModelTracker.weighting)
    import tsdf_amd
    assert tsdf_amd.depth_weights is api.depth_weights and tsdf_amd.depth_weights_device is api.depth_weights_device


def test_the_header_states_the_rule():
    text = open(HEADER).read()
    flat = " ".join(text[text.index("---- weighted integration"):text.index("---- colour fusion")].split())
    assert "nw = w + p" in flat
    assert "new_distance = ((D * w) + (tsdf * p)) / nw" in flat
    assert "nw > (float)cap ? (float)cap : nw" in flat
    assert "there is no weighted removal: fl(fl(w + p) - p) is not w" in flat
    assert "r = z_ref / d ; f = r * r ; f = f > 1 ? 1 : f" in flat
    assert "c = fabsf(np) / (sqrtf(nn) * sqrtf(pp))" in flat
    assert "tsdf_pipeline_step* does not take weights" in flat


def test_bad_arguments_are_refused_without_a_device():
    from tsdf_amd import _capi
    lib, invalid = _capi.lib, _capi.TSDF_ERR_INVALID
    for name in ("tsdf_integrate_weighted", "tsdf_integrate_weighted_device"):
        assert getattr(lib, name)(None, None, None, None, 640, 480, None, None, None, None) == invalid
        assert "tsdf_integrate_weighted: null argument" in _capi.last_error()
    kinv = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    stand_in = C.create_string_buffer(64)      # never read: every refusal below comes first
    p = C.cast(stand_in, C.c_void_p)
    for fn, tail in ((lib.tsdf_depth_weights_device, (None,)), (lib.tsdf_depth_weights, ())):
        assert fn(4, 4, None, kinv, 0, 1.0, p, *tail) == invalid and "null argument" in _capi.last_error()
        assert fn(4, 4, p, kinv, 0, 1.0, None, *tail) == invalid and "null argument" in _capi.last_error()
        assert fn(0, 4, p, kinv, 0, 1.0, p, *tail) == invalid and "bad image size" in _capi.last_error()
        assert fn(4, 4, p, kinv, 4, 1.0, p, *tail) == invalid and "unknown flag bits" in _capi.last_error()
        for z in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(4, 4, p, kinv, 1, z, p, *tail) == invalid and "z_ref" in _capi.last_error()
    assert stand_in.raw == bytes(64)
    assert lib.tsdf_tracker_set_weighting(None, 1, 1.0) == invalid and "tsdf_tracker_set_weighting" in _capi.last_error()
    assert lib.tsdf_tracker_weighting(None, None, None) == invalid and "tsdf_tracker_weighting" in _capi.last_error()
