"""The C ABI of class fusion (include/tsdf_amd.h, "class fusion"): the header declares the twelve entry points and TSDF_CLASS_VOID, the
built library exports them, the Python binding carries the same argument lists, the header states the rule, and null or bad arguments
are refused before a device is touched (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tsdf_amd.h")
MATS = ["const float [16]", "const float [16]", "const float [9]", "const float [9]"]
INTEGRATE = ["tsdf_volume *", "const uint16_t *", "const uint8_t *", "const uint16_t *", "const uint8_t *", "uint32_t", "uint32_t"] + MATS
CAST = ["const tsdf_volume *", "uint32_t", "uint32_t", "const float [16]", "const float [9]", "float *", "float *", "uint16_t *", "uint16_t *"]
EXPECTED = {
    "tsdf_volume_enable_classes": ("int", ["tsdf_volume *", "int"]),
    "tsdf_volume_classes_enabled": ("int", ["const tsdf_volume *", "int *"]),
    "tsdf_volume_classes": ("int", ["const tsdf_volume *", "uint32_t **"]),
    "tsdf_volume_get_class_data": ("int", ["const tsdf_volume *", "uint32_t *"]),
    "tsdf_volume_set_class_data": ("int", ["tsdf_volume *", "const uint32_t *"]),
    "tsdf_integrate_classes": ("int", INTEGRATE),
    "tsdf_integrate_classes_device": ("int", INTEGRATE),
    "tsdf_volume_sample_classes_device": ("int", ["const tsdf_volume *", "uint64_t", "const float *", "uint16_t *", "uint16_t *", "void *"]),
    "tsdf_raycast_classes": ("int", CAST),
    "tsdf_raycast_classes_device": ("int", CAST),
    "tsdf_volume_class_counts": ("int", ["const tsdf_volume *", "uint32_t", "uint32_t", "uint64_t *"]),
    "tsdf_volume_class_counts_device": ("int", ["const tsdf_volume *", "uint32_t", "uint32_t", "uint64_t *", "void *"]),
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
    assert re.search(r"#define\s+TSDF_CLASS_VOID\s+0xFFFFu\b", text)


def test_the_library_exports_them_and_the_binding_carries_the_same_arguments():
    lib_path = os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    from tsdf_amd import _capi, api, synth
    vp, u32, u64, i32, fp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_float)
    for name in EXPECTED:
        assert name in exported, name + " is not exported by libtsdf_hip.so"
        assert name in _capi.EXPORTS, name
        assert getattr(_capi.lib, name).restype == C.c_int
    lib = _capi.lib
    assert lib.tsdf_volume_enable_classes.argtypes == [vp, i32]
    assert lib.tsdf_volume_classes_enabled.argtypes == [vp, C.POINTER(i32)]
    assert lib.tsdf_volume_classes.argtypes == [vp, C.POINTER(vp)]
    assert lib.tsdf_volume_get_class_data.argtypes == [vp, vp] == lib.tsdf_volume_set_class_data.argtypes
    for name in ("tsdf_integrate_classes", "tsdf_integrate_classes_device"):
        assert getattr(lib, name).argtypes == [vp, vp, vp, vp, vp, u32, u32, fp, fp, fp, fp]
    assert lib.tsdf_volume_sample_classes_device.argtypes == [vp, u64, vp, vp, vp, vp]
    for name in ("tsdf_raycast_classes", "tsdf_raycast_classes_device"):
        assert getattr(lib, name).argtypes == [vp, u32, u32, fp, fp, vp, vp, vp, vp]
    assert lib.tsdf_volume_class_counts.argtypes == [vp, u32, u32, vp]
    assert lib.tsdf_volume_class_counts_device.argtypes == [vp, u32, u32, vp, vp]
    assert _capi.TSDF_CLASS_VOID == api.CLASS_VOID == synth.CLASS_VOID == 0xFFFF
    for name in ("enable_classes", "classes_enabled", "class_data", "get_class_data", "set_class_data", "integrate_classes",
                 "integrate_classes_device", "sample_classes", "sample_classes_device", "class_counts", "extract_classed_surface"):
        assert callable(getattr(api.TSDFVolume, name)), name
    assert callable(api.Mesh.sample_classes)
    assert callable(api.GPURaycaster.raycast_classes) and callable(api.GPURaycaster.raycast_classes_device)
    import tsdf_amd
    assert tsdf_amd.CLASS_VOID == 0xFFFF


def test_the_header_states_the_rule():
    text = open(HEADER).read()
    flat = " ".join(text[text.index("---- class fusion"):text.index("---- field queries")].split())
    for line in ("n == 0 -> (k, s)", "c == k -> (k, min(n + s, 65535))", "c != k, n > s -> (c, n - s)", "c != k, n == s -> 0x00000000",
                 "c != k, n < s -> (k, s - n)", "A word with votes == 0 is always 0x00000000", "-trunc <= sdf <= +trunc",
                 "gives (TSDF_CLASS_VOID, 0) for a NaN coordinate", "index or a word with votes == 0",
                 "votes >= max(min_votes, 1)", "counts is overwritten, not accumulated", "tsdf_deintegrate* (a vote is not invertible)",
                 "neither read nor write class words"):
        assert line in flat, line


def test_bad_arguments_are_refused_without_a_device():
    from tsdf_amd import _capi
    lib, invalid = _capi.lib, _capi.TSDF_ERR_INVALID
    stand_in = C.create_string_buffer(64)      # never read or written: every refusal below comes first
    p = C.cast(stand_in, C.c_void_p)
    calls = {
        "tsdf_volume_enable_classes": (None, 1),
        "tsdf_volume_classes_enabled": (None, None),
        "tsdf_volume_classes": (None, C.cast(stand_in, C.POINTER(C.c_void_p))),
        "tsdf_volume_get_class_data": (None, p),
        "tsdf_volume_set_class_data": (None, p),
        "tsdf_integrate_classes": (None, p, None, p, None, 4, 4, None, None, None, None),
        "tsdf_integrate_classes_device": (None, p, None, p, None, 4, 4, None, None, None, None),
        "tsdf_volume_sample_classes_device": (None, 4, p, p, p, None),
        "tsdf_raycast_classes": (None, 4, 4, None, None, p, p, p, p),
        "tsdf_raycast_classes_device": (None, 4, 4, None, None, p, p, p, p),
        "tsdf_volume_class_counts": (None, 4, 1, p),
        "tsdf_volume_class_counts_device": (None, 4, 1, p, None),
    }
    names = {"tsdf_integrate_classes_device": "tsdf_integrate_classes", "tsdf_volume_sample_classes_device": "tsdf_volume_sample_classes",
             "tsdf_raycast_classes_device": "tsdf_raycast_classes", "tsdf_volume_class_counts_device": "tsdf_volume_class_counts"}
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == invalid, name
        assert names.get(name, name) + ": null" in _capi.last_error(), (name, _capi.last_error())
    assert stand_in.raw == bytes(64)
