"""The C ABI of the reachability group (include/tsdf_amd.h, "reachability"): the header declares the fourteen entry points with the
signatures the group gives, the built library exports them, the Python binding carries the same argument lists and struct layouts (the
88-byte info, the 16-byte rank row), and null arguments are refused before a device is touched (no GPU needed)."""
import ctypes as C
import os
import re

from tests.capi_header import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPUTE_ARGS = ["const tsdf_volume *", "uint64_t", "const float *", "uint32_t", "const tsdf_esdf *", "float", "uint32_t", "uint32_t", "tsdf_reach *"]
EXPECTED = {
    "tsdf_reach_create": ("int", ["tsdf_reach **"]),
    "tsdf_reach_destroy": ("void", ["tsdf_reach *"]),
    "tsdf_volume_compute_reach": ("int", COMPUTE_ARGS),
    "tsdf_volume_compute_reach_device": ("int", COMPUTE_ARGS),
    "tsdf_reach_get_info": ("int", ["const tsdf_reach *", "tsdf_reach_info *"]),
    "tsdf_reach_buffer": ("int", ["const tsdf_reach *", "const uint32_t **"]),
    "tsdf_reach_download": ("int", ["const tsdf_reach *", "uint32_t *"]),
    "tsdf_reach_scratch_bytes": ("int", ["const tsdf_reach *", "uint64_t *"]),
    "tsdf_reach_lookup_device": ("int", ["const tsdf_reach *", "uint64_t", "const float *", "uint32_t *", "void *"]),
    "tsdf_reach_lookup": ("int", ["const tsdf_reach *", "uint64_t", "const float *", "uint32_t *"]),
    "tsdf_reach_paths_device": ("int", ["const tsdf_reach *", "uint64_t", "const float *", "uint32_t", "uint32_t *", "uint32_t *", "void *"]),
    "tsdf_reach_paths": ("int", ["const tsdf_reach *", "uint64_t", "const float *", "uint32_t", "uint32_t *", "uint32_t *"]),
    "tsdf_reach_rank_frontiers_device": ("int", ["tsdf_reach *", "const tsdf_explorer *", "tsdf_reach_cluster *", "void *"]),
    "tsdf_reach_rank_frontiers": ("int", ["tsdf_reach *", "const tsdf_explorer *", "tsdf_reach_cluster *"]),
}


def test_the_header_declares_the_signatures():
    text, decl = declarations(EXPECTED)
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    assert re.search(r"typedef\s+struct\s+tsdf_reach\s+tsdf_reach\s*;", text)
    for name, value in (("TSDF_REACH_THROUGH_UNKNOWN", "1u"), ("TSDF_REACH_UNREACHED", "0xFFFFFFFFu"), ("TSDF_REACH_COST_FACE", "10u"),
                        ("TSDF_REACH_COST_EDGE", "14u"), ("TSDF_REACH_COST_CORNER", "17u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), text), name
    info = re.search(r"typedef\s+struct\s+tsdf_reach_info\s*\{(.*?)\}\s*tsdf_reach_info\s*;", text, flags=re.S)
    assert info and " ".join(info.group(1).split()) == ("uint32_t size[3]; uint32_t connectivity; float voxel_size[3]; float offset[3]; "
                                                        "uint32_t flags; float clearance; uint32_t max_cost; uint32_t max_cost_reached; "
                                                        "uint64_t n_traversable, n_reached, n_seed_voxels; uint64_t rounds;")
    row = re.search(r"typedef\s+struct\s+tsdf_reach_cluster\s*\{(.*?)\}\s*tsdf_reach_cluster\s*;", text, flags=re.S)
    assert row and " ".join(row.group(1).split()) == "uint32_t label, cost, voxel, reserved;"
    # the group stands behind "exploration" and in front of "class objects"
    whole = open(os.path.join(ROOT, "include", "tsdf_amd.h")).read()
    assert whole.index("/* ---- exploration") < whole.index("/* ---- reachability") < whole.index("/* ---- class objects")


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments():
    from tsdf_amd import _capi
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    lib = _capi.lib
    assert _capi.TSDF_REACH_THROUGH_UNKNOWN == 1 and _capi.TSDF_REACH_UNREACHED == 0xFFFFFFFF
    assert (_capi.TSDF_REACH_COST_FACE, _capi.TSDF_REACH_COST_EDGE, _capi.TSDF_REACH_COST_CORNER) == (10, 14, 17)
    for name in EXPECTED:
        assert name in _capi.EXPORTS, name
    assert lib.tsdf_reach_create.argtypes == [C.POINTER(vp)] and lib.tsdf_reach_create.restype == C.c_int
    assert lib.tsdf_reach_destroy.argtypes == [vp] and lib.tsdf_reach_destroy.restype is None
    compute = [vp, u64, vp, u32, vp, f32, u32, u32, vp]
    assert lib.tsdf_volume_compute_reach.argtypes == compute and lib.tsdf_volume_compute_reach_device.argtypes == compute
    assert lib.tsdf_reach_get_info.argtypes == [vp, C.POINTER(_capi.ReachInfo)]
    assert lib.tsdf_reach_buffer.argtypes == [vp, C.POINTER(vp)]
    assert lib.tsdf_reach_download.argtypes == [vp, vp]
    assert lib.tsdf_reach_scratch_bytes.argtypes == [vp, C.POINTER(u64)]
    assert lib.tsdf_reach_lookup_device.argtypes == [vp, u64, vp, vp, vp] and lib.tsdf_reach_lookup.argtypes == [vp, u64, vp, vp]
    assert lib.tsdf_reach_paths_device.argtypes == [vp, u64, vp, u32, vp, vp, vp] and lib.tsdf_reach_paths.argtypes == [vp, u64, vp, u32, vp, vp]
    assert lib.tsdf_reach_rank_frontiers_device.argtypes == [vp, vp, vp, vp] and lib.tsdf_reach_rank_frontiers.argtypes == [vp, vp, vp]
    assert [(n, t) for n, t in _capi.ReachInfo._fields_] == [
        ("size", u32 * 3), ("connectivity", u32), ("voxel_size", f32 * 3), ("offset", f32 * 3), ("flags", u32), ("clearance", f32),
        ("max_cost", u32), ("max_cost_reached", u32), ("n_traversable", u64), ("n_reached", u64), ("n_seed_voxels", u64), ("rounds", u64)]
    assert C.sizeof(_capi.ReachInfo) == 88 and _capi.ReachInfo.flags.offset == 40 and _capi.ReachInfo.n_traversable.offset == 56
    assert _capi.ReachInfo.rounds.offset == 80
    assert [(n, t) for n, t in _capi.ReachCluster._fields_] == [("label", u32), ("cost", u32), ("voxel", u32), ("reserved", u32)]
    assert C.sizeof(_capi.ReachCluster) == 16 and _capi.ReachCluster.voxel.offset == 8
    import tsdf_amd
    from tsdf_amd import api
    assert api.REACH_CLUSTER_DTYPE.itemsize == 16 and api.REACH_CLUSTER_DTYPE.fields["cost"][1] == 4 and api.REACH_CLUSTER_DTYPE.fields["voxel"][1] == 8
    assert tsdf_amd.REACH_UNREACHED == 0xFFFFFFFF and tsdf_amd.TSDF_REACH_THROUGH_UNKNOWN == 1
    assert (tsdf_amd.REACH_COST_FACE, tsdf_amd.REACH_COST_EDGE, tsdf_amd.REACH_COST_CORNER) == (10, 14, 17)
    # null arguments are refused before anything touches a device, and leave a message naming the entry point
    invalid = _capi.TSDF_ERR_INVALID
    calls = {
        "tsdf_reach_create": lambda: lib.tsdf_reach_create(None),
        "tsdf_volume_compute_reach": lambda: lib.tsdf_volume_compute_reach(None, 0, None, 26, None, 0.0, 0, 0, None),
        "tsdf_volume_compute_reach_device": lambda: lib.tsdf_volume_compute_reach_device(None, 0, None, 26, None, 0.0, 0, 0, None),
        "tsdf_reach_get_info": lambda: lib.tsdf_reach_get_info(None, None),
        "tsdf_reach_buffer": lambda: lib.tsdf_reach_buffer(None, None),
        "tsdf_reach_download": lambda: lib.tsdf_reach_download(None, None),
        "tsdf_reach_scratch_bytes": lambda: lib.tsdf_reach_scratch_bytes(None, None),
        "tsdf_reach_lookup_device": lambda: lib.tsdf_reach_lookup_device(None, 0, None, None, None),
        "tsdf_reach_lookup": lambda: lib.tsdf_reach_lookup(None, 0, None, None),
        "tsdf_reach_paths_device": lambda: lib.tsdf_reach_paths_device(None, 0, None, 1, None, None, None),
        "tsdf_reach_paths": lambda: lib.tsdf_reach_paths(None, 0, None, 1, None, None),
        "tsdf_reach_rank_frontiers_device": lambda: lib.tsdf_reach_rank_frontiers_device(None, None, None, None),
        "tsdf_reach_rank_frontiers": lambda: lib.tsdf_reach_rank_frontiers(None, None, None),
    }
    for name, call in calls.items():
        assert call() == invalid, name
        message = _capi.last_error()
        assert re.search(r"\b%s\b" % name, message), (name, message)
    lib.tsdf_reach_destroy(None)   # a null handle is ignored
    assert callable(tsdf_amd.TSDFVolume.reach)
    for name in ("costs", "device_buffer", "lookup", "lookup_device", "paths", "rank", "info", "scratch_bytes"):
        assert hasattr(tsdf_amd.Reach, name), name
