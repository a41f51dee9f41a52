"""The C ABI of the exploration queries (include/tsdf_amd.h, "exploration"): the header declares the twelve entry points with the
signatures the group gives, the built library exports them, the Python binding carries the same argument lists and struct layouts (the
56-byte cluster row), and null arguments are refused before a device is touched (no GPU needed)."""
import ctypes as C
import os
import re

from tests.capi_header import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAIN_ARGS = ["const tsdf_volume *", "tsdf_explorer *", "uint64_t", "const float *", "const float *", "const float *", "uint32_t", "uint32_t *",
             "uint32_t *", "uint8_t *", "uint64_t *"]
EXPECTED = {
    "tsdf_explorer_create": ("int", ["tsdf_explorer **"]),
    "tsdf_explorer_destroy": ("void", ["tsdf_explorer *"]),
    "tsdf_volume_find_frontiers": ("int", ["const tsdf_volume *", "uint32_t", "tsdf_explorer *"]),
    "tsdf_explorer_get_info": ("int", ["const tsdf_explorer *", "tsdf_explorer_info *"]),
    "tsdf_explorer_frontier_buffers": ("int", ["const tsdf_explorer *", "const uint32_t **", "const uint64_t **", "const uint32_t **"]),
    "tsdf_explorer_frontier_download": ("int", ["const tsdf_explorer *", "uint32_t *"]),
    "tsdf_explorer_scratch_bytes": ("int", ["const tsdf_explorer *", "uint64_t *"]),
    "tsdf_explorer_cluster_frontiers": ("int", ["tsdf_explorer *", "uint32_t", "uint32_t", "void *"]),
    "tsdf_explorer_cluster_buffers": ("int", ["const tsdf_explorer *", "const uint32_t **", "const tsdf_frontier_cluster **"]),
    "tsdf_explorer_cluster_download": ("int", ["const tsdf_explorer *", "uint32_t *", "tsdf_frontier_cluster *"]),
    "tsdf_volume_view_gain_device": ("int", GAIN_ARGS),
    "tsdf_volume_view_gain": ("int", GAIN_ARGS),
}


def test_the_header_declares_the_signatures():
    text, decl = declarations(EXPECTED)
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    assert re.search(r"typedef\s+struct\s+tsdf_explorer\s+tsdf_explorer\s*;", text)
    assert re.search(r"#define\s+TSDF_GAIN_KEEP_MASK\s+1u\b", text)
    info = re.search(r"typedef\s+struct\s+tsdf_explorer_info\s*\{(.*?)\}\s*tsdf_explorer_info\s*;", text, flags=re.S)
    assert info and " ".join(info.group(1).split()) == ("uint32_t size[3]; uint32_t connectivity; float voxel_size[3]; float offset[3]; "
                                                        "uint64_t n_unknown, n_free, n_occupied, n_frontiers; "
                                                        "uint64_t n_clusters, n_listed_clusters;")
    row = re.search(r"typedef\s+struct\s+tsdf_frontier_cluster\s*\{(.*?)\}\s*tsdf_frontier_cluster\s*;", text, flags=re.S)
    assert row and " ".join(row.group(1).split()) == "uint32_t label, size; uint32_t lo[3], hi[3]; uint64_t sum[3];"


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name


def test_the_binding_carries_the_same_arguments():
    from tsdf_amd import _capi
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    lib = _capi.lib
    assert _capi.TSDF_GAIN_KEEP_MASK == 1
    for name in EXPECTED:
        assert name in _capi.EXPORTS, name
    assert lib.tsdf_explorer_create.argtypes == [C.POINTER(vp)] and lib.tsdf_explorer_create.restype == C.c_int
    assert lib.tsdf_explorer_destroy.argtypes == [vp] and lib.tsdf_explorer_destroy.restype is None
    assert lib.tsdf_volume_find_frontiers.argtypes == [vp, u32, vp]
    assert lib.tsdf_explorer_get_info.argtypes == [vp, C.POINTER(_capi.ExplorerInfo)]
    assert lib.tsdf_explorer_frontier_buffers.argtypes == [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    assert lib.tsdf_explorer_frontier_download.argtypes == [vp, vp]
    assert lib.tsdf_explorer_scratch_bytes.argtypes == [vp, C.POINTER(u64)]
    assert lib.tsdf_explorer_cluster_frontiers.argtypes == [vp, u32, u32, vp]
    assert lib.tsdf_explorer_cluster_buffers.argtypes == [vp, C.POINTER(vp), C.POINTER(vp)]
    assert lib.tsdf_explorer_cluster_download.argtypes == [vp, vp, vp]
    gain = [vp, vp, u64, vp, vp, vp, u32, vp, vp, vp, C.POINTER(u64)]
    assert lib.tsdf_volume_view_gain_device.argtypes == gain and lib.tsdf_volume_view_gain.argtypes == gain
    assert [(n, t) for n, t in _capi.ExplorerInfo._fields_] == [
        ("size", u32 * 3), ("connectivity", u32), ("voxel_size", f32 * 3), ("offset", f32 * 3), ("n_unknown", u64), ("n_free", u64),
        ("n_occupied", u64), ("n_frontiers", u64), ("n_clusters", u64), ("n_listed_clusters", u64)]
    assert C.sizeof(_capi.ExplorerInfo) == 88 and _capi.ExplorerInfo.n_unknown.offset == 40
    assert [(n, t) for n, t in _capi.FrontierCluster._fields_] == [("label", u32), ("size", u32), ("lo", u32 * 3), ("hi", u32 * 3),
                                                                  ("sum", u64 * 3)]
    assert C.sizeof(_capi.FrontierCluster) == 56 and _capi.FrontierCluster.sum.offset == 32
    import tsdf_amd
    from tsdf_amd import api
    assert api.CLUSTER_DTYPE.itemsize == 56 and api.CLUSTER_DTYPE.fields["sum"][1] == 32 and api.CLUSTER_DTYPE.fields["lo"][1] == 8
    # null arguments are refused before anything touches a device, and leave a message naming the entry point
    invalid = _capi.TSDF_ERR_INVALID
    g = u64(0)
    calls = {
        "tsdf_explorer_create": lambda: lib.tsdf_explorer_create(None),
        "tsdf_volume_find_frontiers": lambda: lib.tsdf_volume_find_frontiers(None, 0, None),
        "tsdf_explorer_get_info": lambda: lib.tsdf_explorer_get_info(None, None),
        "tsdf_explorer_frontier_buffers": lambda: lib.tsdf_explorer_frontier_buffers(None, None, None, None),
        "tsdf_explorer_frontier_download": lambda: lib.tsdf_explorer_frontier_download(None, None),
        "tsdf_explorer_scratch_bytes": lambda: lib.tsdf_explorer_scratch_bytes(None, None),
        "tsdf_explorer_cluster_frontiers": lambda: lib.tsdf_explorer_cluster_frontiers(None, 26, 1, None),
        "tsdf_explorer_cluster_buffers": lambda: lib.tsdf_explorer_cluster_buffers(None, None, None),
        "tsdf_explorer_cluster_download": lambda: lib.tsdf_explorer_cluster_download(None, None, None),
        "tsdf_volume_view_gain_device": lambda: lib.tsdf_volume_view_gain_device(None, None, 0, None, None, None, 0, None, None, None, C.byref(g)),
        "tsdf_volume_view_gain": lambda: lib.tsdf_volume_view_gain(None, None, 0, None, None, None, 0, None, None, None, C.byref(g)),
    }
    for name, call in calls.items():
        assert call() == invalid, name
        assert name in _capi.last_error(), (name, _capi.last_error())
    lib.tsdf_explorer_destroy(None)   # a null handle is ignored
    assert callable(tsdf_amd.TSDFVolume.find_frontiers) and callable(tsdf_amd.TSDFVolume.view_gain)
    assert callable(tsdf_amd.TSDFVolume.view_gain_device) and callable(tsdf_amd.pixel_rays)
    for name in ("voxels", "coordinates", "points", "cluster", "labels", "clusters", "centroids", "info", "device_buffers", "scratch_bytes"):
        assert hasattr(tsdf_amd.Explorer, name), name
