"""The C ABI of the sparse snapshot (include/tsdf_amd.h, "sparse snapshot"): the header declares the ten entry points with the
signatures the issue gives, the built library exports them, the Python binding carries the same argument lists and the 80-byte info
struct, null arguments are refused before a device is touched, and tsdf_snapshot_upload checks its arrays on the host (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

from tests.capi_header import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {
    "tsdf_snapshot_create": ("int", ["tsdf_snapshot **"]),
    "tsdf_snapshot_destroy": ("void", ["tsdf_snapshot *"]),
    "tsdf_volume_snapshot": ("int", ["const tsdf_volume *", "uint32_t", "tsdf_snapshot *"]),
    "tsdf_volume_restore": ("int", ["tsdf_volume *", "const tsdf_snapshot *"]),
    "tsdf_snapshot_get_info": ("int", ["const tsdf_snapshot *", "tsdf_snapshot_info *"]),
    "tsdf_snapshot_buffers": ("int", ["const tsdf_snapshot *", "const uint32_t **", "const float **", "const void **", "const uint32_t **"]),
    "tsdf_snapshot_download": ("int", ["const tsdf_snapshot *", "uint32_t *", "float *", "void *", "uint32_t *"]),
    "tsdf_snapshot_upload": ("int", ["tsdf_snapshot *", "const tsdf_snapshot_info *", "const uint32_t *", "const float *", "const void *",
                                     "const uint32_t *"]),
    "tsdf_snapshot_scratch_bytes": ("int", ["const tsdf_snapshot *", "uint64_t *"]),
}
INFO_FIELDS = ("uint32_t size[3]; uint32_t bricks[3]; uint32_t flags; uint32_t weight_bits; uint32_t weight_bound; float fill_distance; "
               "float voxel_size[3]; float offset[3]; uint64_t n_bricks; uint64_t bytes;")


def test_the_header_declares_the_signatures():
    text, decl = declarations(EXPECTED)
    for name, sig in EXPECTED.items():
        assert name in decl, name
        assert decl[name] == sig, (name, decl[name])
    assert re.search(r"typedef\s+struct\s+tsdf_snapshot\s+tsdf_snapshot\s*;", text)
    assert re.search(r"#define\s+TSDF_SNAPSHOT_BRICK\s+8\b", text)
    assert re.search(r"#define\s+TSDF_SNAPSHOT_COLOUR\s+1u\b", text)
    info = re.search(r"typedef\s+struct\s+tsdf_snapshot_info\s*\{(.*?)\}\s*tsdf_snapshot_info\s*;", text, flags=re.S)
    assert info and " ".join(info.group(1).split()) == INFO_FIELDS


def test_the_library_exports_them():
    lib = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so"))
    for name in EXPECTED:
        assert hasattr(lib, name), name
    host = C.CDLL(os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_host.so"))
    assert hasattr(host, "tsdf_host_read_sparse_info")


def test_the_binding_carries_the_same_arguments():
    from tsdf_amd import _capi
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    lib = _capi.lib
    assert _capi.TSDF_SNAPSHOT_BRICK == 8 and _capi.TSDF_SNAPSHOT_COLOUR == 1
    for name in EXPECTED:
        assert name in _capi.EXPORTS, name
    info_p = C.POINTER(_capi.SnapshotInfo)
    assert lib.tsdf_snapshot_create.argtypes == [C.POINTER(vp)] and lib.tsdf_snapshot_create.restype == C.c_int
    assert lib.tsdf_snapshot_destroy.argtypes == [vp] and lib.tsdf_snapshot_destroy.restype is None
    assert lib.tsdf_volume_snapshot.argtypes == [vp, u32, vp]
    assert lib.tsdf_volume_restore.argtypes == [vp, vp]
    assert lib.tsdf_snapshot_get_info.argtypes == [vp, info_p]
    assert lib.tsdf_snapshot_buffers.argtypes == [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    assert lib.tsdf_snapshot_download.argtypes == [vp, vp, vp, vp, vp]
    assert lib.tsdf_snapshot_upload.argtypes == [vp, info_p, vp, vp, vp, vp]
    assert lib.tsdf_snapshot_scratch_bytes.argtypes == [vp, C.POINTER(u64)]
    assert [(n, t) for n, t in _capi.SnapshotInfo._fields_] == [
        ("size", u32 * 3), ("bricks", u32 * 3), ("flags", u32), ("weight_bits", u32), ("weight_bound", u32), ("fill_distance", f32),
        ("voxel_size", f32 * 3), ("offset", f32 * 3), ("n_bricks", u64), ("bytes", u64)]
    assert C.sizeof(_capi.SnapshotInfo) == 80 and _capi.SnapshotInfo.n_bricks.offset == 64
    import tsdf_amd
    assert callable(tsdf_amd.TSDFVolume.snapshot) and callable(tsdf_amd.TSDFVolume.restore)
    assert callable(tsdf_amd.TSDFVolume.save_sparse) and callable(tsdf_amd.TSDFVolume.load_sparse)
    for name in ("info", "n_bricks", "bricks", "distances", "weights", "colours", "device_buffers", "scratch_bytes", "from_arrays", "save", "load"):
        assert hasattr(tsdf_amd.Snapshot, name), name


def test_null_arguments_are_refused_before_a_device_is_touched():
    from tsdf_amd import _capi
    lib, invalid = _capi.lib, _capi.TSDF_ERR_INVALID
    assert lib.tsdf_snapshot_create(None) == invalid
    assert "tsdf_snapshot_create" in _capi.last_error()
    assert lib.tsdf_volume_snapshot(None, 0, None) == invalid
    assert "tsdf_volume_snapshot" in _capi.last_error()
    assert lib.tsdf_volume_restore(None, None) == invalid
    assert "tsdf_volume_restore" in _capi.last_error()
    assert lib.tsdf_snapshot_get_info(None, None) == invalid
    assert "tsdf_snapshot_get_info" in _capi.last_error()
    assert lib.tsdf_snapshot_buffers(None, None, None, None, None) == invalid
    assert "tsdf_snapshot_buffers" in _capi.last_error()
    assert lib.tsdf_snapshot_download(None, None, None, None, None) == invalid
    assert "tsdf_snapshot_download" in _capi.last_error()
    assert lib.tsdf_snapshot_upload(None, None, None, None, None, None) == invalid
    assert "tsdf_snapshot_upload" in _capi.last_error()
    assert lib.tsdf_snapshot_scratch_bytes(None, None) == invalid
    assert "tsdf_snapshot_scratch_bytes" in _capi.last_error()
    lib.tsdf_snapshot_destroy(None)   # a null handle is ignored


def test_upload_checks_its_arrays_on_the_host():
    """Every refusal below returns before the handle is looked at or a device is touched: the handle is a stand-in that is never read."""
    from tsdf_amd import _capi
    lib, invalid = _capi.lib, _capi.TSDF_ERR_INVALID
    stand_in = C.create_string_buffer(4096)
    handle = C.cast(stand_in, C.c_void_p)

    def upload(size=(9, 8, 8), bits=8, ids=(0, 1), flags=0, n=None):
        info = _capi.SnapshotInfo()
        info.size[:] = size
        info.flags, info.weight_bits, info.fill_distance = flags, bits, 10.0
        ids = np.array(ids, np.uint32)
        info.n_bricks = len(ids) if n is None else n
        d = np.zeros(512 * max(len(ids), 1), np.float32)
        w = np.zeros(512 * max(len(ids), 1), np.uint32)   # (large enough for every element type)
        rc = lib.tsdf_snapshot_upload(handle, C.byref(info), ids.ctypes.data, d.ctypes.data, w.ctypes.data, None)
        return rc, _capi.last_error()

    for kw, word in [(dict(ids=(1, 0)), "ascending"), (dict(ids=(1, 1)), "ascending"), (dict(ids=(0, 2)), "below the brick count"),
                     (dict(bits=12), "weight_bits"), (dict(size=(0, 8, 8)), "size"), (dict(size=(9, 8, 65536)), "size"),
                     (dict(n=3), "n_bricks"), (dict(flags=2), "flags"), (dict(flags=1), "null")]:
        rc, msg = upload(**kw)
        assert rc == invalid and "tsdf_snapshot_upload" in msg and word in msg, (kw, rc, msg)
    assert stand_in.raw == bytes(4096)

    # the Python surface makes the same checks before it creates a handle
    import pytest
    import tsdf_amd
    z = np.zeros((2, 512), np.float32)
    for kw, ids in [(dict(size=(9, 8, 8)), (1, 0)), (dict(size=(9, 8, 8)), (0, 2)), (dict(size=(0, 8, 8)), (0, 1))]:
        with pytest.raises(ValueError):
            tsdf_amd.Snapshot.from_arrays(kw["size"], ids, z, z.astype(np.uint8))
    with pytest.raises(ValueError):
        tsdf_amd.Snapshot.from_arrays((9, 8, 8), (0, 1), z, z.astype(np.int32))
