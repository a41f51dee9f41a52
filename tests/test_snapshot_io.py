"""The .tsdfs file of a sparse snapshot.  On the GPU: save_sparse -> load_sparse gives the state, the header fields and
the colour counts back, in every weight storage.  Without one, through the Python reader (tsdf_amd.api.read_sparse_file) and the host
library's (tsdf_host_read_sparse_info): a good file reads back as written, and truncated files, a wrong magic, a wrong brick size,
n_bricks larger than the grid allows, unsorted or out-of-range ids and a bad weight_bits are each refused -- before anything as large
as the header claims is allocated."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import tsdf_amd
from tests import snapshot_cases as K
from tests import snapshot_ref as R
from tsdf_amd import _capi, api

F32, U32 = np.float32, np.uint32
HEADER = {"physical_size": (90.0, 100.0, 72.0), "offset": (1.0, -2.0, 3.5), "truncation_distance": 20.0, "max_weight": 7.0,
          "global_translation": (4.0, 5.0, 6.0), "global_rotation": (0.25, 0.5, 0.75)}
SIZE = (9, 8, 8)
N_HEAD = 8 + 68 + 32


def host_read(path):
    info = _capi.HostSparseInfo()
    msg = C.create_string_buffer(512)
    rc = _capi.host.tsdf_host_read_sparse_info(str(path).encode(), C.byref(info), msg, len(msg))
    return rc, info, msg.value.decode()


def good_file(path, bits=8, colour=True):
    D, Wt, Cl = K.random_case(SIZE, bits, colour, F32(20.0))
    D[0], D[-1] = -1.0, -2.0       # both bricks live
    ids, d, w, c = R.take(D, Wt, SIZE, F32(20.0), bits, Cl)
    assert list(ids) == [0, 1]
    api.write_sparse_file(str(path), SIZE, HEADER, int(w.max()) if bits != 32 else 0, 20.0, ids, d, w, c)
    return ids, d, w, c


@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("colour", [False, True])
def test_a_good_file_reads_back_as_written(tmp_path, bits, colour):
    path = tmp_path / "good.tsdfs"
    ids, d, w, c = good_file(path, bits, colour)
    assert os.path.getsize(path) == N_HEAD + 2 * (4 + 512 * (4 + bits // 8 + (4 if colour else 0)))
    header, info, gi, gd, gw, gc = api.read_sparse_file(str(path))
    assert header == HEADER
    assert tuple(info.size) == SIZE and info.flags == int(colour) and info.weight_bits == bits and info.n_bricks == 2
    assert F32(info.fill_distance) == F32(20.0) and tuple(info.offset) == HEADER["offset"]
    assert np.array_equal(np.array(info.voxel_size, F32), np.array([10.0, 12.5, 9.0], F32))
    assert gi.tobytes() == ids.tobytes() and gd.tobytes() == d.tobytes() and gw.tobytes() == w.tobytes() and gw.dtype == w.dtype
    assert (gc is None and c is None) or gc.tobytes() == c.tobytes()
    rc, hi, msg = host_read(path)
    assert rc == 0 and msg == "", msg
    assert tuple(hi.size) == SIZE and tuple(hi.physical_size) == HEADER["physical_size"] and tuple(hi.offset) == HEADER["offset"]
    assert (hi.truncation_distance, hi.max_weight) == (20.0, 7.0)
    assert tuple(hi.global_translation) == HEADER["global_translation"] and tuple(hi.global_rotation) == HEADER["global_rotation"]
    assert (hi.brick, hi.flags, hi.weight_bits, hi.fill_distance, hi.n_bricks) == (8, int(colour), bits, 20.0, 2)
    assert hi.weight_bound == (int(w.max()) if bits != 32 else 0)


def patched(path, out, offset, fmt, value, truncate=None):
    raw = bytearray(open(path, "rb").read())
    if fmt:
        struct.pack_into(fmt, raw, offset, value)
    open(out, "wb").write(bytes(raw[:truncate] if truncate is not None else raw))
    return str(out)


def refused_by_both(path, word):
    with pytest.raises(ValueError, match=word):
        api.read_sparse_file(path)
    with pytest.raises(ValueError):
        tsdf_amd.Snapshot.load(path)       # (refused by the reader, before a handle is made)
    rc, _, msg = host_read(path)
    assert rc == -1 and word in msg, (rc, msg)


def test_bad_files_are_refused_without_a_large_allocation(tmp_path):
    good = tmp_path / "good.tsdfs"
    good_file(good)
    length = os.path.getsize(good)
    bad = lambda name: tmp_path / name
    # field offsets: magic 0, size 8, brick 76, flags 80, weight_bits 84, weight_bound 88, fill 92, zero 96, n_bricks 100, ids 108
    refused_by_both(patched(good, bad("magic"), 0, "<8s", b"TSDFSPR2"), "magic")
    refused_by_both(patched(good, bad("brick"), 76, "<I", 4), "brick")
    refused_by_both(patched(good, bad("flags"), 80, "<I", 3), "flags")
    refused_by_both(patched(good, bad("bits"), 84, "<I", 12), "weight_bits")
    refused_by_both(patched(good, bad("size0"), 8, "<I", 0), "size")
    refused_by_both(patched(good, bad("size65536"), 16, "<I", 65536), "size")
    # truncated: in the header, in the ids, by one byte at the end; and one byte too many
    for cut in (5, 50, N_HEAD - 1, N_HEAD + 4, length - 1):
        refused_by_both(patched(good, bad("cut%d" % cut), 0, None, None, truncate=cut), "bytes")
    open(bad("long"), "wb").write(open(good, "rb").read() + b"\0")
    refused_by_both(str(bad("long")), "bytes")
    # n_bricks larger than the grid allows: 3 of 2; and a count that would take 2^63 bytes is refused by the count, not by an allocation
    refused_by_both(patched(good, bad("three"), 100, "<Q", 3), "n_bricks")
    refused_by_both(patched(good, bad("huge"), 100, "<Q", 2 ** 62), "n_bricks")
    # a grid that allows the count, but not the file's length: 65535^3 voxels and 2^30 bricks claimed by a 13 KB file
    huge_grid = patched(good, bad("grid"), 8, "<I", 65535)
    huge_grid = patched(huge_grid, bad("grid2"), 12, "<I", 65535)
    huge_grid = patched(huge_grid, bad("grid3"), 16, "<I", 65535)
    refused_by_both(patched(huge_grid, bad("grid4"), 100, "<Q", 2 ** 30), "bytes")
    # ids: descending, equal, out of range
    refused_by_both(patched(patched(good, bad("d1"), 108, "<I", 1), bad("d2"), 112, "<I", 0), "ascending")
    refused_by_both(patched(good, bad("equal"), 108, "<I", 1), "ascending")
    refused_by_both(patched(good, bad("range"), 112, "<I", 2), "brick count")
    rc, _, msg = host_read(tmp_path / "no such file")
    assert rc == -1 and "open" in msg
    assert _capi.host.tsdf_host_read_sparse_info(None, None, None, 0) == -1     # null arguments, no message asked for


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [8, 16, 32])
def test_save_sparse_then_load_sparse_gives_the_volume_back(tmp_path, bits):
    size = (40, 33, 21)
    D, Wt, Cl = K.random_case(size, bits, True)
    gv = tsdf_amd.TSDFVolume(size, K.physical(size))
    gv.offset(*K.OFFSET)
    gv.set_global_transform((0.1, 0.2, 0.3), (7.0, 8.0, 9.0))
    gv.enable_colour()
    gv.set_distance_data(D)
    gv.set_weight_data(Wt)
    gv.set_colour_data(Cl)
    if gv.weight_storage()[0] != bits:
        gv.set_weight_storage(bits)
    assert (Cl >> 24).max() > 1                       # colour counts the .tsdf colour block would drop
    path = str(tmp_path / "volume.tsdfs")
    gv.save_sparse(path)
    ids, d, w, c = R.take(D, Wt, size, K.FILL, bits, Cl)
    assert os.path.getsize(path) == N_HEAD + len(ids) * (4 + 512 * (4 + bits // 8 + 4))
    header, info, gi, gd, gw, gc = api.read_sparse_file(path)
    assert gi.tobytes() == ids.tobytes() and gd.tobytes() == d.tobytes() and gw.tobytes() == w.tobytes() and gc.tobytes() == c.tobytes()
    assert host_read(path)[0] == 0
    back = tsdf_amd.TSDFVolume.load_sparse(path)
    a, b = gv.info(), back.info()
    for field in ("size", "physical_size", "voxel_size", "offset", "global_translation", "global_rotation"):
        assert tuple(getattr(a, field)) == tuple(getattr(b, field)), field
    assert (a.truncation_distance, a.max_weight) == (b.truncation_distance, b.max_weight)
    assert back.get_distance_data().tobytes() == D.tobytes()
    assert back.get_weight_data().tobytes() == Wt.tobytes()
    assert back.get_colour_data().tobytes() == Cl.tobytes()
    assert back.weight_storage() == (bits, False) and back.colour_enabled()
    # Snapshot.save / Snapshot.load by themselves: the same file
    snap = gv.snapshot()
    snap.save(str(tmp_path / "again.tsdfs"))
    assert open(str(tmp_path / "again.tsdfs"), "rb").read() == open(path, "rb").read()
    loaded = tsdf_amd.Snapshot.load(path)
    assert loaded.header == header and loaded.n_bricks == len(ids)
    for o in (snap, loaded, gv, back):
        o.close()
