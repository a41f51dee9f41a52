"""GPU: sparse snapshots (tsdf_volume_snapshot / tsdf_volume_restore; include/tsdf_amd.h, "sparse snapshot") against the CPU reference
tests/snapshot_ref.py, bit for bit and without a tolerance: random fields with whole blocks left cleared on the grids of
tests/snapshot_cases.py in all three weight storages, with and without colour; bricks that are live by one voxel only, for every
reason a voxel can be live; values that would fall into another brick if a row were read past its end; the empty and the full volume;
restore into a fresh volume, into the same volume after more writes, into one holding other data and through download -> from_arrays;
a fused volume that takes a detour through a snapshot against a twin that does not; the storage rules; a warm handle; volumes on other
streams; the refusals."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import snapshot_cases as K
from tests import snapshot_ref as R
from tests.helpers import H, W
from tsdf_amd import _capi, synth

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
lib = _capi.lib


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))
        raise AssertionError("%s: %d bytes differ, first at byte %d" % (what, bad.size, bad[0]))


def make_volume(size, D=None, Wt=None, Cl=None, bits=None, colour=False):
    gv = tsdf_amd.TSDFVolume(size, K.physical(size))
    gv.offset(*K.OFFSET)
    assert np.array_equal(gv.voxel_size(), K.VS) and F32(gv.truncation_distance()) == K.FILL
    if colour or Cl is not None:
        gv.enable_colour()
    if D is not None:
        gv.set_distance_data(D)
        gv.set_weight_data(Wt)
    if Cl is not None:
        gv.set_colour_data(Cl)
    if bits is not None and gv.weight_storage()[0] != bits:
        gv.set_weight_storage(bits)
    return gv


def state(gv):
    return gv.get_distance_data(), gv.get_weight_data(), gv.get_colour_data() if gv.colour_enabled() else None, gv.weight_storage()


def assert_state(gv, D, Wt, Cl, storage, what):
    d, w, c, s = state(gv)
    same_bits(d, np.ascontiguousarray(D, F32).reshape(-1), what + ": distances")
    same_bits(w, np.ascontiguousarray(Wt, F32).reshape(-1), what + ": weights")
    if Cl is None:
        assert c is None or not c.any(), what + ": colours"
    else:
        same_bits(c, np.ascontiguousarray(Cl, U32).reshape(-1), what + ": colours")
    assert s == storage, (what, s, storage)


def assert_snapshot(snap, D, Wt, Cl, size, bits, what):
    """The handle against the reference: ids, arrays and info; returns the reference's brick count."""
    ids, d, w, c = R.take(D, Wt, size, K.FILL, bits, Cl)
    gi, gd, gw, gc = snap.download()
    same_bits(gi, ids, what + ": ids")
    same_bits(gd, d, what + ": brick distances")
    same_bits(gw, w, what + ": brick weights")
    assert (gc is None) == (c is None), what
    if c is not None:
        same_bits(gc, c, what + ": brick colours")
    i = snap.info
    assert tuple(i.size) == tuple(size) and tuple(i.bricks) == R.bricks_per_axis(size), what
    assert i.flags == (1 if Cl is not None else 0) and i.weight_bits == bits, what
    top = int(np.max(Wt)) if bits != 32 else 0
    assert (i.weight_bound == 0) if bits == 32 else (top <= i.weight_bound <= 65535), (what, i.weight_bound, top)
    assert F32(i.fill_distance) == K.FILL and np.array_equal(np.array(i.voxel_size, F32), K.VS) and tuple(i.offset) == K.OFFSET, what
    assert i.n_bricks == len(ids) == snap.n_bricks, what
    assert i.bytes == len(ids) * (4 + 512 * (4 + bits // 8 + (4 if Cl is not None else 0))), what
    return len(ids)


@pytest.mark.parametrize("size", K.GRIDS)
@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("colour", [False, True])
def test_random_fields_snapshot_and_restore_bit_for_bit(size, bits, colour):
    what = "grid %s, %d-bit weights, colour %s" % (size, bits, colour)
    D, Wt, Cl = K.random_case(size, bits, colour)
    gv = make_volume(size, D, Wt, Cl, bits)
    assert gv.weight_storage() == (bits, False)
    before = state(gv)
    occupancy_before = gv.occupancy()
    snap = gv.snapshot()
    n = assert_snapshot(snap, D, Wt, Cl, size, bits, what)
    total = K.total_bricks(size)
    assert (n == 1) if total == 1 else (0 < n < total), what      # (by the CPU reference; the seeds are chosen so)
    assert snap.scratch_bytes <= 8 * total + 16 * ((total + 1023) // 1024 + 1)
    # the volume is as it was
    assert_state(gv, before[0], before[1], before[2], before[3], what + ": the volume after the snapshot")
    assert gv.occupancy() == occupancy_before

    # 1. into a fresh volume: the wider of its 8 bits and the snapshot's
    fresh = make_volume(size)
    fresh.restore(snap)
    assert_state(fresh, D, Wt, Cl, (bits, False), what + ": restored into a fresh volume")
    assert fresh.colour_enabled() == colour
    fresh.close()
    # 2. into the same volume after more writes
    D2, W2, C2 = R.random_field(size, 31 + K.seed_of(size, bits), 8, colour, K.FILL, live_share=0.7)
    gv.set_distance_data(D2)
    if colour:
        gv.set_colour_data(C2)
    gv.restore(snap)
    assert_state(gv, D, Wt, Cl, (bits, False), what + ": restored into the same volume")
    # 3. into one holding other data, 16-bit counts and colour
    other = make_volume(size, D2, W2, R.random_field(size, 5, 8, True, K.FILL, live_share=0.9)[2], 16)
    other.restore(snap)
    assert_state(other, D, Wt, Cl, (max(bits, 16), False), what + ": restored over other data")
    assert other.colour_enabled()            # (a snapshot without colour zeroes the array, it does not free it)
    other.close()
    # 4. download -> from_arrays -> restore
    ids, d, w, c = snap.download()
    again = tsdf_amd.Snapshot.from_arrays(size, ids, d, w, c, fill_distance=K.FILL, voxel_size=K.VS, offset=K.OFFSET)
    assert_snapshot(again, D, Wt, Cl, size, bits, what + ": uploaded")
    if bits != 32:
        assert again.info.weight_bound == int(np.max(w)) if len(ids) else again.info.weight_bound == 0
    fresh = make_volume(size)
    fresh.restore(again)
    assert_state(fresh, D, Wt, Cl, (bits, False), what + ": restored from uploaded arrays")
    for o in (fresh, again, snap, gv):
        o.close()


SIZE_1 = (9, 9, 10)      # 2 x 2 x 2 bricks, the upper ones partial on every axis


def one_voxel(reason, at):
    """(D, Wt, Cl, bits): a cleared 9 x 9 x 10 volume with one voxel live for one reason only."""
    n = SIZE_1[0] * SIZE_1[1] * SIZE_1[2]
    i = at[0] + SIZE_1[0] * (at[1] + SIZE_1[1] * at[2])
    D, Wt, Cl, bits = np.full(n, K.FILL, F32), np.zeros(n, F32), None, 8
    if reason == "weight":
        Wt[i] = 1.0
    elif reason == "weight16":
        Wt[i], bits = 256.0, 16
    elif reason == "distance":
        D[i] = np.nextafter(K.FILL, F32(np.inf))
    elif reason == "colour":
        Cl = np.zeros(n, U32)
        Cl[i] = 0x01000000
    elif reason == "nan weight":
        Wt[i], bits = np.nan, 32
    elif reason == "negative zero weight":
        Wt[i], bits = F32(-0.0), 32
    return D, Wt, Cl, bits


@pytest.mark.parametrize("reason", ["weight", "weight16", "distance", "colour", "nan weight", "negative zero weight"])
def test_bricks_live_by_one_voxel_only(reason):
    handle = tsdf_amd.Snapshot()
    # an inner voxel of the first brick; the last corner of the grid, in the last corner of a partial brick; the first voxel of the
    # brick that is one voxel wide
    for at, brick in [((3, 2, 1), 0), ((8, 8, 9), 7), ((8, 0, 0), 1), ((7, 7, 7), 0), ((0, 8, 8), 6)]:
        D, Wt, Cl, bits = one_voxel(reason, at)
        gv = make_volume(SIZE_1, D, Wt, Cl, bits)
        assert gv.weight_storage()[0] == bits
        snap = gv.snapshot(into=handle)
        assert snap is handle
        what = "%s at %s" % (reason, at)
        assert assert_snapshot(snap, D, Wt, Cl, SIZE_1, bits, what) == 1
        assert list(snap.bricks) == [brick], what
        fresh = make_volume(SIZE_1)
        fresh.restore(snap)
        assert_state(fresh, D, Wt, Cl, (bits, False), what + ": restored")
        fresh.close()
        gv.close()
    handle.close()


@pytest.mark.parametrize("bits", [8, 16, 32])
def test_values_where_the_padding_of_a_larger_grid_would_be_do_not_matter(bits):
    """On 9 x 9 x 9 the second brick along x holds x = 8 only.  Were its rows read as 8 voxels -- as they would lie if the grid were 16
    wide -- x = 9 .. 15 of row y would be x = 0 .. 6 of row y + 1, and likewise y = 9 .. 15 of plane z would be y = 0 .. 6 of plane
    z + 1.  Every voxel with x <= 6, 1 <= y <= 6, 1 <= z <= 6 is live and nothing else: only brick 0 is."""
    size = (9, 9, 9)
    D = np.full(size[::-1], K.FILL, F32)
    Wt = np.zeros(size[::-1], F32)
    Cl = np.zeros(size[::-1], U32)
    D[1:7, 1:7, 0:7] = F32(-3.0)
    Wt[1:7, 1:7, 0:7] = 7.0
    Cl[1:7, 1:7, 0:7] = 0x02112233
    gv = make_volume(size, D, Wt, Cl, bits)
    snap = gv.snapshot()
    assert assert_snapshot(snap, D.reshape(-1), Wt.reshape(-1), Cl.reshape(-1), size, bits, "aliasing rows") == 1
    assert list(snap.bricks) == [0]
    for o in (snap, gv):
        o.close()


@pytest.mark.parametrize("bits", [8, 16, 32])
def test_the_empty_and_the_full_volume(bits):
    size = (17, 8, 9)
    n = size[0] * size[1] * size[2]
    total = K.total_bricks(size)
    gv = make_volume(size, colour=True)
    if bits != 8:
        gv.set_weight_storage(bits)
    cleared = state(gv)
    snap = gv.snapshot()
    assert snap.n_bricks == 0 and snap.info.bytes == 0 and len(snap.bricks) == 0 and snap.distances.shape == (0, 512)
    assert snap.device_buffers() == (0, 0, 0, 0)
    assert_snapshot(snap, cleared[0], cleared[1], cleared[2], size, bits, "empty")
    # the full one: every voxel live, into the same handle
    rng = np.random.default_rng(3)
    D = (rng.uniform(-1.0, 0.5, n).astype(F32) * K.FILL).astype(F32)
    Wt = rng.integers(1, 200, n).astype(F32)
    Cl = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(U32)
    full = make_volume(size, D, Wt, Cl, bits)
    full_snap = full.snapshot()
    assert assert_snapshot(full_snap, D, Wt, Cl, size, bits, "full") == total
    # the empty snapshot clears a volume that holds data; the full one fills a cleared volume
    full.restore(snap)
    assert_state(full, cleared[0], cleared[1], cleared[2], (bits, False), "the empty snapshot restored")
    gv.restore(full_snap)
    assert_state(gv, D, Wt, Cl, (bits, False), "the full snapshot restored")
    for o in (snap, full_snap, gv, full):
        o.close()


# ---- a fused volume: the detour through a snapshot against a twin that never made it -----------------------------------------------
N_TWIN = 64


def frames_of(first, colour):
    out = []
    for i in range(first, first + 3):
        d, cam = synth.depth_frame(i * 9, 40, seed=0x5EEDE5D0)
        out.append((d, synth.colour_frame(i * 9, 40, seed=0x5EEDE5D0)[0] if colour else None, cam))
    return out


def fuse(gv, frames):
    for d, rgb, cam in frames:
        if rgb is None:
            gv.integrate(d, W, H, cam)
        else:
            gv.integrate_colour(d, rgb, W, H, cam)


def pictures(gv, cam, colour):
    """A ray cast and an indexed mesh, as arrays."""
    rc = tsdf_amd.GPURaycaster(W, H)
    out = list(rc.raycast_colour(gv, cam)) if colour else list(rc.raycast(gv, cam))
    mesh = gv.extract_mesh(normals=True, colours=colour)
    out += [mesh.vertices, mesh.indices, mesh.normals] + ([mesh.colours] if colour else [])
    mesh.close()
    return out


@pytest.mark.parametrize("colour", [False, True])
def test_a_detour_through_a_snapshot_leaves_no_trace(colour, oracle):
    first, more = frames_of(0, colour), frames_of(3, colour)
    cam = more[1][2]
    gv = tsdf_amd.TSDFVolume((N_TWIN,) * 3, (3000.0,) * 3)
    twin = tsdf_amd.TSDFVolume((N_TWIN,) * 3, (3000.0,) * 3)
    for v in (gv, twin):
        if colour:
            v.enable_colour()
        fuse(v, first)
    D, Wt, Cl, storage = state(gv)
    fill = F32(gv.truncation_distance())
    snap = gv.snapshot()
    ids, d, w, c = R.take(D, Wt, (N_TWIN,) * 3, fill, storage[0], Cl)
    same_bits(snap.bricks, ids, "fused: ids")
    same_bits(snap.distances, d, "fused: distances")
    same_bits(snap.weights, w, "fused: weights")
    if colour:
        same_bits(snap.colours, c, "fused: colours")
    else:
        # what the CPU oracle's own fusion of the three frames gives: 288 live bricks of 512
        ov = oracle.Volume((N_TWIN,) * 3, (3000.0,) * 3)
        for dm, _, cm in first:
            ov.integrate(dm, W, H, cm.inverse_pose(), cm.k(), cm.kinv(), nthreads=oracle.max_threads())
        assert len(R.take(ov.dist, ov.weight, (N_TWIN,) * 3, fill, 8)[0]) == 288 == snap.n_bricks
    after_first = pictures(gv, cam, colour)
    fuse(gv, more)
    gv.restore(snap)
    # straight after the restore: the state, and a ray cast that equals one after a forced rebuild of the occupancy flags
    assert_state(gv, D, Wt, Cl, storage, "fused: restored")
    straight = pictures(gv, cam, colour)
    gv.occupancy_data(force_rebuild=True)
    rebuilt = pictures(gv, cam, colour)
    for k, (a, b, c0) in enumerate(zip(straight, rebuilt, after_first)):
        same_bits(a, b, "fused: picture %d straight after the restore against a forced rebuild" % k)
        same_bits(a, c0, "fused: picture %d after the restore against before the detour" % k)
    fuse(gv, more)
    fuse(twin, more)
    a, b = state(gv), state(twin)
    assert_state(gv, b[0], b[1], b[2], b[3], "fused: after the detour against the twin")
    assert a[3] == b[3]
    for k, (p, q) in enumerate(zip(pictures(gv, cam, colour), pictures(twin, cam, colour))):
        same_bits(p, q, "fused: picture %d against the twin" % k)
    for o in (snap, gv, twin):
        o.close()


# ---- storage, the warm handle, the refusals -----------------------------------------------------------------------------------------
def test_storage_rules_of_restore():
    size = (40, 33, 21)
    n = size[0] * size[1] * size[2]
    D, W16, _ = K.random_case(size, 16, False)
    assert W16.max() > 255                       # counts past 255
    src = make_volume(size, D, W16, None, 16)
    snap16 = src.snapshot()
    assert snap16.info.weight_bits == 16
    # a 16-bit snapshot into a cleared 8-bit volume ends at 16; a weight cap set on the destination is still set
    dst = make_volume(size)
    dst.set_weight_cap(40)
    assert dst.weight_storage() == (8, False)
    dst.restore(snap16)
    assert_state(dst, D, W16, None, (16, False), "16 bits into 8")
    assert dst.weight_cap() == 40
    assert tuple(dst.offset()) == K.OFFSET
    # 8-bit into a pinned volume stays fp32 and pinned
    D8, W8, _ = K.random_case(size, 8, False)
    src8 = make_volume(size, D8, W8, None, 8)
    snap8 = src8.snapshot()
    assert snap8.info.weight_bits == 8
    pinned = make_volume(size)
    pointer = pinned.weight_data()
    assert pinned.weight_storage() == (32, True)
    pinned.restore(snap8)
    assert_state(pinned, D8, W8, None, (32, True), "8 bits into a pinned volume")
    assert pinned.weight_data() == pointer
    # 8-bit into the 16-bit volume stays 16; then integrate still works on it
    dst.restore(snap8)
    assert_state(dst, D8, W8, None, (16, False), "8 bits into 16")
    # fp32 into 8 bits ends at 32, unpinned
    Wf = np.where(W8 > 0, W8 + F32(0.5), W8).astype(F32)
    srcf = make_volume(size, D8, Wf, None, 32)
    snapf = srcf.snapshot()
    dst8 = make_volume(size)
    dst8.restore(snapf)
    assert_state(dst8, D8, Wf, None, (32, False), "fp32 into 8 bits")
    # the header fields of the destination are its own: another offset and truncation distance survive a restore
    far = make_volume(size)
    far.offset(1.0, 2.0, 3.0)
    far.restore(snap8)
    assert tuple(far.offset()) == (1.0, 2.0, 3.0) and F32(far.truncation_distance()) == K.FILL
    assert n == far.resident_voxels()
    for o in (snap16, snap8, snapf, src, src8, srcf, dst, dst8, pinned, far):
        o.close()


def test_a_warm_handle_allocates_nothing_and_takes_a_smaller_snapshot():
    size = (40, 33, 21)
    D, Wt, Cl = K.random_case(size, 8, True)
    gv = make_volume(size, D, Wt, Cl, 8)
    snap = gv.snapshot()
    n = assert_snapshot(snap, D, Wt, Cl, size, 8, "first")
    scratch, nbytes, pointers = snap.scratch_bytes, snap.info.bytes, snap.device_buffers()
    assert scratch > 0 and nbytes > 0 and all(pointers)
    assert gv.snapshot(into=snap) is snap
    assert_snapshot(snap, D, Wt, Cl, size, 8, "second")
    assert (snap.scratch_bytes, snap.info.bytes, snap.device_buffers()) == (scratch, nbytes, pointers)
    # a smaller snapshot into the same handle: fewer bricks of a smaller grid, the arrays stay where they are
    small_size = (9, 8, 8)
    Ds, Ws, Cs = K.random_case(small_size, 8, True)
    small = make_volume(small_size, Ds, Ws, Cs, 8)
    small.snapshot(into=snap)
    assert assert_snapshot(snap, Ds, Ws, Cs, small_size, 8, "smaller") < n
    assert snap.scratch_bytes == scratch and snap.device_buffers() == pointers
    fresh = make_volume(small_size)
    fresh.restore(snap)
    assert_state(fresh, Ds, Ws, Cs, (8, False), "smaller: restored")
    for o in (snap, gv, small, fresh):
        o.close()


def test_volumes_on_other_streams_order_themselves_behind_the_handle():
    """The handle's event: a restore enqueued on another stream straight after the snapshot reads complete arrays, and the next
    snapshot into the handle does not overwrite them under that restore.  Nothing here waits on the host in between."""
    import torch
    size = (264, 64, 40)
    a_stream, b_stream, c_stream = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    D, Wt, Cl = K.random_case(size, 8, True)
    D2, W2, C2 = R.random_field(size, 4242, 8, True, K.FILL, live_share=0.6)
    a, a2, b, b2 = make_volume(size, D, Wt, Cl, 8), make_volume(size, D2, W2, C2, 8), make_volume(size), make_volume(size)
    a.set_stream(a_stream.cuda_stream)
    a2.set_stream(a_stream.cuda_stream)
    b.set_stream(b_stream.cuda_stream)
    b2.set_stream(c_stream.cuda_stream)
    snap = tsdf_amd.Snapshot()
    for _ in range(3):
        a.snapshot(into=snap)
        b.restore(snap)
        a2.snapshot(into=snap)
        b2.restore(snap)
    torch.cuda.synchronize()
    assert_state(b, D, Wt, Cl, (8, False), "restored on another stream")
    assert_state(b2, D2, W2, C2, (8, False), "restored on a third stream")
    assert_snapshot(snap, D2, W2, C2, size, 8, "the handle after both")
    for o in (snap, a, a2, b, b2):
        o.close()


def test_refusals():
    size = (9, 8, 8)
    gv = make_volume(size)
    snap = gv.snapshot()
    never = tsdf_amd.Snapshot()
    invalid = _capi.TSDF_ERR_INVALID
    p = [C.c_void_p() for _ in range(4)]
    buf = np.zeros(4096, np.uint8)
    info = _capi.SnapshotInfo()
    checks = [
        ("tsdf_volume_snapshot", lambda: lib.tsdf_volume_snapshot(gv._h, 1, snap._h)),                  # flags other than 0
        ("tsdf_volume_snapshot", lambda: lib.tsdf_volume_snapshot(None, 0, snap._h)),
        ("tsdf_volume_snapshot", lambda: lib.tsdf_volume_snapshot(gv._h, 0, None)),
        ("tsdf_volume_restore", lambda: lib.tsdf_volume_restore(None, snap._h)),
        ("tsdf_volume_restore", lambda: lib.tsdf_volume_restore(gv._h, None)),
        ("tsdf_volume_restore", lambda: lib.tsdf_volume_restore(gv._h, never._h)),                      # never filled
        ("tsdf_snapshot_download", lambda: lib.tsdf_snapshot_download(never._h, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None)),
        ("tsdf_snapshot_buffers", lambda: lib.tsdf_snapshot_buffers(never._h, *[C.byref(q) for q in p])),
        ("tsdf_snapshot_download", lambda: lib.tsdf_snapshot_download(snap._h, None, buf.ctypes.data, buf.ctypes.data, None)),
        ("tsdf_snapshot_buffers", lambda: lib.tsdf_snapshot_buffers(snap._h, None, C.byref(p[1]), C.byref(p[2]), C.byref(p[3]))),
        ("tsdf_snapshot_get_info", lambda: lib.tsdf_snapshot_get_info(snap._h, None)),
        ("tsdf_snapshot_scratch_bytes", lambda: lib.tsdf_snapshot_scratch_bytes(snap._h, None)),
        ("tsdf_snapshot_upload", lambda: lib.tsdf_snapshot_upload(snap._h, None, None, None, None, None)),
    ]
    for name, call in checks:
        assert call() == invalid, name
        assert name in _capi.last_error(), (name, _capi.last_error())
    assert lib.tsdf_snapshot_get_info(never._h, C.byref(info)) == 0 and info.n_bricks == 0     # (an empty handle has an info)
    # a grid of another size
    other = make_volume((8, 8, 8))
    with pytest.raises(ValueError, match="tsdf_volume_restore"):
        other.restore(snap)
    # a Z-slab volume, on either call
    slab = tsdf_amd.TSDFVolume(size, K.physical(size), slab=(0, 4))
    with pytest.raises(ValueError, match="tsdf_volume_snapshot.*slab"):
        slab.snapshot()
    with pytest.raises(ValueError, match="tsdf_volume_restore.*slab"):
        slab.restore(snap)
    # a materialised deformation-node array, on either side
    nodes = make_volume(size)
    nodes.deformation()
    with pytest.raises(ValueError, match="tsdf_volume_snapshot.*deformation"):
        nodes.snapshot()
    with pytest.raises(ValueError, match="tsdf_volume_restore.*deformation"):
        nodes.restore(snap)
    with pytest.raises(ValueError, match="deformation"):
        nodes.save_sparse("/nonexistent/never-written.tsdfs")
    # nothing above changed the volume or the handle
    assert snap.n_bricks == 0
    lib.tsdf_snapshot_destroy(None)
    for o in (snap, never, gv, other, slab, nodes):
        o.close()
