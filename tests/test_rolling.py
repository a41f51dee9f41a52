"""GPU: the rolling volume (tsdf_volume_restore_shifted / tsdf_snapshot_select / tsdf_volume_shift; include/tsdf_amd.h, "rolling volume")
against the CPU reference tests/rolling_ref.py, bit for bit and without a tolerance: snapshots of random fields put back at other brick
coordinates, over cleared and over kept data, in every storage, into grids of their own size, smaller and larger; the bricks of a list
inside and outside a box; the shift of a volume's box with what falls out, there and back; fusion that goes on across a shift against
a static volume covering both boxes; the walk of a RollingVolume; the refusals."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tests import rolling_cases as Q
from tests import rolling_ref as RR
from tests import snapshot_cases as K
from tests import snapshot_ref as R
from tsdf_amd import _capi

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
lib = _capi.lib
BIG = (2 ** 31 - 1, -2 ** 31, 0)


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
    return gv.get_distance_data(), gv.get_weight_data(), gv.get_colour_data() if gv.colour_enabled() else None


def assert_state(gv, want, bits, what):
    d, w, c = state(gv)
    same_bits(d, np.ascontiguousarray(want[0], F32).reshape(-1), what + ": distances")
    same_bits(w, np.ascontiguousarray(want[1], F32).reshape(-1), what + ": weights")
    if want[2] is None:
        assert c is None or not c.any(), what + ": colours"
    else:
        same_bits(c, np.ascontiguousarray(want[2], U32).reshape(-1), what + ": colours")
    assert gv.weight_storage()[0] == bits, (what, gv.weight_storage(), bits)


def assert_list(snap, want, what):
    """A handle's arrays against (ids, d, w, c)."""
    got = snap.download()
    for g, w, name in zip(got, want, ("ids", "distances", "weights", "colours")):
        assert (g is None) == (w is None), (what, name)
        if w is not None:
            same_bits(g, w, "%s: brick %s" % (what, name))
    i = snap.info
    assert i.n_bricks == len(want[0]) == snap.n_bricks, what
    bits = {1: 8, 2: 16, 4: 32}[np.asarray(want[2]).dtype.itemsize]
    assert i.weight_bits == bits and i.flags == (1 if want[3] is not None else 0), what
    assert i.bytes == len(want[0]) * (4 + 512 * (4 + bits // 8 + (4 if want[3] is not None else 0))), what


def snapshot_of(size, bits, colour):
    """(Snapshot, its reference arrays, the dense field) of the random case of a grid."""
    D, Wt, Cl = K.random_case(size, bits, colour)
    src = make_volume(size, D, Wt, Cl, bits)
    snap = src.snapshot()
    src.close()
    return snap, R.take(D, Wt, size, K.FILL, bits, Cl), (D, Wt, Cl)


def shifts_for(size, k):
    nb = R.bricks_per_axis(size)
    out = [0, 0, 0]
    out[k % 3] = nb[k % 3] if k % 2 else -nb[k % 3]         # exactly nb on one axis: everything is out
    return [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, -1), (2, -1, 1), tuple(out), BIG]


# ---- tsdf_volume_restore_shifted ------------------------------------------------------------------------------------------------------
GRIDS = [(8, 8, 8), (16, 8, 8), (9, 8, 8), (7, 9, 17), (40, 33, 21), (264, 64, 40)]


@pytest.mark.parametrize("size", GRIDS)
@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("colour", [False, True])
def test_restore_shifted_over_a_cleared_volume(size, bits, colour):
    snap, ref, field = snapshot_of(size, bits, colour)
    # a destination that holds something everywhere: what a restore without flags does not write it must clear
    junk = R.random_field(size, 17 + K.seed_of(size, bits), 8, colour, K.FILL, live_share=1.0)
    dst = make_volume(size, *junk, None)
    for n, shift in enumerate(shifts_for(size, GRIDS.index(size) + bits // 8)):
        what = "grid %s, %d-bit weights, colour %s, shift %s" % (size, bits, colour, shift)
        dst.restore(snap, shift=shift)
        want = RR.restore_shifted(*ref, size, size, shift, K.FILL)
        if shift == (0, 0, 0):
            for a, b in zip(want, field):
                assert (a is None and b is None) or a.tobytes() == b.tobytes()       # (the reference's own: the field comes back)
        elif n >= 5:
            assert not want[1].any()                                                 # (the reference's own: everything is out)
        assert_state(dst, want, bits, what)
        assert dst.colour_enabled() == colour
    # the new entry point with a zero shift and no flags, not the old one Python takes then
    check = make_volume(size, *junk, None)
    _capi.check(lib.tsdf_volume_restore_shifted(check._h, snap._h, (C.c_int32 * 3)(0, 0, 0), 0))
    assert_state(check, field, bits, "zero shift through tsdf_volume_restore_shifted")
    for o in (snap, dst, check):
        o.close()


@pytest.mark.parametrize("dst_size,shift", [((24, 24, 24), (-1, -1, 0)), ((64, 40, 32), (1, 0, 1))])
@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("colour", [False, True])
def test_crop_and_grow(dst_size, shift, bits, colour):
    size = (40, 33, 21)
    snap, ref, _ = snapshot_of(size, bits, colour)
    junk = R.random_field(dst_size, 23, 8, colour, K.FILL, live_share=1.0)
    dst = make_volume(dst_size, *junk, None)
    dst.restore(snap, shift=shift)
    want = RR.restore_shifted(*ref, size, dst_size, shift, K.FILL)
    assert want[1].any()
    assert_state(dst, want, bits, "%s into %s by %s" % (size, dst_size, shift))
    assert tuple(dst.offset()) == K.OFFSET                  # (offsets are not touched)
    for o in (snap, dst):
        o.close()


# ---- TSDF_RESTORE_KEEP_OTHERS ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(9, 8, 8), (7, 9, 17), (40, 33, 21), (264, 64, 40)])
@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("colour", [False, True])
def test_page_in_over_another_field(size, bits, colour):
    snap, ref, _ = snapshot_of(size, bits, colour)
    other = R.random_field(size, 29 + K.seed_of(size, bits), bits, colour, K.FILL, live_share=0.8)
    dst = make_volume(size, *other, bits)
    now = other
    for shift in [(0, 0, 0), (1, 0, 0), (-1, 1, 0), (0, 0, -1), BIG]:
        dst.restore(snap, shift=shift, keep_others=True)
        now = RR.restore_shifted(*ref, size, size, shift, K.FILL, keep=now)
        assert_state(dst, now, bits, "grid %s, %d bits, colour %s: paged in at %s" % (size, bits, colour, shift))
    if bits != 32:
        after = dst.snapshot()
        assert int(np.max(now[1])) <= after.info.weight_bound <= 65535
        after.close()
    for o in (snap, dst):
        o.close()


def test_page_in_storage_and_colour_rules():
    size = (40, 33, 21)
    snap8, ref8, _ = snapshot_of(size, 8, False)
    snap16, ref16, _ = snapshot_of(size, 16, False)
    snapc, refc, _ = snapshot_of(size, 8, True)
    assert np.max(ref16[2]) > 255
    shift = (1, -1, 0)
    # an 8-bit snapshot into a 16-bit volume: it stays 16
    other = R.random_field(size, 61, 16, False, K.FILL, live_share=0.8)
    dst = make_volume(size, *other, 16)
    dst.restore(snap8, shift=shift, keep_others=True)
    assert_state(dst, RR.restore_shifted(*ref8, size, size, shift, K.FILL, keep=other), 16, "8 bits into 16")
    dst.close()
    # a 16-bit snapshot into an 8-bit volume: the volume widens and the old counts are kept
    other = R.random_field(size, 62, 8, False, K.FILL, live_share=0.8)
    dst = make_volume(size, *other, 8)
    assert dst.weight_storage() == (8, False)
    dst.restore(snap16, shift=shift, keep_others=True)
    assert_state(dst, RR.restore_shifted(*ref16, size, size, shift, K.FILL, keep=other), 16, "16 bits into 8")
    after = dst.snapshot()
    assert after.info.weight_bound >= int(np.max(ref16[2]))
    after.close()
    dst.close()
    # a coloured snapshot into a volume without colour: colour is enabled, 0 where nothing is written
    dst = make_volume(size, *other, 8)
    assert not dst.colour_enabled()
    dst.restore(snapc, shift=shift, keep_others=True)
    want = RR.restore_shifted(*refc, size, size, shift, K.FILL, keep=other)
    assert want[2] is not None and want[2].any()
    assert dst.colour_enabled()
    assert_state(dst, want, 8, "colour into none")
    dst.close()
    # a plain snapshot into a volume with colour: colour 0 on the bricks it writes only
    other = R.random_field(size, 63, 8, True, K.FILL, live_share=0.9)
    dst = make_volume(size, *other, 8)
    dst.restore(snap8, shift=shift, keep_others=True)
    want = RR.restore_shifted(*ref8, size, size, shift, K.FILL, keep=other)
    assert 0 < np.count_nonzero(want[2]) < np.count_nonzero(other[2])
    assert_state(dst, want, 8, "no colour into colour")
    for o in (dst, snap8, snap16, snapc):
        o.close()


def test_page_in_fp32_words_are_moved_as_bits():
    size = (16, 16, 9)
    n = size[0] * size[1] * size[2]
    D, Wt = np.full(n, K.FILL, F32), np.zeros(n, F32)
    Wt[3], Wt[5], Wt[9 + 16 * 9] = F32(-0.0), np.nan, 2.5            # brick 0, and brick 3 (x 9, y 9)
    Wt.view(U32)[7] = 0x7fc12345                                     # a NaN with a payload
    src = make_volume(size, D, Wt, None, 32)
    snap = src.snapshot()
    ref = R.take(D, Wt, size, K.FILL, 32)
    assert list(ref[0]) == [0, 3]
    other = R.random_field(size, 64, 32, False, K.FILL, live_share=1.0)
    dst = make_volume(size, *other, 32)
    dst.restore(snap, shift=(1, 0, 0), keep_others=True)             # brick 0 -> 1; brick 3 leaves the grid
    want = RR.restore_shifted(*ref, size, size, (1, 0, 0), K.FILL, keep=other)
    assert np.signbit(want[1][8 + 3]) and want[1].view(U32)[8 + 7] == 0x7fc12345
    assert_state(dst, want, 32, "fp32 page-in")
    for o in (src, snap, dst):
        o.close()


# ---- tsdf_snapshot_select -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,bits,colour", [((40, 33, 21), 8, True), ((40, 33, 21), 32, False), ((264, 64, 40), 16, True)])
def test_select(size, bits, colour):
    snap, ref, _ = snapshot_of(size, bits, colour)
    nb = R.bricks_per_axis(size)
    inner = ((1, 0, 1), (nb[0] - 1, nb[1] - 1, nb[2]))
    out = tsdf_amd.Snapshot()
    for lo, hi in [inner, ((0, 0, 0), nb), ((-2 ** 31,) * 3, (2 ** 31 - 1,) * 3), ((1, 1, 1), (1, 1, 1)), ((3, 0, 0), (2, 9, 9))]:
        for outside in (False, True):
            what = "grid %s, box %s .. %s, outside %s" % (size, lo, hi, outside)
            assert snap.select(lo, hi, outside=outside, into=out) is out
            want = RR.select(*ref, size, lo, hi, outside)
            assert_list(out, want, what)
            a, b = out.info, snap.info
            for f in ("size", "bricks", "voxel_size", "offset"):
                assert tuple(getattr(a, f)) == tuple(getattr(b, f)), (what, f)
            assert (a.flags, a.weight_bits, a.weight_bound) == (b.flags, b.weight_bits, b.weight_bound) and F32(a.fill_distance) == K.FILL, what
            # the result is a snapshot like any other: it restores
            dst = make_volume(size, *R.random_field(size, 3, 8, colour, K.FILL, live_share=1.0), None)
            dst.restore(out)
            assert_state(dst, R.put(*want, size, K.FILL), bits, what + ": restored")
            dst.close()
    n_inner = len(RR.select(*ref, size, *inner)[0])
    assert 0 < n_inner < len(ref[0])                                  # (by the reference: the inner box splits the list)
    # a warm dst allocates nothing
    snap.select(*inner, into=out)
    scratch, pointers = out.scratch_bytes, out.device_buffers()
    snap.select(*inner, outside=True, into=out)
    snap.select(*inner, into=out)
    assert (out.scratch_bytes, out.device_buffers()) == (scratch, pointers)
    assert_list(out, RR.select(*ref, size, *inner), "warm")
    for o in (snap, out):
        o.close()


def test_select_refusals():
    snap, ref, _ = snapshot_of((16, 8, 8), 8, False)
    with pytest.raises(ValueError, match="tsdf_snapshot_select.*dst is src"):
        snap.select((0, 0, 0), (1, 1, 1), into=snap)
    never = tsdf_amd.Snapshot()
    with pytest.raises(ValueError, match="tsdf_snapshot_select.*never been filled"):
        never.select((0, 0, 0), (1, 1, 1))
    three = (C.c_int32 * 3)(0, 0, 0)
    for args in [(None, three, three, 0, never._h), (snap._h, None, three, 0, never._h), (snap._h, three, None, 0, never._h), (snap._h, three, three, 0, None)]:
        assert lib.tsdf_snapshot_select(*args) == _capi.TSDF_ERR_INVALID and "tsdf_snapshot_select" in _capi.last_error()
    assert lib.tsdf_snapshot_select(snap._h, three, three, 2, never._h) == _capi.TSDF_ERR_INVALID and "flags" in _capi.last_error()
    assert_list(snap, ref, "the source after the refusals")
    for o in (snap, never):
        o.close()


# ---- tsdf_volume_shift ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,shifts", [((16, 16, 16), [(1, 0, 0), (0, -1, 1), (2, 0, 0), BIG]),
                                         ((64, 8, 8), [(3, 0, 0), (-8, 0, 0), (0, 1, 0)]),
                                         ((264, 64, 40), [(1, 1, 1), (-5, 0, 2)])])
@pytest.mark.parametrize("bits,colour", [(8, False), (16, True), (32, True)])
def test_shift(size, shifts, bits, colour):
    field = K.random_case(size, bits, colour)
    work, leaving = tsdf_amd.Snapshot(), tsdf_amd.Snapshot()
    for s in shifts:
        what = "grid %s, %d bits, colour %s, box shift %s" % (size, bits, colour, s)
        gv = make_volume(size, *field, bits)
        at_clear = tuple(gv.info().offset_at_clear)
        assert gv.shift(s, work=work, leaving=leaving) is leaving
        after, left = RR.shift(*field, size, s, K.FILL, bits)
        assert_state(gv, after, bits, what)
        assert_list(leaving, left, what + ": leaving")
        assert tuple(leaving.info.offset) == K.OFFSET and tuple(leaving.info.size) == size, what      # the frame before the move
        same_bits(gv.offset(), RR.shifted_offset(K.OFFSET, s, K.VS), what + ": offset")
        assert tuple(gv.info().offset_at_clear) == at_clear, what
        # back again, the bricks that left paged in: the original state
        if max(abs(v) for v in s) < 2 ** 20:
            back = gv.shift([-v for v in s], work=work)
            assert back.n_bricks == 0, what
            back.close()
            gv.restore(leaving, keep_others=True)
            assert_state(gv, field, bits, what + ": there and back")
            same_bits(gv.offset(), np.array(K.OFFSET, F32), what + ": offset there and back")
        gv.close()
    for o in (work, leaving):
        o.close()


def test_a_zero_shift_writes_nothing():
    size = (16, 16, 16)
    field = K.random_case(size, 8, True)
    gv = make_volume(size, *field, 8)
    before = state(gv) + (gv.occupancy(), tuple(gv.offset()))
    three = (C.c_int32 * 3)(0, 0, 0)
    work = tsdf_amd.Snapshot()
    _capi.check(lib.tsdf_volume_shift(gv._h, three, work._h, None))
    leaving = gv.shift((0, 0, 0), work=work)
    assert leaving.n_bricks == 0 and leaving.info.bytes == 0 and tuple(leaving.info.size) == size
    after = state(gv) + (gv.occupancy(), tuple(gv.offset()))
    for a, b in zip(before[:3], after[:3]):
        same_bits(a, b, "a zero shift")
    assert before[3:] == after[3:]
    # an empty handle restores like any other: nothing is stored
    fresh = make_volume(size, *field, 8)
    fresh.restore(leaving)
    assert not fresh.get_weight_data().any()
    for o in (gv, work, leaving, fresh):
        o.close()


def test_shift_refusals():
    size = (16, 16, 16)
    field = K.random_case(size, 8, False)
    gv = make_volume(size, *field, 8)
    work, leaving = tsdf_amd.Snapshot(), tsdf_amd.Snapshot()
    one = (C.c_int32 * 3)(1, 0, 0)
    for args in [(None, one, work._h, leaving._h), (gv._h, None, work._h, leaving._h), (gv._h, one, None, leaving._h)]:
        assert lib.tsdf_volume_shift(*args) == _capi.TSDF_ERR_INVALID and "tsdf_volume_shift" in _capi.last_error()
    with pytest.raises(ValueError, match="tsdf_volume_shift.*leaving is work"):
        gv.shift((1, 0, 0), work=work, leaving=work)
    slab = tsdf_amd.TSDFVolume(size, K.physical(size), slab=(0, 8))
    with pytest.raises(ValueError, match="tsdf_volume_shift.*slab"):
        slab.shift((1, 0, 0))
    nodes = make_volume(size)
    nodes.deformation()
    with pytest.raises(ValueError, match="tsdf_volume_shift.*deformation"):
        nodes.shift((1, 0, 0))
    for odd in [(9, 16, 16), (16, 9, 16), (16, 16, 9)]:
        partial = make_volume(odd)
        with pytest.raises(ValueError, match="tsdf_volume_shift.*multiple of 8"):
            partial.shift((1, 0, 0))
        partial.close()
    classes = make_volume(size)
    classes.enable_classes()
    with pytest.raises(ValueError, match="tsdf_volume_shift.*class words"):
        classes.shift((1, 0, 0))
    # restore_shifted: its own refusals
    never = tsdf_amd.Snapshot()
    with pytest.raises(ValueError, match="tsdf_volume_restore_shifted.*never been filled"):
        gv.restore(never, shift=(1, 0, 0))
    snap = gv.snapshot()
    with pytest.raises(ValueError, match="tsdf_volume_restore_shifted.*slab"):
        slab.restore(snap, shift=(1, 0, 0))
    with pytest.raises(ValueError, match="tsdf_volume_restore_shifted.*deformation"):
        nodes.restore(snap, keep_others=True)
    assert lib.tsdf_volume_restore_shifted(gv._h, snap._h, one, 2) == _capi.TSDF_ERR_INVALID and "flags" in _capi.last_error()
    assert lib.tsdf_volume_restore_shifted(gv._h, snap._h, None, 0) == _capi.TSDF_ERR_INVALID
    # nothing above changed the volume
    assert_state(gv, field, 8, "after the refusals")
    assert tuple(gv.offset()) == K.OFFSET
    for o in (gv, work, leaving, slab, nodes, classes, never, snap):
        o.close()


# ---- fusion across a shift ------------------------------------------------------------------------------------------------------------
def test_fusion_goes_on_across_a_shift():
    """(tests/test_rolling_ref_host.py shows with the oracle's integrate that these identities hold for these inputs.)"""
    cam = Q.camera()

    def volume(size, offset):
        v = tsdf_amd.TSDFVolume(size, Q.physical(size))
        assert np.array_equal(v.voxel_size(), np.full(3, Q.VOXEL, F32))
        v.offset(*offset)
        assert not any(v.info().offset_at_clear)
        return v

    def fuse(v, frames):
        for f in frames:
            v.integrate(Q.depth_frame(f), Q.W, Q.H, cam)

    static, roll = volume(Q.STATIC_SIZE, Q.OFFSET), volume(Q.ROLLING_SIZE, Q.OFFSET)
    fuse(static, range(3))
    fuse(roll, range(3))
    leaving = roll.shift(Q.BOX_SHIFT)
    assert leaving.n_bricks > 0
    moved = tuple(roll.offset())
    assert moved == (Q.OFFSET[0] + 32.0, Q.OFFSET[1], Q.OFFSET[2])
    fresh = volume(Q.ROLLING_SIZE, moved)
    for v in (static, roll, fresh):
        fuse(v, range(3, Q.FRAMES))
    cube = lambda v, a: a.reshape(v.size()[::-1])
    for name in ("get_distance_data", "get_weight_data"):
        s, r, f = (cube(v, getattr(v, name)()) for v in (static, roll, fresh))
        same_bits(r[:, :, :24], s[:, :, 8:32], name + ": the part that moved against the static volume")
        same_bits(r[:, :, 24:], f[:, :, 24:], name + ": the uncovered bricks against a fresh volume")
    assert np.max(roll.get_weight_data()) == 6.0
    for o in (static, roll, fresh, leaving):
        o.close()


# ---- BrickStore, RollingVolume --------------------------------------------------------------------------------------------------------
def test_a_brick_store_gives_back_what_it_took_in_another_frame():
    size = (40, 32, 24)
    snap, ref, _ = snapshot_of(size, 16, True)
    origin, moved = (5, -2, 2 ** 40), (6, -3, 2 ** 40)                # the frame the bricks come back in lies (1, -1, 0) bricks further
    store = tsdf_amd.BrickStore()
    store.put(snap, origin)
    assert len(store) == len(ref[0]) and store.bytes() == len(ref[0]) * 512 * 10
    nb = R.bricks_per_axis(size)
    page = store.take(moved, tuple(o + n for o, n in zip(moved, nb)), moved, size=size, fill_distance=K.FILL, voxel_size=K.VS, offset=K.OFFSET)
    want = RR.restore_shifted(*ref, size, size, (-1, 1, 0), K.FILL)
    assert_list(page, R.take(want[0], want[1], size, K.FILL, 16, want[2]), "taken in the moved frame")
    assert len(store) == len(ref[0]) - page.n_bricks > 0             # what the moved box does not cover stays in the store
    dst = make_volume(size)
    dst.restore(page)
    assert_state(dst, want, 16, "restored from the store")
    for o in (snap, page, dst):
        o.close()



@pytest.mark.parametrize("bits,colour", [(8, False), (16, True)])
def test_a_walk_of_a_rolling_volume_ends_where_it_began(bits, colour):
    size = (32, 16, 16)
    field = K.random_case(size, bits, colour)
    gv = make_volume(size, *field, bits)
    rv = tsdf_amd.RollingVolume(gv)
    held = 0
    for step in [(2, 0, 0), (1, 0, 0), (-3, 0, 0), (1, -1, 1), (-1, 1, -1)]:
        out, back = rv.shift(step)
        held += out - back
        assert len(rv.store) == held
    assert held == 0 and len(rv.store) == 0 and rv.store.bytes() == 0
    assert rv.origin_bricks == (0, 0, 0)
    assert_state(gv, field, bits, "after the walk")
    same_bits(gv.offset(), np.array(K.OFFSET, F32), "offset after the walk")
    # follow: a point in brick 6 along x of a box of 4 bricks, to be kept a brick from the x faces, asks for 4 bricks; then it is inside
    vs = K.VS.astype(np.float64)
    point = [K.OFFSET[0] + 52 * vs[0], K.OFFSET[1] + 4 * vs[1], K.OFFSET[2] + 12 * vs[2]]
    assert rv.follow(point, (1, 0, 0)) == (4, 0, 0) and rv.origin_bricks == (4, 0, 0)
    same_bits(gv.offset(), RR.shifted_offset(K.OFFSET, (4, 0, 0), K.VS), "offset after follow")
    assert rv.follow(point, (1, 0, 0)) == (0, 0, 0) and rv.origin_bricks == (4, 0, 0)
    rv.close()
    gv.close()
