"""The numpy reference of the rolling volume (tests/rolling_ref.py) against itself, and the host arithmetic of tsdf_amd/rolling.py, on the
CPU: select inside and outside partition a list; a zero shift into an equal grid is put; a shift there and back with the leaving
bricks paged in is the identity; BrickStore's keys hold at negative and large origins; follow takes the minimal shift."""
import itertools

import numpy as np
import pytest

from tests import rolling_ref as RR
from tests import snapshot_ref as R
from tsdf_amd import rolling

F32, U32 = np.float32, np.uint32
FILL = F32(37.5)


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def states_equal(a, b):
    return all(bits_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("size", [(16, 8, 8), (7, 9, 17), (40, 33, 21)])
@pytest.mark.parametrize("bits", [8, 32])
def test_select_inside_and_outside_partition_the_list(size, bits):
    D, Wt, Cl = R.random_field(size, 5 + size[0] + bits, bits, True, FILL, live_share=0.7)
    snap = R.take(D, Wt, size, FILL, bits, Cl)
    nb = R.bricks_per_axis(size)
    for lo, hi in [((0, 0, 0), nb), ((1, 0, 1), (3, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((-5, -5, -5), (1, 1, 1)), ((-2 ** 31,) * 3, (2 ** 31 - 1,) * 3)]:
        a, b = RR.select(*snap, size, lo, hi), RR.select(*snap, size, lo, hi, outside=True)
        assert len(a[0]) + len(b[0]) == len(snap[0]) and not set(a[0]) & set(b[0])
        order = np.argsort(np.concatenate([a[0], b[0]]), kind="stable")
        for k in range(4):
            both = np.concatenate([a[k], b[k]])[order]
            assert bits_equal(both, snap[k])
        for ids in (a[0], b[0]):
            assert np.all(ids[1:] > ids[:-1])
        for c in RR.coords(a[0], nb):
            assert all(lo[k] <= c[k] < hi[k] for k in range(3))
    assert len(RR.select(*snap, size, (0, 0, 0), nb)[0]) == len(snap[0])
    assert len(RR.select(*snap, size, (2, 2, 2), (2, 2, 2))[0]) == 0


@pytest.mark.parametrize("size", [(8, 8, 8), (9, 8, 8), (7, 9, 17), (40, 33, 21)])
@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("colour", [False, True])
def test_zero_shift_into_an_equal_grid_is_put(size, bits, colour):
    D, Wt, Cl = R.random_field(size, 11 + size[1] + bits, bits, colour, FILL, live_share=0.5)
    snap = R.take(D, Wt, size, FILL, bits, Cl)
    assert states_equal(RR.restore_shifted(*snap, size, size, (0, 0, 0), FILL), R.put(*snap, size, FILL))
    assert states_equal(RR.restore_shifted(*snap, size, size, (0, 0, 0), FILL), (D, Wt, Cl))
    # over kept data every voxel of a brick that is not stored stays
    D2, W2, C2 = R.random_field(size, 99, 8, colour, FILL, live_share=0.9)
    got = RR.restore_shifted(*snap, size, size, (0, 0, 0), FILL, keep=(D2, W2, C2))
    live = np.zeros(np.prod(R.bricks_per_axis(size)), bool)
    live[snap[0]] = True
    vox = R._unbricked(np.repeat(live[:, None], 512, axis=1), size)
    for g, new, old in zip(got, (D, Wt, Cl), (D2, W2, C2)):
        assert bits_equal(g, None if new is None else np.where(vox, new, old).astype(new.dtype))


@pytest.mark.parametrize("size,s", [((16, 16, 16), (1, 0, 0)), ((64, 8, 8), (-3, 0, 0)), ((32, 16, 24), (1, -1, 2)), ((16, 16, 16), (2, 0, 0)),
                                    ((16, 16, 16), (2 ** 31 - 1, -2 ** 31, 0))])
@pytest.mark.parametrize("bits", [8, 32])
def test_shift_there_and_back_with_the_leaving_bricks_paged_in_is_the_identity(size, s, bits):
    D, Wt, Cl = R.random_field(size, 3 + size[0] + bits, bits, True, FILL, live_share=0.6)
    after, leaving = RR.shift(D, Wt, Cl, size, s, FILL, bits)
    nb = R.bricks_per_axis(size)
    # what stayed and what left partition the list; the content moved by -s
    n_all = len(R.take(D, Wt, size, FILL, bits, Cl)[0])
    n_stay = len(R.take(*after[:2], size, FILL, bits, after[2])[0])
    assert n_stay + len(leaving[0]) == n_all
    if any(abs(s[k]) >= nb[k] for k in range(3)):
        assert n_stay == 0
    back, leaving_back = RR.shift(*after, size, [-v for v in s], FILL, bits)
    assert len(leaving_back[0]) == 0        # (what the return trip uncovers is cleared, so nothing live falls out on the other side)
    paged = RR.restore_shifted(*leaving, size, size, (0, 0, 0), FILL, keep=back)
    assert states_equal(paged, (D, Wt, Cl))


def test_shifted_offset_rounds_in_fp32():
    got = RR.shifted_offset((100.0, -50.0, 25.0), (1, -3, 2 ** 31 - 1), (10.0, 12.5, 9.0))
    assert got.dtype == F32 and got[0] == F32(180.0) and got[1] == F32(-350.0)
    assert got[2] == F32(25.0) + F32(8 * (2 ** 31 - 1)) * F32(9.0)


@pytest.mark.parametrize("origin", [(0, 0, 0), (-3, 5, -70000), (2 ** 40, -2 ** 40 + 1, 2 ** 31 - 1)])
def test_brick_store_keys(origin):
    nb = (5, 3, 4)
    ids = np.array([0, 4, 5, 17, 59], U32)
    keys = rolling.world_keys(ids, nb, origin)
    assert keys == [tuple(o + c for o, c in zip(origin, b)) for b in RR.coords(ids, nb)]
    assert all(isinstance(k, int) for key in keys for k in key)
    assert [rolling.frame_id(k, origin, nb) for k in keys] == list(ids)
    # the same bricks seen from a box one brick further along x: the first column has left it, ids are renumbered
    moved = tuple(o + s for o, s in zip(origin, (1, 0, 0)))
    seen = [rolling.frame_id(k, moved, nb) for k in keys]
    assert seen == [None, 3, None, 16, 58]

    store = rolling.BrickStore()
    rng = np.random.default_rng(4)
    d = rng.random((5, 512)).astype(F32)
    w8 = rng.integers(0, 256, (5, 512)).astype(np.uint8)
    store.put_arrays(ids[:3], nb, d[:3], w8[:3], None, origin)
    w16 = rng.integers(0, 65536, (2, 512)).astype(np.uint16)
    c = rng.integers(0, 2 ** 32, (2, 512), dtype=np.uint64).astype(U32)
    store.put_arrays(ids[3:], nb, d[3:], w16, c, origin)
    assert len(store) == 5 and store.bytes() == 3 * 512 * 5 + 2 * 512 * 10 and keys[3] in store
    hi = tuple(o + n for o, n in zip(moved, nb))
    gi, gd, gw, gc = store.take_arrays(moved, hi, moved, nb)
    assert list(gi) == [3, 16, 58] and gi.dtype == U32 and len(store) == 2
    assert bits_equal(gd, d[[1, 3, 4]])
    assert gw.dtype == np.uint16 and np.array_equal(gw, np.concatenate([w8[1:2].astype(np.uint16), w16]))
    assert np.array_equal(gc, np.concatenate([np.zeros((1, 512), U32), c]))
    # the two that stayed behind come back when the box returns, and only then
    none = store.take_arrays(moved, hi, moved, nb)
    assert len(none[0]) == 0 and none[1].shape == (0, 512) and none[3] is None and len(store) == 2
    gi, gd, gw, gc = store.take_arrays(origin, tuple(o + n for o, n in zip(origin, nb)), origin, nb)
    assert list(gi) == [0, 5] and gw.dtype == np.uint8 and gc is None and len(store) == 0 and store.bytes() == 0


def test_fusion_across_a_shift_holds_for_the_chosen_inputs(oracle):
    """With the oracle's integrate and the reference shift: the rolling volume keeps pace with a static one that covers both boxes, and
    the bricks it uncovers are those of a fresh volume that saw the later frames only (what tests/test_rolling.py asks of the GPU)."""
    from tests import rolling_cases as Q
    cam = Q.camera()

    def volume(size, offset):
        v = oracle.Volume(size, Q.physical(size))
        assert np.array_equal(v.voxel_size(), np.full(3, Q.VOXEL, F32))
        v.offset(*offset)
        assert not np.any(np.array(v.g.offset_at_clear))
        return v

    def fuse(v, frames):
        for f in frames:
            v.integrate(Q.depth_frame(f), Q.W, Q.H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())

    static, roll = volume(Q.STATIC_SIZE, Q.OFFSET), volume(Q.ROLLING_SIZE, Q.OFFSET)
    fuse(static, range(3))
    fuse(roll, range(3))
    fill = F32(roll.truncation_distance())
    assert np.count_nonzero(roll.weight) > 1000 and np.max(roll.weight) == 3.0
    (D, Wt, _), leaving = RR.shift(roll.dist, roll.weight, None, Q.ROLLING_SIZE, Q.BOX_SHIFT, fill, 8)
    assert len(leaving[0]) > 0
    roll.set_distance_data(D)
    roll.set_weight_data(Wt)
    moved = RR.shifted_offset(Q.OFFSET, Q.BOX_SHIFT, (Q.VOXEL,) * 3)
    assert tuple(moved) == (Q.OFFSET[0] + 32.0, Q.OFFSET[1], Q.OFFSET[2])
    roll.offset(*moved)
    fresh = volume(Q.ROLLING_SIZE, moved)
    for v in (static, roll, fresh):
        fuse(v, range(3, Q.FRAMES))
    cube = lambda v, a: a.reshape(v.size()[::-1])
    for name in ("dist", "weight"):
        s, r, f = (cube(v, getattr(v, name)) for v in (static, roll, fresh))
        assert bits_equal(r[:, :, :24], s[:, :, 8:32]), name
        assert bits_equal(r[:, :, 24:], f[:, :, 24:]), name
        assert not bits_equal(r[:, :, :24], f[:, :, :24]), name      # (the part that moved carries the first three frames too)
    assert np.max(roll.weight) == 6.0 and np.count_nonzero(cube(fresh, fresh.weight)[:, :, 24:]) > 100


def test_follow_takes_the_minimal_shift():
    for n, m in [(4, 0), (4, 1), (5, 2), (9, 3), (1, 0)]:
        for c in range(-12, 22):
            s = rolling.follow_shift((c,), (n,), (m,))[0]
            ok = [t for t in range(-40, 40) if m <= c - t <= n - 1 - m]
            assert s == min(ok, key=abs) and (s == 0) == (m <= c <= n - 1 - m), (n, m, c, s)
    assert rolling.follow_shift((7, -1, 2), (4, 4, 4), (1, 1, 1)) == (5, -2, 0)
    assert rolling.follow_shift((2 ** 40, 0, 0), (4, 4, 4), (0, 0, 0)) == (2 ** 40 - 3, 0, 0)
    with pytest.raises(ValueError, match="margin"):
        rolling.follow_shift((0,), (4,), (2,))
