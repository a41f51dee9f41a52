"""The numpy reference of the sparse snapshot (tests/snapshot_ref.py) against itself and against hand-made answers, on the CPU: the round
trip is the identity on random fields in every storage, ids ascend, the padding of partial bricks holds fill, 0 and 0, and a 9 x 8 x 8
grid -- two bricks, the second one voxel wide -- gives the bytes written out here by hand."""
import numpy as np
import pytest

from tests import snapshot_cases as K
from tests import snapshot_ref as R

F32, U32 = np.float32, np.uint32
FILL = F32(37.5)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("size", [(2, 2, 2), (9, 8, 8), (7, 9, 17), (40, 33, 21), (65, 3, 5)])
@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("colour", [False, True])
def test_round_trip_is_the_identity(size, bits, colour):
    D, Wt, Cl = R.random_field(size, 77 + size[0] + bits, bits, colour, FILL, live_share=0.5)
    ids, d, w, c = R.take(D, Wt, size, FILL, bits, Cl)
    nb = R.bricks_per_axis(size)
    assert ids.dtype == U32 and np.all(ids[1:] > ids[:-1]) and (len(ids) == 0 or ids[-1] < nb[0] * nb[1] * nb[2])
    assert d.shape == (len(ids), 512) and w.shape == (len(ids), 512) and w.dtype == R.WEIGHT_DTYPES[bits]
    D2, W2, C2 = R.put(ids, d, w, c, size, FILL)
    assert bits_equal(D2, D) and bits_equal(W2, Wt)
    assert (C2 is None and Cl is None) or bits_equal(C2, Cl)
    # every brick left out is cleared, every brick kept has a voxel that is not
    ids_all, d_all, _, _ = R.take(D2, W2, size, FILL, bits, C2)
    assert np.array_equal(ids_all, ids) and bits_equal(d_all, d)


def test_padding_of_partial_bricks():
    size = (7, 9, 17)
    n = 7 * 9 * 17
    D = np.full(n, F32(-1.0), F32)      # every voxel live
    Wt = np.full(n, F32(3.0), F32)
    Cl = np.full(n, 0x01020304, U32)
    ids, d, w, c = R.take(D, Wt, size, FILL, 8, Cl)
    assert np.array_equal(ids, np.arange(1 * 2 * 3, dtype=U32))
    lx, ly, lz = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    for b in range(6):
        bx, by, bz = b % 1, (b // 1) % 2, b // 2
        for x, y, z in zip(lx.reshape(-1), ly.reshape(-1), lz.reshape(-1)):
            inside = 8 * bx + x < 7 and 8 * by + y < 9 and 8 * bz + z < 17
            at = x + 8 * y + 64 * z
            assert d[b, at] == (F32(-1.0) if inside else FILL)
            assert w[b, at] == (3 if inside else 0)
            assert c[b, at] == (0x01020304 if inside else 0)


def test_known_answers_on_9_8_8():
    size = (9, 8, 8)
    n = 9 * 8 * 8
    idx = lambda x, y, z: x + 9 * y + 72 * z
    D = np.full(n, FILL, F32)
    Wt = np.zeros(n, F32)
    # nothing live: no bricks
    ids, d, w, c = R.take(D, Wt, size, FILL, 8)
    assert len(ids) == 0 and d.shape == (0, 512) and c is None
    # one weight in brick 0 at (3, 2, 1); one distance an ulp from fill in brick 1 at (8, 7, 7)
    Wt[idx(3, 2, 1)] = 5.0
    D[idx(8, 7, 7)] = np.nextafter(FILL, F32(0.0))
    ids, d, w, c = R.take(D, Wt, size, FILL, 8)
    assert np.array_equal(ids, [0, 1])
    exp_w = np.zeros((2, 512), np.uint8)
    exp_w[0, 3 + 8 * 2 + 64 * 1] = 5
    exp_d = np.full((2, 512), FILL, F32)
    exp_d[1, 0 + 8 * 7 + 64 * 7] = np.nextafter(FILL, F32(0.0))
    assert bits_equal(w, exp_w) and bits_equal(d, exp_d)
    # brick 1 alone, by its only column
    Wt[idx(3, 2, 1)] = 0.0
    ids, d, w, c = R.take(D, Wt, size, FILL, 16)
    assert np.array_equal(ids, [1]) and w.dtype == np.uint16 and not w.any()
    # fp32 weights: -0.0 and NaN are not cleared, +0.0 is
    D[:] = FILL
    Wt[idx(0, 0, 0)] = F32(-0.0)
    ids, d, w, c = R.take(D, Wt, size, FILL, 32)
    assert np.array_equal(ids, [0]) and w.view(U32)[0, 0] == 0x80000000
    Wt[idx(0, 0, 0)] = 0.0
    Wt[idx(8, 0, 0)] = np.nan
    ids, d, w, c = R.take(D, Wt, size, FILL, 32)
    assert np.array_equal(ids, [1]) and np.isnan(w[0, 0])
    D2, W2, _ = R.put(ids, d, w, None, size, FILL)
    assert bits_equal(D2, D) and bits_equal(W2, Wt)
    # a colour word alone
    Wt[:] = 0.0
    Cl = np.zeros(n, U32)
    Cl[idx(7, 7, 7)] = 0x01000000
    ids, d, w, c = R.take(D, Wt, size, FILL, 8, Cl)
    assert np.array_equal(ids, [0]) and c[0, 511] == 0x01000000 and c.sum() == 0x01000000


@pytest.mark.parametrize("size", K.GRIDS)
def test_the_random_cases_of_the_gpu_tests_leave_bricks_out(size):
    """tests/test_snapshot.py asserts 0 < n_bricks < total on its random cases; the seeds are chosen so, which is checked here."""
    total = K.total_bricks(size)
    for bits in (8, 16, 32):
        for colour in (False, True):
            D, Wt, Cl = K.random_case(size, bits, colour)
            n = len(R.take(D, Wt, size, K.FILL, bits, Cl)[0])
            assert (n == 1) if total == 1 else (0 < n < total), (size, bits, colour, n, total)
    assert K.total_bricks((264, 64, 40)) == 1320 > 1024
