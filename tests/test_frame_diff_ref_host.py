"""tests/frame_diff_ref.py against brute force on tiny images (no GPU): every mask of a 4 x 3 image at both connectivities against a
transitive closure of the adjacency relation, the state rule at |f - m| == tol and tol +- 1, the tolerance at the ends of its range,
and the dilation against its definition."""
import itertools

import numpy as np

from tests import frame_diff_ref as R


def closure_labels(listed, depth, connectivity, step):
    """Components by the transitive closure of "neighbours in the image and near in depth", as a boolean matrix power."""
    h, w = listed.shape
    ids = [int(p) for p in np.flatnonzero(listed.reshape(-1))]
    n = len(ids)
    A = np.eye(n, dtype=bool)
    for i, p in enumerate(ids):
        for j, q in enumerate(ids):
            dx, dy = abs(p % w - q % w), abs(p // w - q // w)
            near = max(dx, dy) == 1 and (connectivity == 8 or dx + dy == 1)
            if near and abs(int(depth[p // w, p % w]) - int(depth[q // w, q % w])) <= step:
                A[i, j] = True
    for _ in range(max(n, 1).bit_length()):
        A = (A.astype(np.uint8) @ A.astype(np.uint8)) > 0
    return np.array([int(np.flatnonzero(A[i])[0]) for i in range(n)], np.uint32), A


def test_every_mask_of_a_4_by_3_image_against_the_transitive_closure():
    w, h = 4, 3
    depth = np.full((h, w), 1000, np.uint16)
    for connectivity in (4, 8):
        for bits in range(1 << (w * h)):
            listed = np.array([(bits >> k) & 1 for k in range(w * h)], bool).reshape(h, w)
            pixels, labels, rows, kept = R.cluster(listed, depth, connectivity, 0, 2)
            want, A = closure_labels(listed, depth, connectivity, 0)
            assert np.array_equal(labels, want), (connectivity, bits)
            assert np.array_equal(pixels, np.flatnonzero(listed.reshape(-1)))
            sizes = {int(l): int((want == l).sum()) for l in set(want.tolist())}
            assert [(int(r["label"]), int(r["size"])) for r in rows] == sorted(sizes.items())
            assert [int(r["label"]) for r in kept] == [l for l, s in sorted(sizes.items()) if s >= 2]


def test_the_depth_rule_and_the_rows_on_a_small_image():
    rng = np.random.default_rng(7)
    for connectivity in (4, 8):
        for _ in range(40):
            listed = rng.random((5, 6)) < 0.6
            depth = rng.integers(1, 4, (5, 6)).astype(np.uint16) * 10
            pixels, labels, rows, kept = R.cluster(listed, depth, connectivity, 10, 1)
            want, _ = closure_labels(listed, depth, connectivity, 10)
            assert np.array_equal(labels, want)
            for r in rows:
                mem = pixels[labels == r["label"]].astype(np.int64)
                xs, ys, ds = mem % 6, mem // 6, depth.reshape(-1)[mem].astype(np.int64)
                assert tuple(r["lo"]) == (xs.min(), ys.min()) and tuple(r["hi"]) == (xs.max(), ys.max())
                assert (r["min_depth"], r["max_depth"]) == (ds.min(), ds.max())
                assert (r["sum_x"], r["sum_y"], r["sum_depth"], r["size"]) == (xs.sum(), ys.sum(), ds.sum(), mem.size)


def test_the_state_rule_at_the_tolerance_and_one_either_side():
    tol = 50
    for m in (1000, 51, 65535):
        for d in (tol - 1, tol, tol + 1):
            for sign in (-1, 1):
                f = m + sign * d
                if not 0 < f <= 65535:
                    continue
                s = int(R.states(np.array([[f]]), np.array([[m]]), tol, 0)[0, 0])
                want = R.SAME if d <= tol else (R.NEARER if sign < 0 else R.FARTHER)
                assert s == want, (f, m, d)
    grid = np.array([0, 1, 65535])
    s = R.states(grid[:, None] * np.ones((1, 3), int), np.ones((3, 1), int) * grid[None, :], 0, 0)
    assert s.tolist() == [[R.NO_FRAME] * 3, [R.NO_MODEL, R.SAME, R.NEARER], [R.NO_MODEL, R.FARTHER, R.SAME]]
    assert R.counts(s).tolist() == [3, 2, 2, 1, 1]


def test_the_tolerance_at_the_ends_of_its_range():
    q = 2 ** 32 - 1
    assert int(R.tolerance(np.array([65535]), 0, q)[0]) == 65535                       # 65535^2 * (2^32 - 1) >> 32 = 4294836224: saturated
    assert int(R.tolerance(np.array([255]), 0, q)[0]) == (q * 255 * 255) >> 32 == 65024
    assert int(R.tolerance(np.array([1000]), 7, 0)[0]) == 7
    assert int(R.tolerance(np.array([0]), 2 ** 32 - 1, q)[0]) == 65535
    assert int(R.tolerance(np.array([4000]), 10, 1 << 12)[0]) == 10 + ((4000 * 4000) >> 20)
    # f + tol at 65535 + 65535: no wrap
    assert int(R.states(np.array([[65535]]), np.array([[65535]]), 65535, 0)[0, 0]) == R.SAME
    assert int(R.states(np.array([[1]]), np.array([[65535]]), 65533, 0)[0, 0]) == R.NEARER


def test_the_dilation_against_its_definition():
    rng = np.random.default_rng(11)
    for h, w in ((1, 1), (3, 7), (9, 5), (12, 12)):
        for radius in (0, 1, 2, 5, 32):
            k = rng.random((h, w)) < 0.08
            got = R.dilate(k, radius)
            want = np.zeros((h, w), np.uint8)
            for y, x in itertools.product(range(h), range(w)):
                want[y, x] = k[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1].any()
            assert np.array_equal(got, want), (h, w, radius)
