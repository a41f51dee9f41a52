"""GPU: the frame differences (include/tsdf_amd.h, "frame differences") against the CPU reference tests/frame_diff_ref.py.  Every output
-- states, counts, the list, labels, rows, blob index, mask, masked frame -- is compared byte for byte: the results are integers and
sets, so there is no tolerance anywhere."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import frame_diff_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (64, 1), (65, 2), (70, 3), (37, 29), (64, 48)]   # (width, height): one chunk, chunks that straddle rows, odd sides, many blocks
DEFAULT = dict(tolerance_mm=20, quadratic=0, connectivity=8, depth_step=30, min_pixels=2, dilate_px=1)


def device_run(frame, model, p, fd=None, outputs=("mask", "blob_index", "frame"), in_place=False, states=True):
    """compare, cluster and mask on the device through device pointers; returns what R.run returns, for the outputs asked for."""
    import tsdf_amd
    from tsdf_amd import _capi, api
    lib, check = _capi.lib, _capi.check
    fd = fd or tsdf_amd.FrameDiff()
    h, w = frame.shape
    n = w * h
    f, m = np.ascontiguousarray(frame, np.uint16), np.ascontiguousarray(model, np.uint16)
    out = {}
    A = api._DeviceArray
    with A(f) as df, A(m) as dm, A(nbytes=n) as ds, A(nbytes=n) as dmask, A(nbytes=4 * n) as dbi, A(nbytes=2 * n) as dfo:
        fd.compare_device(df.ptr.value, dm.ptr.value, w, h, p["tolerance_mm"], p["quadratic"], ds.ptr.value if states else 0)
        out["counts"] = fd.counts
        if states:
            out["states"] = np.empty((h, w), np.uint8)
            check(lib.tsdf_device_download(out["states"].ctypes.data, ds.ptr, n))
        fd.cluster(p["connectivity"], p["depth_step"], p["min_pixels"])
        out["pixels"], out["labels"], out["blobs"] = fd.pixels, fd.labels, fd.blobs
        out["info"] = fd.info
        fo = df if in_place else dfo
        fd.mask_device(p["dilate_px"], dmask.ptr.value if "mask" in outputs else 0, dbi.ptr.value if "blob_index" in outputs else 0,
                       df.ptr.value if "frame" in outputs else 0, fo.ptr.value if "frame" in outputs else 0)
        fd.device_buffers()   # (waits)
        for name, ptr, dtype in (("mask", dmask, np.uint8), ("blob_index", dbi, np.uint32), ("frame", fo, np.uint16)):
            if name in outputs:
                a = np.empty((h, w), dtype)
                check(lib.tsdf_device_download(a.ctypes.data, ptr.ptr, a.nbytes))
                out["frame_out" if name == "frame" else name] = a
    return out, fd


def assert_same(got, want, what=""):
    assert np.array_equal(got["counts"], want["counts"]), (what, got["counts"], want["counts"])
    assert int(got["counts"].sum()) == want["states"].size
    for k in ("states", "pixels", "labels", "mask", "blob_index", "frame_out"):
        if k in got:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
    assert got["blobs"].tobytes() == want["blobs"].tobytes(), (what, got["blobs"], want["blobs"])
    assert int(got["info"].n_blobs) == len(want["rows"]) and int(got["info"].n_kept_blobs) == len(want["blobs"]), what


def check_case(frame, model, fd=None, what="", **over):
    p = dict(DEFAULT, **over)
    got, fd = device_run(np.asarray(frame, np.uint16), np.asarray(model, np.uint16), p, fd)
    want = R.run(frame, model, **p)
    assert_same(got, want, what)
    return got, want, fd


def random_pair(w, h, seed, blobs=6):
    """A model with holes and a frame that agrees with it except for dropouts, noise, some farther pixels and `blobs` nearer patches."""
    rng = np.random.default_rng(seed)
    model = rng.integers(1500, 2500, (h, w)).astype(np.int64)
    model[rng.random((h, w)) < 0.1] = 0
    frame = model + rng.integers(-15, 16, (h, w))
    frame[model == 0] = rng.integers(0, 3000, int((model == 0).sum()))
    frame[rng.random((h, w)) < 0.05] = 0
    far = rng.random((h, w)) < 0.03
    frame[far] = model[far] + 400
    for _ in range(blobs):
        x, y, rx, ry = rng.integers(0, w), rng.integers(0, h), rng.integers(1, max(w // 6, 2)), rng.integers(1, max(h // 4, 2))
        frame[max(0, y - ry):y + ry, max(0, x - rx):x + rx] = rng.integers(600, 900)
    return np.clip(frame, 0, 65535).astype(np.uint16), model.astype(np.uint16)


@pytest.fixture(scope="module")
def handle():
    import tsdf_amd
    return tsdf_amd.FrameDiff()


@pytest.mark.parametrize("w,h", SIZES)
def test_random_images_at_every_size(w, h, handle):
    for seed, connectivity in ((1, 4), (2, 8)):
        frame, model = random_pair(w, h, seed * 1000 + w)
        got, want, _ = check_case(frame, model, handle, (w, h, seed), connectivity=connectivity)
    if w * h > 500:
        assert len(want["pixels"]) > 20 and len(want["blobs"]) >= 1 and want["counts"].min() > 0


def planted(w, h, nearer, depth=800, model_depth=2000):
    """A flat model and a frame equal to it except at the `nearer` pixels [(x, y) or (x, y, depth)]."""
    model = np.full((h, w), model_depth, np.uint16)
    frame = model.copy()
    for q in nearer:
        frame[q[1], q[0]] = q[2] if len(q) > 2 else depth
    return frame, model


def test_row_ends_do_not_join():
    w, h = 70, 3
    frame, model = planted(w, h, [(w - 2, 0), (w - 1, 0), (0, 1), (1, 1)])
    for connectivity in (4, 8):
        got, want, _ = check_case(frame, model, connectivity=connectivity, min_pixels=1, dilate_px=0)
        assert len(got["blobs"]) == 2 and got["blobs"]["size"].tolist() == [2, 2]
        assert got["blobs"]["hi"][0].tolist() == [w - 1, 0] and got["blobs"]["lo"][1].tolist() == [0, 1]


def test_diagonal_touch_at_both_connectivities():
    frame, model = planted(37, 29, [(5, 5), (6, 5), (7, 6), (8, 6)])
    got4, _, _ = check_case(frame, model, connectivity=4, min_pixels=1)
    got8, _, _ = check_case(frame, model, connectivity=8, min_pixels=1)
    assert len(got4["blobs"]) == 2 and len(got8["blobs"]) == 1 and int(got8["blobs"]["size"][0]) == 4


def test_a_blob_across_a_chunk_boundary_and_the_depth_step():
    # ids 60 .. 68 of a 70-wide image: one blob over the chunk boundary at id 64
    frame, model = planted(70, 3, [(x, 0) for x in range(60, 69)])
    got, _, _ = check_case(frame, model, min_pixels=1)
    assert len(got["blobs"]) == 1 and int(got["blobs"]["size"][0]) == 9 and int(got["blobs"]["sum_x"][0]) == sum(range(60, 69))
    # two overlapping objects: depths differ by exactly depth_step (one blob) and by depth_step + 1 (two)
    for gap, n_blobs in ((30, 1), (31, 2)):
        near = [(x, y, 800) for x in range(4, 10) for y in range(4, 10)] + [(x, y, 800 + gap) for x in range(10, 16) for y in range(6, 12)]
        frame, model = planted(37, 29, near)
        got, _, _ = check_case(frame, model, depth_step=30, min_pixels=1)
        assert len(got["blobs"]) == n_blobs, gap
    # depth_step >= 65535 joins any neighbours
    frame, model = planted(37, 29, [(3, 3, 1), (4, 3, 1900)])
    got, _, _ = check_case(frame, model, depth_step=65535, min_pixels=1)
    assert len(got["blobs"]) == 1


def test_min_pixels_and_one_fewer():
    near = [(x, 2) for x in range(2, 7)] + [(x, 10) for x in range(2, 6)]   # 5 and 4 pixels
    frame, model = planted(37, 29, near)
    got, _, _ = check_case(frame, model, min_pixels=5)
    assert got["blobs"]["size"].tolist() == [5] and int(got["info"].n_blobs) == 2
    got, _, _ = check_case(frame, model, min_pixels=0)   # max(min_pixels, 1)
    assert got["blobs"]["size"].tolist() == [5, 4]
    assert int((got["blob_index"] == 1).sum()) == 4


def test_every_pixel_listed_and_none():
    for w, h in ((65, 2), (64, 48)):
        model = np.full((h, w), 3000, np.uint16)
        got, _, fd = check_case(np.full((h, w), 500, np.uint16), model, min_pixels=1)
        assert len(got["pixels"]) == w * h and len(got["blobs"]) == 1 and got["mask"].all() and not got["frame_out"].any()
        got, _, _ = check_case(model, model, fd, min_pixels=1, dilate_px=32)   # an empty list: cluster and mask still run
        assert len(got["pixels"]) == 0 and len(got["blobs"]) == 0 and not got["mask"].any() and (got["blob_index"] == R.NO_BLOB).all()
        assert np.array_equal(got["frame_out"], model)


def test_the_extreme_values_and_the_tolerances():
    v = np.array([0, 1, 65535], np.uint16)
    frame, model = np.repeat(v, 3).reshape(1, 9), np.tile(v, 3).reshape(1, 9)
    for tolerance_mm, quadratic in ((0, 0), (1, 0), (65534, 0), (65535, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0, 0xFFFFFFFF), (0, 1 << 16), (3, 1 << 31)):
        check_case(frame, model, tolerance_mm=tolerance_mm, quadratic=quadratic, min_pixels=1, what=(tolerance_mm, quadratic))
    # at the tolerance and one either side, with a quadratic term that matters and one that saturates
    rng = np.random.default_rng(5)
    model = rng.integers(1, 65536, (29, 37)).astype(np.int64)
    for quadratic in (0, 1 << 12, 1 << 20, 0xFFFFFFFF):
        tol = R.tolerance(model, 10, quadratic)
        frame = np.clip(model + rng.choice([-1, 1], model.shape) * (tol + rng.integers(-1, 2, model.shape)), 0, 65535)
        got, want, _ = check_case(frame.astype(np.uint16), model.astype(np.uint16), tolerance_mm=10, quadratic=quadratic, min_pixels=1, what=quadratic)
    assert want["counts"][R.SAME] > 0


def test_dilation_at_every_border_and_corner():
    w, h = 70, 40
    spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2), (33, 17)]
    for dilate in (0, 1, 32):
        for spot in spots:
            frame, model = planted(w, h, [spot])
            got, _, _ = check_case(frame, model, min_pixels=1, dilate_px=dilate, what=(dilate, spot))
            x0, x1, y0, y1 = max(0, spot[0] - dilate), min(w - 1, spot[0] + dilate), max(0, spot[1] - dilate), min(h - 1, spot[1] + dilate)
            assert int(got["mask"].sum()) == (x1 - x0 + 1) * (y1 - y0 + 1)
        frame, model = planted(w, h, spots)
        check_case(frame, model, min_pixels=1, dilate_px=dilate, what=dilate)


def test_every_subset_of_the_outputs_and_in_place():
    frame, model = random_pair(64, 48, 77)
    want = R.run(frame, model, **DEFAULT)
    fd = None
    for k in range(4):
        for outputs in itertools.combinations(("mask", "blob_index", "frame"), k):
            for in_place in ((False, True) if "frame" in outputs else (False,)):
                for states in (False, True):
                    got, fd = device_run(frame, model, DEFAULT, fd, outputs, in_place, states)
                    assert set(got) >= set("frame_out" if o == "frame" else o for o in outputs)
                    assert_same(got, want, (outputs, in_place, states))


def test_three_hundred_blobs_and_two_runs():
    w, h = 128, 96
    rng = np.random.default_rng(300)
    model = np.full((h, w), 3000, np.uint16)
    frame = model.copy()
    cells = [(x, y) for y in range(1, h - 3, 4) for x in range(1, w - 3, 4)]
    for i in rng.choice(len(cells), 300, replace=False):
        x, y = cells[i]
        sx, sy = rng.integers(1, 4, 2)
        frame[y:y + sy, x:x + sx] = rng.integers(400, 2000)
    got, want, fd = check_case(frame, model, min_pixels=1, depth_step=65535, dilate_px=2)
    assert len(got["blobs"]) == 300
    again, _ = device_run(frame, model, dict(DEFAULT, min_pixels=1, depth_step=65535, dilate_px=2))
    for k in ("states", "pixels", "labels", "blobs", "mask", "blob_index", "frame_out"):
        assert again[k].tobytes() == got[k].tobytes(), k


def test_sixty_four_roots_in_a_wave_and_one_row_for_three_waves():
    """129 x 2, NEARER at even x on row 0 and odd x on row 1: 129 listed pixels in waves of 64, 64 and 1.  At connectivity 4 every pixel is
    its own blob (a wave reduces 64 distinct roots); at 8 the three waves all add to one row.  One compare, then both clusterings in
    either order on the same handle: the root counter is reset before the second."""
    import tsdf_amd
    from tsdf_amd import api
    w, h = 129, 2
    frame, model = planted(w, h, [(x, 0, 700 + x) for x in range(0, w, 2)] + [(x, 1, 900 + x) for x in range(1, w, 2)])
    p = dict(DEFAULT, depth_step=65535, min_pixels=1)
    want = {c: R.run(frame, model, **dict(p, connectivity=c)) for c in (4, 8)}
    assert len(want[4]["pixels"]) == 129 and len(want[4]["blobs"]) == 129 and len(want[8]["blobs"]) == 1
    for order in ((4, 8), (8, 4)):
        fd = tsdf_amd.FrameDiff()
        with api._DeviceArray(frame) as df, api._DeviceArray(model) as dm:
            fd.compare_device(df.ptr.value, dm.ptr.value, w, h, p["tolerance_mm"], p["quadratic"], 0)
            for c in order:
                fd.cluster(c, p["depth_step"], p["min_pixels"])
                got = dict(counts=fd.counts, pixels=fd.pixels, labels=fd.labels, blobs=fd.blobs, info=fd.info)
                assert_same(got, want[c], (order, c))
                assert int(got["info"].connectivity) == c and got["blobs"]["size"].sum() == 129
        fd.close()


def scratch_formula(calls):
    """The handle's scratch after `calls` [(pixels, listed)]: every array at the largest size it was asked for."""
    chunks = lambda n: (n + 63) // 64
    nc = max(chunks(n) for n, _ in calls)
    nl = max(l for _, l in calls)
    parts = max(2 * ((chunks(n) + 1023) // 1024 + 1) for n, _ in calls)
    return 8 * nc + 4 * nc + 8 * parts + 2 * max(n for n, _ in calls) + 8 * nc + 8 * 8 + 56 * nl + 8 * chunks(nl) + 4 * chunks(nl)


def test_a_warm_handle_small_large_small():
    import tsdf_amd
    warm, calls = tsdf_amd.FrameDiff(), []
    for w, h, seed in ((37, 29, 1), (128, 96, 2), (65, 2, 3), (37, 29, 1)):
        frame, model = random_pair(w, h, seed)
        got, want, _ = check_case(frame, model, warm, (w, h))
        fresh, _ = device_run(frame, model, DEFAULT)
        for k in ("states", "pixels", "labels", "blobs", "mask", "blob_index", "frame_out"):
            assert fresh[k].tobytes() == got[k].tobytes(), k
        calls.append((w * h, len(want["pixels"])))
        assert warm.scratch_bytes == scratch_formula(calls), calls


def test_refusals_with_a_handle():
    import tsdf_amd
    fd = tsdf_amd.FrameDiff()
    with pytest.raises(ValueError, match="holds no comparison"):
        fd.cluster()
    with pytest.raises(ValueError, match="has not been clustered"):
        fd.mask_device(0, 0, 0, 0, 0)
    frame, model = random_pair(37, 29, 4)
    fd.compare(frame, model)
    with pytest.raises(ValueError, match="has not been clustered"):
        fd.mask(1)
    with pytest.raises(ValueError, match="has not been clustered"):
        fd.blobs
    with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
        fd.cluster(connectivity=6)
    fd.cluster(min_pixels=1)
    with pytest.raises(ValueError, match="above 32"):
        fd.mask(33)
    m, f, b = fd.mask(2, frame=frame, blob_index=True)
    want = R.run(frame, model, 50, 0, 8, 50, 1, 2)
    assert np.array_equal(m, want["mask"]) and np.array_equal(f, want["frame_out"]) and np.array_equal(b, want["blob_index"])
    assert np.array_equal(fd.compare(frame, model, states=True).states, want["states"])
    with pytest.raises(ValueError, match="has not been clustered"):   # a compare forgets the clustering
        fd.mask(1)
