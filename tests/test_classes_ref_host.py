"""The vote rule of class fusion (include/tsdf_amd.h, "class fusion") in tests/classes_ref.py, checked on hand-made words, and
synth.class_frame against the analytic scene (no GPU needed)."""
import hashlib

import numpy as np

from tests import classes_ref as R
from tsdf_amd import synth

W = R.word


def one(old, k, s):
    return int(R.vote(np.array([old], np.uint32), np.array([k], np.uint16), np.array([s], np.uint32))[0])


def test_the_five_branches_of_the_vote():
    assert one(0, 7, 3) == W(7, 3)                       # n == 0          -> (k, s)
    assert one(W(7, 3), 7, 4) == W(7, 7)                 # c == k          -> (k, n + s)
    assert one(W(7, 9), 2, 4) == W(7, 5)                 # c != k, n >  s  -> (c, n - s)
    assert one(W(7, 4), 2, 4) == 0                       # c != k, n == s  -> the unclassified word
    assert one(W(7, 1), 2, 255) == W(2, 254)             # c != k, n <  s  -> (k, s - n)
    assert one(0, 0, 1) == W(0, 1) == 0x00010000         # class 0 is a class: its word is not the unclassified one
    assert one(W(0, 1), 0, 1) == W(0, 2) and one(W(0, 1), 5, 1) == 0


def test_void_and_zero_strength_leave_words_alone():
    for old in (0, W(7, 3), W(0, 1), W(65534, 65535)):
        assert one(old, R.VOID, 200) == old
        assert one(old, 7, 0) == old and one(old, 3, 0) == old


def test_votes_saturate_at_65535():
    assert one(W(9, 65535), 9, 1) == W(9, 65535)
    assert one(W(9, 65400), 9, 255) == W(9, 65535)
    assert one(W(9, 65280), 9, 255) == W(9, 65535)
    assert one(W(9, 65279), 9, 255) == W(9, 65534)
    assert one(W(9, 65535), 4, 255) == W(9, 65280)


def test_null_confidence_is_all_ones_and_zero_votes_mean_the_zero_word():
    rng = np.random.default_rng(11)
    n, pixels = 5000, 4096
    words = np.where(rng.random(n) < 0.3, 0, rng.integers(0, 5, n) | (rng.integers(1, 4, n) << 16)).astype(np.uint32)
    voted = rng.random(n) < 0.7
    pidx = rng.integers(0, pixels, n)
    for step in range(40):
        classes = np.where(rng.random(pixels) < 0.1, R.VOID, rng.integers(0, 5, pixels)).astype(np.uint16)
        conf = rng.integers(0, 4, pixels).astype(np.uint8)
        a = R.apply_votes(words, voted, pidx, classes, None)
        b = R.apply_votes(words, voted, pidx, classes, np.ones(pixels, np.uint8))
        assert np.array_equal(a, b)
        assert np.array_equal(a[~voted], words[~voted])
        words = R.apply_votes(words, voted, pidx, classes, conf)
        assert not np.any(((words >> 16) == 0) & (words != 0)), "a word without votes must be 0x00000000"
    assert np.any(words == 0) and np.any(words != 0)


def test_counts_and_sample_on_a_tiny_grid():
    dims = (3, 2, 2)
    geom = (dims, np.array([10, 10, 10], np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), np.float32(30))
    words = np.array([W(1, 1), W(1, 3), 0, W(2, 5), W(9, 2), W(0, 1), 0, 0, W(1, 2), 0, 0, W(2, 1)], np.uint32)
    assert R.counts(words, 4).tolist() == [1, 3, 2, 0]
    assert R.counts(words, 4, 0).tolist() == [1, 3, 2, 0]            # min_votes 0 counts as 1: unclassified words are never counted
    assert R.counts(words, 4, 3).tolist() == [0, 1, 1, 0]
    assert R.counts(words, 1).tolist() == [1] and R.counts(words, 10)[9] == 1
    pts = np.array([[5, 5, 5], [15, 5, 5], [25, 5, 5], [5, 15, 5], [25, 15, 15], [np.nan, 5, 5], [-1, 5, 5], [30, 5, 5]], np.float32)
    c, n = R.sample(words, geom, pts)
    assert c.tolist() == [1, 1, R.VOID, 2, 2, R.VOID, R.VOID, R.VOID] and n.tolist() == [1, 3, 0, 5, 1, 0, 0, 0]


def test_class_frame_is_the_object_map_of_the_trace():
    assert (synth.WALL_CLASS, synth.SPHERE_CLASS, synth.BOX_CLASS, synth.CLASS_VOID) == (1, 2, 3, 0xFFFF)
    for i, n, inside in ((0, 200, False), (5, 40, False), (3, 40, True)):
        classes, cam = synth.class_frame(i, n, seed=0x5EED0003, inside=inside)
        assert classes.dtype == np.uint16 and classes.shape == (synth.WIDTH * synth.HEIGHT,)
        z = synth.trace_depth(cam).reshape(-1)
        assert np.array_equal(classes == synth.CLASS_VOID, ~np.isfinite(z))
        assert set(np.unique(classes)) <= {1, 2, 3, 0xFFFF}
        blue = synth.trace_colour(cam)[:, 2]
        for b, k in ((synth.WALL_B, 1), (synth.SPHERE_B, 2), (synth.BOX_B, 3)):
            assert np.array_equal(classes == k, blue == b)
    assert set(np.unique(synth.class_frame(0, 200, seed=0)[0])) >= {1, 2, 3}


def test_depth_and_colour_frames_are_the_bytes_they_were():
    """sha256 of depth_frame / colour_frame outputs, taken at the commit before class_frame was added."""
    pins = {0: ("fcdbd4f56845e432afad349f04e4b5721669a1c8cb75a79ea062dafee13e2d20", "a58f07625a84d702b7c61b2ec294bb6b32999ee6d25afe56fc09519165285ed2"),
            1: ("cb2d03f5a659816b5083e1daf308198045e89b08690b32bacf58dc563d885d84", "51b9a342cf33193565d2d5de503ba8bcb1d1f1f090d6b6aa37ea2b3bda604928"),
            7: ("fcd830be0635004a175d757f429ee12649b9dd3fa9aec28dcd2b393d29c542b0", "6328bfa78aa6026cae009f5622f9734e74816e6745c40c57a46e13be73693bf4")}
    sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
    for i, (hd, hc) in pins.items():
        assert sha(synth.depth_frame(i, 200, seed=0x5EED0003)[0]) == hd
        assert sha(synth.colour_frame(i, 200, seed=0x5EED0003)[0]) == hc
    assert sha(synth.depth_frame(3, 40, seed=0x5EED0001, inside=True)[0]) == "9fc9ee364cc6e1411bf8bd55855a2993a8e327461867658cb343bd427618ef9f"
    assert sha(synth.colour_frame(3, 40, seed=0x5EED0001, inside=True)[0]) == "69e8b578b242dc7cd08f73608c262c9b01dbc7c203a1f5cab038fb53369464be"
