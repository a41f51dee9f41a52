"""The users of the band pass (tsdf_amd/csrc/band_pass.hpp) against each other: band_pass_kernel<STD, ColourBlend>, band_pass_kernel<STD,
ClassVote> and the colour update inside integrate_packed_colour_kernel must visit the same voxels.  Grids and cameras are aimed rows of
tests/class_cases.py; the frames are this file's: three per row, every pixel with a depth (a row's dropouts take its largest depth),
class 7 with no confidence image (strength 1) and an rgb without a zero byte.  Then a colour word's observation count and a class
word's votes both count the frames that met the voxel in the band, so on every voxel

    colour >> 24 == class >> 16,    and the class is 7 wherever there are votes,

once with fp32 weights (pinned through weight_data(), as tests/test_weight_storage.py pins them: colour is the separate pass) and once
with packed counts (the packed kernel makes the colour update itself), and the words of the two storages are equal.  Integers only.

ROWS covers: an x extent that is no multiple of 64 and a y extent that is no multiple of 4 (70 x 9 and 130 x 18), 33 and 37 planes (the
planes appended to the last brick layer) and 69, a camera inside the grid, a general camera (K(3,3) != 1: the kernels without STD, and
fp32 weights whatever the volume began with) and an odd image width.  The host twin below shows on tests/classes_ref.py alone that no
row is vacuous.
"""
import functools

import numpy as np
import pytest

from tests import class_cases as CC

U16, U32 = np.uint16, np.uint32
CLASS = 7
ROWS = (5, 7, 9, 10, 12, 17)     # image 65x40; 33, 37 and 69 planes; camera inside, turned; exact truncation distance through K(3,3) = 1.03


@functools.lru_cache(maxsize=None)
def cross_case(seed):
    """The row's volume and cameras without start words, with the three frames described above."""
    c = CC.case(seed)
    rng = np.random.default_rng(0xBA9D + seed)
    frames = []
    for i in range(3):
        f = c["frames"][i % len(c["frames"])]
        n = f["width"] * f["height"]
        depth = np.where(f["depth"] == 0, max(int(f["depth"].max()), 1), f["depth"]).astype(U16)
        frames.append({"depth": depth, "classes": np.full(n, CLASS, U16), "confidence": None,
                       "rgb": rng.integers(1, 256, (n, 3)).astype(np.uint8), "cam": f["cam"], "width": f["width"], "height": f["height"]})
    return dict(c, start=None, colour=True, frames=frames)


def test_the_rows_are_the_ones_the_band_pass_can_go_wrong_on():
    cases = [cross_case(s) for s in ROWS]
    assert any(c["dims"][0] % 64 for c in cases) and any(c["dims"][1] % 4 for c in cases)
    assert {33, 37, 69} <= {c["dims"][2] for c in cases}
    assert any("behind_camera" in c["claims"] for c in cases)
    assert any(c["kind"] is not None for c in cases) and any(c["kind"] is None for c in cases)
    assert any(f["width"] % 2 for c in cases for f in c["frames"])
    assert all(f["depth"].all() and f["rgb"].all() and f["confidence"] is None for c in cases for f in c["frames"])


def test_no_row_is_vacuous_on_the_reference(oracle):
    """Per row: at least 100 voxels in the band; a voxel the distance update wrote that never was in the band, so the band is narrower
    than the update set; and among the rows one whose band reaches the planes appended to the last brick layer."""
    appended = 0
    for seed in ROWS:
        c = cross_case(seed)
        ref = CC.Reference(oracle, c, distances=False)
        updated = np.zeros(len(ref.centres), bool)
        for f in c["frames"]:
            updated |= ref.apply(f)["updated"]
        what = "seed %d (%s)" % (seed, c["name"])
        assert int(ref.voted.sum()) >= 100, what
        assert (updated & ~ref.voted).any(), what
        assert not (ref.voted & ~updated).any(), what
        votes = ref.words >> U32(16)
        assert np.all(votes[ref.voted] >= 1) and not votes[~ref.voted].any() and np.all((ref.words & U32(0xFFFF))[ref.voted] == CLASS), what
        Z = c["dims"][2]
        if Z // CC.CHUNK_Z >= 1 and 1 <= Z % CC.CHUNK_Z <= 4:
            appended += int(ref.voted.reshape(Z, -1)[Z - Z % CC.CHUNK_Z:].any())
    assert appended >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("seed", ROWS)
def test_colour_counts_are_class_votes_on_both_weight_storages(seed):
    from tests.helpers import Cam
    from tests.test_class_fuzz import _volume
    c = cross_case(seed)
    what = "seed %d (%s)" % (seed, c["name"])
    words = {}
    for storage in ("fp32", "packed"):
        v = _volume(c)
        try:
            v.enable_colour()
            v.enable_classes()
            if storage == "fp32":
                assert v.weight_data()
            for f in c["frames"]:
                v.integrate_classes(f["depth"], f["classes"], f["width"], f["height"], Cam(*f["cam"]), rgb=f["rgb"])
            assert v.weight_storage()[0] == (8 if storage == "packed" and c["kind"] is None else 32), what
            colour, cls = v.get_colour_data(), v.get_class_data()
        finally:
            v.close()
        votes = cls >> U32(16)
        bad = np.flatnonzero((colour >> U32(24)) != votes)
        assert not bad.size, "%s, %s: %d voxels, first %d: colour %08x, class %08x" % (what, storage, bad.size, bad[0], colour[bad[0]], cls[bad[0]])
        assert int((votes != 0).sum()) >= 100 and int(votes.max()) >= 2, what
        assert np.all((cls & U32(0xFFFF))[votes != 0] == CLASS) and not cls[votes == 0].any(), what + ", " + storage
        words[storage] = (colour, cls)
    assert np.array_equal(words["fp32"][0], words["packed"][0]), what + ": colour words of the two storages"
    assert np.array_equal(words["fp32"][1], words["packed"][1]), what + ": class words of the two storages"
