"""Host (no GPU): the cases of tests/class_cases.py reach what they are aimed at.  Every case runs on the CPU reference alone
(tests/classes_ref.py over the oracle's pinned transforms), every vote is classified by its outcome -- silent (VOID or s == 0), first
(n == 0), same class, saturating (n + s > 65535), lead kept, tie, take-over -- and

  1. every aimed row holds its claims: a vote cast; the width's parity; a vote in each of the last four planes (and the planes riding as
     z_extra where the row says so); voxels behind the camera in a brick that also votes; the word of the voxel under the camera; voxels
     with sdf == +trunc and == -trunc that vote beside ones just outside that do not; every start count and every strength of the sweep;
  2. over the 36 drawn seeds, as caps against vacuity: at least 30 scenes cast a vote, each of the seven outcomes occurs in at least 12
     scenes, at least 4 general-camera scenes vote.  (With default_rng(0xC1A55 + seed): 36 scenes vote, 15 of them through a general
     camera; silent 35, first 36, same 27, saturate 17, lead 23, tie 21, take-over 23.  The whole survey takes under a second.)
  3. the drawn seeds are what the issue describes: the planes of every fifth seed, the moved offsets, the start words, rgb and the device
     variant by seed, growing images within a device case;
  4. three plausible defects of band_pass_kernel and ClassVote, switched into the reference (class_cases.MUTANTS), change the final words of
     the cases aimed at them and of at least one drawn seed: sdf < trunc for <=, the appended planes left out of the z bound, a
     vote count that wraps at 16 bits;
  5. classify() agrees with the vote rule of tests/classes_ref.py on every (n, s) of a grid round the edges.
"""
import numpy as np
import pytest

from tests import class_cases as CC
from tests import classes_ref as R

U32 = np.uint32
BRICK = (64, 4, 32)


@pytest.fixture(scope="module")
def runs(oracle):
    """seed -> (case, Reference after every frame, the per-frame results): computed once, shared and left unchanged."""
    out = {}
    for seed in CC.SEEDS:
        c = CC.case(seed)
        ref = CC.Reference(oracle, c, distances=False)
        out[seed] = (c, ref, [ref.apply(f) for f in c["frames"]])
    return out


def _cast(results):
    """Votes that were not silent."""
    return sum(int((r["outcome"] != 0).sum()) for r in results)


@pytest.mark.parametrize("seed", range(CC.N_AIMED))
def test_an_aimed_row_holds_its_claims(oracle, runs, seed):
    c, ref, results = runs[seed]
    X, Y, Z = c["dims"]
    assert c["claims"], "an aimed row without a claim"
    for claim in c["claims"]:
        what = "seed %d (%s): %s" % (seed, c["name"], claim)
        if claim == "voted":
            assert _cast(results) >= 1, what
        elif claim in ("odd_width", "even_width"):
            assert all(f["width"] % 2 == (claim == "odd_width") for f in c["frames"]), what
        elif claim == "last_planes":
            wrote = (ref.words != (0 if c["start"] is None else c["start"])).reshape(Z, -1)
            assert all(wrote[z].any() for z in range(Z - 4, Z)), what
        elif claim == "z_extra":
            assert Z // CC.CHUNK_Z >= 1 and 1 <= Z % CC.CHUNK_Z <= 4, what
        elif claim == "behind_camera":
            cam_z = oracle.world_to_camera_n(ref.centres, c["frames"][0]["cam"][1])[:, 2]
            behind = cam_z < 0
            assert behind.sum() > 1000 and (~behind).sum() > 1000, what
            z, y, x = np.unravel_index(np.arange(X * Y * Z), (Z, Y, X))
            brick = (x // BRICK[0]) + 100 * (y // BRICK[1]) + 10000 * (z // BRICK[2])
            assert np.intersect1d(brick[behind], brick[ref.voted]).size >= 1, what + ": no brick straddles the camera plane and votes"
            assert not (ref.voted & behind).any(), what
        elif claim == "centre_word":
            at, r = c["aim"]["voxel"], results[0]
            assert r["voted"][at] and r["pidx"][at] == 0, what
            assert int(ref.words[at]) == c["aim"]["word"], what
        elif claim == "exact_trunc":
            trunc = ref.geom[4]
            assert trunc == 60.0
            for f, r in zip(c["frames"], results):
                sdf, _ = CC.voxel_sdf(oracle, ref.centres, f)
                for name, group, votes in (("+trunc", sdf == trunc, True), ("-trunc", sdf == -trunc, True),
                                           ("just above", (sdf > trunc) & (sdf <= trunc + 2), False),
                                           ("just below", (sdf < -trunc) & (sdf >= -trunc - 2), False)):
                    assert group.any(), what + ": no voxel " + name
                    assert np.all(r["voted"][group] == votes), what + ": " + name
                spoke = np.zeros(len(sdf), bool)
                spoke[r["idx"][r["outcome"] != 0]] = True
                assert (spoke & (sdf == trunc)).any() and (spoke & (sdf == -trunc)).any(), what + ": no vote on the band's edge"
        elif claim == "surface_ulp":
            f = c["frames"][0]
            sdf, d = CC.voxel_sdf(oracle, ref.centres, f)
            exact = d.astype(np.float32) - (20 * (np.arange(X * Y * Z) // (X * Y)) + 844).astype(np.float32)
            assert ((np.abs(exact) == 60.0) & (sdf != exact) & (d > 0)).any(), what
        elif claim == "sweep":
            old_n = np.concatenate([r["old"] >> U32(16) for r in results])
            assert set(CC.SWEEP_VOTES.tolist()) <= set(np.unique(old_n).tolist()), what + ": start counts"
            assert set(np.unique(results[0]["s"]).tolist()) == set(range(256)), what + ": strengths"
            assert ref.reached() == set(CC.OUTCOMES), what
            r = results[0]
            edge = (r["outcome"] == 3)
            below = (r["outcome"] == 2) & ((r["old"] >> U32(16)) + r["s"] >= 65535 - 255)      # within one strength of the edge, not over it
            assert edge.sum() >= 100 and below.sum() >= 10, what + ": the saturation edge"
            assert ((r["outcome"] == 5) & (r["s"] <= 255)).sum() >= 3, what + ": ties"
        else:
            raise AssertionError("unknown claim %r" % claim)


def test_the_aimed_rows_are_the_ones_the_gaps_ask_for():
    cases = [CC.case(s) for s in range(CC.N_AIMED)]
    images = {(f["width"], f["height"]) for c in cases for f in c["frames"]}
    assert {(1, 1), (1, 37), (57, 1), (63, 5), (64, 48), (65, 40)} <= images
    planes = {c["dims"][2] for c in cases if "last_planes" in c["claims"]}
    assert planes == {32, 33, 36, 37, 69}
    assert all(c["dims"][0] % 64 and c["dims"][1] % 4 for c in cases if "last_planes" in c["claims"])
    inside = [c for c in cases if "behind_camera" in c["claims"]]
    assert len(inside) == 3 and all(-(-c["dims"][0] // 64) >= 3 and -(-c["dims"][1] // 4) >= 3 and -(-c["dims"][2] // 32) >= 2 for c in inside)
    assert [c["aim"]["voxel"] for c in cases if "centre_word" in c["claims"]][-1] == 0
    assert sorted(c["kind"] or "standard" for c in cases if "exact_trunc" in c["claims"]) == ["k33", "standard"]
    assert sum("sweep" in c["claims"] for c in cases) == 1


def test_the_drawn_seeds_are_not_vacuous(runs):
    voting = general = 0
    scenes = dict.fromkeys(CC.OUTCOMES, 0)
    for seed in CC.DRAWN:
        c, ref, results = runs[seed]
        cast = _cast(results) >= 1
        voting += cast
        general += bool(cast and c["kind"])
        for o in ref.reached():
            scenes[o] += 1
    print("\nclass cases, drawn seeds: %d scenes vote, %d through a general camera; scenes by outcome %s" % (voting, general, scenes))
    assert len(CC.DRAWN) == 36
    assert voting >= 30
    assert all(m >= 12 for m in scenes.values()), scenes
    assert general >= 4


def test_the_drawn_seeds_follow_the_draw():
    appended = short = 0
    for j, seed in enumerate(CC.DRAWN):
        c = CC.case(seed)
        X, Y, Z = c["dims"]
        assert all(5 <= s <= 72 for s in (X, Y)) and 1 <= len(c["frames"]) <= 4
        if j % 5 == 1:
            assert Z // 32 in (1, 2) and 1 <= Z % 32 <= 4
            appended += 1
        elif j % 5 == 3:
            assert Z < 32
            short += 1
        assert (c["bake"] is not None) == (c["move"] is not None) == (j % 3 == 0)
        assert (c["start"] is not None) == (j % 2 == 1)
        assert c["colour"] == (j % 4 == 1 or j % 8 == 7) and c["device"] == (j % 4 == 3)
        assert c["kind"] == CC.KINDS[j % 12]
        sizes = [f["width"] * f["height"] for f in c["frames"]]
        assert all(1 <= f["width"] <= 230 and 1 <= f["height"] <= 180 for f in c["frames"])
        if c["device"]:
            assert len(sizes) >= 2 and all(b > a for a, b in zip(sizes, sizes[1:]))
        for f in c["frames"]:
            assert set(np.unique(f["classes"]).tolist()) <= set(CC.CLASSES.tolist()) | {CC.VOID}
            assert (f["rgb"] is not None) == c["colour"]
        if c["start"] is not None:
            n = c["start"] >> U32(16)
            assert ((n == 0) & (c["start"] != 0)).any() and (n >= 65026).any() and ((n >= 1) & (n <= 3)).any()
    assert appended >= 7 and short >= 7
    assert sum(all(f["confidence"] is None for f in CC.case(s)["frames"]) for s in CC.DRAWN) >= 4


def test_a_case_is_the_same_case_every_time():
    for seed in (0, CC.N_AIMED - 1, CC.N_AIMED + 5):
        a = CC.case(seed)
        CC.case.cache_clear()
        b = CC.case(seed)
        assert a["dims"] == b["dims"] and (a["start"] is None or np.array_equal(a["start"], b["start"]))
        for f, g in zip(a["frames"], b["frames"]):
            assert all(np.array_equal(f[k], g[k]) for k in ("depth", "classes")) and all(np.array_equal(x, y) for x, y in zip(f["cam"], g["cam"]))


@pytest.mark.parametrize("mutant", CC.MUTANTS)
def test_a_defect_of_the_kernel_changes_the_words_of_the_cases_aimed_at_it(oracle, runs, mutant):
    def differs(seed):
        c, ref, _ = runs[seed]
        m = CC.Reference(oracle, c, distances=False, mutant=mutant)
        for f in c["frames"]:
            m.apply(f)
        return not np.array_equal(m.words, ref.words)
    aimed = {"open_band": "exact_trunc", "no_z_extra": "z_extra", "wrapping_add": "sweep"}[mutant]
    rows = [s for s in range(CC.N_AIMED) if aimed in CC.case(s)["claims"]]
    assert rows and all(differs(s) for s in rows), "%s: not every row aimed at it sees it" % mutant
    assert any(differs(s) for s in CC.DRAWN), "%s: no drawn seed sees it" % mutant


def test_classify_agrees_with_the_vote_rule():
    n = np.concatenate([np.arange(0, 300), np.arange(65200, 65536)]).astype(U32)
    s = np.arange(0, 256, dtype=U32)
    nn, ss = [a.reshape(-1) for a in np.meshgrid(n, s, indexing="ij")]
    for c, k in ((4, 4), (4, 9), (0, 0), (65534, 0), (0, CC.VOID)):
        old = (U32(c) | (nn << U32(16))).astype(U32)
        new = R.vote(old, np.full(nn.size, k, np.uint16), ss)
        o = CC.classify(old, np.full(nn.size, k), ss)
        n64, s64 = nn.astype(np.int64), ss.astype(np.int64)
        want = {0: old, 1: U32(k) | (ss << U32(16)), 2: U32(k) | ((nn + ss) << U32(16)), 3: np.full(nn.size, U32(k) | U32(65535 << 16)),
                4: U32(c) | ((n64 - s64).clip(0).astype(U32) << U32(16)), 5: np.zeros(nn.size, U32), 6: U32(k) | ((s64 - n64).clip(0).astype(U32) << U32(16))}
        for code, words in want.items():
            sel = o == code
            assert np.array_equal(new[sel], np.broadcast_to(words, new.shape)[sel].astype(U32)), (c, k, CC.OUTCOMES[code])
