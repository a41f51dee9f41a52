"""No GPU: the cases (tests/weighted_cases.py) and sequences (tests/weighted_sequences.py) that tests/test_weighted_fuzz.py drives through
the library test something -- shown from the CPU reference alone.

1. The cases.  Conditions on the 48 cases (20 aimed, 28 drawn from seed base 0x3E16), computed from the model alone.  Achieved (asserted
   below, each at or above its condition):
   every image shape, grid, prior state and switch of the list in at least two seeds -- width odd in 31 seeds and even in 29 (a device
   variant's images change parity as they grow), 1 x N in 3 and 10, N x 1 in 11 and 14, 2 x 2 in 5 and 13, width 63 in 0 and 7, 64 in
   1, 8, 11, 15, 65 in 2 and 9; the grids (65, 9, 33) in 0 and 7, (130, 5, 8) in 1 and 8, (16, 16, 16) in 2, 9, 17, (72, 12, 40) with its
   offset in 3 and 10; kChunkZ + 1 = 33 planes in 2 seeds, kChunkZ + kBatchZ = 36 in 9, kChunkZ + kBatchZ + 1 = 37 in 2; prior state
   cleared in 13 seeds, counts <= 255 in 7, counts in 256..65535 in 7, 16 bits by set_weight_storage in 7, uploaded fp32 weights in 7,
   pinned in 7; cap 0 in 18 seeds, 1 in 9, 3 in 8, 300 in 13; counting on in 31 and off in 17; colour in 8, a skewed K in 9, explicit
   nodes in 5, two slabs in 4; 1 weighted frame in 3 seeds, 2 in 32, 3 in 13; a plain frame before the last weighted one in 18 seeds,
   a removal in 3 (21 of 48: a third asked for); the device variant in 12;
   the aimed properties, each asserted in the seeds that claim it: a brick whose pixel box exceeds kTilePixels in seed 6 (8960 pixels;
   >= 1 seed); a skipped weight store -- fl(w + p) has the bits of w while the distance changes -- on 16 voxels and more in seeds 4 and
   12 (>= 2); a subnormal pixel weight that updates a voxel in 4, 6, 7 (>= 2); a NaN prior weight inside the frame's voxel set in 4
   and 12 (>= 2); a removal that meets 0 < w < 1 and one that leaves 0 < w - 1 < 1 in 12 and 17 (>= 2 each); FLT_MAX in the pixel
   weights of exactly seeds 16 and 18, both ending with 16 and more infinite weights and NaN distances;
   0 of 48 cases update fewer than 16 voxels over their frames (<= 10 %); 64 of 93 final ray casts hit 50 pixels or more (>= 60 %).
2. The sequences.  12 sequences of 10 to 13 ops (10 to 14 asked for); all 19 ordered pairs of a weighted writer with the nine writer kinds
   and itself; a weighted frame between prepare and its integrate in sequences 5 and 6 (>= 2), the model the same either way; a
   weighted frame that finds 8-bit storage in 10 sequences and 16-bit in 1, 6, 9 (>= 1 each); an 8-bit snapshot restored between two
   weighted frames in sequence 0; a snapshot of fractional fp32 weights restored after a clear in 1 and 6; a remove after weighted
   frames in 6 sequences; cap on, weighted, cap off, remove in 2, 7, 9, 10; rays and a fuse onto fractional weights under a cap in 2 and
   9; one refused depth_weighted_colour (sequence 4); a ray cast straight behind a weighted frame in 11 sequences (>= 4); 42 of 42
   weighted frames change 16 voxels or more; 16 of 17 ray casts hit 50 pixels or more.
3. Sensitivity: the model with one defect of integrate_weighted at a time ends at least two sequences and three cases in another state
   than the true model.  Achieved: a cap that clamps the divisor as well: sequences 2, 7, 9, 10 and 30 cases; a pixel of invalid
   weight that still colours its voxels: sequences 8, 10 and cases 7, 14, 26, 27, 32, 41, 43, 47; the weight of pixel (px + 1, py):
   all 12 sequences and 47 cases (all but seed 10, whose images are one pixel wide).
4. The weight models' cases: with the cosine flag (flags 2 and 3, either kinv) every weight is 0 below 3 x 3 and positive pixels number
   1 at 3 x 3, 115 at 63 x 5, 89 at 64 x 4, 214 at 65 x 6, 102 at 129 x 3, 1090 at 200 x 9.

The whole file takes 8 s on 16 host cores, the oracle work included.
"""
import functools

import numpy as np
import pytest

from tests import deintegrate_ref
from tests import op_sequences as S
from tests import weighted_cases as WC
from tests import weighted_ref as R
from tests import weighted_sequences as WS
from tests.helpers import Cam
from tests.volume_model import WEIGHTED_MUTANTS, ModelRun, Refused

F32, U32 = np.float32, np.uint32


def _bits(a):
    return np.asarray(a, F32).view(U32)


def _same_state(a, b):
    if a is None or b is None:
        return False
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(np.asarray(x).view(U32), np.asarray(y).view(U32)))
               for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def _oracle():
    import oracle as O
    O.build()
    return O


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _largest_box(c, in_set, pidx, width):
    """The largest pixel box the updated voxels of one integrate brick use (tests/test_weighted.py's measure)."""
    X, Y, _ = c["dims"]
    idx = np.flatnonzero(in_set)
    if not idx.size:
        return 0
    x, y, z = idx % X, (idx // X) % Y, idx // (X * Y)
    nbx, nby = -(-X // WC.BRICK[0]), -(-Y // WC.BRICK[1])
    brick = (x // WC.BRICK[0]) + nbx * ((y // WC.BRICK[1]) + nby * (z // WC.BRICK[2]))
    worst = 0
    for b in np.unique(brick):
        px = pidx[idx[brick == b]]
        worst = max(worst, int((px % width).max() - (px % width).min() + 1) * int((px // width).max() - (px // width).min() + 1))
    return worst


@functools.lru_cache(maxsize=None)
def survey_case(seed):
    """One run of the true model over a case: what its frames met, and the final state."""
    O = _oracle()
    c = WC.case(seed)
    model = WC.CaseModel(O, c)
    m = model.m
    out = {"updated": 0, "box": 0, "absorbed": 0, "subnormal": 0, "nan_prior": 0, "remove_meets_fraction": 0, "remove_leaves_fraction": 0, "hits": [],
           "flt_max_pixels": 0}
    cams = []
    for op in c["ops"]:
        cam, (w, h) = Cam(*op[-3]), op[-2:]
        before = m.state()
        if op[0] == "weighted":
            p_image = np.asarray(op[2], F32)
            in_set, _, pidx = R.frame(O, m.ov, op[1], p_image, cam, w, h)
            p = p_image[pidx]
            out["box"] = max(out["box"], _largest_box(c, in_set, pidx, w))
            with np.errstate(invalid="ignore"):
                out["subnormal"] += int((in_set & (p > 0) & (p < F32(2.0 ** -126))).sum())
                out["nan_prior"] += int((in_set & np.isnan(before[1])).sum())
            out["flt_max_pixels"] += int((p_image == WC.FLT_MAX).sum())
            cams.append((cam, w, h))
        elif op[0] == "remove":
            in_set, _ = deintegrate_ref.frame_set(O, m.ov, op[1], cam, w, h)
            with np.errstate(invalid="ignore"):
                wt = before[1]
                out["remove_meets_fraction"] += int((in_set & (wt > 0) & (wt < 1)).sum())
                out["remove_leaves_fraction"] += int((in_set & (wt >= 1) & (wt - F32(1.0) > 0) & (wt - F32(1.0) < 1)).sum())
        updated, _ = model.apply(op)
        out["updated"] += updated
        if op[0] == "weighted":
            # the weight store is skipped -- fl(w + p) has the bits of w -- while the distance moves
            out["absorbed"] += int((in_set & (_bits(m.weight) == _bits(before[1])) & (_bits(m.dist) != _bits(before[0]))).sum())
    for cam, w, h in cams[-2:]:
        out["hits"].append(int((~np.isnan(m.raycast(cam, w, h)[0][:, 0])).sum()))
    out["inf_weights"], out["nan_distances"] = int(np.isinf(m.weight).sum()), int(np.isnan(m.dist).sum())
    return out, m.state()


CLAIMS = {"odd_width": lambda c, s: c["ops"][-1][-2] % 2 == 1 or any(op[0] == "weighted" and op[-2] % 2 == 1 for op in c["ops"]),
          "even_width": lambda c, s: any(op[0] == "weighted" and op[-2] % 2 == 0 for op in c["ops"]),
          "tile": lambda c, s: s["box"] > WC.TILE_PIXELS,
          "absorbing": lambda c, s: s["absorbed"] >= 16,
          "subnormal": lambda c, s: s["subnormal"] >= 1,
          "nan_prior": lambda c, s: s["nan_prior"] >= 1,
          "remove_meets_fraction": lambda c, s: s["remove_meets_fraction"] >= 1,
          "remove_leaves_fraction": lambda c, s: s["remove_leaves_fraction"] >= 1,
          "flt_max": lambda c, s: s["flt_max_pixels"] > 0 and s["inf_weights"] >= 16 and s["nan_distances"] >= 16}


def _images(c):
    return [op[-2:] for op in c["ops"] if op[0] == "weighted"]


SHAPES = {"width odd": lambda c: any(w % 2 == 1 for w, h in _images(c)), "width even": lambda c: any(w % 2 == 0 for w, h in _images(c)),
          "1 x N": lambda c: any(w == 1 and h > 1 for w, h in _images(c)), "N x 1": lambda c: any(h == 1 and w > 1 for w, h in _images(c)),
          "2 x 2": lambda c: (2, 2) in _images(c), "width 63": lambda c: any(w == 63 for w, h in _images(c)),
          "width 64": lambda c: any(w == 64 for w, h in _images(c)), "width 65": lambda c: any(w == 65 for w, h in _images(c))}
SHAPES.update({"grid %s" % (g[0],): (lambda c, g=g: c["dims"] == g[0] and c["offset"] == g[2]) for g in S.GRIDS[1:]})
SHAPES.update({"%d planes" % z: (lambda c, z=z: c["dims"][2] == z) for z in (WC.CHUNK_Z + 1, WC.CHUNK_Z + WC.BATCH_Z, WC.CHUNK_Z + WC.BATCH_Z + 1)})
SHAPES.update({"prior %s" % k: (lambda c, k=k: c["prior"][0] == k) for k in WC.PRIORS})
SHAPES.update({"cap %d" % k: (lambda c, k=k: c["cap"] == k) for k in WC.CAPS})
SHAPES.update({"counting on": lambda c: c["counting"], "counting off": lambda c: not c["counting"], "colour": lambda c: c["colour"],
               "skewed K": lambda c: c["skew"], "explicit nodes": lambda c: c["nodes"] is not None, "two slabs": lambda c: c["slabs"] is not None,
               "a plain frame before the last weighted one": lambda c: len(c["ops"]) >= 2 and c["ops"][-2][0] == "plain",
               "a removal before the last weighted one": lambda c: len(c["ops"]) >= 2 and c["ops"][-2][0] == "remove",
               "1 weighted frame": lambda c: len(_images(c)) == 1, "2 weighted frames": lambda c: len(_images(c)) == 2,
               "3 weighted frames": lambda c: len(_images(c)) == 3, "the device variant": lambda c: c["device"]})


def case_coverage():
    out = {"seeds with " + name: [s for s in WC.SEEDS if f(WC.case(s))] for name, f in SHAPES.items()}
    for claim, holds in CLAIMS.items():
        out["seeds showing " + claim] = [s for s in WC.SEEDS if claim in WC.case(s)["claims"] and holds(WC.case(s), survey_case(s)[0])]
    out["seeds whose pixel weights hold FLT_MAX"] = [s for s in WC.SEEDS if survey_case(s)[0]["flt_max_pixels"]]
    out["cases updating fewer than 16 voxels"] = [s for s in WC.SEEDS if survey_case(s)[0]["updated"] < 16]
    hits = [h for s in WC.SEEDS for h in survey_case(s)[0]["hits"]]
    out["final ray casts"], out["final ray casts hitting 50 pixels or more"] = len(hits), sum(h >= 50 for h in hits)
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    return case_coverage()


def test_there_are_48_cases_and_they_are_deterministic_data():
    assert len(WC.SEEDS) >= 48 and len(WC.AIMED) >= 16
    a = WC.describe(WC.case(21)), WC.case(21)["ops"][0][1].tobytes()
    WC.case.cache_clear()
    assert (WC.describe(WC.case(21)), WC.case(21)["ops"][0][1].tobytes()) == a
    for s in WC.SEEDS:
        c = WC.case(s)
        n = sum(op[0] == "weighted" for op in c["ops"])
        assert 1 <= n <= 3 and c["ops"][-1][0] == "weighted", s
        assert all(5 <= d <= 71 for d in c["dims"]) or c["aimed"], s
        for op in c["ops"]:
            assert op[1].dtype == np.uint16 and op[1].size == op[-2] * op[-1] and 1 <= op[-2] <= 199 + 14 and 1 <= op[-1] <= 159 + 10
            if op[0] == "weighted":
                assert op[2].dtype == F32 and op[2].size == op[1].size and (op[3] is None) == (not c["colour"])


def test_every_aimed_shape_grid_prior_and_switch_occurs_in_two_seeds(cases):
    for name in SHAPES:
        assert len(cases["seeds with " + name]) >= 2, (name, cases["seeds with " + name])


@pytest.mark.parametrize("seed", range(len(WC.AIMED)))
def test_an_aimed_seed_shows_what_it_claims(oracle, seed):
    c = WC.case(seed)
    got = survey_case(seed)[0]
    for claim in c["claims"]:
        assert CLAIMS[claim](c, got), (seed, claim, {k: v for k, v in got.items() if k != "hits"})


def test_every_claim_has_its_seeds(cases):
    for claim in CLAIMS:
        assert len(cases["seeds showing " + claim]) >= (1 if claim == "tile" else 2), (claim, cases["seeds showing " + claim])
    assert tuple(cases["seeds whose pixel weights hold FLT_MAX"]) == WC.FLT_MAX_SEEDS and len(WC.FLT_MAX_SEEDS) == 2


def test_the_special_weights_are_all_there():
    for s in (4, 7, 21):
        p = np.concatenate([op[2] for op in WC.case(s)["ops"] if op[0] == "weighted"])
        for v in WC.SPECIALS:
            assert np.any(_bits(p) == _bits(v)), (s, v)
        with np.errstate(invalid="ignore"):
            ordinary = p[np.isfinite(p) & (p >= F32(2.0 ** -24))]
        assert 0.85 * p.size <= ordinary.size and ordinary.min() < 2.0 ** -20 and ordinary.max() > 2.0 ** 20 and ordinary.max() <= 2.0 ** 24


def test_the_cases_do_work(cases):
    assert len(cases["cases updating fewer than 16 voxels"]) <= 0.1 * len(WC.SEEDS), cases["cases updating fewer than 16 voxels"]
    assert cases["final ray casts hitting 50 pixels or more"] >= 0.6 * cases["final ray casts"], cases


# ---- the sequences ------------------------------------------------------------------------------------------------------------------------
def _is_fractional(w):
    with np.errstate(invalid="ignore"):
        return bool(np.any((w > 0) & np.isfinite(w) & (w != np.round(w))))


@functools.lru_cache(maxsize=None)
def survey_sequence(i):
    """One run of the true model over a weighted sequence: a record per op in the order they act, and the final state.  `bits` is the
    storage the library's rules give the volume before the op, as far as these sequences need it: 8 on a new or cleared volume, raised
    by set_weight_storage, by uploaded or fused counts above 255 and 65535, and to 32 by anything fractional and by a weighted frame."""
    O = _oracle()
    base, ops = WS.sequence(i)
    info, image, _ = S.sequence(base)
    run = ModelRun(O, info, image)
    m = run.model
    records, bits, snapshots = [], 8, []
    for top_level in ops:
        acting = S.flatten([top_level])
        for op in acting:
            between = len(acting) == 2 and op is acting[0]
            before = m.state()
            if op[0] == "depth_prepared":
                out = m.integrate(op[1], image[0], image[1], Cam(*op[2]))
            else:
                out = run.apply(op)
            after = m.state()
            rec = {"kind": op[0], "op": op, "between": between, "bits": bits, "cap": before[3], "fractional_before": _is_fractional(before[1]),
                   "fractional_after": _is_fractional(after[1]), "changed": int(((_bits(before[0]) != _bits(after[0])) | (_bits(before[1]) != _bits(after[1]))).sum())}
            if op[0] == "raycast":
                rec["hits"] = int((~np.isnan(out[0][:, 0])).sum())
            if op[0] == "snapshot":
                snapshots.append({"bits": bits, "fractional": rec["fractional_before"]})
            if op[0] == "restore":
                rec["snapshot"] = snapshots[op[1]]
                bits = max(bits, snapshots[op[1]]["bits"])
            if op[0] == "storage":
                bits = max(bits, op[1])
            if op[0] == "clear":
                bits = 8
            if WS.kind_of(op) is not None and op[0] != "clear":
                top = float(np.nanmax(after[1]))
                bits = max(bits, 32 if (op[0] in (WS.W, WS.WC) or rec["fractional_after"] or top > 65535) else 16 if top > 255 else 8)
            records.append(rec)
    return records, m.state()


def sequence_coverage():
    out = {"ops per sequence": (min(len(WS.sequence(i)[1]) for i in range(WS.N)), max(len(WS.sequence(i)[1]) for i in range(WS.N)))}
    pairs = {}
    for i in range(WS.N):
        chain = [WS.kind_of(r["op"]) for r in survey_sequence(i)[0] if WS.kind_of(r["op"])]
        for a, b in zip(chain, chain[1:]):
            if "weighted" in (a, b):
                pairs.setdefault((a, b), set()).add(i)
    out["ordered pairs with a weighted writer"] = sorted(pairs)
    with_ = lambda f: [i for i in range(WS.N) if f(survey_sequence(i)[0])]
    weighted = lambda r: r["kind"] in (WS.W, WS.WC)
    out["sequences with a weighted frame between prepare and integrate"] = with_(lambda rs: any(r["between"] and weighted(r) for r in rs))
    out["sequences where a weighted frame finds 8-bit storage"] = with_(lambda rs: any(weighted(r) and r["bits"] == 8 and r["changed"] >= 16 for r in rs))
    out["sequences where a weighted frame finds 16-bit storage"] = with_(lambda rs: any(weighted(r) and r["bits"] == 16 and r["changed"] >= 16 for r in rs))

    def writers(rs):
        return [r for r in rs if WS.kind_of(r["op"])]
    out["sequences restoring an 8-bit snapshot between two weighted frames"] = with_(lambda rs: any(
        b["kind"] == "restore" and b["snapshot"]["bits"] == 8 and weighted(a) and weighted(c_) for a, b, c_ in zip(writers(rs), writers(rs)[1:], writers(rs)[2:])))
    out["sequences restoring a snapshot of fractional weights after a clear"] = with_(lambda rs: any(
        b["kind"] == "restore" and b["snapshot"]["fractional"] and b["snapshot"]["bits"] == 32 and a["kind"] == "clear" for a, b in zip(writers(rs), writers(rs)[1:])))
    out["sequences with a remove after weighted frames"] = with_(lambda rs: any(
        r["kind"] == "remove" and r["changed"] >= 16 and any(weighted(q) for q in rs[:j]) for j, r in enumerate(rs)))

    def cap_weighted_off_remove(rs):
        stage = 0
        for r in rs:
            if stage == 0 and r["kind"] == "cap" and r["op"][1] > 0:
                stage = 1
            elif stage == 1 and weighted(r):
                stage = 2
            elif stage == 2 and r["kind"] == "cap" and r["op"][1] == 0:
                stage = 3
            elif stage == 3 and r["kind"] == "remove":
                return True
        return False
    out["sequences with cap on, weighted, cap off, remove"] = with_(cap_weighted_off_remove)
    for k in ("rays", "fuse"):
        out["sequences with a %s onto fractional weights under a cap" % k] = with_(lambda rs, k=k: any(
            r["kind"] == k and r["cap"] > 0 and r["fractional_before"] and r["changed"] >= 16 for r in rs))
    out["sequences with a refused depth_weighted_colour"] = [i for i in range(WS.N) if any(op[0] == "refused" and op[1][0] == WS.WC for op in WS.sequence(i)[1])]
    out["sequences with a ray cast straight behind a weighted frame"] = [i for i in range(WS.N) if any(
        b[0] == "raycast" and (a[0] in (WS.W, WS.WC) or (a[0] == "depth_prepared" and a[3] is not None and a[3][0] in (WS.W, WS.WC)))
        for a, b in zip(WS.sequence(i)[1], WS.sequence(i)[1][1:]))]
    casts = [r["hits"] for i in range(WS.N) for r in survey_sequence(i)[0] if r["kind"] == "raycast"]
    out["ray casts"], out["ray casts with 50 hit pixels or more"] = len(casts), sum(h >= 50 for h in casts)
    w = [r for i in range(WS.N) for r in survey_sequence(i)[0] if weighted(r)]
    out["weighted frames"], out["weighted frames changing 16 voxels or more"] = len(w), sum(r["changed"] >= 16 for r in w)
    return out


@pytest.fixture(scope="module")
def sequences(oracle):
    return sequence_coverage()


def test_the_sequences_hold_all_19_pairs_with_a_weighted_writer(sequences):
    want = {("weighted", k) for k in S.WRITERS} | {(k, "weighted") for k in S.WRITERS} | {("weighted", "weighted")}
    assert len(want) == 19 and set(sequences["ordered pairs with a weighted writer"]) == want, want - set(sequences["ordered pairs with a weighted writer"])
    assert 10 <= WS.N <= 14 and 10 <= sequences["ops per sequence"][0] and sequences["ops per sequence"][1] <= 14, sequences["ops per sequence"]


def test_the_sequences_hold_what_they_were_built_for(sequences):
    least = {"sequences with a weighted frame between prepare and integrate": 2, "sequences where a weighted frame finds 8-bit storage": 1,
             "sequences where a weighted frame finds 16-bit storage": 1, "sequences restoring an 8-bit snapshot between two weighted frames": 1,
             "sequences restoring a snapshot of fractional weights after a clear": 1, "sequences with a remove after weighted frames": 1,
             "sequences with cap on, weighted, cap off, remove": 1, "sequences with a rays onto fractional weights under a cap": 1,
             "sequences with a fuse onto fractional weights under a cap": 1, "sequences with a ray cast straight behind a weighted frame": 4}
    for name, n in least.items():
        assert len(sequences[name]) >= n, (name, sequences[name])
    assert len(sequences["sequences with a refused depth_weighted_colour"]) == 1
    assert sequences["weighted frames changing 16 voxels or more"] >= 0.9 * sequences["weighted frames"], sequences
    assert sequences["ray casts with 50 hit pixels or more"] >= 0.6 * sequences["ray casts"], sequences


def test_a_prepared_list_with_a_weighted_frame_in_between_is_the_two_calls_in_order(oracle):
    """The preparation writes nothing and is used up by the weighted call: the model of ("depth_prepared", d, cam, weighted op) is the
    weighted frame and then the plain one."""
    for i in sequence_coverage()["sequences with a weighted frame between prepare and integrate"]:
        base, ops = WS.sequence(i)
        info, image, _ = S.sequence(base)
        a, b = ModelRun(oracle, info, image), ModelRun(oracle, info, image)
        for op in ops:
            if op[0] in ("raycast", "surface", "flags"):
                continue
            a.apply(op)
            for single in S.flatten([op]):
                b.apply(single[:3] + (None,) if single[0] == "depth_prepared" else single)
        assert _same_state(a.model.state(), b.model.state()), i


# ---- sensitivity --------------------------------------------------------------------------------------------------------------------------
def sequence_end(i, mutant):
    O = _oracle()
    base, ops = WS.sequence(i)
    info, image, _ = S.sequence(base)
    run = ModelRun(O, info, image, mutant)
    for op in ops:
        if op[0] in ("raycast", "surface", "flags", "refused"):
            continue          # (observers change nothing in a model; the refusal is the true model's to show, in survey_sequence)
        try:
            run.apply(op)
        except Refused:
            return None
    return run.model.state()


def case_end(seed, mutant):
    model = WC.CaseModel(_oracle(), WC.case(seed), mutant)
    for op in WC.case(seed)["ops"]:
        model.apply(op)
    return model.m.state()


def sensitivity():
    return {mutant: ([i for i in range(WS.N) if not _same_state(sequence_end(i, mutant), survey_sequence(i)[1])],
                     [s for s in WC.SEEDS if not _same_state(case_end(s, mutant), survey_case(s)[1])]) for mutant in WEIGHTED_MUTANTS}


@pytest.fixture(scope="module")
def caught(oracle):
    return sensitivity()


@pytest.mark.parametrize("mutant", WEIGHTED_MUTANTS)
def test_a_defect_of_integrate_weighted_changes_the_end_of_two_sequences_and_three_cases(caught, mutant):
    in_sequences, in_cases = caught[mutant]
    assert len(in_sequences) >= 2 and len(in_cases) >= 3, (mutant, in_sequences, in_cases)


def test_the_model_without_a_defect_repeats_itself(oracle):
    assert _same_state(sequence_end(2, None), survey_sequence(2)[1]) and _same_state(case_end(12, None), survey_case(12)[1])


# ---- the weight models' cases ---------------------------------------------------------------------------------------------------------------
def model_coverage():
    out = {}
    for w, h in WC.MODEL_SIZES:
        d = WC.model_depth(w, h)
        out["%d x %d" % (w, h)] = tuple(int((R.depth_weights(d, w, h, WC.model_kinv(g), f, WC.MODEL_Z_REF) > 0).sum()) for f in (2, 3) for g in (False, True))
    return out


def test_the_weight_model_cases_have_weights_from_3_x_3_up_and_none_below():
    for (w, h), counts in zip(WC.MODEL_SIZES, model_coverage().values()):
        d = WC.model_depth(w, h)
        assert (w * h < 2 or (65535 in d and 1 in d)) and (w * h < 40 or 0.02 * d.size <= (d == 0).sum() <= 0.2 * d.size), (w, h)
        if w >= 4:
            assert d.reshape(h, w)[0, 1] == 0 and d.reshape(h, w)[h // 2, w - 1 if h > 1 else w - 3] == 0      # beside a corner, on a border
        if w >= 3 and h >= 3:
            assert min(counts) >= 1, (w, h, counts)
        else:
            assert max(counts) == 0, (w, h, counts)
        for f in (0, 1):
            assert (R.depth_weights(d, w, h, WC.model_kinv(False), f, WC.MODEL_Z_REF) > 0).sum() == (d > 0).sum()
    g = R.depth_weights(WC.model_depth(200, 9), 200, 9, WC.model_kinv(True), 3, WC.MODEL_Z_REF)
    s = R.depth_weights(WC.model_depth(200, 9), 200, 9, WC.model_kinv(False), 3, WC.MODEL_Z_REF)
    assert np.unique(g).size > 50 and not np.array_equal(g, s)


if __name__ == "__main__":
    import json
    import time
    t = time.time()
    print(json.dumps(case_coverage(), indent=1, default=str))
    print("case seconds", round(time.time() - t, 1))
    t = time.time()
    print(json.dumps(sequence_coverage(), indent=1, default=str))
    print(json.dumps(sensitivity(), default=str))
    print(json.dumps(model_coverage(), default=str))
    print("sequence and sensitivity seconds", round(time.time() - t, 1))
