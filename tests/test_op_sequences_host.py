"""No GPU: the composed CPU model (tests/volume_model.py) and the sequences (tests/op_sequences.py) that tests/test_op_sequences.py
drives through the library.

1. The model agrees with each reference: one op from a non-trivial state through the model equals the same op through the reference
   that pins it, called the way that reference's own GPU test calls it.
2. Coverage: conditions on the 32 sequences, computed from the model alone.  Achieved (asserted below, each at or above its condition):
   32 sequences of 13 or 14 ops; all 81 ordered pairs of writer kinds held; a ray cast straight after depth in 5 sequences,
   depth_colour 7, remove 7, rays 7, rays_colour 7, fuse 6, restore 8, upload 9, clear 3, depth_prepared 7 (>= 2 each); 228 of 236 writer
   ops change 16 voxels or more (>= 90 %); the largest weight passes 255 by a depth in 2 sequences, by a rays in 3, by a fuse in 3 (>= 2
   each) and 65535 in 2 (>= 2); a snapshot from below 255 is restored above it in 8 sequences and one from above it below in 10 (>= 4
   each); 10 sequences switch a cap on (>= 8), 6 of them switch it off and then remove (>= 4), 3 with a cap above 255 and 7 with one of
   at most 255 (>= 2 each); 11 sequences hold an op between prepare and integrate (>= 6): rays 4, fuse 3, restore 2, remove 1, raycast 1;
   16 sequences enable colour after distances exist (>= 6), 4 of them disable and re-enable it (>= 3); 60 of 73 ray casts hit 50 pixels
   or more (>= 80 %).
3. Sensitivity: the model with one plausible defect at a time ends at least three sequences in another state than the true model.
   Achieved: counts that wrap modulo 256 in rays and fuse: seeds 2, 3, 4, 24; a restore that leaves the colour words: 18, 19, 20, 21; rays
   that ignore the cap: 10, 14, 16; a removal that keeps the distance where the weight reaches 0: 8, 10, 26, 30, 31.
4. Class words (tests/class_sequences.py, run on the GPU by tests/test_class_fuzz.py): the twelve sequences run to their end on the model;
   every class frame but the refused ones changes 16 words or more; a class frame takes the largest weight past 255 and one past 65535;
   class frames stand on both sides of a storage switch, a pin, a cap switched on and off, a removal, rays, a fuse, a weighted frame, a
   restore, a clear and a change of the image size; only a class frame, a clear, an upload of words and the switch itself change a
   word -- a restore leaves the words voted since its snapshot in place; both refusals occur and leave the state alone; each of three
   defects (a restore that zeroes the words, a removal that takes the votes of the voxels it empties, a vote in free space) ends at
   least two sequences in another state.
"""
import functools

import numpy as np
import pytest

from tests import colour_ref, deintegrate_ref, fuse_ref, rays_colour_ref, rays_integrate_ref, snapshot_ref
from tests import op_sequences as S
from tests.helpers import Cam, assert_same_floats
from tests import class_sequences as CS
from tests.volume_model import CLASS_MUTANTS, ModelRun, Refused, VolumeModel, WEIGHTED_MUTANTS
from tests.volume_model import MUTANTS as ALL_MUTANTS
from tests.weight_cap_ref import oracle_step

F32, U32 = np.float32, np.uint32
# the defects of integrate_weighted have sequences of their own (tests/weighted_sequences.py, tests/test_weighted_fuzz_host.py): the 32
# pinned sequences hold no weighted frame
MUTANTS = tuple(m for m in ALL_MUTANTS if m not in WEIGHTED_MUTANTS and m not in CLASS_MUTANTS)


def _same_state(a, b):
    if a is None or b is None:
        return False
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(np.asarray(x).view(U32), np.asarray(y).view(U32)))
               for x, y in zip(a[:3] + a[4:], b[:3] + b[4:])) and a[3] == b[3]


def _changed(before, after):
    """Voxels of which the distance, the weight or the colour word has other bits."""
    ch = (before[0].view(U32) != after[0].view(U32)) | (before[1].view(U32) != after[1].view(U32))
    if (before[2] is None) != (after[2] is None):
        words = before[2] if before[2] is not None else after[2]
        return int((ch | (words != 0)).sum())
    if before[2] is not None:
        ch |= before[2] != after[2]
    return int(ch.sum())


@functools.lru_cache(maxsize=None)
def survey(seed):
    """One run of the true model over a sequence: a record per op in the order they act, and the final state."""
    import oracle as O
    O.build()
    info, image, ops = S.sequence(seed)
    run = ModelRun(O, info, image)
    m = run.model
    fill_bits = m.trunc().reshape(1).view(U32)[0]
    records, snapshot_tops = [], []
    for top_level in ops:
        acting = S.flatten([top_level])
        for op in acting:
            between = len(acting) == 2 and op is acting[0]
            before = m.state()
            if op[0] == "depth_prepared":
                # (the op in between has its own record: apply only the integrate here)
                out = m.integrate(op[1], image[0], image[1], Cam(*op[2]))
            else:
                out = run.apply(op)
            after = m.state()
            rec = {"kind": op[0], "op": op, "between": between, "top_before": float(np.nanmax(before[1])), "top_after": float(np.nanmax(after[1])),
                   "changed": _changed(before, after), "cap": after[3], "colour_before": before[2] is not None, "colour_after": after[2] is not None,
                   "distances_before": bool((before[0].view(U32) != fill_bits).any())}
            if op[0] == "raycast":
                rec["hits"] = int((~np.isnan(out[0][:, 0])).sum())
            if op[0] == "snapshot":
                snapshot_tops.append(rec["top_before"])
            if op[0] == "restore":
                rec["snapshot_top"] = snapshot_tops[op[1]]
            records.append(rec)
    return records, m.state()


def _writer_chain(records):
    return [S.writer_kind(r["op"]) for r in records if S.writer_kind(r["op"])]


# ---- 1. the model against each reference -------------------------------------------------------------------------------------------
GRID = ((40, 24, 36), (1000.0, 600.0, 900.0), (30.0, -20.0, 45.0))
IMAGE = (64, 48)


@pytest.fixture()
def busy(oracle):
    """A model in a non-trivial state -- an uploaded field and counts, colour words, one fused frame -- and a generator for more."""
    rng = np.random.default_rng(77)
    m = VolumeModel(oracle, *GRID)
    n = m.dist.size
    m.set_distance_data(S._ball_field(rng, GRID[0], GRID[1], GRID[2], m.trunc()))
    m.set_weight_data(S._counts(rng, n, None, None))
    m.enable_colour(True)
    m.set_colour_data(np.where(rng.random(n) < 0.5, rng.integers(0, 2 ** 32, n, dtype=np.uint64), 0).astype(U32))
    d, c = S._frame(rng, GRID, IMAGE)
    assert m.integrate(d, IMAGE[0], IMAGE[1], Cam(*c)) >= 16
    return m, rng


def _twin(oracle, m):
    """An oracle.Volume holding the model's distances and weights, and a copy of its colour words."""
    ov = oracle.Volume(GRID[0], GRID[1])
    ov.offset(*GRID[2])
    ov.set_distance_data(m.dist)
    ov.set_weight_data(m.weight)
    return ov, None if m.colour is None else m.colour.copy()


def _same(m, dist, weight, colour, what):
    assert_same_floats(m.dist, dist, what + ": distances")
    assert_same_floats(m.weight, weight, what + ": weights")
    assert np.array_equal(m.colour, colour), what + ": colours"


@pytest.mark.parametrize("cap", [0, 3])
def test_depth_is_the_oracles_integrate_and_the_cap_references_clamp(oracle, busy, cap):
    m, rng = busy
    ov, words = _twin(oracle, m)
    d, c = S._frame(rng, GRID, IMAGE)
    cam = Cam(*c)
    m.set_weight_cap(cap)
    updated = m.integrate(d, IMAGE[0], IMAGE[1], cam)
    before = ov.weight.copy()
    if cap:
        oracle_step(oracle, ov, d, cam, cap, *IMAGE)
        assert ov.weight.max() > cap        # (counts uploaded above the cap, outside the frame, stay)
    else:
        ov.integrate(d, IMAGE[0], IMAGE[1], cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    _same(m, ov.dist, ov.weight, words, "depth, cap %d" % cap)
    assert updated == int((ov.weight != before).sum()) >= 16


def test_depth_colour_is_the_colour_references_blend_beside_the_oracles_integrate(oracle, busy):
    m, rng = busy
    ov, words = _twin(oracle, m)
    d, c = S._frame(rng, GRID, IMAGE)
    rgb = rng.integers(0, 256, (IMAGE[0] * IMAGE[1], 3)).astype(np.uint8)
    cam = Cam(*c)
    m.integrate_colour(d, rgb, IMAGE[0], IMAGE[1], cam)
    geom = (GRID[0], ov.voxel_size(), ov.offset(), np.zeros(3, F32), F32(ov.truncation_distance()))
    want, _, coloured = colour_ref.integrate_colour(oracle, words, geom, d, rgb, IMAGE[0], IMAGE[1], cam)
    ov.integrate(d, IMAGE[0], IMAGE[1], cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    _same(m, ov.dist, ov.weight, want, "depth_colour")
    assert coloured.sum() >= 16 and not np.array_equal(want, words)


def test_remove_is_the_deintegrate_reference(oracle, busy):
    m, rng = busy
    d, c = S._frame(rng, GRID, IMAGE)
    cam = Cam(*c)
    m.integrate(d, IMAGE[0], IMAGE[1], cam)
    ov, words = _twin(oracle, m)
    updated = m.deintegrate(d, IMAGE[0], IMAGE[1], cam)
    want, _ = deintegrate_ref.oracle_remove(oracle, ov, d, cam, *IMAGE)
    _same(m, ov.dist, ov.weight, words, "remove")
    assert updated == want >= 16


@pytest.mark.parametrize("cap", [0, 2])
def test_rays_are_the_ray_references(oracle, busy, cap):
    m, rng = busy
    m.set_weight_cap(cap)
    ov, words = _twin(oracle, m)
    geom = rays_integrate_ref.geometry(ov)
    o, p, band, lo, hi = S._rays(rng, GRID, m.trunc())
    updated = m.integrate_rays(o, p, None, band, lo, hi)
    d, w, upd, _ = rays_integrate_ref.integrate(geom, ov.dist, ov.weight, o, p, lo, hi, rays_integrate_ref.BAND_ONLY if band else 0, cap)
    _same(m, d, w, words, "rays")
    assert updated == int(upd.sum()) >= 16
    rgb = rng.integers(0, 256, (len(p), 3)).astype(np.uint8)
    m.integrate_rays(o, p, rgb, band, lo, hi)
    d, w, _, want, _, col = rays_colour_ref.integrate(geom, d, w, words, o, p, rgb, lo, hi, rays_integrate_ref.BAND_ONLY if band else 0, cap)
    _same(m, d, w, want, "rays_colour")
    assert len(col) >= 16 and (cap == 0 or w.max() > cap)


@pytest.mark.parametrize("cap", [0, 5])
def test_fuse_is_the_fuse_reference(oracle, busy, cap):
    m, rng = busy
    m.set_weight_cap(cap)
    ov, words = _twin(oracle, m)
    s = S._source(rng, GRID, 3)
    src = VolumeModel(oracle, s["dims"], s["phys"], s["offset"])
    src.set_distance_data(s["dist"])
    src.set_weight_data(s["weight"])
    mat = fuse_ref.rotation((0.2, 1.0, -0.4), 11.0, (40.0, -25.0, 10.0))
    updated = m.fuse(src, mat)
    d, w, upd = fuse_ref.fuse(oracle, fuse_ref.geometry(ov), ov.g.trunc, ov.dist, ov.weight, fuse_ref.geometry(src.ov), src.dist, src.weight, mat, cap=cap)
    _same(m, d, w, words, "fuse")
    assert updated == int(upd.sum()) >= 16


@pytest.mark.parametrize("with_colour", [True, False])
def test_restore_is_the_snapshot_references_round_trip_and_the_headers_colour_rules(oracle, busy, with_colour):
    m, rng = busy
    if not with_colour:
        m.enable_colour(False)
    D, Wt, Cl, _ = m.state()[:4]
    assert Wt.max() <= 255
    snap = m.snapshot()
    # the reference as tests/test_snapshot.py calls it, at the storage a volume with these counts has
    ids, d, w, c = snapshot_ref.take(D, Wt, GRID[0], m.trunc(), 8, Cl)
    assert 0 < len(ids) and np.array_equal(ids, snap["ids"])
    assert_same_floats(snap["dist"], d, "brick distances")
    assert np.array_equal(snap["weight"], w.astype(F32)) and (c is None) == (snap["colour"] is None)
    m.clear()
    m.enable_colour(True)
    m.set_colour_data(np.full(D.size, 0x01020304, U32))
    frame = S._frame(rng, GRID, IMAGE)
    m.integrate(frame[0], IMAGE[0], IMAGE[1], Cam(*frame[1]))
    m.restore(snap)
    rd, rw, rc = snapshot_ref.put(ids, d, w, c, GRID[0], m.trunc())
    _same(m, rd, rw, rc if with_colour else np.zeros(D.size, U32), "restore")      # (without colour: an enabled array is zeroed)
    _same(m, D, Wt, Cl if with_colour else np.zeros(D.size, U32), "restore against the state the snapshot was taken from")
    bare = VolumeModel(oracle, *GRID)
    bare.restore(snap)
    assert (bare.colour is not None) == with_colour                                   # (with colour: enabled by the restore)


def test_upload_clear_and_the_switches(oracle, busy):
    m, rng = busy
    n = m.dist.size
    D, Wt, Cl = rng.normal(size=n).astype(F32), rng.integers(0, 9, n).astype(F32), rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(U32)
    m.set_distance_data(D); m.set_weight_data(Wt); m.set_colour_data(Cl)
    _same(m, D, Wt, Cl, "upload")
    m.set_weight_cap(7)
    m.set_weight_storage(16)
    _same(m, D, Wt, Cl, "switches")
    m.clear()
    ov = oracle.Volume(GRID[0], GRID[1])
    _same(m, ov.dist, ov.weight, np.zeros(n, U32), "clear")
    assert m.cap == 7
    m.enable_colour(False)
    assert m.colour is None
    m.enable_colour(True)
    assert not m.colour.any()


# ---- 2. coverage --------------------------------------------------------------------------------------------------------------------
def _sequences_with(predicate):
    return [s for s in S.SEEDS if predicate(survey(s)[0])]


def coverage():
    """Every count the conditions are about, from the model alone."""
    out = {}
    pairs = {}
    for s in S.SEEDS:
        chain = _writer_chain(survey(s)[0])
        for a, b in zip(chain, chain[1:]):
            pairs.setdefault((a, b), set()).add(s)
    out["writer pairs held"] = len(pairs)
    out["ops per sequence"] = (min(len(S.sequence(s)[2]) for s in S.SEEDS), max(len(S.sequence(s)[2]) for s in S.SEEDS))
    follow = {}
    for s in S.SEEDS:
        ops = S.sequence(s)[2]
        for a, b in zip(ops, ops[1:]):
            if b[0] == "raycast" and (a[0] in S.WRITERS or a[0] == "depth_prepared"):
                follow.setdefault(a[0], set()).add(s)
    out["sequences with a ray cast straight after"] = {k: len(follow.get(k, ())) for k in S.WRITERS + ("depth_prepared",)}
    writers = [r for s in S.SEEDS for r in survey(s)[0] if S.writer_kind(r["op"])]
    out["writer ops"] = len(writers)
    out["writer ops that change 16 voxels or more"] = sum(r["changed"] >= 16 for r in writers)
    for by, kinds in (("depth", ("depth", "depth_prepared")), ("rays", ("rays",)), ("fuse", ("fuse",))):
        out["sequences passing 255 by a %s" % by] = len(_sequences_with(
            lambda rs: any(r["kind"] in kinds and r["top_before"] <= 255 < r["top_after"] for r in rs)))
    out["sequences passing 65535"] = len(_sequences_with(lambda rs: any(S.writer_kind(r["op"]) and r["top_before"] <= 65535 < r["top_after"] for r in rs)))
    out["sequences restoring a snapshot from below 255 above it"] = len(_sequences_with(
        lambda rs: any(r["kind"] == "restore" and r["snapshot_top"] <= 255 < r["top_before"] for r in rs)))
    out["sequences restoring a snapshot from above 255 below it"] = len(_sequences_with(
        lambda rs: any(r["kind"] == "restore" and r["top_before"] <= 255 < r["snapshot_top"] for r in rs)))

    def cap_off_then_remove(rs):
        kinds = [(r["kind"], r["op"][1] if r["kind"] == "cap" else None) for r in rs]
        on = next((i for i, k in enumerate(kinds) if k[0] == "cap" and k[1] > 0), None)
        if on is None:
            return False
        off = next((i for i, k in enumerate(kinds) if i > on and k == ("cap", 0)), None)
        return off is not None and any(k[0] == "remove" for k in kinds[off:])
    caps = {s: [r["op"][1] for r in survey(s)[0] if r["kind"] == "cap" and r["op"][1] > 0] for s in S.SEEDS}
    out["sequences switching a cap on"] = sum(bool(c) for c in caps.values())
    out["of them switching it off and then removing"] = len(_sequences_with(cap_off_then_remove))
    out["sequences with a cap above 255"] = sum(any(c > 255 for c in cs) for cs in caps.values())
    out["sequences with a cap of at most 255"] = sum(any(c <= 255 for c in cs) for cs in caps.values())
    between = {}
    for s in S.SEEDS:
        for op in S.sequence(s)[2]:
            if op[0] == "depth_prepared" and op[3] is not None:
                between.setdefault(op[3][0], set()).add(s)
    out["sequences with an op between prepare and integrate"] = len(set().union(*between.values()))
    out["the ops in between"] = {k: len(v) for k, v in sorted(between.items())}
    out["sequences enabling colour after distances exist"] = len(_sequences_with(
        lambda rs: any(not r["colour_before"] and r["colour_after"] and r["distances_before"] for r in rs)))

    def off_and_on_again(rs):
        states = [rs[0]["colour_before"]] + [r["colour_after"] for r in rs]
        runs = [a for a, b in zip(states, states[1:] + [None]) if a != b]      # the state, with repeats folded
        return any(runs[i:i + 3] == [True, False, True] for i in range(len(runs)))
    out["of them disabling and re-enabling it"] = len(_sequences_with(off_and_on_again))
    casts = [r for s in S.SEEDS for r in survey(s)[0] if r["kind"] == "raycast"]
    out["ray casts"] = len(casts)
    out["ray casts with 50 hit pixels or more"] = sum(r["hits"] >= 50 for r in casts)
    return out


@pytest.fixture(scope="module")
def counts(oracle):
    return coverage()


def test_every_ordered_pair_of_writer_kinds_occurs(counts):
    assert counts["writer pairs held"] == len(S.WRITERS) ** 2 == 81
    assert len(S.SEEDS) == 32 and 12 <= counts["ops per sequence"][0] and counts["ops per sequence"][1] <= 14


def test_a_ray_cast_follows_every_writer_kind_in_two_sequences(counts):
    assert all(n >= 2 for n in counts["sequences with a ray cast straight after"].values()), counts["sequences with a ray cast straight after"]


def test_the_writers_do_work(counts):
    assert counts["writer ops that change 16 voxels or more"] >= 0.9 * counts["writer ops"], counts


def test_the_storage_thresholds_are_passed(counts):
    for by in ("depth", "rays", "fuse"):
        assert counts["sequences passing 255 by a %s" % by] >= 2, counts
    assert counts["sequences passing 65535"] >= 2, counts
    assert counts["sequences restoring a snapshot from below 255 above it"] >= 4, counts
    assert counts["sequences restoring a snapshot from above 255 below it"] >= 4, counts


def test_caps_are_switched(counts):
    assert counts["sequences switching a cap on"] >= 8 and counts["of them switching it off and then removing"] >= 4, counts
    assert counts["sequences with a cap above 255"] >= 2 and counts["sequences with a cap of at most 255"] >= 2, counts


def test_prepared_lists_see_other_ops_before_their_integrate(counts):
    assert counts["sequences with an op between prepare and integrate"] >= 6, counts
    assert set(counts["the ops in between"]) >= {"rays", "fuse", "remove", "restore", "raycast"}, counts


def test_colour_has_a_history(counts):
    assert counts["sequences enabling colour after distances exist"] >= 6 and counts["of them disabling and re-enabling it"] >= 3, counts


def test_ray_casts_hit_something(counts):
    assert counts["ray casts with 50 hit pixels or more"] >= 0.8 * counts["ray casts"], counts


def test_a_refused_call_in_every_sequence_at_most_one(oracle):
    kinds = Counter_of_refusals()
    assert set(kinds) == {"remove", "rays_colour", "restore_other"} and all(n >= 3 for n in kinds.values()), kinds


def Counter_of_refusals():
    from collections import Counter
    kinds = Counter()
    for s in S.SEEDS:
        refused = [op[1][0] for op in S.sequence(s)[2] if op[0] == "refused"]
        assert len(refused) <= 1, (s, refused)
        kinds.update(refused)
    return kinds


def test_sequences_are_deterministic_data():
    a = S.describe(S.sequence(5)[2])
    S.sequence.cache_clear()
    assert S.describe(S.sequence(5)[2]) == a and "depth_prepared" in S.describe(S.sequence(4)[2])

    def plain(v):
        return isinstance(v, (np.ndarray, int, float, bool, str, type(None))) or (isinstance(v, tuple) and all(plain(x) for x in v))
    assert all(plain(op) for s in S.SEEDS for op in S.sequence(s)[2])


# ---- 3. sensitivity -----------------------------------------------------------------------------------------------------------------
def final_state(seed, mutant):
    """The state a sequence ends in on the model with one defect; observers, which change nothing in a model, are left out."""
    import oracle as O
    info, image, ops = S.sequence(seed)
    run = ModelRun(O, info, image, mutant)
    for op in ops:
        if op[0] in ("raycast", "surface", "flags"):
            continue
        if op[0] == "depth_prepared" and op[3] is not None and op[3][0] == "raycast":
            op = op[:3] + (None,)
        try:
            run.apply(op)
        except Refused:
            return None          # (the defect made the model refuse a later call: an end the true model does not have)
    return run.model.state()


def sensitivity():
    return {mutant: [s for s in S.SEEDS if not _same_state(final_state(s, mutant), survey(s)[1])] for mutant in MUTANTS}


@pytest.fixture(scope="module")
def caught(oracle):
    return sensitivity()


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_defect_of_this_kind_changes_the_end_of_three_sequences(caught, mutant):
    assert len(caught[mutant]) >= 3, (mutant, caught[mutant])


def test_the_model_without_a_defect_repeats_itself(oracle):
    assert _same_state(final_state(9, None), survey(9)[1])


# ---- 4. class words among the writers ---------------------------------------------------------------------------------------------------
def _flat_class_ops(ops):
    """The ops in the order they act: a "classes_prepared" is its class frame and then the plain frame the list was prepared for."""
    out = []
    for op in ops:
        if op[0] == CS.KP:
            out += [(CS.K, op[1], op[2], op[3], None, op[4]), ("depth", op[1], op[4])]
        else:
            out.append(op)
    return out


@functools.lru_cache(maxsize=None)
def class_survey(i, mutant=None):
    """One run of the model over a class sequence: a record per acting op (observers left out) and the final state, or None where a
    defect made the model refuse a call."""
    import oracle as O
    O.build()
    base, ops = CS.sequence(i)
    info, image, _ = S.sequence(base)
    run = ModelRun(O, info, image, mutant)
    m = run.model
    records = []
    for op in _flat_class_ops(ops):
        if op[0] in ("raycast", "surface", "flags"):
            continue
        before = m.state()
        try:
            run.apply(op)
        except Refused:
            return records, None
        after = m.state()
        words = 0 if before[4] is None or after[4] is None else int((before[4] != after[4]).sum())
        records.append({"kind": op[0], "op": op, "words": words, "had_words": before[4] is not None and bool(before[4].any()),
                        "top_before": float(np.nanmax(before[1])), "top_after": float(np.nanmax(after[1])),
                        "state_changed": _changed(before, after), "image": (run.width, run.height)})
    return records, m.state()


def test_the_class_sequences_hold_what_they_were_built_for(oracle):
    assert 10 <= CS.N <= 14
    runs = [class_survey(i) for i in range(CS.N)]
    assert all(end is not None for _, end in runs)
    frames = [r for recs, _ in runs for r in recs if r["kind"] == CS.K]
    assert len(frames) >= 40 and sum(r["words"] >= 16 for r in frames) >= 0.9 * len(frames), [r["words"] for r in frames]
    assert any(r["top_before"] <= 255 < r["top_after"] for r in frames) and any(r["top_before"] <= 65535 < r["top_after"] for r in frames)
    # only the class writers change a word; the other writers do their own work beside words that are there
    others = [r for recs, _ in runs for r in recs if r["kind"] not in (CS.K, "clear", "upload_classes", "classes", "refused")]
    assert all(r["words"] == 0 for r in others)
    beside = {r["kind"] for r in others if r["had_words"] and (r["state_changed"] or r["kind"] in ("storage", "pin", "cap", "image", "snapshot"))}
    assert {"depth", "depth_colour", "depth_weighted", "remove", "rays", "fuse", "restore", "storage", "pin", "cap", "image", "snapshot"} <= beside, beside
    # a class frame straight or one op behind each of them, and in front of each
    for recs, _ in runs:
        kinds = [r["kind"] for r in recs]
        for a, b in zip(kinds, kinds[1:]):
            if a in beside and b == CS.K:
                beside = beside - {a}
    assert not beside - {"snapshot", "cap"}, beside
    # a restore leaves the words voted since its snapshot in place
    for i in (0, 7):
        recs = class_survey(i)[0]
        at = [k for k, r in enumerate(recs) if r["kind"] == "restore"][0]
        assert recs[at]["had_words"] and recs[at]["words"] == 0 and recs[at]["state_changed"] > 0
    clears = [r for recs, _ in runs for r in recs if r["kind"] == "clear"]
    assert len(clears) >= 3 and all(r["words"] > 0 for r in clears if r["had_words"]) and any(r["had_words"] for r in clears)
    # the image size changes between class frames and returns
    sizes = [r["image"] for r in class_survey(8)[0] if r["kind"] == CS.K]
    assert len(set(sizes)) == 3 and sizes[0] == sizes[-1]
    # both refusals, with words to lose
    refused = [r for recs, _ in runs for r in recs if r["kind"] == "refused"]
    assert sorted((r["op"][1][4] is not None) for r in refused) == [False, True, True] and all(r["had_words"] and not r["state_changed"] for r in refused)
    assert sum(op[0] == CS.KP for i in range(CS.N) for op in CS.sequence(i)[1]) >= 2
    assert sum(op == ("counting", True) for i in range(CS.N) for op in CS.sequence(i)[1]) >= 2


def test_class_sequences_are_deterministic_data():
    a = S.describe(CS.sequence(3)[1])
    CS.sequence.cache_clear()
    assert S.describe(CS.sequence(3)[1]) == a


@pytest.mark.parametrize("mutant", CLASS_MUTANTS)
def test_a_defect_round_the_class_words_changes_the_end_of_two_class_sequences(oracle, mutant):
    caught = [i for i in range(CS.N) if not _same_state(class_survey(i, mutant)[1], class_survey(i)[1])]
    assert len(caught) >= 2, (mutant, caught)


if __name__ == "__main__":
    import json
    import time
    t = time.time()
    each = []
    for s in S.SEEDS:
        t0 = time.time()
        survey(s)
        each.append(round(time.time() - t0, 2))
    print(json.dumps(coverage(), indent=1, default=str))
    print(json.dumps(sensitivity(), default=str))
    print("model seconds per seed", each, "all", round(time.time() - t, 1))
