"""Coloured ray integration on the CPU: what the reference of tests/rays_colour_ref.py (the header's rules 9 - 12) must itself satisfy
before the GPU is compared with it in tests/test_integrate_rays_colour.py, the coverage of the shared case sets, and the one-line
mutants the sets must tell from the rules.  No GPU."""
import inspect

import numpy as np
import pytest

from tests import rays_colour_cases as CC
from tests import rays_colour_ref as cref
from tests import rays_integrate_ref as ref

F = np.float32
# the voxels of G2 (67 x 6 x 35) fall into 2 x 2 x 2 integrate bricks of 64 x 4 x 32
BRICK = (64, 4, 32)
OFFSET_AT_CLEAR = (81.0, -88.0, 67.0)     # about one voxel of G1 on every axis


def oracle_module():
    import oracle as O
    O.build()
    return O


def unpack(words):
    words = np.asarray(words, np.uint32)
    return [(words >> np.uint32(8 * k)) & np.uint32(0xFF) for k in range(4)]


def test_the_python_surface_takes_the_colour_keywords():
    import tsdf_amd
    V = tsdf_amd.TSDFVolume
    assert inspect.signature(V.integrate_rays).parameters["rgb"].default is None
    assert inspect.signature(V.integrate_rays_device).parameters["rgb"].default is None
    assert inspect.signature(V.cast_rays).parameters["colours"].default is False
    assert inspect.signature(V.cast_rays_device).parameters["colours_ptr"].default is None
    assert callable(V.ray_scratch_bytes)


def test_five_permutations_leave_every_colour_word():
    O = oracle_module()
    sets = CC.permutation_sets()
    _, geom = CC.RC.make_geometry(O, CC.G1)
    d, w, words = CC.start_state(geom)
    results = [cref.integrate(geom, d, w, words, o, p, c) for o, p, c in sets]
    assert not np.array_equal(sets[0][2], sets[1][2])
    for r in results[1:]:
        assert r[5] == results[0][5] and np.array_equal(r[3], results[0][3])
        assert np.array_equal(r[0].view(np.uint32), results[0][0].view(np.uint32)) and np.array_equal(r[1], results[0][1])
    assert (results[0][3] != words).sum() >= 1000


@pytest.mark.parametrize("name", CC.NAMES)
def test_every_case_set_keeps_its_coverage(name):
    O = oracle_module()
    c = CC.case(name)
    _, geom = CC.make_geometry(O, c)
    _, _, start = CC.start_state(geom)
    d, w, words, masks, accs, cols = CC.reference(name)
    coloured = set()
    for (o, p, rgb, lo, hi, flags), acc, col in zip(c.calls, accs, cols):
        assert set(col) <= set(acc)                                        # the colour set is a subset of the distance set
        assert all(0 < v[0] <= acc[cell][0] for cell, v in col.items())
        coloured |= set(col)
    assert len(coloured) >= 7
    # every voxel without a colour observation -- those observed only with sdf > trunc among them -- keeps its word
    m = cref.mask(geom, coloured)
    assert np.array_equal(words[~m], start[~m])
    n_old, n_new = unpack(start)[3], unpack(words)[3]
    times = np.zeros(m.size, np.int64)
    for col in cols:
        times += cref.mask(geom, col)
    assert np.array_equal(n_new, np.minimum(n_old + times, 255))
    # coverage: a distance observation without a colour observation; a start word at n == 255 in the colour set; where the set has
    # more than one colour, a voxel that averages at least two different ones
    assert any(cell not in col for acc, col in zip(accs, cols) for cell in acc)
    assert (n_old[m] == 255).any() and all((n_old[m] == k).any() for k in CC.START_N if len(coloured) >= 70)
    if c.differing:
        assert any(v[0] >= 2 and any(s % v[0] for s in v[1:]) for col in cols for v in col.values())
    if name == "g2_scan":
        bricks = {tuple(cell[k] // BRICK[k] for k in range(3)) for cell in coloured}
        assert len(bricks) == 8, bricks                                    # every brick, so every brick column, of G2
    if name in ("contention", "identical"):
        assert max(v[0] for v in cols[0].values()) >= 70000                # a count past 2^16 beside the sums
    if name == "fan_even":
        # half the rays 0, half 255: a voxel all 400 cross has the mean 127.5, which rounds up
        full = [cell for cell, v in cols[0].items() if v[0] == 400]
        assert full and all(cols[0][cell][1:] == [200 * 255] * 3 for cell in full)
        zero = cref.apply_colour(geom, np.zeros(start.size, np.uint32), cols[0])
        assert (zero[cref.mask(geom, full)] == 0x01808080).all()           # 128, not 127
    if name == "fan_odd":
        assert any(v[0] == 401 and v[1] == 200 * 255 for v in cols[0].values())


def test_a_uniform_scan_into_a_cleared_volume_leaves_exactly_that_colour():
    O = oracle_module()
    c = CC.case("uniform")
    _, geom = CC.make_geometry(O, c)
    d, w, _ = CC.start_state(geom)
    o, p, rgb, lo, hi, flags = c.calls[0]
    _, _, upd, words, acc, col = cref.integrate(geom, d, w, np.zeros(d.size, np.uint32), o, p, rgb, lo, hi, flags)
    m = cref.mask(geom, col)
    want = CC.UNIFORM[0] | CC.UNIFORM[1] << 8 | CC.UNIFORM[2] << 16 | 1 << 24
    assert m.sum() >= 2000 and (words[m] == want).all() and (words[~m] == 0).all()
    assert (upd & ~m).sum() >= 10000                                       # carved free space: updated, not coloured


def test_identical_rays_give_the_colour_itself():
    O = oracle_module()
    c = CC.case("identical")
    _, geom = CC.make_geometry(O, c)
    d, w, _ = CC.start_state(geom)
    o, p, rgb, lo, hi, flags = c.calls[0]
    words = cref.integrate(geom, d, w, np.zeros(d.size, np.uint32), o, p, rgb, lo, hi, flags)[3]
    want = CC.IDENTICAL[0] | CC.IDENTICAL[1] << 8 | CC.IDENTICAL[2] << 16 | 1 << 24
    assert sorted(set(words.tolist())) == [0, want]


def test_the_band_ends_exactly_at_plus_and_minus_trunc():
    O = oracle_module()
    c = CC.case("trunc_edges")
    _, geom = CC.make_geometry(O, c)
    trunc = float(geom[3])
    assert trunc == CC.G3_TRUNC and trunc % 64.0 == 0.0
    o, p, rgb, lo, hi, flags = c.calls[0]
    plus = minus = beyond_plus = 0
    for j in range(len(p)):
        cells, obs = ref.walk(geom, o[j], p[j])
        _, col = cref.accumulate(geom, o[j:j + 1], p[j:j + 1], rgb[j:j + 1])
        for i, cell in enumerate(cells):
            sdf = float(obs[cell][0]) if cell in obs else None
            assert sdf is None or sdf % 64.0 == 0.0                        # exact: through voxel centres on a 64 mm grid
            assert (cell in col) == (sdf is not None and -trunc <= sdf <= trunc)
            if sdf == trunc:
                plus += 1
                if i > 0:                                                  # the step before it along the ray: free space, carved only
                    assert float(obs[cells[i - 1]][0]) == trunc + 64.0 and cells[i - 1] not in col
                    beyond_plus += 1
            if sdf == -trunc:
                minus += 1
                # the walk ends with the band: a voxel beyond it, if visited at all, has no observation of any kind
                assert all(nxt not in obs and nxt not in col for nxt in cells[i + 1:])
    assert plus >= 10 and minus >= 10 and beyond_plus >= 6


@pytest.mark.parametrize("mutant", cref.MUTANTS)
def test_every_mutant_changes_a_word_of_some_set(mutant):
    names = {"sdf_lt_trunc": ("trunc_edges",), "band_on_clamped_tsdf": ("uniform", "g2_scan"), "mean_rounded_down": ("inside", "outside"),
             "blend_without_half": ("inside", "g2_scan"), "n_not_saturating": ("inside", "trunc_edges"),
             "offset_at_clear_subtracted": ("inside", "g2_scan")}[mutant]
    differing = 0
    for name in names:
        good = CC.reference(name)[2]
        bad = CC.reference(name, mutant, OFFSET_AT_CLEAR)[2]
        differing += int((good != bad).sum())
        assert (good != bad).any(), (mutant, name)
    print("%s: %d words differ over %s" % (mutant, differing, names))


def test_the_hit_sample_reads_the_voxel_a_field_query_reports():
    O = oracle_module()
    c = CC.case("inside")
    _, geom = CC.make_geometry(O, c)
    dims, vs, offset, _ = geom
    words = CC.reference("inside")[2]
    top = [F(F(dims[k]) * vs[k]) + offset[k] for k in range(3)]
    pts = np.array([[offset[0] + 10, offset[1] + 10, offset[2] + 10], [np.nan, 0, 0], [offset[0] - 1, offset[1] + 10, offset[2] + 10],
                    [top[0], offset[1] + 10, offset[2] + 10], [np.nextafter(F(top[0]), F(-np.inf)), offset[1] + 10, offset[2] + 10],
                    [np.inf, 0, 0]], F)
    cells = cref.sample_cells(geom, pts)
    assert cells[0] == (0, 0, 0) and cells[1] is None and cells[2] is None and cells[3] is None and cells[5] is None
    assert cells[4] in (None, (dims[0] - 1, 0, 0))
    # voxel centres sample their own voxel: n > 0 gives the channels, n == 0 gives black
    X, Y, Z = dims
    idx = np.random.RandomState(2).choice(X * Y * Z, 400, replace=False)
    centres = np.array([[F(F(F(i % X) + F(0.5)) * vs[0]) + offset[0], F(F(F(i // X % Y) + F(0.5)) * vs[1]) + offset[1],
                         F(F(F(i // (X * Y)) + F(0.5)) * vs[2]) + offset[2]] for i in idx], F)
    got = cref.sample(geom, words, centres)
    r, g, b, n = unpack(words[idx])
    want = np.where((n > 0)[:, None], np.stack([r, g, b], 1), 0).astype(np.uint8)
    assert np.array_equal(got, want) and (n == 0).any() and (n > 0).any()
