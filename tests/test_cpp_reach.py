"""The reachability group through the C++ class surface (libtsdf_host.so: TSDFVolume::reach, TSDFVolume::Reach): build/test_reach
(tests/cpp/test_reach.cpp) computes the cost field of a random 13 x 7 x 5 state field and of the 24^3 serpentine this test writes,
looks points up, walks paths, ranks the field's frontier clusters, checks the class against the C ABI and the refusals as exceptions;
what it prints and dumps must be the CPU reference's (tests/reach_ref.py), integer for integer."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import explore_ref, reach_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_reach")
F32 = np.float32
VS, OFFSET = np.array([10.0, 12.5, 9.0], F32), (100.0, -50.0, 25.0)


def serpentine():
    """As tests/test_reach.py::serpentine: walls x = 1, 3, ..., 23 with one free voxel each, at (y, z) = (23, 23) and (0, 0) in turn."""
    D = np.full((24, 24, 24), 0.5, F32)
    for k, x in enumerate(range(1, 24, 2)):
        D[:, :, x] = -0.5
        gap = 23 if k % 2 == 0 else 0
        D[gap, gap, x] = 0.5
    return D.reshape(-1), np.ones(24 ** 3, F32)


@pytest.mark.gpu
def test_cpp_reach_matches_the_reference(tmp_path):
    if not os.path.exists(BIN):
        pytest.fail("build/test_reach missing: run `make cpptest` (build() does)")
    size, big = (13, 7, 5), (24, 24, 24)
    D, Wt = explore_ref.random_state_field(size, 2468, 0.5)
    trav = reach_ref.traversable(D, Wt, True)
    open_ids = np.flatnonzero(trav)
    seeds = np.concatenate([reach_ref.centres(open_ids[[5, 150]], size, VS, OFFSET), np.array([[np.nan, 0, 0], [1e6, 0, 0]], F32)])
    rng = np.random.default_rng(13)
    goals = np.concatenate([reach_ref.centres(np.arange(13 * 7 * 5), size, VS, OFFSET),
                            (np.array(OFFSET) + rng.uniform(-1.0, np.array(size) + 1.0, (40, 3)) * VS).astype(F32),
                            np.array([[0, np.inf, 0]], F32)]).astype(F32)
    Ds, Ws = serpentine()
    s_seeds = reach_ref.centres([0], big, VS, OFFSET)
    for name, array in (("a_dist", D), ("a_weight", Wt), ("a_seeds", seeds), ("a_goals", goals), ("s_dist", Ds), ("s_weight", Ws), ("s_seeds", s_seeds)):
        np.ascontiguousarray(array, F32).tofile(str(tmp_path / (name + ".f32")))
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "reach ok" in r.stdout

    want, seed_ids = reach_ref.cost_field(trav, size, VS, OFFSET, seeds, 26, 400)
    assert len(seed_ids) == 2 and (want != reach_ref.UNREACHED).sum() > 50
    s_trav = reach_ref.traversable(Ds, Ws)
    s_want, _ = reach_ref.cost_field(s_trav, big, VS, OFFSET, s_seeds, 26, 0)
    a, s = reach_ref.info(trav, want), reach_ref.info(s_trav, s_want)
    printed = [int(v) for v in re.findall(r"\d+", r.stdout.split("reach ok:")[1])]
    assert printed[:7] == [a["n_traversable"], a["n_reached"], a["n_seed_voxels"], a["max_cost_reached"], s["n_traversable"], s["n_reached"],
                           s["max_cost_reached"]], r.stdout
    assert printed[7] >= 24          # rounds: a diagnostic, but the serpentine is 24 bricks long
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    assert np.array_equal(load("a_costs.u32", np.uint32), want)
    assert np.array_equal(load("s_costs.u32", np.uint32), s_want)
    assert np.array_equal(load("a_lookup.u32", np.uint32), reach_ref.lookup(want, size, VS, OFFSET, goals))
    routes = [reach_ref.path(want, trav, size, 26, reach_ref.point_voxel(g, size, VS, OFFSET)) for g in goals]
    assert load("a_lengths.u32", np.uint32).tolist() == [len(p) for p in routes]
    assert load("a_paths.u32", np.uint32).tolist() == [v for p in routes for v in p]
    ids, _ = explore_ref.frontiers(D, Wt, size)
    labels, rows, _ = explore_ref.clusters(ids, size, 26, 1)
    assert load("a_rank.bin", reach_ref.CLUSTER_DTYPE).tobytes() == reach_ref.rank(want, ids, labels, rows).tobytes()
