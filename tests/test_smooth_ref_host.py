"""The CPU reference of the mesh smoothing (tests/smooth_ref.py) on its own (no GPU): it matches a plain loop over triples on the small
hand-made cases, the order of the triples changes no byte, zero iterations and zero factors are the identity, rule 3 keeps a diverging
run finite, Taubin's two factors smooth a noisy sphere without shrinking it where the plain Laplacian shrinks it, the face normals point
out of an extracted surface -- and the inputs of tests/test_smooth.py meet the conditions those tests rely on."""
import math

import numpy as np
import pytest

from tests import components_ref
from tests import mesh_ref
from tests import smooth_ref as ref
from tests.test_components_ref_host import MESH_GRIDS, OFF, VS, mesh_seed

CASES = ref.hand_made_cases()
SMALL = sorted(name for name, c in CASES.items() if len(c[0]) <= 400)
F32 = np.float32
bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32)


def plain_smooth(V, I, iterations, lam, mu, pin):
    """Rules 1-5 one triple and one vertex at a time, in Python integers and floats (a Python float is a double)."""
    V = np.ascontiguousarray(V, F32).reshape(-1, 3)
    n = len(V)
    ok = lambda x: math.isfinite(x) and abs(x) < 2.0 ** 21
    loose = [not all(ok(float(c)) for c in v) for v in V]
    live = [t for t in np.asarray(I, np.int64).reshape(-1, 3).tolist() if len(set(t)) == 3 and not any(loose[c] for c in t)]
    edges = {}
    for a, b, c in live:
        for u, v in ((a, b), (b, c), (a, c)):
            edges[(min(u, v), max(u, v))] = edges.get((min(u, v), max(u, v)), 0) + 1
    fixed = set()
    if pin:
        for (u, v), m in edges.items():
            if m == 1:
                fixed |= {u, v}
    P = V.copy()
    for _ in range(iterations):
        for f in (lam, mu):
            if F32(f) == 0:
                continue
            S, deg = [[0, 0, 0] for _ in range(n)], [0] * n
            q = [[0 if loose[v] else int(np.rint(P[v, a] * F32(1024.0))) for a in range(3)] for v in range(n)]
            for t in live:
                for k in range(3):
                    v, u1, u2 = t[k], t[(k + 1) % 3], t[(k + 2) % 3]
                    deg[v] += 2
                    for a in range(3):
                        S[v][a] += q[u1][a] + q[u2][a]
            out = P.copy()
            for v in range(n):
                if deg[v] == 0 or v in fixed:
                    continue
                new = []
                for a in range(3):
                    p = float(P[v, a])
                    d = (float(S[v][a]) / float(deg[v])) / 1024.0
                    with np.errstate(all="ignore"):
                        new.append(F32(p + float(F32(f)) * (d - p)))
                if all(ok(float(x)) for x in new):
                    out[v] = new
            P = out
    return P


@pytest.mark.parametrize("name", SMALL)
def test_the_reference_matches_a_plain_loop(name):
    V, I, it, lam, mu = CASES[name]
    for flags in (0, ref.PIN_BOUNDARY):
        assert np.array_equal(bits(ref.smooth(V, I, min(it, 6), lam, mu, flags)), bits(plain_smooth(V, I, min(it, 6), lam, mu, bool(flags)))), (name, flags)


@pytest.mark.parametrize("name", sorted(CASES))
def test_permuting_the_triples_changes_no_byte(name):
    V, I, it, lam, mu = CASES[name]
    tri = I.reshape(-1, 3)
    order = np.random.default_rng(len(tri)).permutation(len(tri))
    for flags in (0, ref.PIN_BOUNDARY):
        assert np.array_equal(bits(ref.smooth(V, I, it, lam, mu, flags)), bits(ref.smooth(V, tri[order], it, lam, mu, flags))), name
    assert np.array_equal(ref.pinned(V, I), ref.pinned(V, tri[order]))
    assert bits(ref.vertex_normals(V, I)).tobytes() == bits(ref.vertex_normals(V, tri[order])).tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_zero_iterations_and_zero_factors_are_the_identity(name):
    V, I, it, lam, mu = CASES[name]
    for args in ((0, lam, mu), (5, 0.0, 0.0), (5, -0.0, 0.0), (5, 0.0, -0.0)):
        assert np.array_equal(bits(ref.smooth(V, I, *args)), bits(V)), (name, args)


def test_the_hand_made_cases_are_what_their_names_say():
    pins = {name: ref.pinned(c[0], c[1]) for name, c in CASES.items()}
    assert pins["one triangle"].all() and pins["two triangles"].all()
    for name in ("tetrahedron", "same triple twice", "same triple thrice"):      # closed; m == 2; m == 3, which does not pin
        assert not pins[name].any(), name
    assert pins["three on one edge"].all()                            # by the six outer edges, not by the shared one
    V, I = CASES["three on one edge"][:2]
    assert ref.degrees(V, I).tolist() == [6, 6, 2, 2, 2]
    V, I = CASES["degenerate triples"][:2]
    assert ref.live_triples(V, I).tolist() == [[0, 1, 2]] and ref.degrees(V, I).tolist() == [2, 2, 2, 0]
    V, I, it, lam, mu = CASES["loose corners"]
    assert ref.loose_vertices(V).tolist() == [False] * 4 + [True] * 4 + [False]
    assert ref.live_triples(V, I).tolist() == [[0, 1, 2], [0, 2, 3], [8, 0, 2]]
    out = ref.smooth(V, I, it, lam, mu)
    assert np.array_equal(bits(out[4:8]), bits(V[4:8])) and np.isfinite(out[[0, 1, 2, 3, 8]]).all()
    without = np.delete(I.reshape(-1, 3), [2, 3, 4, 5], axis=0)      # the dead triples pull nothing
    assert np.array_equal(bits(out), bits(ref.smooth(V, without, it, lam, mu)))
    V, I, it, lam, mu = CASES["kept bytes"]
    assert np.array_equal(bits(ref.smooth(V, I, it, lam, mu)[4:]), bits(V[4:]))
    V, I, it, lam, mu = CASES["to the mean"]
    assert np.abs(ref.smooth(V, I, it, lam, mu) - np.array([V[[1, 2, 3]].mean(0), V[[0, 2, 3]].mean(0), V[[0, 1, 3]].mean(0), V[[0, 1, 2]].mean(0)])).max() < 1e-3
    V = CASES["far out"][0]
    assert np.abs(np.rint(V * F32(1024.0))).max() > 2.0 ** 31 - 4096 and not ref.loose_vertices(V).any()
    for first in ("first", "last"):
        V, I = CASES["fan hub %s" % first][:2]
        assert ref.degrees(V, I).max() == 600
    V, I = CASES["random 1000"][:2]
    tri = ref.live_triples(V, I)
    assert len(tri) < len(I) // 3 and ref.pinned(V, I).any() and ref.degrees(V, I).max() > 30


def test_rule_3_keeps_a_diverging_run_finite():
    V, I, it, lam, mu = CASES["guard"]
    assert (it, lam, mu) == (40, -1.0, -1.0)
    out = ref.smooth(V, I, it, lam, mu)
    assert np.isfinite(out).all() and (np.abs(out) < 2.0 ** 21).all()
    assert not np.array_equal(bits(out), bits(V))
    # the guard did hold something: one more pair of passes moves no vertex any further out than the limit, and some vertex is stuck
    again = ref.smooth(out, I, 1, lam, mu)
    assert (np.abs(again) < 2.0 ** 21).all() and (bits(again) == bits(out)).all(axis=1).any()


@pytest.fixture(scope="module")
def sphere(oracle):
    V, I, _, _ = mesh_ref.indexed(oracle, components_ref.sphere_scene(), components_ref.SCENE_SIZE, (10.0, 10.0, 10.0))
    return V, I


def large_sphere(V):
    """(member mask, radius per member, outward unit vector per member) of the scene's large sphere."""
    (centre, radius), _ = components_ref.SCENE_SPHERES
    away = np.asarray(V, np.float64) - (np.array(centre) + 0.5) * 10.0
    r = np.linalg.norm(away, axis=1)
    near = np.abs(r - radius * 10.0) < 20.0
    return near, r[near], away[near] / r[near, None]


def test_taubin_smooths_a_noisy_sphere_and_the_normals_point_outwards(sphere):
    V, I = sphere
    assert (len(V), len(I) // 3) == (4422, 8824)
    assert not ref.loose_vertices(V).any() and not ref.pinned(V, I).any()
    near, _, outward = large_sphere(V)
    assert near.sum() > 3000
    N = ref.vertex_normals(V, I).astype(np.float64)
    assert ((N[near] * outward).sum(axis=1) > 0.99).all()             # the sign convention: out of the surface
    noisy = (V + np.random.default_rng(1).normal(0, 1.5, V.shape)).astype(F32)
    radius = components_ref.SCENE_SPHERES[0][1] * 10.0
    rms = lambda P: float(np.sqrt(np.mean((large_sphere(P)[1] - radius) ** 2)))
    mean = lambda P: float(large_sphere(P)[1].mean())
    taubin, laplace = ref.smooth(noisy, I, 10, 0.5, -0.53), ref.smooth(noisy, I, 10, 0.5, 0.0)
    assert rms(taubin) <= rms(noisy) / 2
    assert abs(mean(taubin) - mean(noisy)) < 0.001 * mean(noisy)
    assert mean(laplace) < 0.99 * mean(noisy)
    near, _, outward = large_sphere(taubin)
    N = ref.vertex_normals(taubin, I).astype(np.float64)
    assert ((N[near] * outward).sum(axis=1) > 0.97).all()


def test_a_box_mesh_has_a_border_that_pins(oracle):
    V, I, _, _ = mesh_ref.indexed(oracle, components_ref.sphere_scene(), components_ref.SCENE_SIZE, (10.0, 10.0, 10.0), box=(0, 0, 0, 24, 64, 64))
    pins = ref.pinned(V, I)
    assert len(V) == 1960 and pins.sum() == 108
    out = ref.smooth(V, I, 10, 0.5, -0.53, ref.PIN_BOUNDARY)
    moved = (bits(out) != bits(V)).any(axis=1)
    assert not moved[pins].any() and moved.any()
    assert (bits(ref.smooth(V, I, 10, 0.5, -0.53)) != bits(V)).any(axis=1)[pins].any()    # ... which the flag is there to stop


@pytest.mark.parametrize("size", MESH_GRIDS)
def test_the_random_field_meshes_carry_dead_triples_loose_and_unnamed_vertices_and_pins(oracle, size):
    V, I, _, _ = mesh_ref.indexed(oracle, mesh_ref.random_field(size, mesh_seed(size)), size, VS, OFF)
    live, loose, deg, pins = ref.live_triples(V, I), ref.loose_vertices(V), ref.degrees(V, I), ref.pinned(V, I)
    assert 0 < len(live) < len(I) // 3 and loose.any() and (deg == 0).any() and pins.any()
    assert not pins[loose].any() and (deg[loose] == 0).all()
