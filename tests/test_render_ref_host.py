"""The mesh renderer's CPU reference (tests/render_ref.py) against exact arithmetic, without a GPU.  The inputs are built so that every
screen coordinate is an exact multiple of 1/256 -- an identity pose, power-of-two focal lengths and depths, vertices placed by hand --
so the reference's fixed-point corners are the intended ones exactly, and coverage can be decided in Python integers by an argument the
reference does not use: a centre on an edge belongs to the triangle iff the centre moved by (eps, eps^2) lies strictly inside."""
from fractions import Fraction

import numpy as np

from tests import render_ref as ref

F = np.float32
W, H = 16, 12
FX, CX, CY = 64.0, 8.0, 6.0
IDENTITY = np.eye(4, dtype=F).reshape(-1)
K = np.array([FX, 0, 0, 0, FX, 0, CX, CY, 1], F)
NEAR, FAR = 1.0, 4096.0


def vertex(sx, sy, z):
    """The world point (identity pose) whose screen point is exactly (sx, sy) at depth z: sx, sy multiples of 1/256, z a power of two."""
    x, y = (sx - CX) * z / FX, (sy - CY) * z / FX
    v = np.array([x, y, z], F)
    assert float(v[0]) == x and float(v[1]) == y                      # exact in fp32
    return v


def mesh(corners):
    """corners: per triangle three (sx, sy, z) in the WIRED order; returns V, I (I[3t+1] and I[3t+2] swapped back)."""
    V = np.array([vertex(*c) for tri in corners for c in tri], F).reshape(-1, 3)
    I = np.arange(len(V), dtype=np.uint32).reshape(-1, 3)[:, [0, 2, 1]].reshape(-1)
    return V, I


def exact_cover(tri, i, j):
    """Python integers only: is the centre of (i, j) in the triangle, ties broken by the move (eps, eps^2)?"""
    P = [(round(Fraction(sx) * 256), round(Fraction(sy) * 256)) for sx, sy, _ in tri]
    for (sx, sy, _), (X, Y) in zip(tri, P):
        assert Fraction(X, 256) == Fraction(sx) and Fraction(Y, 256) == Fraction(sy)
    (x0, y0), (x1, y1), (x2, y2) = P
    a2 = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    if a2 == 0:
        return False, False
    s = 1 if a2 > 0 else -1
    on_edge = False
    for (ax, ay), (bx, by) in ((P[1], P[2]), (P[2], P[0]), (P[0], P[1])):
        E = lambda px, py: s * ((bx - ax) * (py - ay) - (by - ay) * (px - ax))
        here = E(256 * i, 256 * j)
        first = next((v for v in (here, E(256 * i + 1, 256 * j) - here, E(256 * i, 256 * j + 1) - here) if v != 0), 0)
        on_edge |= here == 0
        if first <= 0:
            return False, on_edge
    return True, on_edge


def coverage_of(corners, flags=0, far=FAR):
    V, I = mesh(corners)
    out = ref.render(V, I, W, H, IDENTITY, K, NEAR, far, flags)
    X, Y, _, usable = ref.project(V, IDENTITY, K, NEAR, far)
    assert usable.all()
    for t, tri in enumerate(corners):                                   # the fixed-point corners are the intended ones, exactly
        for c, (sx, sy, _) in enumerate(tri):
            assert (int(X[3 * t + c]), int(Y[3 * t + c])) == (int(Fraction(sx) * 256), int(Fraction(sy) * 256))
    return out


TRIANGLES = [
    ((2, 2, 64), (10, 2, 64), (2, 8, 64)),                               # legs along pixel rows and columns, hypotenuse through centres
    ((2, 2, 64), (2, 8, 64), (10, 2, 64)),                               # the other winding
    ((3.5, 1.25, 128), (12.75, 4.5, 128), (5.0, 10.0, 128)),             # a vertex on a pixel centre, edges through none... or some
    ((0, 0, 32), (15, 0, 32), (15, 11, 32)),                             # corner to corner of the image
    ((4, 4, 64), (8, 8, 64), (4, 8, 64)),                                # a diagonal through centres
    ((4.5, 4.5, 64), (4.5 + 1 / 256, 4.5, 64), (4.5, 4.5 + 1 / 256, 64)),  # the smallest triangle: between centres
    ((-3, -2, 64), (20, 5, 64), (6, 15, 64)),                            # partly off every side
    ((5, 5, 64), (9, 5, 64), (13, 5, 64)),                               # zero area
]


def test_coverage_agrees_with_exact_arithmetic_and_centres_lie_on_edges():
    on_edges = 0
    for tri in TRIANGLES:
        out = coverage_of([tri])
        cov = out["coverage"]
        for j in range(H):
            for i in range(W):
                want, on_edge = exact_cover(tri, i, j)
                assert bool(cov[j, i]) == want, (tri, i, j)
                on_edges += on_edge
        hit = out["triangle"].reshape(H, W) != ref.MISS
        assert np.array_equal(hit, cov > 0)                              # fronto-parallel, inside [near, far]: every covered pixel is a fragment
    assert on_edges > 0                                                  # by the exact side alone: the inputs really put centres on edges


def test_two_triangles_that_share_an_edge_cover_each_centre_on_it_once():
    pairs = [(((2, 2, 64), (10, 2, 64), (10, 10, 64)), ((2, 2, 64), (10, 10, 64), (2, 10, 64))),       # the diagonal of a square
             (((2, 2, 64), (10, 10, 64), (10, 2, 64)), ((2, 2, 64), (10, 10, 64), (2, 10, 64))),       # one of them wound the other way
             (((6, 1, 64), (6, 11, 64), (1, 6, 64)), ((6, 1, 64), (14, 6, 64), (6, 11, 64))),          # a vertical shared edge on a pixel column
             (((1, 6, 64), (14, 6, 64), (6, 1, 64)), ((1, 6, 64), (6, 11, 64), (14, 6, 64)))]          # a horizontal one on a pixel row
    on_shared = 0
    for a, b in pairs:
        cov = coverage_of([a, b])["coverage"]
        shared = [c for c in a if c in b]
        assert len(shared) == 2
        (ax, ay, _), (bx, by, _) = shared
        for j in range(H):
            for i in range(W):
                cross = (Fraction(bx) - Fraction(ax)) * (j - Fraction(ay)) - (Fraction(by) - Fraction(ay)) * (i - Fraction(ax))
                between = min(ax, bx) <= i <= max(ax, bx) and min(ay, by) <= j <= max(ay, by)
                if cross == 0 and between and (i, j) not in ((ax, ay), (bx, by)):
                    on_shared += 1
                    assert cov[j, i] == 1, (a, b, i, j)
        assert cov.max() == 1
    assert on_shared > 0


def test_a_fan_that_tiles_the_image_covers_every_pixel_exactly_once():
    hub = (8, 6, 64)                                                     # on a pixel centre
    rim = [(-0.5, -0.5), (8, -0.5), (W - 0.5, -0.5), (W - 0.5, 6), (W - 0.5, H - 0.5), (8, H - 0.5), (-0.5, H - 0.5), (-0.5, 6)]
    for order in (1, -1):
        fan = [(hub, rim[k] + (64,), rim[(k + 1) % 8] + (64,))[::order] for k in range(8)]
        out = coverage_of(fan)
        assert (out["coverage"] == 1).all()
        assert (out["triangle"] != ref.MISS).all() and out["info"]["n_pixels_hit"] == W * H
        assert set(out["triangle"].tolist()) == set(range(8))
    # with back faces culled the clockwise fan (A2 > 0 ... or < 0) is all there or all gone
    kept = [coverage_of([(hub, rim[k] + (64,), rim[(k + 1) % 8] + (64,))[::order] for k in range(8)], ref.CULL_BACK)["info"]["n_live"] for order in (1, -1)]
    assert sorted(kept) == [0, 8]


def test_fronto_parallel_triangles_at_a_power_of_two_depth_give_exactly_that_depth():
    for z in (2.0, 64.0, 1024.0, 4096.0):
        out = coverage_of([((1.25, 0.5, z), (14.5, 2.75, z), (6.0, 11.0, z))])
        hit = out["triangle"] != ref.MISS
        assert hit.sum() > 20
        assert (out["z"][hit] == F(z)).all() and np.isnan(out["z"][~hit]).all()
        assert (out["depth"][hit] == int(z)).all() and (out["depth"][~hit] == 0).all()
        assert (out["vertices"][hit, 2] == F(z)).all()
        assert np.array_equal(out["normals"][hit], np.tile(np.array([0, 0, 1], F), (hit.sum(), 1)))   # cross(V1 - V0, V2 - V0): a back face here


def test_permuting_the_triangles_keeps_the_depths_and_maps_the_ids():
    rng = np.random.default_rng(11)
    corners = []
    for t in range(40):
        z = float(2 ** (t + 1))                                          # a depth of its own: only the copies below tie
        corners.append(tuple((float(rng.integers(-2 * 4, (W + 2) * 4)) / 4, float(rng.integers(-2 * 4, (H + 2) * 4)) / 4, z) for _ in range(3)))
    corners += corners[:5]                                               # identical triangles: the smaller index wins
    far = float(2 ** 41)
    base = coverage_of(corners, far=far)
    assert base["info"]["n_pixels_hit"] > W * H // 2
    perm = rng.permutation(len(corners))
    moved = coverage_of([corners[p] for p in perm], far=far)
    assert ref.same_bytes(base["z"], moved["z"]) and ref.same_bytes(base["depth"], moved["depth"])
    hit = base["triangle"] != ref.MISS
    assert np.array_equal(hit, moved["triangle"] != ref.MISS)
    # the id image names the same geometry: the winner of `moved` is a copy of the winner of `base` at the smallest new index
    new_index = {}
    for new, old in enumerate(perm):
        new_index.setdefault(corners[old], new)
    want = np.array([new_index[corners[t]] for t in base["triangle"][hit]], np.uint32)
    assert np.array_equal(moved["triangle"][hit], want)
    assert (base["triangle"][hit] < 40).all()                            # never the later copy


def test_extract_surface_wiring_is_front_facing_from_outside_and_normals_point_out():
    """Host marching cubes of a sphere (distance positive outside, as a fused surface has it), seen from outside."""
    import tsdf_amd
    n = 16
    c = (np.arange(n) + 0.5) * 10.0
    zz, yy, xx = np.meshgrid(c, c, c, indexing="ij")
    D = (np.sqrt((xx - 80) ** 2 + (yy - 80) ** 2 + (zz - 80) ** 2) - 50).astype(F)
    V = tsdf_amd.marching_cubes(D.reshape(-1), (n, n, n), (10.0, 10.0, 10.0))
    I = np.arange(len(V), dtype=np.uint32)
    inv_pose = np.eye(4, dtype=F)
    inv_pose[:3, 3] = (-80, -80, 200)
    inv_pose = inv_pose.T.reshape(-1)                                    # column-major
    k = np.array([64, 0, 0, 0, 64, 0, 32, 24, 1], F)
    both = ref.render(V, I, 64, 48, inv_pose, k, 1.0, 1000.0)
    culled = ref.render(V, I, 64, 48, inv_pose, k, 1.0, 1000.0, ref.CULL_BACK)
    assert both["info"]["n_pixels_hit"] > 300
    for name in ("triangle", "z", "depth", "vertices", "normals"):
        assert ref.same_bytes(both[name], culled[name]), name            # the front faces are the ones that were seen
    assert culled["info"]["n_live"] < both["info"]["n_live"] * 0.6
    hit = both["triangle"] != ref.MISS
    assert (((both["vertices"][hit] - 80.0) * both["normals"][hit]).sum(axis=1) > 0).all()     # out of the sphere
    assert (both["normals"][hit, 2] < 0).all()                           # towards the camera
