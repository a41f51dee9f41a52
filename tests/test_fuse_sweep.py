"""A seeded sweep of volume fusion (tsdf_amd/csrc/fuse.hip) against its CPU reference (tests/fuse_ref.py) over the grids, transforms,
contents and storages of tests/fuse_cases.py, with the cull looked at from both sides: it must list every brick the reference updates
a voxel of, and no more than the documented design allows.  The conditions on the reference alone run without a GPU."""
import numpy as np
import pytest

import tsdf_amd
from tests import fuse_cases as fc
from tests import fuse_ref
from tests.helpers import Cam, assert_same_floats
from tests.test_fuse import assert_state, set_truncation

F = np.float32
CAST_W, CAST_H = 64, 48


def gpu_volume(spec):
    v = tsdf_amd.TSDFVolume(spec["dims"], spec["physical"])
    v.offset(*spec["offset"])
    if spec["trunc"]:
        set_truncation(v, spec["trunc"])
    return v


def gpu_pair(c):
    """The two volumes of a case (fuse_cases.case), filled and in the storage the case states."""
    dst, src = gpu_volume(c["dst"]), gpu_volume(c["src"])
    src.set_distance_data(c["src_dist"])
    src.set_weight_data(c["src_weight"])
    if c["dst_dist"] is not None:
        dst.set_distance_data(c["dst_dist"])
    dst.set_weight_data(c["dst_weight"])
    for vol, bits in ((dst, c["dst_storage"]), (src, c["src_storage"])):
        if vol.weight_storage()[0] != bits:
            vol.set_weight_storage(bits)
        assert vol.weight_storage() == (bits, False)
    if c["cap"]:
        dst.set_weight_cap(c["cap"])
    return dst, src


def assert_fuse(c, r, dst, src, what, upper=True):
    """One fuse of a case against its reference: count, bits, the source untouched, the cull's list between its two bounds
    (upper=False: the lower one alone, for the cases that reach the cull's 4096-byte limit)."""
    assert_same_floats(dst.get_distance_data(), r.start_d, what + ": distances before")
    assert fuse_ref.geometry(dst)[1].tolist() == r.dgeom[1].tolist() and fuse_ref.geometry(src)[1].tolist() == r.sgeom[1].tolist()
    assert dst.truncation_distance() == r.trunc
    n = dst.fuse(src, c["matrix"])
    listed, total = dst.last_fuse_bricks()
    kept = fc.bricks_updated(r.updated, c["dst"]["dims"])
    assert total == kept.size == int(np.prod(fc.brick_counts(c["dst"]["dims"])))
    assert listed >= int(kept.sum()), "%s: the cull listed %d bricks, the reference updates voxels in %d" % (what, listed, kept.sum())
    assert n == int(r.updated.sum())
    assert_state(dst, r.dist, r.weight, what)
    assert dst.weight_storage() == (fc.storage_after(c["dst_storage"], c["dst_weight"], c["cap"], c["src_weight"]), False)
    assert_state(src, c["src_dist"], c["src_weight"], what + ": source after")
    assert src.weight_storage() == (c["src_storage"], False)
    if upper:
        most, finite = fc.cull_upper_bound(r.dgeom, r.sgeom, c["matrix"], c["src_weight"])
        assert finite, what + ": a box of the cull is not finite"
        assert listed <= most, "%s: the cull listed %d bricks, the design allows %d" % (what, listed, most)
    return listed, total


def assert_cast_after(c, r, dst, what):
    """The occupancy hand-over: a cast of the fused volume against a cast of a fresh volume that holds the reference's distances."""
    dims, vs, off = r.dgeom
    ext = np.array(dims) * vs.astype(np.float64)
    centre = off + ext / 2
    cam = tsdf_amd.Camera.default_depth_camera()
    cam.move_to(*(centre + np.array([0.3, 0.2, -1.0]) * (ext.max() * 1.5 + 100.0)))
    cam.look_at(*centre)
    import oracle
    k, kinv = oracle.camera_k(591.1 / 10, 590.1 / 10, CAST_W / 2, CAST_H / 2)
    cam = Cam(cam.pose(), cam.inverse_pose(), k, kinv)
    caster = tsdf_amd.GPURaycaster(CAST_W, CAST_H)
    v, n = caster.raycast(dst, cam)
    fresh = gpu_volume(c["dst"])
    fresh.set_distance_data(r.dist)
    fv, fn = caster.raycast(fresh, cam)
    fresh.close()
    assert_same_floats(v, fv, what + ": vertices after the fuse")
    assert_same_floats(n, fn, what + ": normals after the fuse")


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------
def test_batched_trilinear_is_the_single_call(oracle):
    """orc_trilinear_n against orc_trilinear, bit for bit, on points inside, on faces and centres, outside and not finite."""
    rng = np.random.default_rng(0x7121)
    dims, vs = (7, 5, 9), np.array([10.0, 12.5, 7.0], F)
    dist = rng.normal(0, 30, 7 * 5 * 9).astype(F)
    dist[[3, 100]] = np.nan
    ext = np.array(dims) * vs
    P = np.concatenate([rng.uniform(-0.1, 1.1, (3000, 3)) * ext, rng.integers(-1, 2 * np.array(dims) + 2, (1000, 3)) * (vs / 2),
                        [[np.nan, 1, 1], [np.inf, 1, 1], [1, -np.inf, 1], [-0.0, 0.0, -0.0]]]).astype(F)
    with np.errstate(all="ignore"):
        many = oracle.trilinear_n(P, dims, vs, dist)
        one = np.array([oracle.trilinear(p, dims, vs, dist) for p in P], F)
    assert np.isnan(one).sum() >= 10 and (~np.isnan(one)).sum() >= 3000
    assert_same_floats(many, one, "orc_trilinear_n")


def test_every_kind_occurs_in_the_seed_range():
    cases = [fc.case(s) for s in fc.SEEDS]
    assert len(cases) >= 32
    assert {c["matrix_kind"] for c in cases} == set(fc.MATRIX_KINDS)
    assert {c["weight_kind"] for c in cases} == set(fc.WEIGHT_KINDS)
    assert {(c["dst_storage"], c["src_storage"]) for c in cases} == {(d, s) for d in fc.STORAGES for s in fc.STORAGES}
    assert {c["cap"] for c in cases} == set(fc.CAPS)
    X, Y, Z = ({c["dst"]["dims"][a] for c in cases} for a in range(3))
    assert {63, 64, 65} <= X and {1, 4, 5} <= Y and {31, 32, 33} <= Z and any(z > 32 and z % 2 for z in Z)
    assert 1 in X and 1 in Z
    assert max(int(np.prod(c["dst"]["dims"])) for c in cases) <= fc.MAX_DST and max(int(np.prod(c["src"]["dims"])) for c in cases) <= fc.MAX_SRC
    src = [c["src"]["dims"] for c in cases]
    assert sum(1 in d for d in src) >= 6 and sum(any(n % 8 for n in d) for d in src) >= 32       # one-voxel axes, partial summary bricks
    # edges: cubic and not, on either side; round (powers of two) and arbitrary; the ratio of edges over about 1/6 .. 6
    edge = lambda g: np.array(g["physical"]) / np.array(g["dims"])
    ratio = np.array([edge(c["dst"]).mean() / edge(c["src"]).mean() for c in cases])
    assert ratio.min() < 0.3 and ratio.max() > 3.5 and ratio.min() >= 1 / 8 and ratio.max() <= 8    # (1/6 .. 6, then rounded to a power of two)
    for side in ("dst", "src"):
        e = [edge(c[side]) for c in cases]
        assert sum(np.ptp(x) == 0 for x in e) >= 8 and sum(np.ptp(x) > 0 for x in e) >= 8
        assert sum(bool((np.log2(x) % 1 == 0).all()) for x in e) >= 8 and sum(bool((np.log2(x) % 1 != 0).all()) for x in e) >= 8
        off = [np.abs(c[side]["offset"]).max() for c in cases]
        assert sum(o == 0 for o in off) >= 6 and sum(0 < o <= 400 for o in off) >= 6 and sum(o >= 5000 for o in off) >= 6
        assert sum(c[side]["trunc"] is None for c in cases) >= 8 and sum(c[side]["trunc"] is not None for c in cases) >= 8
    assert sum(c["small"] for c in cases) >= 8 and all((edge(c["src"]) < 1).all() == c["small"] for c in cases)
    assert sum(c["dst_cleared"] for c in cases) >= 8 and sum(not c["dst_cleared"] for c in cases) >= 8


def test_the_sweep_is_not_vacuous():
    """The reference alone over range(64), no seed left out.  Seeds reached (the bound asserted in brackets): between 2 % and 98 % of
    the destination updated 40 (32); a destination brick without an updated voxel 29 (16); updated voxels in a brick with bz > 0
    28 (6); in the partial last dword of 16-bit counts 7 (6); a sample beyond the destination's truncation before the clamp 41 (6); a
    NaN sample behind eight observed taps 15 (4); an explicit source truncation above the destination's 11, below it 16 (4 each)."""
    n = dict.fromkeys(("band", "idle brick", "bz > 0", "partial 16-bit dword", "clamped", "NaN sample", "source truncation above", "below"), 0)
    for seed in fc.SEEDS:
        c, r = fc.reference(seed)
        X, Y, Z = c["dst"]["dims"]
        grid = r.updated.reshape(Z, Y, X)
        n["band"] += 0.02 <= r.updated.mean() <= 0.98
        n["idle brick"] += not fc.bricks_updated(r.updated, c["dst"]["dims"]).all()
        n["bz > 0"] += bool(grid[32:].any())
        after = fc.storage_after(c["dst_storage"], c["dst_weight"], c["cap"], c["src_weight"])
        n["partial 16-bit dword"] += bool(Z % 2 == 1 and after == 16 and grid[Z - 1].any())
        s = r.detail["sample"][r.detail["tapped"]]
        with np.errstate(invalid="ignore"):
            n["clamped"] += bool((np.abs(s) > F(r.trunc)).any())
        n["NaN sample"] += bool(np.isnan(s).any())
        if c["src"]["trunc"]:
            n["source truncation above" if c["src"]["trunc"] > r.trunc else "below"] += 1
    print(n)
    half, quarter = len(fc.SEEDS) // 2, len(fc.SEEDS) // 4
    assert n["band"] >= half and n["idle brick"] >= quarter
    assert n["bz > 0"] >= 6 and n["partial 16-bit dword"] >= 6 and n["clamped"] >= 6 and n["NaN sample"] >= 4
    assert n["source truncation above"] >= 4 and n["below"] >= 4


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", fc.SEEDS)
def test_fuse_parity_and_cull_bounds(seed):
    c, r = fc.reference(seed)
    dst, src = gpu_pair(c)
    what = "seed %d (%s, %s weights, %d <- %d bits, cap %d)" % (seed, c["matrix_kind"], c["weight_kind"], c["dst_storage"], c["src_storage"], c["cap"])
    if seed % 3 == 1:
        tsdf_amd.GPURaycaster(CAST_W, CAST_H).raycast(dst, _any_camera(r))      # (the flags of the distances before the fuse exist)
    assert_fuse(c, r, dst, src, what)
    if seed % 3 == 1:
        assert_cast_after(c, r, dst, what)
    dst.close()
    src.close()


def _any_camera(r):
    dims, vs, off = r.dgeom
    ext = np.array(dims) * vs.astype(np.float64)
    cam = tsdf_amd.Camera.default_depth_camera()
    cam.move_to(*(off + ext / 2 + np.array([0.0, 0.0, -1.0]) * (ext.max() * 1.5 + 100.0)))
    cam.look_at(*(off + ext / 2))
    return cam


@pytest.mark.gpu
def test_both_instances_of_the_division_run_in_the_sweep():
    """src->fast_div picks the kernel instance: the proof passes for the sweep's source edges above a millimetre, round or not, and
    fails for those below (a divisor < 1 lets a / b overflow where the reciprocal sequence gives NaN)."""
    proved = {}
    for seed in fc.SEEDS:
        c = fc.case(seed)
        v = gpu_volume(c["src"])
        proved[seed] = bool(v.info().fast_division_verified)
        v.close()
    print("fast division proved in %d of %d sources" % (sum(proved.values()), len(proved)))
    small = [s for s in fc.SEEDS if fc.case(s)["small"]]
    assert len(small) >= 8 and not any(proved[s] for s in small)
    assert sum(proved.values()) >= 32
