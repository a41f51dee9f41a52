"""Volume fusion at the places the seeded sweep (tests/test_fuse_sweep.py) cannot reach by drawing: a sparse source the cull must drop
bricks for, a box at and over the cull's 4096-byte limit, matrices whose products overflow, points exactly on the source's lattice,
every layout of the destination's last weight dword, the boundaries of the widening rule, and a fuse between two pipeline steps.
Every case is a dict like fuse_cases.case's and goes through the sweep's assert_fuse; every group has a precondition on the reference
alone that runs without a GPU."""
import functools

import numpy as np
import pytest

import tsdf_amd
from tests import fuse_cases as fc
from tests import fuse_ref
from tests.helpers import H, W, assert_same_floats, camera_at
from tests.test_fuse import AXIS, SHIFT, assert_state, frame, state
from tests.test_fuse_sweep import assert_fuse, gpu_pair

F = np.float32


def smooth(dims, amp, seed):
    rng = np.random.default_rng(seed)
    zi, yi, xi = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    return (amp * np.sin(0.31 * xi + 0.23 * yi + 0.17 * zi) + rng.normal(0, 0.05 * amp, xi.shape)).astype(F).reshape(-1)


def grid(dims, physical, offset=(0.0, 0.0, 0.0), trunc=None):
    return {"dims": tuple(dims), "physical": tuple(float(p) for p in physical), "offset": tuple(float(o) for o in offset), "trunc": trunc}


def make(dst, src, src_dist, src_weight, matrix=None, dst_dist=None, dst_weight=None, cap=0, dst_bits=8, src_bits=8):
    n = int(np.prod(dst["dims"]))
    dst_weight = np.zeros(n, F) if dst_weight is None else np.asarray(dst_weight, F)
    src_weight = np.asarray(src_weight, F)
    return {"dst": dst, "src": src, "src_dist": np.asarray(src_dist, F), "src_weight": src_weight, "dst_dist": dst_dist, "dst_weight": dst_weight,
            "matrix": np.eye(4, dtype=F).reshape(-1) if matrix is None else np.asarray(matrix, F), "cap": cap,
            "dst_storage": max(dst_bits, fc.needed_storage(dst_weight)), "src_storage": max(src_bits, fc.needed_storage(src_weight))}


def about(centre, axis, degrees):
    """A turn about `centre`: x -> R (x - centre) + centre."""
    R = fuse_ref.rotation(axis, degrees).reshape(4, 4).T[:3, :3].astype(np.float64)
    c = np.asarray(centre, np.float64)
    return fuse_ref.rotation(axis, degrees, c - R @ c)


def translation(t):
    m = np.eye(4, dtype=F)
    m[:3, 3] = t
    return m.T.reshape(-1).copy()


@functools.lru_cache(maxsize=None)
def ref(build, *args):
    """(case, reference) of build(*args): computed once a process."""
    import oracle as O
    O.build()
    c = build(*args)
    return c, fc.reference_of(O, c)


def run(c, r, what, **kw):
    dst, src = gpu_pair(c)
    out = assert_fuse(c, r, dst, src, what, **kw)
    dst.close()
    src.close()
    return out


# ---- sparse source ------------------------------------------------------------------------------------------------------------------
def sparse(degrees):
    w = np.zeros((40, 40, 40), F)
    w[16:24, 16:24, 16:24] = 2
    m = about((320.0, 320.0, 320.0), (1.0, 2.0, 3.0), degrees) if degrees else None
    return make(grid((130, 9, 66), (640.0,) * 3), grid((40, 40, 40), (640.0,) * 3), smooth((40, 40, 40), 30.0, 1), w, m)


@pytest.mark.parametrize("degrees", (0, 30))
def test_sparse_source_precondition(degrees):
    c, r = ref(sparse, degrees)
    kept = fc.bricks_updated(r.updated, c["dst"]["dims"])
    most, finite = fc.cull_upper_bound(r.dgeom, r.sgeom, c["matrix"], c["src_weight"])
    assert kept.size == 27 and 1 <= kept.sum() <= most < 27 and finite
    assert r.updated.sum() >= 200        # (the block's 7^3 tap cells, 112 mm a side, hold about 23 x 1.5 x 11.5 destination voxels)


@pytest.mark.gpu
@pytest.mark.parametrize("degrees", (0, 30))
def test_sparse_source_drops_bricks(degrees):
    c, r = ref(sparse, degrees)
    listed, total = run(c, r, "sparse source, %d degrees" % degrees)
    assert listed < total == 27


# ---- the cull's box limit -----------------------------------------------------------------------------------------------------------
def box_limit(n, observed):
    """A 5 degree turn and a scale of 1.3 about the centre: the brick's corner voxels land outside the source on every axis, so the
    clamped box is the whole grid."""
    m = about((n * 4.0,) * 3, (3.0, 1.0, 2.0), 5.0).reshape(4, 4).T.astype(np.float64)
    m[:3, :3] *= 1.3
    m[:3, 3] = n * 4.0 - m[:3, :3] @ np.full(3, n * 4.0)
    return make(grid((16, 4, 8), (n * 8.0,) * 3), grid((n, n, n), (n * 8.0,) * 3), smooth((n, n, n), 20.0, 2),
                np.full(n ** 3, 1 if observed else 0, F), m.T.astype(F).reshape(-1).copy(),
                dst_dist=smooth((16, 4, 8), 10.0, 3), dst_weight=np.full(512, 2, F))


@pytest.mark.parametrize("n", (128, 136))
def test_box_limit_precondition(n):
    """One destination brick over the whole source: 16^3 = 4096 summary bytes at 128^3 (looked at), 17^3 at 136^3 (kept unseen)."""
    c, r = ref(box_limit, n, True)
    assert fc.brick_counts(c["dst"]["dims"]) == (1, 1, 1) and r.updated.mean() > 0.2
    # the cull's box without its slack: every voxel's q (the corners among them), two voxels either side, clamped, in summary bricks
    cells = 1
    for a in r.detail["q"]:
        lo, hi = max(int(np.floor(a.min() / 8.0)) - 2, 0), min(int(np.floor(a.max() / 8.0)) + 2, n - 1)
        cells *= (hi >> 3) - (lo >> 3) + 1
    assert cells == (4096 if n == 128 else 4913)


@pytest.mark.gpu
@pytest.mark.parametrize("n, observed", ((128, True), (136, True), (128, False), (136, False)))
def test_box_at_and_over_the_limit(n, observed):
    c, r = ref(box_limit, n, observed)
    listed, total = run(c, r, "%d^3 source, weights %d" % (n, observed), upper=False)
    assert total == 1
    if observed:
        assert listed == 1
    else:   # nothing observed: the box at the limit is looked at and the brick dropped; over it the brick is kept unseen
        assert r.updated.sum() == 0 and listed == (0 if n == 128 else 1)


# ---- off the scale ------------------------------------------------------------------------------------------------------------------
OFF_SCALE = ("t1e8", "t1e12", "t3e38", "r1e30", "r3e38")


def off_scale(which):
    m = np.eye(4, dtype=F)
    if which == "t1e12":
        m[:3, 3] = (1e12, -1e12, 1e12)
    elif which == "t1e8":
        m[:3, 3] = (1e8, 0.0, 0.0)
    elif which == "t3e38":
        m[:3, 3] = (3e38, 3e38, -3e38)
    else:
        m[:3, :3] = np.array([[1, -1, 1], [1, 1, -1], [-1, 1, 1]]) * (1e30 if which == "r1e30" else 3e38)
    return make(grid((70, 6, 37), (700.0, 60.0, 370.0), (300.0, 0.0, -200.0)), grid((20, 20, 20), (400.0,) * 3, (50.0, 60.0, 70.0)),
                smooth((20, 20, 20), 15.0, 4), np.full(8000, 3, F), m.T.reshape(-1).copy(), dst_dist=smooth((70, 6, 37), 10.0, 5),
                dst_weight=np.full(70 * 6 * 37, 7, F))


@pytest.mark.parametrize("which", OFF_SCALE)
def test_off_the_scale_precondition(which):
    c, r = ref(off_scale, which)
    assert r.updated.sum() == 0 and np.isfinite(c["matrix"]).all()
    q = np.stack(r.detail["q"])
    if which == "r3e38":
        assert np.isinf(q).sum() >= 1000 and np.isnan(q).sum() >= 1000      # products overflow, and inf - inf
    else:   # finite and outside; in source voxels of 20 mm below 1e9 for t1e8 alone (the cull drops), beyond an int for the others
        assert np.isfinite(q).all() and (np.abs(q).max(axis=0) > (1e7 if which == "t1e8" else 1e11)).all()
        assert (np.abs(q).max() / 20 < 1e9) == (which == "t1e8")


@pytest.mark.gpu
@pytest.mark.parametrize("which", OFF_SCALE)
def test_off_the_scale_fuses_nothing(which):
    c, r = ref(off_scale, which)
    dst, src = gpu_pair(c)
    before = state(dst)
    assert dst.fuse(src, c["matrix"]) == 0
    after = state(dst)
    assert_same_floats(after[0], before[0], "distances")
    assert_same_floats(after[1], before[1], "weights")
    assert after[2] == before[2] and state(src)[2] == (8, False)
    listed, total = dst.last_fuse_bricks()
    # wholly outside: dropped; beyond 1e9 voxels or not finite: no statement about the box, every brick kept unseen (fuse_cull_kernel)
    assert total == 8 and listed == (0 if which == "t1e8" else 8)
    dst.close()
    src.close()


# ---- exact lattice ------------------------------------------------------------------------------------------------------------------
LATTICE_DST, LATTICE_SRC = (24, 10, 34), (20, 18, 22)
# translations in units of 8 mm, half a voxel: -1 puts the first plane of q on 0, 2 (S - D) + 1 the last plane on the upper bound
LATTICE_K = ((0, 0, 0), (-1, -1, -1), tuple(2 * (s - d) + 1 for s, d in zip(LATTICE_SRC, LATTICE_DST)), (1, 16, -25), (2, 7, -12), (-2, 17, -23))


def lattice(k):
    rng = np.random.default_rng(6)
    nd, ns = int(np.prod(LATTICE_DST)), int(np.prod(LATTICE_SRC))
    return make(grid(LATTICE_DST, [d * 16.0 for d in LATTICE_DST]), grid(LATTICE_SRC, [s * 16.0 for s in LATTICE_SRC]),
                smooth(LATTICE_SRC, 25.0, 7), rng.integers(1, 4, ns).astype(F), translation([8.0 * a for a in k]),
                dst_dist=smooth(LATTICE_DST, 20.0, 8), dst_weight=rng.integers(0, 3, nd).astype(F))


def test_exact_lattice_precondition():
    on_faces = on_centres = first_on_zero = last_on_bound = 0
    for k in LATTICE_K:
        c, r = ref(lattice, k)
        assert r.dgeom[1].tolist() == [16.0] * 3 and r.sgeom[1].tolist() == [16.0] * 3
        q = np.stack(r.detail["q"]).astype(np.float64)
        on_faces += int(((q / 16) % 1 == 0).all(axis=0).sum())
        on_centres += int(((q / 8) % 2 == 1).all(axis=0).sum())
        first_on_zero += int((q.min(axis=1) == 0).sum())
        last_on_bound += int((q.max(axis=1) == np.array(LATTICE_SRC) * 16.0).sum())
        assert r.updated.sum() >= 100
    assert on_faces >= 1000 and on_centres >= 1000 and first_on_zero >= 3 and last_on_bound >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("k", LATTICE_K)
def test_points_exactly_on_the_lattice(k):
    c, r = ref(lattice, k)
    run(c, r, "lattice, translation %s x 8 mm" % (k,))


# ---- destination layout -------------------------------------------------------------------------------------------------------------
LAYOUT_PHYS, LAYOUT_OFF = (2900.0, 3100.0, 3300.0), (-150.0, 40.0, 275.0)     # the box of tests/test_fuse.py: frame(18) sees it


def layout(bits, Z, xy):
    dims = (xy[0], xy[1], Z)
    rng = np.random.default_rng(9)
    n = int(np.prod(dims))
    sd = (37, 34, 45)
    return make(grid(dims, LAYOUT_PHYS, LAYOUT_OFF), grid(sd, (3000.0,) * 3, (60.0, -90.0, 120.0)), smooth(sd, 120.0, 10),
                rng.integers(1, 4, int(np.prod(sd))).astype(F), fuse_ref.rotation(AXIS, 20.0, SHIFT), dst_dist=smooth(dims, 100.0, 11),
                dst_weight=rng.integers(0, 3, n).astype(F), dst_bits=bits)


LAYOUTS = [(bits, Z, xy) for bits in (8, 16) for Z in (33, 34, 35, 65) for xy in ((64, 4), (65, 5), (1, 1))]


def test_destination_layout_precondition():
    for bits, Z, xy in LAYOUTS:
        c, r = ref(layout, bits, Z, xy)
        g = r.updated.reshape(Z, xy[1], xy[0])
        assert g[32:].any() and g[:32].any(), (bits, Z, xy)                   # both layers of bricks
        if xy != (1, 1):
            assert g[Z - 1].any() and (~g[Z - 1]).any(), (bits, Z, xy)        # the last dword: updated and skipped lanes
        assert c["dst_storage"] == bits == fc.storage_after(bits, c["dst_weight"], 0, c["src_weight"])


@pytest.mark.gpu
@pytest.mark.parametrize("bits, Z, xy", LAYOUTS)
def test_destination_layout_then_an_integrate(oracle, bits, Z, xy):
    c, r = ref(layout, bits, Z, xy)
    dst, src = gpu_pair(c)
    assert_fuse(c, r, dst, src, "layout %d bits, %s x %d" % (bits, xy, Z))
    d, cam = frame(18)
    dst.integrate(d, W, H, cam)
    ov = fc.oracle_volume(oracle, c["dst"])
    ov.set_distance_data(r.dist)
    ov.set_weight_data(r.weight)
    ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    assert_state(dst, ov.dist, ov.weight, "fuse, then integrate")
    if xy != (1, 1):
        assert (ov.weight != r.weight).sum() >= 10                           # the frame reached the grid
    dst.close()
    src.close()


# ---- widening boundaries ------------------------------------------------------------------------------------------------------------
WIDEN = {255: (250, 5, 0, 8, 8), 256: (250, 6, 0, 8, 16), 65535: (65000, 535, 0, 16, 16), 65536: (65000, 536, 0, 16, 32),
         "cap 255": (250, 150, 255, 8, 8), "cap 300": (250, 150, 300, 8, 16)}      # dst top, src top, cap, storage before, after


def widen(key):
    top_d, top_s, cap = WIDEN[key][:3]
    dd, sd = (70, 6, 37), (20, 20, 20)
    return make(grid(dd, (700.0, 60.0, 370.0)), grid(sd, (400.0,) * 3, (50.0, -20.0, 70.0)), smooth(sd, 15.0, 12),
                np.full(8000, top_s, F), about((200.0, 30.0, 180.0), (1.0, 1.0, 0.0), 15.0), dst_dist=smooth(dd, 10.0, 13),
                dst_weight=np.full(int(np.prod(dd)), top_d, F), cap=cap)


@pytest.mark.parametrize("key", list(WIDEN))
def test_widening_precondition(key):
    """Every weight is the top count on both sides, so every updated voxel holds exactly the sum (or the cap)."""
    top_d, top_s, cap, before, after = WIDEN[key]
    c, r = ref(widen, key)
    assert c["dst_storage"] == before and fc.storage_after(before, c["dst_weight"], cap, c["src_weight"]) == after
    assert r.updated.sum() >= 500 and (~r.updated).sum() >= 500
    want = min(top_d + top_s, cap) if cap else top_d + top_s
    assert (r.weight[r.updated] == want).all() and (key in (255, 256, 65535, 65536)) == (want == key)
    if cap:   # the divisor is the sum, not the cap: the distances are those of the fuse without a cap
        import oracle as O
        c0 = dict(c, cap=0)
        assert np.array_equal(fc.reference_of(O, c0).dist.view(np.uint32), r.dist.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(WIDEN))
def test_widening_boundaries(key):
    c, r = ref(widen, key)
    dst, src = gpu_pair(c)
    assert_fuse(c, r, dst, src, "widening, %s" % (key,))
    assert dst.weight_storage() == (WIDEN[key][4], False)
    dst.close()
    src.close()


# ---- between pipeline steps ---------------------------------------------------------------------------------------------------------
PIPE_DIMS, PIPE_PHYS = (64, 40, 36), (1920.0, 1200.0, 1080.0)


def pipe_case(top):
    sd = (30, 28, 26)
    return make(grid(PIPE_DIMS, PIPE_PHYS), grid(sd, (900.0, 840.0, 780.0), (400.0, 200.0, 150.0)), smooth(sd, 60.0, 14),
                np.full(int(np.prod(sd)), top, F), about((960.0, 600.0, 540.0), (2.0, 1.0, 3.0), 10.0))


def pipe_frame():
    d = np.zeros((H, W), np.uint16)
    d[120:360, 160:480] = 1250
    return d.reshape(-1), camera_at((960.0, 600.0, -700.0))


@functools.lru_cache(maxsize=None)
def pipe_reference(top):
    """The oracle's integrate of the filtered frame, the reference's fuse from that state, the oracle's integrate again."""
    import oracle as O
    O.build()
    c = pipe_case(top)
    d, cam = pipe_frame()
    f = O.bilateral_u16(d, W, H, 30.0, 4.5, nthreads=O.max_threads()).reshape(-1)
    ov = fc.oracle_volume(O, c["dst"])
    step = lambda: ov.integrate(f, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=O.max_threads())
    step()
    c["dst_dist"], c["dst_weight"] = ov.dist.copy(), ov.weight.copy()
    r = fc.reference_of(O, c)
    ov.set_distance_data(r.dist)
    ov.set_weight_data(r.weight)
    step()
    return c, r, ov.dist.copy(), ov.weight.copy()


@pytest.mark.parametrize("top", (3, 255))
def test_pipeline_precondition(top):
    c, r, d, w = pipe_reference(top)
    assert c["dst_weight"].max() == 1 and fc.storage_after(8, c["dst_weight"], 0, c["src_weight"]) == (16 if top == 255 else 8)
    both = r.updated & (c["dst_weight"] > 0)
    assert both.sum() >= 500 and (w[both] == top + 2).all() and w.max() == top + 2     # frame, fuse, frame in the same voxels


@pytest.mark.gpu
@pytest.mark.parametrize("top", (3, 255))
def test_a_fuse_between_two_pipeline_steps(top):
    """The first step leaves the next frame's brick list prepared ahead; the fuse keeps it when the storage stays (top 3) and drops
    it when the counts widen to 16 bits (1 + 255); the second step's integrate gives the oracle's volume either way."""
    import torch
    from tsdf_amd.pipeline import FusionPipeline
    c, r, want_d, want_w = pipe_reference(top)
    d, cam = pipe_frame()
    dst = tsdf_amd.TSDFVolume(PIPE_DIMS, PIPE_PHYS)
    src = tsdf_amd.TSDFVolume(c["src"]["dims"], c["src"]["physical"])
    src.offset(*c["src"]["offset"])
    src.set_distance_data(c["src_dist"])
    src.set_weight_data(c["src_weight"])
    pipe = FusionPipeline(dst, tsdf_amd.BilateralFilter(30.0, 4.5), tsdf_amd.GPURaycaster(W, H), W, H, overlap=True)
    bufs = (torch.from_numpy(d.view(np.int16)).cuda(), torch.from_numpy(d.view(np.int16)).cuda())
    vert = torch.empty((H * W, 3), dtype=torch.float32, device="cuda")
    norm = torch.empty_like(vert)
    pipe.step(bufs[0].data_ptr(), cam, vert.data_ptr(), norm.data_ptr(), bufs[1].data_ptr(), cam)
    assert dst.fuse(src, c["matrix"]) == int(r.updated.sum())
    assert dst.weight_storage() == (16 if top == 255 else 8, False)
    pipe.step(bufs[1].data_ptr(), cam, vert.data_ptr(), norm.data_ptr(), None, None)
    pipe.synchronize()
    assert_state(dst, want_d, want_w, "step, fuse, step")
    pipe.close()
    dst.close()
    src.close()
