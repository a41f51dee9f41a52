"""Seeded cases of weighted integration, as data: what tests/test_weighted_fuzz.py drives through tsdf_amd.TSDFVolume.integrate_weighted*
and tests/test_weighted_fuzz_host.py surveys on the CPU reference (tests/weighted_ref.py).  case(seed) -> dict, deterministic, no GPU.

    python -m tests.weighted_cases SEED...     prints the cases

The first len(AIMED) seeds are aimed, not drawn: each row of AIMED fixes the image, the grid, the prior state and the switches that reach
one path of integrate_weighted_kernel (tsdf_amd/csrc/integrate_body.hpp) nobody would draw -- a 1 x N image, widths round one wave, a
grid with kChunkZ + 1 planes, a brick whose pixel box exceeds the depth tile, fp32 weights so large that fl(w + p) == w.  The seeds
behind them draw grid, image, camera and depth as tests/test_fuzz_parity.py does and the rest from small lists.  Keys of a case:

    dims, phys, offset (set and baked in by a clear(), or None), prior = (kind, dist or None, weight or None) with kind one of PRIORS,
    cap, counting, colour, skew, nodes ((voxels, 3) float32 translations or None), slabs ((lo, hi) pairs or None), device (the
    device variant of the GPU test: every fourth seed), claims (names of the aimed properties the host test asserts for this seed), ops:

    ("weighted", depth, weights, rgb or None, cam, width, height)   ("plain", depth, cam, width, height)   ("remove", depth, cam, width, height)

cam = (pose, inverse_pose, k, kinv) as float32 arrays (tests.helpers.Cam(*cam)).  CaseModel is the CPU side of a case: the composed
model of tests/volume_model.py brought to the case's starting state.
"""
import functools
import sys

import numpy as np

from tests import op_sequences as S
from tests.test_fuzz_parity import random_camera, random_case, random_depth

F32, U32 = np.float32, np.uint32
BASE = 0x3E16
N_SEEDS = 48
SEEDS = tuple(range(N_SEEDS))
CHUNK_Z, BATCH_Z, TILE_PIXELS = 32, 4, 8192        # kChunkZ, kBatchZ, kTilePixels (tsdf_amd/csrc/integrate_grid.hpp)
BRICK = (64, 4, CHUNK_Z)                           # integrate's brick: one wave along x, four rows, kChunkZ planes
FLT_MAX = np.finfo(F32).max
SUBNORMAL = F32(2.0 ** -149)
# a tenth of the pixels carry one of these: six that make the pixel one without depth, two that are "finite and > 0" all the same
SPECIALS = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, SUBNORMAL, 2.0 ** -127], F32)
PRIORS = ("cleared", "counts8", "counts16", "storage16", "fp32", "pinned")
CAPS = (0, 1, 3, 300)

GRIDS = {"A": S.GRIDS[1], "B": S.GRIDS[4], "C": S.GRIDS[3], "D": S.GRIDS[2], "G": S.GRIDS[0],          # G has kChunkZ + kBatchZ planes too
         "E": ((24, 20, CHUNK_Z + BATCH_Z), (720.0, 600.0, 1080.0), None),                              # the appended batch
         "F": ((24, 20, CHUNK_Z + BATCH_Z + 1), (720.0, 600.0, 1110.0), None),                          # a second layer of bricks instead
         "T": ((64, 4, CHUNK_Z), (1600.0, 800.0, 800.0), None)}                                         # one brick, for the close camera


def _row(image, grid, prior="cleared", cap=0, counting=True, frames=2, extra=None, colour=False, skew=False, nodes=False, slabs=False,
         flt_max=False, claims=()):
    return dict(image=image, grid=grid, prior=prior, cap=cap, counting=counting, frames=frames, extra=extra, colour=colour, skew=skew,
                nodes=nodes, slabs=slabs, flt_max=flt_max, claims=tuple(claims))


# extra: what comes before the last weighted frame -- "plain": a plain integrate; "remove": a plain frame first of all, taken out
# twice before the last weighted frame (the first removal leaves 0 < w - 1 < 1, the second meets 0 < w < 1 and leaves it alone)
AIMED = (
    _row((63, 5), "A", counting=True, claims=("odd_width",)),
    _row((64, 48), "B", "counts8", cap=1, counting=False, claims=("even_width",)),
    _row((65, 40), "C", "counts16", cap=3, frames=3, extra="plain", claims=("odd_width",)),
    _row((1, 37), "D", "storage16", cap=300, counting=False, claims=("odd_width",)),
    _row((90, 61), "E", "fp32", claims=("even_width", "absorbing", "nan_prior", "subnormal")),
    _row((2, 2), "F", "pinned", counting=False, claims=("even_width",)),
    _row((112, 80), "T", claims=("tile", "even_width", "subnormal")),
    _row((63, 47), "A", colour=True, counting=False, frames=3, claims=("odd_width", "subnormal")),
    _row((64, 30), "B", "counts8", cap=3, skew=True, claims=("even_width",)),
    _row((65, 33), "C", cap=1, counting=False, nodes=True, claims=("odd_width",)),
    _row((1, 50), "D", "counts16", cap=300, claims=("odd_width",)),
    _row((57, 1), "E", counting=False, slabs=True, claims=("odd_width",)),
    _row((81, 60), "F", "fp32", frames=3, extra="remove", claims=("odd_width", "absorbing", "nan_prior", "remove_meets_fraction", "remove_leaves_fraction")),
    _row((2, 2), "G", "pinned", cap=1, claims=("even_width",)),
    _row((41, 1), "G", "storage16", counting=False, colour=True, claims=("odd_width",)),
    _row((64, 48), "G", counting=False, nodes=True, claims=("even_width",)),
    _row((80, 56), "G", counting=False, flt_max=True, claims=("even_width", "flt_max")),
    _row((33, 21), "C", skew=True, frames=3, extra="remove", claims=("odd_width", "remove_meets_fraction", "remove_leaves_fraction")),
    _row((72, 40), "G", flt_max=True, claims=("even_width", "flt_max")),
    _row((40, 30), "E", cap=300, frames=3, extra="plain", slabs=True, claims=("even_width",)),
)
FLT_MAX_SEEDS = tuple(i for i, r in enumerate(AIMED) if r["flt_max"])


# ---- the data inside a case -----------------------------------------------------------------------------------------------------------
def pixel_weights(rng, n, flt_max=False, lo=-24.0, hi=24.0):
    """Log-uniform over [2^lo, 2^hi]; on about a tenth of the pixels one of SPECIALS; FLT_MAX on four in ten where asked for."""
    p = np.exp2(rng.uniform(lo, hi, n)).astype(F32)
    s = rng.random(n) < 0.1
    p[s] = SPECIALS[rng.integers(0, SPECIALS.size, int(s.sum()))]
    if flt_max:
        p[rng.random(n) < 0.4] = FLT_MAX
    return p


def _skewed(cam):
    """The same camera with a skew term in K (column-major: K[0][1] is element 3): not the standard shape."""
    pose, inv, k, _ = cam
    k = k.copy()
    k[3] = F32(0.03) * k[0]
    kinv = np.linalg.inv(k.reshape(3, 3).T.astype(np.float64)).T.astype(F32).reshape(-1)
    return pose, inv, k, kinv


def _small_image_frame(rng, grid, image):
    """A camera across the grid whose principal point lies inside an image of a few pixels, so wide that each pixel sees a wedge of
    the grid, and a wall through the grid's centre."""
    import tsdf_amd
    dims, phys, offset = grid
    centre = np.asarray(phys) / 2.0 + (np.zeros(3) if offset is None else np.asarray(offset, np.float64))
    to = rng.normal(size=3)
    to[int(np.argmax(phys))] *= 0.2
    to /= np.linalg.norm(to)
    far = max(phys) * rng.uniform(0.9, 1.3)
    f = 0.85 * max(image[0], image[1], 4) * far / max(phys)
    cam = tsdf_amd.Camera(float(f), float(f * rng.uniform(0.9, 1.1)), image[0] / 2.0 + float(rng.uniform(-0.4, 0.4)), image[1] / 2.0 + float(rng.uniform(-0.4, 0.4)))
    cam.move_to(*(centre + to * far))
    cam.look_at(*(centre + rng.normal(size=3) * 0.03 * min(phys)))
    return S._wall_depth(rng, image, far, min(phys)), S.cam4(cam)


def _close_frame(rng, grid, image):
    """tests/test_weighted.py's close camera at the smallest size that shows it: 150 mm in front of a grid of one integrate brick, wide
    enough that the brick's voxels use pixels from every edge of a 112 x 80 image -- 8960 pixels, more than the tile holds."""
    import tsdf_amd
    dims, phys, _ = grid
    cam = tsdf_amd.Camera(30.0, 30.0, image[0] / 2.0, image[1] / 2.0)
    cam.move_to(phys[0] / 2.0 + float(rng.uniform(-5, 5)), phys[1] / 2.0, -150.0)
    cam.look_at(phys[0] / 2.0, phys[1] / 2.0, phys[2])
    d = np.full(image[0] * image[1], 550.0) + rng.integers(-20, 21, image[0] * image[1])
    return d.astype(np.uint16), S.cam4(cam)


def _prior(rng, kind, dims, phys, offset):
    """(kind, dist, weight): the arrays uploaded before the first frame, or None twice."""
    n = dims[0] * dims[1] * dims[2]
    if kind in ("cleared", "storage16", "pinned"):
        return kind, None, None
    trunc = S._truncation(dims, phys)
    dist = S._ball_field(rng, dims, phys, offset, trunc)
    if kind == "counts8":
        weight = np.where(rng.random(n) < 0.8, rng.integers(1, 256, n), 0).astype(F32)
    elif kind == "counts16":
        weight = np.where(rng.random(n) < 0.8, rng.integers(256, 65536, n), 0).astype(F32)
    else:
        # half of the distances shrunk towards 0: where a weight of 2^24 or 2^30 absorbs p, tsdf * p still moves them
        dist = (dist * np.where(rng.random(n) < 0.5, F32(1.0), F32(2.0 ** -6))).astype(F32)
        weight = rng.uniform(0.05, 3.0, n).astype(F32)
        pick = rng.random(n)
        for lo, hi, val in ((0.0, 0.05, np.nan), (0.05, 0.1, np.inf), (0.1, 0.35, 2.0 ** 24), (0.35, 0.6, 2.0 ** 30)):
            weight[(pick >= lo) & (pick < hi)] = val
    return kind, dist, weight


@functools.lru_cache(maxsize=None)
def case(seed):
    rng = np.random.default_rng(BASE + seed)
    aimed = AIMED[seed] if seed < len(AIMED) else None
    device = seed % 4 == 3
    if aimed is not None:
        r = dict(aimed)
        dims, phys, offset = GRIDS[r["grid"]]
        image = r["image"]
    else:
        dims, phys, w, h, offset = random_case(rng)
        image = (w, h)
        plain_grid = offset is None
        r = _row(image, None, prior=PRIORS[int(rng.integers(len(PRIORS)))], cap=int(rng.choice((0, 0, 1, 3, 300))), counting=bool(rng.random() < 0.5),
                 frames=int(rng.integers(1, 4)), extra=(None, None, "plain", "remove")[int(rng.integers(4))], colour=bool(rng.random() < 0.25),
                 skew=bool(rng.random() < 0.2))
        r["nodes"] = bool(plain_grid and not r["colour"] and rng.random() < 0.2)
        r["slabs"] = bool(plain_grid and not r["nodes"] and not r["colour"] and r["prior"] in ("cleared", "storage16", "pinned") and dims[2] >= 8 and rng.random() < 0.3)
        if device:
            r["frames"] = max(r["frames"], 2)
        r["claims"] = ("odd_width",) if image[0] % 2 else ("even_width",)
    if r["extra"] == "remove" and r["cap"]:
        r["extra"] = "plain"                      # (a removal is refused under a cap)
    if r["frames"] == 1 and r["extra"]:
        r["frames"] = 2
    grid = (dims, phys, offset)
    n = dims[0] * dims[1] * dims[2]
    repeat = [None]

    def frame(i):
        """Frame i's image size, depth and camera.  Device variant: every image larger than the one before, so the scratch grows."""
        size = (image[0] + 7 * i, image[1] + 5 * i) if device else image
        if aimed is None:
            cam, far = random_camera(rng, dims, phys, offset, *size)
            d, c = random_depth(rng, size[0], size[1], max(far, 50.0)), S.cam4(cam)
        elif r["grid"] == "T":
            d, c = _close_frame(rng, grid, size)
        elif min(size) <= 2:
            d, c = _small_image_frame(rng, grid, size)
        else:
            d, c = S._frame(rng, grid, size)
        return d, (_skewed(c) if r["skew"] else c), size

    def weighted(i):
        if r["flt_max"] and repeat[0] is not None:
            return repeat[0]                      # the same frame again: w + p overflows where both weights are FLT_MAX
        d, c, size = frame(i)
        rgb = rng.integers(0, 256, (size[0] * size[1], 3)).astype(np.uint8) if r["colour"] else None
        repeat[0] = ("weighted", d, pixel_weights(rng, d.size, r["flt_max"]), rgb, c, size[0], size[1])
        return repeat[0]

    ops = []
    first_plain = None
    if r["extra"] == "remove":
        d, c, size = frame(0)
        first_plain = ("plain", d, c, size[0], size[1])
        ops.append(first_plain)
    for i in range(r["frames"]):
        if i == r["frames"] - 1 and i > 0:
            if r["extra"] == "plain":
                d, c, size = frame(i)
                ops.append(("plain", d, c, size[0], size[1]))
            elif r["extra"] == "remove":
                ops += [("remove",) + first_plain[1:]] * 2
        ops.append(weighted(i))
    nodes = None
    if r["nodes"]:
        vs = [phys[a] / dims[a] for a in range(3)]
        zz, yy, xx = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
        nodes = np.stack([(xx + 0.5) * vs[0], (yy + 0.5) * vs[1], (zz + 0.5) * vs[2]], -1).astype(F32).reshape(-1, 3)
        nodes += rng.uniform(-0.3, 0.3, nodes.shape).astype(F32) * np.array(vs, F32)
    slabs = None
    if r["slabs"]:
        cut = int(rng.integers(2, dims[2] - 1))
        slabs = ((0, cut), (cut, dims[2]))
    return {"seed": seed, "dims": dims, "phys": phys, "offset": offset, "prior": _prior(rng, r["prior"], dims, phys, offset), "cap": r["cap"],
            "counting": r["counting"], "colour": r["colour"], "skew": r["skew"], "nodes": nodes, "slabs": slabs, "device": device,
            "claims": r["claims"], "ops": ops, "aimed": aimed is not None}


# ---- the weight models' cases --------------------------------------------------------------------------------------------------------
MODEL_SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (2, 9), (63, 5), (64, 4), (65, 6), (129, 3), (200, 9))
MODEL_Z_REF = 900.0


def model_kinv(general):
    """Column-major inverse intrinsics: the standard shape, or one with a skew term and a third row that is not (0, 0, 1), so that
    ip.z differs from pixel to pixel."""
    k = np.array([1.0 / 591.1, 0.0, 0.0, 0.0, 1.0 / 590.1, 0.0, -331.0 / 591.1, -234.6 / 590.1, 1.0], F32)
    if general:
        k[3], k[2], k[5] = 2.0e-5, 1.0e-4, -2.0e-4
    return k


def model_depth(width, height):
    """A ramp with relief, 65535 and 1 in it; from 4 pixels a side on, a dropout on a border and one beside a corner (at 3 x 3 either
    would be a neighbour of the only pixel that has four), and in images of 40 pixels and more 5 % dropouts."""
    rng = np.random.default_rng(1000 * width + height)
    y, x = np.mgrid[0:height, 0:width]
    d = (800 + 3 * x + 5 * y + 40 * ((7 * x + 3 * y) % 5 == 0)).astype(np.uint16)
    if width * height >= 40:
        d[rng.random(d.shape) < 0.05] = 0
    if width >= 8 and height >= 3:
        d[height // 2 - 1:height // 2 + 2, width // 2 - 1:width // 2 + 4] = d[height // 2, width // 2]     # (neighbours for the two below)
        d[height // 2, width // 2], d[height // 2, width // 2 + 2] = 65535, 1
    if width >= 4:
        d[0, 1] = 0
        d[height // 2, width - 1 if height > 1 else width - 3] = 0          # (the last pixel of a single row holds the 1)
    flat = d.reshape(-1)
    if flat.size >= 2:
        flat[0], flat[-1] = 65535, 1
    return np.ascontiguousarray(flat)


# ---- the CPU side of a case -------------------------------------------------------------------------------------------------------------
class CaseModel:
    """tests/volume_model.VolumeModel in the case's starting state; apply(op) -> (voxels updated, distance stores or None)."""

    def __init__(self, O, c, mutant=None):
        from tests.helpers import Cam
        from tests.volume_model import VolumeModel
        self.Cam, self.c = Cam, c
        self.m = m = VolumeModel(O, c["dims"], c["phys"], c["offset"], mutant)
        if c["offset"] is not None:
            m.ov.clear()                          # (bakes the offset in: offset_at_clear)
        if c["nodes"] is not None:
            m.ov.translation = np.ascontiguousarray(c["nodes"].reshape(-1))
        _, dist, weight = c["prior"]
        if dist is not None:
            m.set_distance_data(dist)
            m.set_weight_data(weight)
        m.set_weight_cap(c["cap"])
        if c["colour"]:
            m.enable_colour(True)

    def apply(self, op):
        m, cam, (w, h) = self.m, self.Cam(*op[-3]), op[-2:]
        if op[0] == "weighted":
            return m.integrate_weighted(op[1], op[2], w, h, cam, op[3]), m.last_stores
        if op[0] == "remove":
            return m.deintegrate(op[1], w, h, cam), None
        if m.cap:
            # the unit property: a plain frame is a weighted one of weight 1 (tests/weight_cap_ref.py's clamp passes over a weight of
            # 2^24 and more, which + 1 leaves as it is; the uploaded fp32 weights of these cases hold such)
            return m.integrate_weighted(op[1], np.ones(w * h, F32), w, h, cam), m.last_stores
        return m.integrate(op[1], w, h, cam), None


def describe(c):
    sw = [k for k in ("counting", "colour", "skew", "device", "aimed") if c[k]] + (["nodes"] if c["nodes"] is not None else []) + (["slabs %s" % (c["slabs"],)] if c["slabs"] else [])
    head = "seed %d: grid %s, physical size %s, offset %s, prior %s, cap %d, %s; claims %s" % (
        c["seed"], c["dims"], c["phys"], c["offset"], c["prior"][0], c["cap"], ", ".join(sw), ", ".join(c["claims"]))
    return head + "\n" + "\n".join("%2d  %s %dx%d" % (i, op[0], op[-2], op[-1]) for i, op in enumerate(c["ops"]))


if __name__ == "__main__":
    for s in [int(a) for a in sys.argv[1:]] or SEEDS:
        print(describe(case(s)))
