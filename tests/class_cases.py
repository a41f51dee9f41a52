"""Seeded cases of class fusion, as data: what tests/test_class_fuzz.py drives through tsdf_amd.TSDFVolume.integrate_classes* and
tests/test_class_fuzz_host.py surveys on the CPU reference (tests/classes_ref.py).  case(seed) -> dict, deterministic, no GPU.

    python -m tests.class_cases SEED...     prints the cases

The first len(AIMED) seeds are aimed, not drawn: each row of AIMED reaches one path of band_pass_kernel<STD, ClassVote> (tsdf_amd/csrc/band_pass.hpp)
nobody would draw -- a 1 x 1 image, widths round one wave, planes appended to the last brick layer, a camera inside the grid and one
exactly on a voxel centre, voxels with sdf == +-trunc, start votes and strengths over the saturation edge.  The N_DRAWN seeds behind them
draw grid, voxel sizes and image as tests/test_colour_parity.py::random_case does, cameras and depths as tests/test_fuzz_parity.py, and
the rest from small lists: by the seed's number j, every fifth seed has 32 k + 1..4 planes and every fifth fewer than 32; every third
bakes an offset at clear() and then moves it; every second starts from uploaded words (start_words); the camera kind follows
test_random_colour_scene's table; j % 4 == 1 carries rgb, j % 4 == 3 is the device variant (every second of those with rgb), j % 6 == 4
has no confidence image; j % 9 == 4 sets the truncation distance to the sdf one of its own voting voxels has in the first frame, so
that a drawn scene, too, holds a voxel exactly on the band's edge (no draw of float cameras puts one there by chance).  Keys of a case:

    seed, aimed, name, dims, phys, bake (an offset set before a clear(), so baked into offset_at_clear, or None), move (the offset set
    after that, or None), trunc (a truncation distance set through the header before the clear, or None), start (uint32 class words
    uploaded before the first frame, or None), colour (the volume has colour and every frame carries rgb), device (the device variant of
    the GPU test), kind (None, "skew", "projective" or "k33": the camera), cast / surface (the GPU test casts / meshes at the end),
    claims (names of the aimed properties the host test asserts), aim (what those claims need), frames: dicts of

    depth (uint16), classes (uint16), confidence (uint8 or None), rgb ((n, 3) uint8 or None), cam, width, height

cam = (pose, inverse_pose, k, kinv) as float32 arrays (tests.helpers.Cam(*cam)).  Reference is the CPU side of a case: the oracle's volume
and the reference words brought to the case's starting state, one apply() per frame, every vote classified by its outcome.
"""
import functools
import sys
from collections import Counter

import numpy as np

from tests import classes_ref as R
from tests import op_sequences as S
from tests.colour_ref import update_sets, voxel_centres
from tests.test_fuzz_parity import random_camera, random_depth

F32, U16, U32 = np.float32, np.uint16, np.uint32
BASE = 0xC1A55
N_DRAWN = 36
VOID = R.VOID
CLASSES = np.array([0, 1, 2, 7, 300, 65534], U32)
STRENGTHS = np.array([0, 1, 1, 2, 3, 128, 254, 255], np.uint8)
KINDS = (None, "skew", None, None, "skew", "projective", None, "skew", None, "k33", None, None)     # test_random_colour_scene's table
OUTCOMES = ("silent", "first", "same", "saturate", "lead", "tie", "takeover")
SWEEP_VOTES = np.concatenate([np.arange(0, 301), np.arange(65200, 65536)]).astype(U32)
CHUNK_Z = 32                                       # kChunkZ (tsdf_amd/csrc/integrate_grid.hpp)


# ---- the data inside a case ------------------------------------------------------------------------------------------------------------
def pixel_classes(rng, n):
    k = CLASSES[rng.integers(0, CLASSES.size, n)].astype(U16)
    k[rng.random(n) < 0.1] = VOID
    return k


def pixel_strengths(rng, n, i):
    """Frame i's confidence: uniform over 0..255 on even frames, a draw from STRENGTHS on odd ones."""
    return rng.integers(0, 256, n, dtype=np.uint8) if i % 2 == 0 else STRENGTHS[rng.integers(0, STRENGTHS.size, n)]


def start_words(rng, n):
    """Words whose votes come from five kinds with equal chance: 0 (the class bits stay in the upload), 1..255, 65026..65535, 1..3,
    1..65535."""
    kind = rng.integers(0, 5, n)
    votes = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                      [np.zeros(n, np.int64), rng.integers(1, 256, n), rng.integers(65026, 65536, n), rng.integers(1, 4, n)], rng.integers(1, 65536, n))
    return (CLASSES[rng.integers(0, CLASSES.size, n)] | (votes.astype(U32) << U32(16))).astype(U32)


def noise_rgb(rng, n):
    return rng.integers(0, 256, (n, 3)).astype(np.uint8)


def general_camera(rng, cam, kind):
    """tests/test_colour_parity.py::general_camera on a 4-tuple: a skewed, off-centre K, a projective last row of the inverse pose, or
    K(2,2) != 1."""
    import oracle as O
    pose, ip, k, _ = (a.copy() for a in cam)
    if kind == "skew":
        k[3] = float(rng.uniform(-8.0, 8.0))
        k[6] += float(rng.uniform(-20.0, 20.0))
        k[7] += float(rng.uniform(-20.0, 20.0))
    elif kind == "projective":
        ip[3] = float(rng.uniform(-2e-5, 2e-5))
        ip[7] = float(rng.uniform(-2e-5, 2e-5))
        ip[15] = float(rng.uniform(0.97, 1.03))
    else:
        k[8] = float(rng.choice([1.02, 0.97, 1.03]))
    return pose, ip, k, np.asarray(O.mat3_inverse(k), F32).reshape(-1)


def pinhole(image, f, position, ypr=None):
    """A camera of focal length f with the principal point in the image's centre, at `position`; the identity rotation or
    tests.helpers.camera_at's yaw, pitch and roll."""
    import tsdf_amd
    from tests.helpers import camera_at
    cam = tsdf_amd.Camera(float(f), float(f), image[0] / 2.0, image[1] / 2.0)
    cam.set_pose(camera_at(tuple(float(p) for p in position), yaw_pitch_roll=ypr).pose())
    return S.cam4(cam)


def _frame(depth, classes, confidence, rgb, cam, image):
    n = image[0] * image[1]
    assert depth.size == n and classes.size == n and (confidence is None or confidence.size == n)
    return {"depth": np.ascontiguousarray(depth, U16), "classes": np.ascontiguousarray(classes, U16), "confidence": confidence, "rgb": rgb,
            "cam": cam, "width": image[0], "height": image[1]}


def _geometry(dims, phys, bake, move, trunc):
    """(dims, vs, offset, offset_at_clear, trunc) as the volume of a case has them, from the oracle's volume."""
    import oracle as O
    O.build()
    return Reference.volume(O, dims, phys, bake, move, trunc)[1]


def _case(seed, name, dims, phys, frames, **kw):
    c = {"seed": seed, "aimed": True, "name": name, "dims": tuple(dims), "phys": tuple(float(p) for p in phys), "bake": None, "move": None,
         "trunc": None, "start": None, "colour": False, "device": False, "kind": None, "cast": False, "surface": False, "claims": (), "aim": {},
         "frames": frames}
    assert set(kw) <= set(c), kw.keys()
    c.update(kw)
    c["colour"] = any(f["rgb"] is not None for f in frames)
    return c


# ---- aimed rows ------------------------------------------------------------------------------------------------------------------------
def _images(seed, rng, image, grid, start, conf):
    """An image size the class pass never saw, on one of the sequences' grids (its offset set without a clear)."""
    from tests.weighted_cases import _small_image_frame
    dims, phys, offset = grid
    n = image[0] * image[1]
    frames = []
    for i in range(2):
        d, cam = _small_image_frame(rng, grid, image) if min(image) <= 2 else S._frame(rng, grid, image)
        if min(image) <= 2:
            d = np.where(d == 0, d.max() if d.max() else U16(1), d).astype(U16)        # (a dropout on the only row would leave nothing)
        frames.append(_frame(d, pixel_classes(rng, n), pixel_strengths(rng, n, i) if conf else None, None, cam, image))
    return _case(seed, "image %dx%d" % image, dims, phys, frames, move=offset, start=start_words(rng, int(np.prod(dims))) if start else None,
                 claims=("voted", "odd_width" if image[0] % 2 else "even_width"), cast=True)


def _planes(seed, rng, planes):
    """70 x 9 x planes: partial bricks in x (64 + 6) and y (2 x 4 + 1); the second frame puts a sloped wall into the last planes."""
    image, vs = (80, 60), 37.5
    dims, phys = (70, 9, planes), (70 * vs, 9 * vs, planes * vs)
    n = image[0] * image[1]
    d0, cam0 = S._frame(rng, (dims, phys, None), image)
    cam1 = pinhole(image, 74.0, (phys[0] / 2.0, phys[1] / 2.0, -1000.0))
    xx = np.tile(np.arange(image[0]), image[1])
    wall = np.rint(1000.0 + (planes - 5) * vs + xx * (6 * vs / image[0])).astype(U16)
    frames = [_frame(d0, pixel_classes(rng, n), pixel_strengths(rng, n, 0), None, cam0, image),
              _frame(wall, pixel_classes(rng, n), pixel_strengths(rng, n, 1), None, cam1, image)]
    extra = planes % CHUNK_Z
    return _case(seed, "%d planes" % planes, dims, phys, frames, claims=("voted", "last_planes") + (("z_extra",) if 1 <= extra <= 4 else ()),
                 surface=planes == 36)


def _inside(seed, rng, ypr):
    """A camera inside a grid of 3 x 5 x 3 bricks: bricks that straddle the camera plane, voxels behind the camera."""
    image, vs = (160, 120), 25.0
    dims = (130, 18, 70)
    phys = tuple(d * vs for d in dims)
    n = image[0] * image[1]
    cam = pinhole(image, 148.0, (1610.0, 230.0, 880.0), ypr)
    frames = [_frame(random_depth(rng, image[0], image[1], 600.0), pixel_classes(rng, n), pixel_strengths(rng, n, 0), None, cam, image),
              _frame(np.full(n, 300, U16), pixel_classes(rng, n), None, None, cam, image)]
    return _case(seed, "camera inside, ypr %s" % (ypr,), dims, phys, frames, start=start_words(rng, int(np.prod(dims))),
                 claims=("voted", "behind_camera"), cast=True)


def _on_centre(seed, rng, voxel):
    """The voxel under the camera projects to 0 / 0 and takes pixel (0, 0); a depth of 1 there puts it in the band."""
    image, vs = (80, 60), 25.0
    dims = (66, 10, 34)
    phys = tuple(d * vs for d in dims)
    n = image[0] * image[1]
    cam = pinhole(image, 74.0, tuple((v + 0.5) * vs for v in voxel))
    depth = np.full(n, 300, U16)
    depth[0] = 1
    classes, conf = pixel_classes(rng, n), pixel_strengths(rng, n, 0)
    classes[0], conf[0] = 300, 200
    at = voxel[0] + dims[0] * (voxel[1] + dims[1] * voxel[2])
    return _case(seed, "camera on the centre of voxel %s" % (voxel,), dims, phys, [_frame(depth, classes, conf, None, cam, image)],
                 claims=("voted", "centre_word"), aim={"voxel": at, "word": int(R.word(300, 200))})


def _exact_trunc(seed, rng, kind):
    """tests/test_colour_parity.py::test_band_edges_at_an_exact_truncation_distance at 80 x 60 on 24 x 12 x 40: trunc = 60 mm, voxel
    centres 20 i + 10 mm, the camera on the -z side looking along +z, integer depths 20 j + 4 and their neighbours."""
    import oracle as O
    image, dims, phys = (80, 60), (24, 12, 40), (480.0, 240.0, 800.0)
    n = image[0] * image[1]
    cam = pinhole(image, 74.0, (240.0, 120.0, -834.0))          # camera z: voxel z = 20 k + 844
    if kind == "k33":
        pose, ip, k, _ = cam
        k = k.copy()
        k[8] = 1.03
        cam = (pose, ip, k, np.asarray(O.mat3_inverse(k), F32).reshape(-1))
    frames = []
    for i in range(2):
        depth = (20 * rng.integers(50, 80, size=n) + 4 + rng.choice([-1, 0, 0, 0, 1], size=n)).astype(U16)
        frames.append(_frame(depth, pixel_classes(rng, n), pixel_strengths(rng, n, i), None, cam, image))
    return _case(seed, "exact truncation distance, %s camera" % (kind or "standard"), dims, phys, frames, trunc=60.0, kind=kind,
                 claims=("voted", "exact_trunc") + (("surface_ulp",) if kind else ()))


def _sweep(seed, rng):
    """On the voxels a fixed pair of frames votes on, the start votes cover every n of SWEEP_VOTES; the strengths of the first frame
    cover every s in 0..255."""
    dims, phys, offset = grid = S.GRIDS[0]
    image = (80, 56)
    n, pixels = int(np.prod(dims)), image[0] * image[1]
    geom = _geometry(dims, phys, None, offset, None)
    import oracle as O
    centres = voxel_centres(*geom[:4])
    frames, will = [], np.zeros(n, bool)
    for i in range(2):
        cam, far = S._view(rng, grid, image)
        depth = S._wall_depth(rng, image, far, min(phys))
        cam = S.cam4(cam)
        will |= update_sets(O, centres, geom[4], depth, image[0], image[1], cam[1], cam[2], cam[3])[1]
        conf = rng.permutation(np.arange(pixels) % 256).astype(np.uint8) if i == 0 else pixel_strengths(rng, pixels, 1)
        classes = CLASSES[rng.integers(0, 3, pixels)].astype(U16)          # three classes: the same class meets itself often
        classes[rng.random(pixels) < 0.05] = VOID
        frames.append(_frame(depth, classes, conf, None, cam, image))
    idx = rng.permutation(np.flatnonzero(will))
    words = start_words(rng, n)
    words[idx] = CLASSES[rng.integers(0, 3, idx.size)] | (SWEEP_VOTES[np.arange(idx.size) % SWEEP_VOTES.size] << U32(16))
    return _case(seed, "word sweep", dims, phys, frames, move=offset, start=words, claims=("voted", "sweep"))


AIMED = ([(_images, (image, S.GRIDS[g], start, conf)) for image, g, start, conf in
          (((1, 1), 3, False, True), ((1, 37), 2, True, True), ((57, 1), 4, False, False), ((63, 5), 1, True, True), ((64, 48), 0, False, True),
           ((65, 40), 1, True, False))] +
         [(_planes, (p,)) for p in (32, 33, 36, 37, 69)] +
         [(_inside, (ypr,)) for ypr in ((0.0, 0.0, 0.0), (1.2, 0.4, -0.7), (3.0, 0.1, 0.0))] +
         [(_on_centre, (v,)) for v in ((40, 5, 20), (0, 0, 0))] +
         [(_exact_trunc, (k,)) for k in (None, "k33")] +
         [(_sweep, ())])
N_AIMED = len(AIMED)
SEEDS = tuple(range(N_AIMED + N_DRAWN))
DRAWN = SEEDS[N_AIMED:]


# ---- drawn seeds ---------------------------------------------------------------------------------------------------------------------------
def _drawn(seed, j):
    from tests.test_colour_parity import random_case
    rng = np.random.default_rng(BASE + j)
    dims, phys, width, height = random_case(rng, j)
    n = int(np.prod(dims))
    bake = move = shift = None
    if j % 3 == 0:             # an offset baked at clear(), then moved: offset != offset_at_clear
        bake = tuple(float(v) for v in rng.uniform(-500, 500, size=3))
        move = tuple(float(v) for v in rng.uniform(-300, 300, size=3))
        shift = tuple(a + b for a, b in zip(bake, move))
    start = start_words(rng, n) if j % 2 == 1 else None
    kind = KINDS[j % 12]
    device = j % 4 == 3
    colour = j % 4 == 1 or j % 8 == 7          # (every second device seed carries rgb as well)
    no_confidence = j % 6 == 4
    n_frames = int(rng.integers(1, 5))
    if device:
        n_frames = max(n_frames, 2)
    frames = []
    for i in range(n_frames):
        w, h = (width + 7 * i, height + 5 * i) if device else (width, height)       # (device: every image larger than the one before)
        cam, far = random_camera(rng, dims, phys, shift, w, h)
        cam = S.cam4(cam)
        if kind:
            cam = general_camera(rng, cam, kind)
        depth = random_depth(rng, w, h, max(far, 50.0))
        frames.append(_frame(depth, pixel_classes(rng, w * h), None if no_confidence else pixel_strengths(rng, w * h, i),
                             noise_rgb(rng, w * h) if colour else None, cam, (w, h)))
    # every ninth seed: the truncation distance is the sdf one of the first frame's voting voxels has, so that voxel sits on the band's edge
    trunc = _trunc_on_a_voxel(dims, phys, bake, move, frames[0]) if j % 9 == 4 else None
    c = _case(seed, "drawn %d" % j, dims, phys, frames, bake=bake, move=move, trunc=trunc, start=start, device=device, kind=kind, cast=j % 2 == 0,
              surface=j % 4 == 2)
    c["aimed"] = False
    return c


def _trunc_on_a_voxel(dims, phys, bake, move, f):
    """The largest sdf below the grid's own truncation distance among the voxels whose pixel has a class and a strength, or None."""
    import oracle as O
    O.build()
    geom = Reference.volume(O, dims, phys, bake, move, None)[1]
    centres = voxel_centres(*geom[:4])
    sdf, _ = voxel_sdf(O, centres, f)
    _, voted, pidx = update_sets(O, centres, geom[4], f["depth"], f["width"], f["height"], f["cam"][1], f["cam"][2], f["cam"][3])
    speaks = voted & (f["classes"][pidx] != VOID) & (True if f["confidence"] is None else f["confidence"][pidx] > 0)
    speaks &= (sdf > F32(0.5) * geom[4]) & (sdf < geom[4])
    return float(sdf[speaks].max()) if speaks.any() else None


@functools.lru_cache(maxsize=None)
def case(seed):
    if seed < N_AIMED:
        build, args = AIMED[seed]
        return build(seed, np.random.default_rng(BASE + 1000 + seed), *args)
    return _drawn(seed, seed - N_AIMED)


# ---- the CPU side of a case ----------------------------------------------------------------------------------------------------------------
def classify(old, k, s):
    """The outcome of every vote (old word, class k, strength s): an array of indices into OUTCOMES."""
    old, k, s = np.asarray(old, U32), np.asarray(k).astype(np.int64), np.asarray(s).astype(np.int64)
    c, n = (old & U32(0xFFFF)).astype(np.int64), (old >> U32(16)).astype(np.int64)
    return np.select([(k == VOID) | (s == 0), n == 0, (c == k) & (n + s <= 65535), c == k, n > s, n == s], [0, 1, 2, 3, 4, 5], 6)


def sampling_points(rng, geom, n=4000):
    """The points of tests/test_colour_parity.py::Fusion.check_sampling: random ones in and around the grid, the float each cell face's
    index gives back through the rule's own subtraction with its nextafter neighbours both ways, points with one coordinate on a face,
    and the grid's centre with NaN, inf and 1e30 coordinates (the last seven)."""
    dims, vs, off, off0, _ = geom
    lo = (off0 + off).astype(np.float64)
    ext = np.array(dims) * vs.astype(np.float64)
    pts = rng.uniform(lo - 0.2 * ext, lo + 1.2 * ext, size=(n, 3)).astype(F32)
    i = rng.integers(0, np.array(dims) + 1, size=(n // 4, 3)).astype(F32)
    face = ((i * vs) + off0) + off
    face = np.concatenate([face, np.nextafter(face, F32(np.inf)), np.nextafter(face, F32(-np.inf))])
    mixed = pts[:len(face)].copy()
    axis = rng.integers(0, 3, size=len(face))
    mixed[np.arange(len(face)), axis] = face[np.arange(len(face)), axis]
    special = np.tile((lo + 0.5 * ext).astype(F32), (7, 1))
    special[[0, 1, 2], [0, 1, 2]] = np.nan
    special[3] = np.nan
    special[4, 0], special[5, 1], special[6] = np.inf, -np.inf, 1e30
    return np.concatenate([pts, face, mixed, special]).astype(F32)


def voxel_sdf(O, centres, f):
    """Per voxel: the integrate sdf of frame f (NaN where there is none) and the depth of the voxel's pixel (0 where none), from the
    oracle's transforms as tests/colour_ref.py::update_sets forms them."""
    (_, ip, k, kinv), w, h = f["cam"], f["width"], f["height"]
    pix = O.world_to_pixel_n(centres, ip, k)
    inb = (pix[:, 0] >= 0) & (pix[:, 0] < w) & (pix[:, 1] >= 0) & (pix[:, 1] < h)
    pidx = np.where(inb, pix[:, 1].astype(np.int64) * w + pix[:, 0], 0)
    d = np.where(inb, f["depth"][pidx], 0).astype(U16)
    sel = np.flatnonzero(d > 0)
    sdf = np.full(len(centres), np.nan, F32)
    surf = O.pixel_to_camera_n(pix[sel], d[sel].astype(F32), kinv)[:, 2]
    sdf[sel] = surf - O.world_to_camera_n(centres[sel], ip)[:, 2]
    return sdf, d


MUTANTS = ("open_band", "no_z_extra", "wrapping_add")      # the defects tests/test_class_fuzz_host.py shows the cases see


class Reference:
    """The oracle's volume and the reference class words of a case; apply(frame) -> what the frame did.  `mutant=` switches in one
    plausible defect of band_pass_kernel or ClassVote: sdf < trunc in place of <=, the appended planes left out of the z bound, n + s that
    wraps at 16 bits."""

    @staticmethod
    def volume(O, dims, phys, bake, move, trunc):
        ov = O.Volume(dims, phys)
        if bake is not None:
            ov.offset(*bake)
        if trunc is not None:
            ov.g.trunc = float(trunc)
        ov.clear()
        if move is not None:
            ov.offset(*move)
        g = ov.g
        return ov, (tuple(int(s) for s in g.dims), np.array(g.vs, F32), np.array(g.offset, F32), np.array(g.offset_at_clear, F32), F32(g.trunc))

    def __init__(self, O, c, distances=True, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.O, self.c, self.distances, self.mutant = O, c, distances, mutant
        self.ov, self.geom = self.volume(O, c["dims"], c["phys"], c["bake"], c["move"], c["trunc"])
        self.centres = voxel_centres(*self.geom[:4])
        n = len(self.centres)
        self.words = np.zeros(n, U32) if c["start"] is None else c["start"].copy()
        self.voted = np.zeros(n, bool)             # every voxel a frame so far visited in the band
        self.outcomes = Counter()

    def apply(self, f):
        """One frame: the words and (with distances) the oracle's integrate.  -> dict(updated, voted, idx, old, k, s, outcome)."""
        O, (pose, ip, k, kinv), w, h = self.O, f["cam"], f["width"], f["height"]
        updated, voted, pidx = update_sets(O, self.centres, self.geom[4], f["depth"], w, h, ip, k, kinv)
        if self.mutant == "open_band":
            voted = voted & ~(voxel_sdf(O, self.centres, f)[0] == self.geom[4])
        if self.mutant == "no_z_extra":
            planes = self.geom[0][2]
            if planes // CHUNK_Z >= 1 and 1 <= planes % CHUNK_Z <= 4:
                voted = voted.copy()
                voted.reshape(planes, -1)[planes - planes % CHUNK_Z:] = False
        idx = np.flatnonzero(voted)
        kk = f["classes"][pidx[idx]]
        s = np.ones(idx.size, U32) if f["confidence"] is None else f["confidence"][pidx[idx]].astype(U32)
        old = self.words[idx]
        outcome = classify(old, kk, s)
        self.words = R.apply_votes(self.words, voted, pidx, f["classes"], f["confidence"])
        if self.mutant == "wrapping_add":
            wrapped = idx[outcome == 3]
            self.words[wrapped] = (old[outcome == 3] & U32(0xFFFF)) | (((old[outcome == 3] >> U32(16)) + s[outcome == 3]) << U32(16))
        self.voted |= voted
        self.outcomes.update(dict(zip(*np.unique(outcome, return_counts=True))))
        if self.distances:
            self.ov.integrate(f["depth"], w, h, ip, k, kinv, nthreads=O.max_threads())
        return {"updated": updated, "voted": voted, "idx": idx, "pidx": pidx, "old": old, "k": kk, "s": s, "outcome": outcome}

    def reached(self):
        """The names of the outcomes met so far."""
        return {OUTCOMES[int(o)] for o, m in self.outcomes.items() if m}


def describe(c):
    sw = [k for k in ("colour", "device", "cast", "surface") if c[k]] + (["start words"] if c["start"] is not None else [])
    head = "seed %d (%s): grid %s, physical size %s, baked offset %s, then %s, trunc %s, camera %s, %s; claims %s" % (
        c["seed"], c["name"], c["dims"], c["phys"], c["bake"], c["move"], c["trunc"], c["kind"] or "standard", ", ".join(sw) or "-",
        ", ".join(c["claims"]) or "-")
    return head + "\n" + "\n".join("%2d  %dx%d  confidence %s  depth %s" % (i, f["width"], f["height"], "none" if f["confidence"] is None else "yes",
                                                                            S._short(f["depth"])) for i, f in enumerate(c["frames"]))


if __name__ == "__main__":
    for s in [int(a) for a in sys.argv[1:]] or SEEDS:
        print(describe(case(s)))
