"""Seeded sequences of volume operations, as data: what tests/test_op_sequences.py drives through one tsdf_amd.TSDFVolume and the
composed CPU model (tests/volume_model.py) side by side.  sequence(seed) -> (grid, image, ops): `grid` a dict (dims, phys, offset, the
source volume of the sequence's fuses, two cameras and one more frame for the end of the run), `image` = (width, height) of every depth
frame and ray cast, `ops` a list of tuples that carry arrays and parameters and no callables.  Deterministic; no GPU.

    python -m tests.op_sequences SEED...     prints the lists

Built constructively, not drawn: the order of the writer kinds comes from a greedy cover of all 81 ordered pairs of the nine data
writers over skeletons that fix, seed by seed, what the coverage conditions of tests/test_op_sequences_host.py ask for (uploaded
counts just below a storage threshold and the op that crosses it, snapshots on both sides of it, caps switched on and off around a
removal, colour switched off and on, a brick list prepared ahead with another op before its integrate, one refused call); only the
cameras, images, rays and fields inside an op are random.  Op tuples:

    ("depth", depth, cam)   ("depth_prepared", depth, cam, between op or None)   ("depth_colour", depth, rgb, cam)
    ("remove", depth, cam)  ("rays", origins, points, band_only, min_range, max_range)
    ("rays_colour", origins, points, rgb, band_only, min_range, max_range)   ("fuse", m)   ("restore", index of an earlier snapshot)
    ("upload", dist or None, weight or None, colour or None)   ("clear",)   ("cap", c)   ("storage", bits)   ("colour", on)
    ("raycast", cam)   ("surface",)   ("flags", force_rebuild)   ("snapshot",)
    ("refused", op)         op: a "remove" under a cap, a "rays_colour" without colour, or ("restore_other", dims)

cam = (pose, inverse_pose, k, kinv) as float32 arrays (tests.helpers.Cam(*cam)).  "depth_prepared" is integrate_prepare_device, then
the op in between -- only kinds the header's contract for a prepared list allows: they write the volume, not the image, its tile maxima
or the grid's position -- then integrate_device with the same arguments.
"""
import functools
import sys
import zlib
from collections import Counter

import numpy as np

from tests import fuse_ref
from tests.test_fuzz_parity import random_camera, random_depth

F32, U32 = np.float32, np.uint32
N_SEEDS = 32
SEEDS = tuple(range(N_SEEDS))
MIN_OPS, MAX_OPS = 12, 14
WRITERS = ("depth", "depth_colour", "remove", "rays", "rays_colour", "fuse", "restore", "upload", "clear")
OBSERVERS = ("raycast", "surface", "flags", "snapshot")
SWITCHES = ("cap", "storage", "colour")

# Grids against the granularities in play: occupancy brick 4, snapshot brick 8, packed weights 4 or 2 planes a dword, integrate brick
# 64 x 4 x 32, one wave of 64 along x.  (dims, physical size, offset -- set without a clear, so offset_at_clear stays zero.)
GRIDS = (((40, 24, 36), (1000.0, 600.0, 900.0), None),
         ((65, 9, 33), (1300.0, 180.0, 660.0), None),
         ((72, 12, 40), (1440.0, 300.0, 1000.0), (30.0, -20.0, 45.0)),
         ((16, 16, 16), (640.0, 640.0, 640.0), None),
         ((130, 5, 8), (1950.0, 75.0, 120.0), None))
IMAGES = ((80, 56), (64, 48), (40, 30), (33, 21), (72, 40))

# ---- what each seed is for --------------------------------------------------------------------------------------------------------
CROSS_255 = {0: "depth", 1: "depth", 2: "rays", 3: "rays", 24: "rays", 4: "fuse", 5: "fuse", 25: "fuse"}
CROSS_65535 = {6: "depth", 7: "rays"}
CROSS_BETWEEN = (2, 3, 4)            # the crossing op runs between a prepare call and its integrate
CAPS = {8: 1, 9: 2, 10: 300, 11: 3, 12: 1000, 13: 2, 14: 1, 15: 40, 16: 3, 17: 260}
CAP_THEN_REMOVE = (8, 9, 10, 11, 12, 13)
COLOUR_TOGGLE = (18, 19, 20, 21)
BETWEEN = {22: "rays", 23: "fuse", 26: "remove", 27: "restore", 28: "raycast", 29: "rays", 30: "fuse", 31: "restore"}
STORAGE = {13: 32, 19: 16, 21: 32, 28: 16}
FRACTIONAL = (30, 31)                # uploaded weights that are no counts: fp32 storage


def _skeleton(seed, n_free):
    """Items ("W", kind, opts) a writer that is set, ("?",) a writer the cover chooses, ("O", kind, opts) an observer or a switch."""
    free = [("?",)] * n_free
    if seed in CROSS_255 or seed in CROSS_65535:
        by = CROSS_255.get(seed) or CROSS_65535[seed]
        top = 255 if seed in CROSS_255 else 65535
        start = ("W", "upload", {"weights": "below", "top": 150 if by == "fuse" else top})
        cross = ("W", "depth_prepared", {"between": by}) if seed in CROSS_BETWEEN else ("W", by, {})
        return [start, ("O", "snapshot", {}), cross, ("O", "snapshot", {}), ("W", "restore", {"index": 0})] + free[:1] + \
               [("W", "clear", {}), ("W", "restore", {"index": 1})] + free[1:]
    if seed in CAPS:
        cap = CAPS[seed]
        head = [("W", "upload", {"weights": "below", "top": cap}), ("O", "snapshot", {})] if cap >= 40 else [("?",), ("O", "snapshot", {})]
        tail = [("W", "remove", {})] if seed in CAP_THEN_REMOVE else []
        n = max(n_free - (0 if cap >= 40 else 1), 0)
        # (where the cap stays on to the end, nothing behind it wipes the whole state: its trace is still there when the sequence ends)
        rest = free[1:n] if tail else [("?", ("upload", "clear", "restore"))] * max(n - 1, 0)
        return head + free[:1] + [("O", "cap", {"cap": cap}), ("W", "rays", {})] + rest[:1] + tail + rest[1:]
    if seed in COLOUR_TOGGLE:
        return [("O", "colour", {"on": True}), ("W", "depth_colour", {}), ("O", "snapshot", {})] + free[:1] + \
               [("O", "colour", {"on": False})] + free[1:2] + [("W", "rays_colour", {})] + free[2:] + [("W", "restore", {"index": 0})]
    first = [("W", "upload", {"weights": "fractional"})] if seed in FRACTIONAL else free[:1]
    if seed in BETWEEN:
        return first + [("O", "snapshot", {})] + free[1:3] + [("W", "depth_prepared", {"between": BETWEEN[seed]})] + free[3:]
    return first + [("O", "snapshot", {})] + free[1:]


def _flat(item):
    """The data writers an item stands for, in the order they write."""
    if item[0] != "W":
        return []
    if item[1] == "depth_prepared":
        between = item[2].get("between")
        return ([between] if between in WRITERS else []) + ["depth"]
    return [item[1]]


def _fill(seed, items, uncovered):
    """The free writers, left to right: the kind that covers most pairs still open with its neighbours."""
    items = list(items)
    for i, item in enumerate(items):
        if item[0] != "?":
            continue
        before = [k for it in items[:i] for k in _flat(it)]
        after = next((k for it in items[i + 1:] if it[0] == "W" for k in _flat(it)[:1]), None)
        best, best_gain = None, -1
        for r in range(len(WRITERS)):
            kind = WRITERS[(seed * 5 + i * 2 + r) % len(WRITERS)]
            if kind == "restore" and len(before) < 2:
                continue          # (straight after the first snapshot it would restore what is there)
            if len(item) > 1 and kind in item[1]:
                continue
            if kind in ("remove", "clear") and not before:
                continue          # (nothing to take out of a new volume)
            if kind == "clear" and (not before or before[-1] == "clear") and ("clear", "clear") not in uncovered:
                continue
            gain = (2 if before and (before[-1], kind) in uncovered else 0) + (2 if after and (kind, after) in uncovered else 0)
            gain += 1 if any(a == kind for a, _ in uncovered) else 0
            if gain > best_gain:
                best, best_gain = kind, gain
        variant = "depth_prepared" if best == "depth" and (seed + i) % 3 == 0 else best
        items[i] = ("W", variant, {})
        if before:
            uncovered.discard((before[-1], best))
    chain = [k for it in items for k in _flat(it)]
    for a, b in zip(chain, chain[1:]):
        uncovered.discard((a, b))
    return items


def _expand(seed, items, ray_after):
    """Items -> op kinds with their options: the switches a writer needs, the refused call, the ray casts and the other observers."""
    ops, colour, cap, refused, writers, snaps = [], False, 0, False, 0, []
    want = "remove_under_cap" if seed in CAPS else ("rays_without_colour", "restore_other", "restore_other")[seed % 3]
    for kind_of, kind, opts in items:
        opts = dict(opts)
        flat = _flat((kind_of, kind, opts)) if kind_of == "W" else []
        if kind_of == "O":
            if kind == "colour":
                colour = opts["on"]
            if kind == "cap":
                cap = opts["cap"]
            if kind == "snapshot":
                snaps.append(colour)
            ops.append((kind, opts))
            continue
        if not refused and want == "rays_without_colour" and not colour and writers >= 1:
            ops.append(("refused", {"op": "rays_colour"}))
            refused = True
        if not refused and want == "restore_other" and writers >= 2:
            ops.append(("refused", {"op": "restore_other"}))
            refused = True
        if ("depth_colour" in flat or "rays_colour" in flat or kind == "depth_colour") and not colour:
            ops.append(("colour", {"on": True}))
            colour = True
        if "remove" in flat and cap:
            if not refused and want == "remove_under_cap":
                ops.append(("refused", {"op": "remove"}))
                refused = True
            ops.append(("cap", {"cap": 0}))
            cap = 0
        if "restore" in flat:      # which snapshot: settled here, because one taken with colour switches colour on again
            key = "index" if kind == "restore" else "between_index"
            opts.setdefault(key, (seed + writers) % len(snaps))
            colour = colour or snaps[opts[key]]
        ops.append((kind, opts))
        writers += 1
        if seed in STORAGE and writers == 4:
            ops.append(("storage", {"bits": STORAGE[seed]}))
    if not refused:
        ops.append(("refused", {"op": "remove" if cap else ("restore_other" if colour else "rays_colour")}))
    # ray casts: straight behind the writers whose kind has had fewest so far
    # (a cleared volume shows nothing: no more casts behind a clear than the two that are asked for)
    spots = [(min(ray_after[k], 2), k == "clear", ray_after[k], -i, i, k) for i, (k, _) in enumerate(ops) if k in WRITERS or k == "depth_prepared"]
    for spot in sorted(spots)[:2]:
        ray_after[spot[-1]] += 1
    chosen = sorted(spot[-2] for spot in sorted(spots)[:2])
    for i in reversed(chosen):
        ops.insert(i + 1, ("raycast", {}))
    # one of the other observers in every sequence, and more up to the length every sequence has
    extra = (("flags", {"force": False}), ("surface", {}), ("flags", {"force": True}), ("raycast", {}))
    n = 0
    while n < 1 or len(ops) < MIN_OPS + 1:
        at = 2 + (seed * 3 + n * 5) % (len(ops) - 2)
        while at < len(ops) and ops[at][0] == "raycast":
            at += 1           # (not between a writer and the cast behind it)
        ops.insert(at, extra[(seed + n) % len(extra)])
        n += 1
    return ops


@functools.lru_cache(maxsize=None)
def plans():
    """The op kinds of every seed.  The cover is global: a seed's free writers are chosen against what the seeds before it left open."""
    uncovered = {(a, b) for a in WRITERS for b in WRITERS}
    ray_after = Counter()
    out = []
    for seed in SEEDS:
        for n_free in range(8, -1, -1):
            trial, counts = set(uncovered), Counter(ray_after)
            ops = _expand(seed, _fill(seed, _skeleton(seed, n_free), trial), counts)
            if len(ops) <= MAX_OPS:
                break
        assert MIN_OPS <= len(ops) <= MAX_OPS, (seed, len(ops))
        uncovered, ray_after = trial, counts
        out.append(tuple((k, tuple(sorted(o.items()))) for k, o in ops))
    assert not uncovered, "writer pairs no sequence holds: %s" % sorted(uncovered)
    return tuple(out)


# ---- the data inside the ops ------------------------------------------------------------------------------------------------------
def cam4(cam):
    return tuple(np.array(m, F32).reshape(-1).copy() for m in (cam.pose(), cam.inverse_pose(), cam.k(), cam.kinv()))


@functools.lru_cache(maxsize=None)
def _truncation(dims, phys):
    import oracle as O
    O.build()
    return F32(O.Volume(dims, phys).truncation_distance())


def _centres(dims, phys, offset):
    """Voxel centres per axis (float64; inputs only)."""
    off = np.zeros(3) if offset is None else np.asarray(offset, np.float64)
    return [(np.arange(dims[a]) + 0.5) * (phys[a] / dims[a]) + off[a] for a in range(3)]


def _ball_field(rng, dims, phys, offset, trunc):
    """A sphere's clamped distance field about a random centre: flat float32, x fastest."""
    x, y, z = _centres(dims, phys, offset)
    c = [rng.uniform(a[0] + 0.3 * (a[-1] - a[0]), a[0] + 0.7 * (a[-1] - a[0])) for a in (x, y, z)]
    r = rng.uniform(0.25, 0.45) * min(max(phys) * 0.5, 2.0 * min(phys))
    d = np.sqrt((x[None, None, :] - c[0]) ** 2 + (y[None, :, None] - c[1]) ** 2 + (z[:, None, None] - c[2]) ** 2) - r
    return np.clip(d, -trunc, trunc).astype(F32).reshape(-1)


def _counts(rng, n, weights, top):
    if weights == "below":       # most voxels at `top`, the rest anywhere up to it
        return np.where(rng.random(n) < 0.7, top, rng.integers(0, top + 1, n)).astype(F32)
    if weights == "fractional":
        return np.where(rng.random(n) < 0.8, rng.uniform(0.25, 4.0, n), 0.0).astype(F32)
    return np.where(rng.random(n) < 0.8, rng.integers(1, 7, n), 0).astype(F32)


def _view(rng, grid, image):
    """A camera across the grid's longest axis that fills the image with it, and its distance to the centre: what a thin grid needs
    to be seen at all at 80 x 56."""
    import tsdf_amd
    dims, phys, offset = grid
    centre = np.asarray(phys) / 2.0 + (np.zeros(3) if offset is None else np.asarray(offset, np.float64))
    to = rng.normal(size=3)
    to[int(np.argmax(phys))] *= 0.2
    to /= np.linalg.norm(to)
    far = max(phys) * rng.uniform(0.9, 1.3)
    f = 0.85 * image[0] * far / max(phys)
    cam = tsdf_amd.Camera(float(f), float(f * rng.uniform(0.9, 1.1)), image[0] / 2.0 + float(rng.uniform(-2, 2)), image[1] / 2.0 + float(rng.uniform(-2, 2)))
    cam.move_to(*(centre + to * far))
    cam.look_at(*(centre + rng.normal(size=3) * 0.03 * min(phys)))
    return cam, far


def _wall_depth(rng, image, far, thickness):
    """A wavy wall through the grid's centre that stays inside a grid `thickness` deep; a few pixels without a measurement."""
    yy, xx = np.mgrid[0:image[1], 0:image[0]]
    d = far + 0.3 * thickness * np.sin(xx / rng.uniform(4.0, 9.0) + rng.uniform(0, 6.28)) * np.cos(yy / rng.uniform(3.0, 7.0))
    d = np.clip(np.rint(d), 0, 65535).reshape(-1)
    d[rng.random(d.size) < rng.choice([0.0, 0.02, 0.2])] = 0
    return d.astype(np.uint16)


def _frame(rng, grid, image):
    """A depth frame and its camera: the fuzz's random camera and image (tests/test_fuzz_parity.py), or -- more often the thinner the
    grid -- a view across the grid and a wall inside it."""
    dims, phys, offset = grid
    thin = min(phys) < 0.2 * max(phys)
    if rng.random() < (0.8 if thin else 0.4):
        cam, far = _view(rng, grid, image)
        return _wall_depth(rng, image, far, min(phys)), cam4(cam)
    cam, far = random_camera(rng, dims, phys, offset, *image)
    return random_depth(rng, image[0], image[1], max(far, 50.0)), cam4(cam)


def _rays(rng, grid, trunc):
    """A sensor outside the grid and a noisy wall through it: (origins (1, 3) or (n, 3), points (n, 3), band_only, min, max)."""
    dims, phys, offset = grid
    off = np.zeros(3) if offset is None else np.asarray(offset, np.float64)
    centre = np.asarray(phys) / 2.0 + off
    n = int(rng.integers(80, 161))
    to = rng.normal(size=3)
    to /= np.linalg.norm(to)
    origin = centre + to * max(phys) * rng.uniform(0.7, 1.4)
    u = np.cross(to, [0.3, 0.5, 0.81])
    u /= np.linalg.norm(u)
    v = np.cross(to, u)
    reach = 0.5 * float(np.abs(np.asarray(phys)) @ np.abs(u)), 0.5 * float(np.abs(np.asarray(phys)) @ np.abs(v))
    a, b = rng.uniform(-reach[0], reach[0], n), rng.uniform(-reach[1], reach[1], n)
    points = centre + a[:, None] * u + b[:, None] * v + to * rng.normal(scale=0.5 * float(trunc), size=n)[:, None]
    origins = origin[None, :] if rng.random() < 0.6 else origin + rng.normal(scale=5.0, size=(n, 3))
    r = np.linalg.norm(points - origins, axis=1)
    lo = float(np.quantile(r, 0.1)) if rng.random() < 0.3 else 0.0
    hi = float(np.quantile(r, 0.9)) if rng.random() < 0.3 else float("inf")
    return origins.astype(F32), points.astype(F32), bool(rng.random() < 0.3), lo, hi


def _source(rng, grid, top):
    """The volume the sequence's fuses read: a plane through the grid's centre, observed `top` times inside a box that covers it."""
    dims, phys, offset = grid
    off = np.zeros(3) if offset is None else np.asarray(offset, np.float64)
    centre = np.asarray(phys) / 2.0 + off
    sphys = tuple(float(p) for p in (0.5 * phys[0], max(2.0 * phys[1], 0.3 * phys[0]), max(2.0 * phys[2], 0.3 * phys[0])))
    vs = 1.3 * max(phys[a] / dims[a] for a in range(3))
    sdims = tuple(int(max(4, np.ceil(p / vs))) for p in sphys)
    soff = tuple(float(v) for v in centre - np.asarray(sphys) / 2.0)
    trunc = _truncation(sdims, sphys)
    x, y, z = _centres(sdims, sphys, soff)
    nrm = rng.normal(size=3)
    nrm /= np.linalg.norm(nrm)
    d = (x[None, None, :] - centre[0]) * nrm[0] + (y[None, :, None] - centre[1]) * nrm[1] + (z[:, None, None] - centre[2]) * nrm[2]
    dist = np.clip(d, -trunc, trunc).astype(F32).reshape(-1)
    weight = np.full(dist.size, float(top), F32)
    if rng.random() < 0.5:       # unobserved outside a ball: taps without weight skip the voxels around its rim
        r2 = (x[None, None, :] - centre[0]) ** 2 + (y[None, :, None] - centre[1]) ** 2 + (z[:, None, None] - centre[2]) ** 2
        weight[(r2 > (0.45 * max(sphys)) ** 2).reshape(-1)] = 0.0
    return {"dims": sdims, "phys": sphys, "offset": soff, "dist": dist, "weight": weight}


def _fuse_matrix(rng, grid):
    """dst -> src: a small rotation about the grid's centre and a shift, or the identity."""
    if rng.random() < 0.25:
        return np.eye(4, dtype=F32).reshape(-1).copy()
    dims, phys, offset = grid
    off = np.zeros(3) if offset is None else np.asarray(offset, np.float64)
    centre = np.asarray(phys) / 2.0 + off
    axis, degrees = rng.normal(size=3), float(rng.uniform(-20.0, 20.0))
    R = fuse_ref.rotation(axis, degrees).reshape(4, 4).T[:3, :3].astype(np.float64)
    shift = rng.uniform(-0.05, 0.05, 3) * np.asarray(phys)
    return fuse_ref.rotation(axis, degrees, centre - R @ centre + shift)


@functools.lru_cache(maxsize=None)
def sequence(seed, variant=0):
    """variant: the same op kinds on another grid of the list, with other cameras, images, rays and fields -- for sweeps beyond the 32
    sequences the tests pin (variant 0)."""
    plan = plans()[seed]
    rng = np.random.default_rng(0x0B5E9 + seed + 1000 * variant)
    grid = GRIDS[(seed + variant) % len(GRIDS)]
    dims, phys, offset = grid
    thin = min(phys) < 0.2 * max(phys)          # (a thin grid is a few pixels high in the smallest images)
    image = IMAGES[(seed // len(GRIDS) + seed) % len(IMAGES)] if not thin else (IMAGES[0], IMAGES[4], IMAGES[1])[(seed // len(GRIDS)) % 3]
    n = dims[0] * dims[1] * dims[2]
    trunc = _truncation(dims, phys)
    source = _source(rng, grid, 120 if CROSS_255.get(seed) == "fuse" else int(rng.integers(1, 4)))
    colour, live, n_snapshots = False, [], 0
    last_cam = [None]

    def frame():
        d, c = _frame(rng, grid, image)
        last_cam[0] = c
        return d, c

    def rgb_of(count):
        return rng.integers(0, 256, (count, 3)).astype(np.uint8)

    def make(kind, opts):
        nonlocal colour, live, n_snapshots
        if kind == "depth":
            live.append(frame())
            return ("depth",) + live[-1]
        if kind == "depth_prepared":
            d, c = frame()
            between = opts.get("between")
            mid = None if between is None else make(between, {"index": opts["between_index"]} if between == "restore" else {})
            live.append((d, c))
            return ("depth_prepared", d, c, mid)
        if kind == "depth_colour":
            d, c = frame()
            live.append((d, c))
            return ("depth_colour", d, rgb_of(image[0] * image[1]), c)
        if kind == "remove":
            if live and rng.random() < 0.85:
                d, c = live.pop(int(rng.integers(len(live))))
            else:
                d, c = _frame(rng, grid, image)      # a frame that never was integrated
            return ("remove", d, c)
        if kind in ("rays", "rays_colour"):
            o, p, band, lo, hi = _rays(rng, grid, trunc)
            return ("rays", o, p, band, lo, hi) if kind == "rays" else ("rays_colour", o, p, rgb_of(len(p)), band, lo, hi)
        if kind == "fuse":
            return ("fuse", _fuse_matrix(rng, grid))
        if kind == "restore":
            live = []
            assert 0 <= opts["index"] < n_snapshots
            return ("restore", int(opts["index"]))
        if kind == "upload":
            live = []
            words = np.where(rng.random(n) < 0.5, rng.integers(0, 2 ** 32, n, dtype=np.uint64), 0).astype(U32) if colour else None
            return ("upload", _ball_field(rng, dims, phys, offset, trunc), _counts(rng, n, opts.get("weights"), opts.get("top")), words)
        if kind == "clear":
            live = []
            return ("clear",)
        if kind == "colour":
            colour = bool(opts["on"])
            return ("colour", colour)
        if kind == "cap":
            return ("cap", int(opts["cap"]))
        if kind == "storage":
            return ("storage", int(opts["bits"]))
        if kind == "raycast":
            return ("raycast", last_cam[0] if last_cam[0] is not None and rng.random() < 0.6 else cam4(_view(rng, grid, image)[0]))
        if kind == "surface":
            return ("surface",)
        if kind == "flags":
            return ("flags", bool(opts["force"]))
        if kind == "snapshot":
            n_snapshots += 1
            return ("snapshot",)
        if kind == "refused":
            what = opts["op"]
            if what == "remove":
                return ("refused", ("remove",) + _frame(rng, grid, image))
            if what == "rays_colour":
                o, p, band, lo, hi = _rays(rng, grid, trunc)
                return ("refused", ("rays_colour", o, p, rgb_of(len(p)), band, lo, hi))
            return ("refused", ("restore_other", (8, 8, 8)))
        raise ValueError(kind)

    ops = [make(kind, dict(opts)) for kind, opts in plan]
    info = {"dims": dims, "phys": phys, "offset": offset, "source": source,
            "cameras": [_frame(rng, grid, image)[1], last_cam[0] if last_cam[0] is not None else _frame(rng, grid, image)[1]],
            "last_frame": _frame(rng, grid, image)}
    return info, image, ops


# ---- reading a sequence -----------------------------------------------------------------------------------------------------------
def flatten(ops):
    """The ops in the order they act: a "depth_prepared" with an op in between becomes that op and then the "depth_prepared"."""
    out = []
    for op in ops:
        if op[0] == "depth_prepared" and op[3] is not None:
            out.append(op[3])
        out.append(op)
    return out


def writer_kind(op):
    """The data writer kind of an op ("depth_prepared" counts as "depth"), or None."""
    kind = "depth" if op[0] == "depth_prepared" else op[0]
    return kind if kind in WRITERS else None


def _short(v):
    if isinstance(v, np.ndarray):
        return "%s%s#%08x" % (v.dtype, list(v.shape), zlib.crc32(np.ascontiguousarray(v).tobytes()))
    if isinstance(v, tuple):
        return "(" + ", ".join(_short(x) for x in v) + ")"
    return repr(v)


def describe(ops, upto=None):
    """One line per op, arrays as dtype, shape and checksum: what a failure prints, and `python -m tests.op_sequences SEED`."""
    return "\n".join("%2d  %s" % (i, _short(op)) for i, op in enumerate(ops[:upto]))


if __name__ == "__main__":
    for s in [int(a) for a in sys.argv[1:]] or SEEDS:
        info, image, ops = sequence(s)
        print("seed %d: grid %s, physical size %s, offset %s, image %dx%d, source grid %s" %
              (s, info["dims"], info["phys"], info["offset"], image[0], image[1], info["source"]["dims"]))
        print(describe(ops))
