"""Weighted frames among the other writers of a volume: twelve sequences in the op-tuple grammar of tests/op_sequences.py, with two new
kinds

    ("depth_weighted", depth, weights, cam)   ("depth_weighted_colour", depth, weights, rgb, cam)

built constructively (PLANS below says what each one is for), on the grids, images, fuse sources and closing frames of the pinned
sequences of the same number: tests/test_weighted_fuzz.py runs them through tests/test_op_sequences.drive(oracle, base, ops=...), so
the twin and the one-more-frame check at the end apply unchanged.  Only the cameras, images, rays, fields and pixel weights inside an op
are random.  Deterministic; no GPU.

    python -m tests.weighted_sequences N...     prints the lists

The pixel weights are log-uniform over [2^-6, 2^4] with the special values of tests/weighted_cases.py on a tenth of the pixels: the
sums stay far below 2^24, where the composed model's capped plain integrate (tests/weight_cap_ref.py) is exact.
"""
import functools
import sys

import numpy as np

from tests import op_sequences as S
from tests.weighted_cases import pixel_weights

F32, U32 = np.float32, np.uint32
W, WC = "depth_weighted", "depth_weighted_colour"

# (kind, option) per op.  Options: upload -- "counts8" | "counts16" | "fractional"; remove -- index of the frame to take out among the
# depth frames integrated so far (plain or weighted: the removal is the plain one either way) or None for a frame never integrated;
# depth_prepared -- the kind of the op in between.
PLANS = (
    # 0: a weighted frame that finds 8-bit counts; the 8-bit snapshot restored behind it, then weighted again, behind itself
    (0, (("depth", None), ("snapshot", None), (W, None), ("raycast", None), ("restore", 0), (W, None), ("raycast", None), (W, None),
         ("depth", None), ("remove", -1), ("flags", True), ("surface", None))),
    # 1: one that finds 16-bit counts; a snapshot of fractional fp32 weights restored after a clear
    (1, (("upload", "counts16"), (W, None), ("raycast", None), ("clear", None), (W, None), ("snapshot", None), ("clear", None), ("restore", 0),
         ("raycast", None), (W, None), ("upload", "counts8"), (W, None), ("flags", False))),
    # 2: rays and a fuse onto fractional weights under a cap; cap on, weighted, cap off, remove
    (2, (("depth", None), ("cap", 3), (W, None), ("rays", None), ("raycast", None), ("fuse", None), (W, None), ("raycast", None), ("cap", 0),
         ("remove", 0), ("surface", None))),
    # 3: fuse and rays between weighted frames; a weighted frame's depth taken out as a plain frame
    (3, ((W, None), ("raycast", None), ("fuse", None), (W, None), ("rays", None), (W, None), ("remove", -1), (W, None), ("flags", True),
         ("surface", None), ("raycast", None))),
    # 4: colour: weighted colour frames round depth_colour and rays_colour, and the refused one once colour is off
    (4, (("colour", True), (WC, None), ("raycast", None), ("depth_colour", None), (WC, None), ("rays_colour", None), (WC, None), ("snapshot", None),
         ("colour", False), ("refused", WC), (W, None), ("flags", False))),
    # 5: a weighted frame between prepare and its integrate, on 8-bit counts: it widens the storage the list was culled for
    (5, (("upload", "counts8"), ("depth_prepared", W), ("raycast", None), (W, None), ("raycast", None), ("clear", None), ("depth", None),
         ("depth_prepared", W), ("flags", True), ("surface", None))),
    # 6: the same on storage widened to 16 bits by hand
    (6, (("storage", 16), ("depth", None), ("depth_prepared", W), ("raycast", None), (W, None), ("snapshot", None), ("clear", None), ("restore", 0),
         (W, None), ("flags", True))),
    # 7: cap 1: every second weighted frame is clamped
    (7, (("cap", 1), (W, None), (W, None), ("raycast", None), ("depth", None), (W, None), ("cap", 0), ("remove", 2), ("fuse", None), (W, None),
         ("surface", None))),
    # 8: colour words uploaded, weighted colour frames round a clear
    (8, (("colour", True), ("upload", "fractional"), (WC, None), ("raycast", None), (WC, None), ("clear", None), (WC, None), ("rays_colour", None),
         ("snapshot", None), ("restore", 0), (W, None))),
    # 9: a cap above 255
    (9, (("cap", 300), ("upload", "counts16"), (W, None), ("rays", None), (W, None), ("fuse", None), ("raycast", None), ("cap", 0), (W, None),
         ("remove", -1), ("flags", False))),
    # 10: colour under a cap
    (10, (("colour", True), ("depth_colour", None), (WC, None), ("cap", 2), (WC, None), ("raycast", None), ("rays_colour", None), (WC, None),
          ("cap", 0), ("remove", 0), ("surface", None))),
    # 11: uploads and restores between weighted frames
    (11, ((W, None), ("snapshot", None), ("upload", "fractional"), (W, None), ("restore", 0), (W, None), ("clear", None), (W, None),
          ("raycast", None), ("fuse", None), (W, None), ("flags", True))),
)
N = len(PLANS)


def _upload_weights(rng, n, how):
    if how == "counts8":
        return np.where(rng.random(n) < 0.8, rng.integers(1, 256, n), 0).astype(F32)
    if how == "counts16":
        return np.where(rng.random(n) < 0.8, rng.integers(256, 65536, n), 0).astype(F32)
    return S._counts(rng, n, "fractional", None)


@functools.lru_cache(maxsize=None)
def sequence(i):
    """-> (base, ops): the pinned sequence whose grid, image, fuse source, cameras and closing frame it runs on, and its own ops."""
    base, plan = PLANS[i]
    info, image, _ = S.sequence(base)
    grid = (info["dims"], info["phys"], info["offset"])
    dims, phys, offset = grid
    n = dims[0] * dims[1] * dims[2]
    trunc = S._truncation(dims, phys)
    rng = np.random.default_rng(0x3E16A + i)
    frames, last_cam, colour = [], [None], False
    pixels = image[0] * image[1]

    def frame():
        d, c = S._frame(rng, grid, image)
        frames.append((d, c))
        last_cam[0] = c
        return d, c

    def make(kind, opt):
        nonlocal colour
        if kind == "depth":
            return ("depth",) + frame()
        if kind == W:
            d, c = frame()
            return (W, d, pixel_weights(rng, pixels, lo=-6.0, hi=4.0), c)
        if kind == WC:
            d, c = frame()
            return (WC, d, pixel_weights(rng, pixels, lo=-6.0, hi=4.0), rng.integers(0, 256, (pixels, 3)).astype(np.uint8), c)
        if kind == "depth_colour":
            d, c = frame()
            return ("depth_colour", d, rng.integers(0, 256, (pixels, 3)).astype(np.uint8), c)
        if kind == "depth_prepared":
            d, c = S._frame(rng, grid, image)
            mid = make(opt, None)
            frames.append((d, c))
            last_cam[0] = c
            return ("depth_prepared", d, c, mid)
        if kind == "remove":
            return ("remove",) + (S._frame(rng, grid, image) if opt is None else frames[opt])
        if kind in ("rays", "rays_colour"):
            o, p, band, lo, hi = S._rays(rng, grid, trunc)
            return ("rays", o, p, band, lo, hi) if kind == "rays" else ("rays_colour", o, p, rng.integers(0, 256, (len(p), 3)).astype(np.uint8), band, lo, hi)
        if kind == "fuse":
            return ("fuse", S._fuse_matrix(rng, grid))
        if kind == "upload":
            words = np.where(rng.random(n) < 0.5, rng.integers(0, 2 ** 32, n, dtype=np.uint64), 0).astype(U32) if colour else None
            return ("upload", S._ball_field(rng, dims, phys, offset, trunc), _upload_weights(rng, n, opt), words)
        if kind == "colour":
            colour = bool(opt)
            return ("colour", colour)
        if kind == "raycast":
            return ("raycast", last_cam[0] if last_cam[0] is not None else S.cam4(S._view(rng, grid, image)[0]))
        if kind == "refused":
            return ("refused", make(opt, None))
        if kind in ("restore", "cap", "storage", "flags"):
            return (kind, opt)
        if kind in ("clear", "snapshot", "surface"):
            return (kind,)
        raise ValueError(kind)

    return base, [make(kind, opt) for kind, opt in plan]


def kind_of(op):
    """The writer kind of an op, weighted frames (with or without colour) as "weighted"; None for observers and switches."""
    return "weighted" if op[0] in (W, WC) else S.writer_kind(op)


if __name__ == "__main__":
    for i in [int(a) for a in sys.argv[1:]] or range(N):
        base, ops = sequence(i)
        info, image, _ = S.sequence(base)
        print("sequence %d on the grid of seed %d: %s, image %dx%d" % (i, base, info["dims"], image[0], image[1]))
        print(S.describe(ops))
