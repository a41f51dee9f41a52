"""Class frames among the other writers of a volume: twelve sequences in the op-tuple grammar of tests/op_sequences.py, with the kinds

    ("depth_classes", depth, classes, confidence or None, rgb or None, cam)     a class integrate (with rgb: on a colour volume)
    ("classes_prepared", depth, classes, confidence or None, cam)              integrate_prepare_device for a frame, then
                                                                                integrate_classes_device with its depth pointer and
                                                                                camera, then the integrate_device it was prepared for
    ("classes", on)   ("upload_classes", words)   ("nodes",)   ("pin",)   ("counting", on)   ("image", (width, height))

built constructively (PLANS below says what each one is for), on the grids, images, fuse sources and closing frames of the pinned
sequences of the same number: tests/test_class_fuzz.py runs them through tests/test_op_sequences.drive(oracle, base, ops=...), so the
twin and the one-more-frame check at the end apply unchanged.  "nodes" makes the deformation nodes explicit (the regular grid: every
writer writes the bits it wrote before, a class integrate is refused from then on), "pin" pins the weights to fp32 (weight_data()),
"image" changes the size of every image behind it (a sequence ends at the size it began with).  Only the cameras, images, rays, fields,
classes and strengths inside an op are random.  Deterministic; no GPU.

    python -m tests.class_sequences N...     prints the lists
"""
import functools
import sys

import numpy as np

from tests import op_sequences as S
from tests.class_cases import noise_rgb, pixel_classes, pixel_strengths, start_words

F32, U32 = np.float32, np.uint32
K, KP = "depth_classes", "classes_prepared"

# (kind, option) per op.  Options: depth_classes -- "rgb" for a frame with colours; upload -- ("below", top) | "fractional" | "counts";
# remove -- index of the frame to take out among the depth frames integrated so far; image -- (dw, dh) added to the sequence's size, or
# None for that size itself.
PLANS = (
    # 0: a class frame takes 8-bit counts past 255; the 8-bit snapshot restored behind it leaves the later words in place
    (0, (("classes", True), ("upload", ("below", 255)), ("snapshot", None), (K, None), ("raycast", None), (K, None), ("restore", 0), (K, None),
         ("flags", True), ("surface", None))),
    # 1: ... and 16-bit counts past 65535
    (6, (("classes", True), ("upload", ("below", 65535)), (K, None), ("snapshot", None), (K, None), ("raycast", None), ("clear", None),
         ("restore", 0), (K, None), ("flags", False))),
    # 2: class frames round set_weight_storage
    (1, (("classes", True), (K, None), ("storage", 16), (K, None), ("raycast", None), ("clear", None), ("storage", 32), (K, None), ("depth", None),
         (K, None), ("flags", True))),
    # 3: ... and round a pinned fp32
    (3, (("classes", True), ("upload_classes", None), (K, None), ("pin", None), (K, None), ("raycast", None), ("clear", None), (K, None),
         ("surface", None))),
    # 4: a weight cap switched on and off, counting on: the counters are the model's
    (8, (("counting", True), ("classes", True), (K, None), ("cap", 2), (K, None), (K, None), ("raycast", None), ("cap", 0), (K, None),
         ("remove", -1), (K, None), ("flags", True))),
    # 5: a cap above 255 on uploaded counts, counting on
    (10, (("counting", True), ("classes", True), ("upload", ("below", 300)), ("cap", 300), (K, None), (K, None), ("cap", 0), (K, None),
          ("remove", -1), ("raycast", None))),
    # 6: rays, a fuse and a removal between class frames: none of them reads or writes a word
    (2, (("classes", True), ("upload_classes", None), (K, None), ("rays", None), (K, None), ("fuse", None), ("raycast", None), (K, None),
         ("remove", 0), (K, None), ("depth_weighted", None), (K, None), ("flags", True))),
    # 7: a snapshot taken before classes exist, restored after class frames: the words stay; one taken with words in place, restored
    # behind one more class frame: its votes stay too
    (4, (("depth", None), ("snapshot", None), ("classes", True), (K, None), (K, None), ("restore", 0), (K, None), ("snapshot", None),
         (K, None), ("restore", 1), ("raycast", None), (K, None))),
    # 8: the image size changes between two class frames on packed weights (the padded depth copy is reallocated)
    (5, (("classes", True), (K, None), ("image", (9, 6)), (K, None), ("raycast", None), ("image", (-7, 3)), (K, None), ("image", None),
         (K, None), ("flags", True))),
    # 9: a brick list prepared for a frame whose depth pointer and camera the class call reuses
    (7, (("classes", True), ("depth", None), (KP, None), ("raycast", None), (K, None), ("storage", 16), (KP, None), ("flags", True),
         ("surface", None))),
    # 10: rgb beside classes, and the refusal once colour is off
    (9, (("classes", True), (K, None), ("refused", (K, "rgb")), ("colour", True), (K, "rgb"), ("depth_colour", None), (K, "rgb"), ("raycast", None),
         ("colour", False), ("refused", (K, "rgb")), (K, None), ("classes", False), ("depth", None), ("classes", True), (K, None))),
    # 11: explicit deformation nodes: refused, every array as it was
    (11, (("classes", True), (K, None), ("depth", None), (K, None), ("raycast", None), ("nodes", None), ("refused", (K, None)), ("flags", True))),
)
N = len(PLANS)


@functools.lru_cache(maxsize=None)
def sequence(i):
    """-> (base, ops): the pinned sequence whose grid, image, fuse source, cameras and closing frame it runs on, and its own ops."""
    base, plan = PLANS[i]
    info, base_image, _ = S.sequence(base)
    grid = (info["dims"], info["phys"], info["offset"])
    dims, phys, offset = grid
    n = dims[0] * dims[1] * dims[2]
    trunc = S._truncation(dims, phys)
    rng = np.random.default_rng(0xC1A55E + i)
    frames, last_cam, image, count = [], [None], [base_image], [0]

    def frame():
        d, c = S._frame(rng, grid, image[0])
        frames.append((d, c))
        last_cam[0] = c
        return d, c

    def class_frame(opt):
        d, c = frame()
        pixels = image[0][0] * image[0][1]
        count[0] += 1
        conf = None if count[0] % 3 == 0 else pixel_strengths(rng, pixels, count[0])
        return d, pixel_classes(rng, pixels), conf, noise_rgb(rng, pixels) if opt == "rgb" else None, c

    def make(kind, opt):
        pixels = image[0][0] * image[0][1]
        if kind == "depth":
            return ("depth",) + frame()
        if kind == K:
            d, k, s, rgb, c = class_frame(opt)
            return (K, d, k, s, rgb, c)
        if kind == KP:
            d, k, s, _, c = class_frame(None)
            frames.append((d, c))            # (fused twice)
            return (KP, d, k, s, c)
        if kind == "depth_colour":
            d, c = frame()
            return ("depth_colour", d, noise_rgb(rng, pixels), c)
        if kind == "depth_weighted":
            from tests.weighted_cases import pixel_weights
            d, c = frame()
            return ("depth_weighted", d, pixel_weights(rng, pixels, lo=-6.0, hi=4.0), c)
        if kind == "remove":
            return ("remove",) + frames[opt]
        if kind == "rays":
            return ("rays",) + S._rays(rng, grid, trunc)
        if kind == "fuse":
            return ("fuse", S._fuse_matrix(rng, grid))
        if kind == "upload":
            weights = S._counts(rng, n, *opt) if isinstance(opt, tuple) else S._counts(rng, n, opt if opt == "fractional" else None, None)
            return ("upload", S._ball_field(rng, dims, phys, offset, trunc), weights, None)
        if kind == "upload_classes":
            return ("upload_classes", start_words(rng, n))
        if kind == "raycast":
            return ("raycast", last_cam[0] if last_cam[0] is not None else S.cam4(S._view(rng, grid, image[0])[0]))
        if kind == "refused":
            return ("refused", make(*opt))
        if kind == "image":
            image[0] = base_image if opt is None else (base_image[0] + opt[0], base_image[1] + opt[1])
            return ("image", image[0])
        if kind in ("restore", "cap", "storage", "flags", "classes", "colour", "counting"):
            return (kind, opt)
        if kind in ("clear", "snapshot", "surface", "nodes", "pin"):
            return (kind,)
        raise ValueError(kind)

    ops = [make(kind, opt) for kind, opt in plan]
    assert image[0] == base_image, "sequence %d ends at another image size than it began with" % i
    return base, ops


def kind_of(op):
    """The writer kind of an op, class frames (prepared or not) as "classes"; None for observers and switches."""
    if op[0] in (K, KP):
        return "classes"
    return "weighted" if op[0] == "depth_weighted" else S.writer_kind(op)


if __name__ == "__main__":
    for i in [int(a) for a in sys.argv[1:]] or range(N):
        base, ops = sequence(i)
        info, image, _ = S.sequence(base)
        print("sequence %d on the grid of seed %d: %s, image %dx%d" % (i, base, info["dims"], image[0], image[1]))
        print(S.describe(ops))
