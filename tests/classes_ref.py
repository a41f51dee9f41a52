"""CPU reference of class fusion (include/tsdf_amd.h, "class fusion"), pure numpy over the oracle's pinned transforms.

The voxels a class integrate updates are the ones the colour update touches (tests/colour_ref.py: update_sets); the rule is the weighted
Boyer-Moore majority vote on uint32 words {class: bits 0-15, votes: bits 16-31}.  Test infrastructure only (uses oracle/).
"""
import numpy as np

from tests.colour_ref import geometry, update_sets, voxel_centres  # noqa: F401  (geometry is part of this module's surface)

VOID = 0xFFFF


def word(c, n):
    return np.uint32(int(c) | (int(n) << 16))


def vote(words, k, s):
    """The rule on arrays: old words (uint32), the observed class k (uint16) and strength s per word -> new words.  k == VOID or
    s == 0 leaves a word alone."""
    old = np.asarray(words, np.uint32)
    k = np.asarray(k).astype(np.uint32)
    s = np.asarray(s).astype(np.uint32)
    c, n = old & np.uint32(0xFFFF), old >> np.uint32(16)
    pack = lambda cls, votes: (cls.astype(np.uint32) | (votes.astype(np.uint32) << np.uint32(16))).astype(np.uint32)
    n64, s64 = n.astype(np.int64), s.astype(np.int64)
    new = np.where(n == 0, pack(k, s),
          np.where(c == k, pack(k, np.minimum(n64 + s64, 65535)),
          np.where(n64 > s64, pack(c, np.maximum(n64 - s64, 0)),
          np.where(n64 == s64, np.uint32(0), pack(k, np.maximum(s64 - n64, 0))))))
    return np.where((k == VOID) | (s == 0), old, new).astype(np.uint32)


def apply_votes(words, voted, pidx, classes, confidence):
    """The vote at the voxels of the mask `voted`, each with the class and strength of its pixel pidx: a new array."""
    out = np.array(words, np.uint32, copy=True)
    idx = np.nonzero(voted)[0]
    k = np.asarray(classes, np.uint16).reshape(-1)[pidx[idx]]
    s = np.ones(len(idx), np.uint32) if confidence is None else np.asarray(confidence, np.uint8).reshape(-1)[pidx[idx]]
    out[idx] = vote(out[idx], k, s)
    return out


def integrate_classes(O, words, geom, depth, classes, confidence, width, height, camera):
    """One class integrate on the CPU: -> (new class words, updated mask, voted mask)."""
    dims, vs, offset, offset_at_clear, trunc = geom
    centres = voxel_centres(dims, vs, offset, offset_at_clear)
    updated, voted, pidx = update_sets(O, centres, trunc, depth, width, height, camera.inverse_pose(), camera.k(), camera.kinv())
    return apply_votes(words, voted, pidx, classes, confidence), updated, voted


def sample(words, geom, points):
    """sample_classes on the CPU: (n, 3) float32 points -> (classes (n,) uint16, votes (n,) uint16)."""
    dims, vs, offset, offset_at_clear, _ = geom
    p = np.asarray(points, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(((p - offset) - offset_at_clear) / vs).astype(np.float32)
        ok = np.all((f >= 0) & (f < np.array(dims, np.float32)), axis=1)
    fi = np.where(ok[:, None], f, 0).astype(np.int64)
    w = np.asarray(words, np.uint32)[fi[:, 0] + dims[0] * (fi[:, 1] + dims[1] * fi[:, 2])]
    n = np.where(ok, w >> np.uint32(16), 0).astype(np.uint16)
    c = np.where(n != 0, w & np.uint32(0xFFFF), VOID).astype(np.uint16)
    return c, n


def counts(words, n_classes, min_votes=1):
    """class_counts on the CPU: (n_classes,) uint64."""
    w = np.asarray(words, np.uint32)
    c, n = w & np.uint32(0xFFFF), w >> np.uint32(16)
    sel = (n >= max(int(min_votes), 1)) & (c < n_classes)
    return np.bincount(c[sel].astype(np.int64), minlength=n_classes).astype(np.uint64)
