"""A volume that follows the camera (include/tsdf_amd.h, "rolling volume"): TSDFVolume.shift moves the box by whole bricks
of 8^3 voxels, BrickStore keeps the bricks that fall out on the host under their world brick coordinates, and RollingVolume pages
them back in when the box covers them again.

World brick coordinates are integer triples: the box's origin in bricks -- a Python int triple that accumulates every shift -- plus the
brick's coordinates in the box.  Nothing here goes through fp32, so keys never drift however far the box travels."""
import math

import numpy as np

BRICK = 8
_WIDTH = {np.dtype(np.uint8): 8, np.dtype(np.uint16): 16, np.dtype(np.float32): 32}
_DTYPE = {8: np.uint8, 16: np.uint16, 32: np.float32}


def world_keys(ids, bricks, origin):
    """Brick ids b = bx + by nb[0] + bz nb[0] nb[1] of a grid of `bricks` bricks whose brick (0, 0, 0) sits at `origin` -> the world
    brick coordinates, a list of int triples."""
    nbx, nby = int(bricks[0]), int(bricks[1])
    ox, oy, oz = (int(o) for o in origin)
    return [(ox + b % nbx, oy + (b // nbx) % nby, oz + b // (nbx * nby)) for b in (int(i) for i in ids)]


def frame_id(key, origin, bricks):
    """The brick id of world brick `key` in a grid of `bricks` bricks at `origin`, or None if the grid does not hold it."""
    c = [int(k) - int(o) for k, o in zip(key, origin)]
    if any(v < 0 or v >= int(n) for v, n in zip(c, bricks)):
        return None
    return c[0] + int(bricks[0]) * (c[1] + int(bricks[1]) * c[2])


def follow_shift(coordinate, bricks, margin):
    """Per axis, the smallest shift s (in bricks) after which `coordinate` - s lies in [margin, bricks - 1 - margin]; 0 where it does."""
    out = []
    for c, n, m in zip(coordinate, bricks, margin):
        c, n, m = int(c), int(n), int(m)
        if m < 0 or 2 * m + 1 > n:
            raise ValueError("follow: a margin of %d bricks does not fit an axis of %d bricks" % (m, n))
        out.append(c - m if c < m else c - (n - 1 - m) if c > n - 1 - m else 0)
    return tuple(out)


class BrickStore:
    """A host dictionary of paged-out bricks: world brick coordinates -> (512 distances, 512 weights in their own element type, 512 colour
    words or None)."""

    def __init__(self):
        self._bricks = {}

    def __len__(self):
        return len(self._bricks)

    def __contains__(self, key):
        return tuple(int(k) for k in key) in self._bricks

    def bytes(self):
        return sum(d.nbytes + w.nbytes + (c.nbytes if c is not None else 0) for d, w, c in self._bricks.values())

    def put_arrays(self, ids, bricks, distances, weights, colours, origin):
        """The host arrays of a snapshot (Snapshot.download()) of a grid of `bricks` bricks whose brick (0, 0, 0) is world brick `origin`."""
        distances = np.asarray(distances, np.float32).reshape(-1, BRICK ** 3)
        weights = np.asarray(weights).reshape(-1, BRICK ** 3)
        if weights.dtype not in _WIDTH:
            raise ValueError("BrickStore: weights must be uint8, uint16 or float32, not %s" % weights.dtype)
        colours = None if colours is None else np.asarray(colours, np.uint32).reshape(-1, BRICK ** 3)
        for n, key in enumerate(world_keys(ids, bricks, origin)):
            self._bricks[key] = (distances[n].copy(), weights[n].copy(), None if colours is None else colours[n].copy())

    def take_arrays(self, lo, hi, origin, bricks):
        """Remove the stored bricks with world coordinates in [lo, hi) that a grid of `bricks` bricks at `origin` holds, and return them
        in that grid's frame: (ids ascending, distances, weights, colours or None).  Weights come in the widest element type among the
        bricks taken (counts widen exactly); bricks without colour get zeros beside bricks with."""
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        found = []
        for key in self._bricks:
            if all(l <= k < h for k, l, h in zip(key, lo, hi)):
                b = frame_id(key, origin, bricks)
                if b is not None:
                    found.append((b, key))
        found.sort()
        rows = [self._bricks.pop(key) for _, key in found]
        ids = np.array([b for b, _ in found], np.uint32)
        bits = max([_WIDTH[w.dtype] for _, w, _ in rows] or [8])
        n = len(rows)
        distances = np.empty((n, BRICK ** 3), np.float32)
        weights = np.empty((n, BRICK ** 3), _DTYPE[bits])
        colours = np.zeros((n, BRICK ** 3), np.uint32) if any(c is not None for _, _, c in rows) else None
        for i, (d, w, c) in enumerate(rows):
            distances[i] = d
            weights[i] = w          # (uint8 -> uint16 -> float32: exact)
            if c is not None:
                colours[i] = c
        return ids, distances, weights, colours

    def put(self, snapshot, origin):
        """The bricks of a Snapshot whose brick (0, 0, 0) is world brick `origin` (one blocking download)."""
        ids, d, w, c = snapshot.download()
        self.put_arrays(ids, tuple(snapshot.info.bricks), d, w, c, origin)

    def take(self, lo, hi, origin, size=None, fill_distance=0.0, voxel_size=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0), into=None):
        """A Snapshot (Snapshot.from_arrays) of the stored bricks in the world box [lo, hi), in the brick frame of a volume of `size`
        voxels whose brick (0, 0, 0) is world brick `origin` (default size: up to hi); what it returns leaves the store."""
        from .api import Snapshot
        if size is None:
            size = tuple(BRICK * (int(h) - int(o)) for h, o in zip(hi, origin))
        bricks = tuple((int(s) + BRICK - 1) // BRICK for s in size)
        ids, d, w, c = self.take_arrays(lo, hi, origin, bricks)
        return Snapshot.from_arrays(size, ids, d, w, c, fill_distance=fill_distance, voxel_size=voxel_size, offset=offset, into=into)


class RollingVolume:
    """A TSDFVolume whose box moves by whole bricks: what falls out goes into `store`, what the box covers again comes back."""

    def __init__(self, volume, store=None):
        self.volume = volume
        self.store = BrickStore() if store is None else store
        self.origin_bricks = (0, 0, 0)
        self._work = self._leaving = self._page = None

    def close(self):
        for s in (self._work, self._leaving, self._page):
            if s is not None:
                s.close()
        self._work = self._leaving = self._page = None

    def shift(self, box_shift):
        """Move the box by `box_shift` bricks: shift the volume, put the leaving bricks into the store, page in the stored bricks that
        the new box covers.  Returns (bricks paged out, bricks paged in)."""
        from .api import Snapshot
        box_shift = tuple(int(s) for s in box_shift)
        if box_shift == (0, 0, 0):
            return 0, 0
        v = self.volume
        if self._work is None:
            self._work, self._leaving, self._page = Snapshot(), Snapshot(), Snapshot()
        leaving = v.shift(box_shift, work=self._work, leaving=self._leaving)
        out = leaving.n_bricks
        if out:
            self.store.put(leaving, self.origin_bricks)
        self.origin_bricks = tuple(o + s for o, s in zip(self.origin_bricks, box_shift))
        size = v.size()
        bricks = tuple(s // BRICK for s in size)
        hi = tuple(o + n for o, n in zip(self.origin_bricks, bricks))
        ids, d, w, c = self.store.take_arrays(self.origin_bricks, hi, self.origin_bricks, bricks) if len(self.store) else ((), 0, 0, 0)
        if len(ids):
            i = v.info()
            page = Snapshot.from_arrays(size, ids, d, w, c, fill_distance=i.truncation_distance, voxel_size=tuple(i.voxel_size),
                                        offset=tuple(i.offset), into=self._page)
            v.restore(page, keep_others=True)
        return out, len(ids)

    def follow(self, point_mm, margin_bricks):
        """The smallest shift that puts the world point at least `margin_bricks` bricks from every face of the box, taken (nothing is
        done if it already is).  Returns the shift."""
        i = self.volume.info()
        margin = (margin_bricks,) * 3 if np.isscalar(margin_bricks) else tuple(margin_bricks)
        c = [math.floor((float(p) - float(o) - float(oc)) / (BRICK * float(vs)))
             for p, o, oc, vs in zip(point_mm, i.offset, i.offset_at_clear, i.voxel_size)]
        s = follow_shift(c, [int(n) // BRICK for n in i.size], margin)
        self.shift(s)
        return s
