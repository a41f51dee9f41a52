"""CPU reference of the rolling volume (include/tsdf_amd.h, "rolling volume"), on the sparse snapshot's reference (tests/snapshot_ref.py):
a snapshot put back at other brick coordinates, into a grid that need not be its own, over a cleared volume or over kept data; the
bricks of a list inside or outside a box; and the shift of a volume's box with the snapshot of what falls out.  Brick coordinates are
Python ints, so no shift wraps.  Words are moved as bits.  The checker, never the thing under test."""
import numpy as np

from tests import snapshot_ref as R

F32, U32 = np.float32, np.uint32
V = R.BRICK ** 3


def coords(ids, nb):
    return [(int(b) % nb[0], (int(b) // nb[0]) % nb[1], int(b) // (nb[0] * nb[1])) for b in ids]


def _as_f32_bits(weights):
    """Brick weights of any storage as the fp32 bits every accessor reports."""
    weights = np.ascontiguousarray(weights).reshape(-1, V)
    return (weights if weights.dtype == np.float32 else weights.astype(F32)).view(U32)


def restore_shifted(ids, d, w, c, src_size, dst_size, shift, fill, keep=None):
    """The dense state (dist float32, weight float32, colour uint32 or None) of a `dst_size` grid after the snapshot (ids, d, w, c) of a
    `src_size` grid went in with `shift`: destination brick bD takes source brick bD - shift.  keep = None: every other voxel is cleared;
    keep = (dist, weight, colour or None), the dense state before: every other voxel keeps its bits (a snapshot without colour writes 0
    on the bricks it writes, one with colour makes the volume have colour)."""
    nbS, nbD = R.bricks_per_axis(src_size), R.bricks_per_axis(dst_size)
    total = nbD[0] * nbD[1] * nbD[2]
    fill_bits = F32(fill).reshape(1).view(U32)[0]
    colour = c is not None or (keep is not None and keep[2] is not None)
    if keep is None:
        D, Wt, Cl = np.full((total, V), fill_bits, U32), np.zeros((total, V), U32), np.zeros((total, V), U32)
    else:
        D = R._bricked(np.ascontiguousarray(keep[0], F32).reshape(-1).view(U32), dst_size, fill_bits)
        Wt = R._bricked(np.ascontiguousarray(keep[1], F32).reshape(-1).view(U32), dst_size, 0)
        Cl = R._bricked(np.ascontiguousarray(keep[2], U32).reshape(-1), dst_size, 0) if keep[2] is not None else np.zeros((total, V), U32)
    d = np.ascontiguousarray(d, F32).reshape(-1, V).view(U32)
    wb = _as_f32_bits(w)
    for n, s in enumerate(coords(ids, nbS)):
        t = [s[a] + int(shift[a]) for a in range(3)]
        if all(0 <= t[a] < nbD[a] for a in range(3)):
            b = t[0] + nbD[0] * (t[1] + nbD[1] * t[2])
            D[b], Wt[b] = d[n], wb[n]
            Cl[b] = np.ascontiguousarray(c, U32).reshape(-1, V)[n] if c is not None else 0
    return R._unbricked(D, dst_size).view(F32), R._unbricked(Wt, dst_size).view(F32), R._unbricked(Cl, dst_size) if colour else None


def select(ids, d, w, c, size, lo, hi, outside=False):
    """The entries of the list whose brick coordinates lie inside [lo, hi) (outside: the others), in order."""
    nb = R.bricks_per_axis(size)
    inside = np.array([all(int(lo[a]) <= b[a] < int(hi[a]) for a in range(3)) for b in coords(ids, nb)], bool).reshape(-1)
    keep = ~inside if outside else inside
    pick = lambda a: None if a is None else np.ascontiguousarray(a).reshape(-1, V)[keep]
    return np.asarray(ids, U32)[keep], pick(d), pick(w), pick(c)


def shift(dist, weight, colour, size, box_shift, fill, weight_bits):
    """The box of a volume moves by `box_shift` bricks: ((dist, weight, colour) after, (ids, d, w, c) of the bricks that fall out, in
    the frame before the move)."""
    snap = R.take(dist, weight, size, fill, weight_bits, colour)
    nb = R.bricks_per_axis(size)
    lo = [int(s) for s in box_shift]
    hi = [int(s) + n for s, n in zip(box_shift, nb)]          # the bricks b that stay: b - box_shift in [0, nb)
    leaving = select(*snap, size, lo, hi, outside=True)
    return restore_shifted(*snap, size, size, [-int(s) for s in box_shift], fill), leaving


def shifted_offset(offset, box_shift, voxel_size):
    """offset + (float)(8 box_shift) voxel_size per axis, every operation in fp32."""
    return np.array([F32(o) + F32(8 * int(s)) * F32(v) for o, s, v in zip(offset, box_shift, voxel_size)], F32)
