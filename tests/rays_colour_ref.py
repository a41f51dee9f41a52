"""CPU reference of coloured ray integration (include/tsdf_amd.h, "ray integration", rules 9 - 12) and of the colour at ray-query hits
("ray queries", "Colour at the hits"), written from the header alone.  Rules 1 - 6 are tests/rays_integrate_ref.walk, which returns
the unclamped sdf of every observed cell; here: a dict voxel -> [c_v, R_v, G_v, B_v] in Python integers, the rounded mean, the blend.
`mutant=` switches in one deliberately wrong line at a time (tests/test_integrate_rays_colour_host.py shows that the case sets tell
each from the rule).  Test infrastructure only."""
import numpy as np

from tests import rays_integrate_ref as ref

F = np.float32
MUTANTS = ("sdf_lt_trunc", "band_on_clamped_tsdf", "mean_rounded_down", "blend_without_half", "n_not_saturating", "offset_at_clear_subtracted")

_SEEN = {}   # (geometry, ranges, flags) -> {ray bytes -> [(cell, q, sdf, tsdf)]}


def observations(geom, o, p, min_range=0.0, max_range=np.inf, flags=0):
    """Rules 1 - 6 for one ray -> [(cell, q, sdf, tsdf)] of its observed cells.  A ray that repeats an earlier one bit for bit reuses
    that ray's list: the rules are a function of the ray alone."""
    dims, vs, offset, trunc = geom
    call = (tuple(dims), np.asarray(vs, F).tobytes(), np.asarray(offset, F).tobytes(), F(trunc).tobytes(), F(min_range).tobytes(),
            F(max_range).tobytes(), int(flags))
    seen = _SEEN.setdefault(call, {})
    key = np.asarray(o, F).tobytes() + np.asarray(p, F).tobytes()
    obs = seen.get(key)
    if obs is None:
        obs = seen[key] = [(cell, v[2], v[0], v[1]) for cell, v in ref.walk(geom, o, p, min_range, max_range, flags)[1].items()]
    return obs


def _colour_cell(geom, cell, mutant, offset_at_clear):
    """The voxel whose colour word an observation of `cell` goes to: the cell itself (None: nowhere)."""
    if mutant != "offset_at_clear_subtracted":
        return cell
    # the mutant: the cell tsdf_volume_sample_colours_device would read at the voxel's centre
    dims, vs, offset, _ = geom
    out = []
    for k in range(3):
        c = F(F(F(F(cell[k]) + F(0.5)) * F(vs[k])) + F(offset[k]))
        i = int(np.floor(F(F(F(c - F(offset[k])) - F(offset_at_clear[k])) / F(vs[k]))))
        if i < 0 or i >= dims[k]:
            return None
        out.append(i)
    return tuple(out)


def accumulate(geom, origins, points, rgb, min_range=0.0, max_range=np.inf, flags=0, mutant=None, offset_at_clear=(0.0, 0.0, 0.0)):
    """Rules 7, 9 and 10 -> (acc {(x, y, z): [n_v, S_v]}, col {(x, y, z): [c_v, R_v, G_v, B_v]}) over the whole set."""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    Og = np.ascontiguousarray(origins, F).reshape(-1, 3)
    C = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    n = len(P)
    assert len(Og) in (1, n) and len(C) == n and n <= ref.MAX_RAYS
    trunc = F(geom[3])
    acc, col = {}, {}
    for j in range(n):
        r, g, b = int(C[j, 0]), int(C[j, 1]), int(C[j, 2])
        for cell, q, sdf, tsdf in observations(geom, Og[j if len(Og) == n else 0], P[j], min_range, max_range, flags):
            e = acc.get(cell)
            if e is None:
                acc[cell] = [1, q]
            else:
                e[0] += 1
                e[1] += q
            if mutant == "sdf_lt_trunc":
                in_band = sdf < trunc
            elif mutant == "band_on_clamped_tsdf":
                in_band = tsdf <= trunc
            else:
                in_band = sdf <= trunc
            if not in_band:
                continue
            at = _colour_cell(geom, cell, mutant, offset_at_clear)
            if at is None:
                continue
            e = col.get(at)
            if e is None:
                col[at] = [1, r, g, b]
            else:
                e[0] += 1
                e[1] += r
                e[2] += g
                e[3] += b
    return acc, col


def apply_colour(geom, words, col, mutant=None):
    """Rules 11 and 12 -> the colour words as a new flat uint32 array, x fastest."""
    X, Y, _ = geom[0]
    out = np.array(words, np.uint32).reshape(-1)
    for (x, y, z), (c, *sums) in col.items():
        at = (z * Y + y) * X + x
        old = int(out[at])
        n = old >> 24
        n1 = n + 1
        half = 0 if mutant == "blend_without_half" else n1 >> 1
        new = ((n1 & 0xFF) if mutant == "n_not_saturating" else min(n1, 255)) << 24
        for ch in range(3):
            m = sums[ch] // c if mutant == "mean_rounded_down" else (2 * sums[ch] + c) // (2 * c)
            assert 0 <= m <= 255
            new |= ((((old >> (8 * ch)) & 0xFF) * n + m + half) // n1) << (8 * ch)
        out[at] = new
    return out


def integrate(geom, dist, weight, words, origins, points, rgb, min_range=0.0, max_range=np.inf, flags=0, cap=0, mutant=None,
              offset_at_clear=(0.0, 0.0, 0.0)):
    """One call of tsdf_integrate_rays_colour -> (distances, weights, updated mask, colour words, acc, col)."""
    acc, col = accumulate(geom, origins, points, rgb, min_range, max_range, flags, mutant, offset_at_clear)
    d, w, upd = ref.apply(geom, dist, weight, acc, cap)
    return d, w, upd, apply_colour(geom, words, col, mutant), acc, col


def mask(geom, cells):
    """A flat bool array, x fastest, true at `cells`."""
    X, Y, Z = geom[0]
    m = np.zeros(X * Y * Z, bool)
    for x, y, z in cells:
        m[(z * Y + y) * X + x] = True
    return m


def sample_cells(geom, points):
    """"Colour at the hits": per point the voxel (x, y, z) it reads, or None (a miss, an invalid q, an index that reaches the size)."""
    dims, vs, offset, _ = geom
    out = []
    with np.errstate(all="ignore"):
        for p in np.asarray(points, F).reshape(-1, 3):
            q = [F(p[k] - F(offset[k])) for k in range(3)]
            if not all(np.isfinite(q[k]) and q[k] >= F(0) and q[k] < F(F(dims[k]) * F(vs[k])) for k in range(3)):
                out.append(None)
                continue
            i = [int(np.floor(F(q[k] / F(vs[k])))) for k in range(3)]
            out.append(tuple(i) if all(i[k] < dims[k] for k in range(3)) else None)
    return out


def sample(geom, words, points):
    """tsdf_volume_cast_rays_colour's colours of hit points -> (n, 3) uint8."""
    X, Y, _ = geom[0]
    words = np.asarray(words, np.uint32).reshape(-1)
    cells = sample_cells(geom, points)
    out = np.zeros((len(cells), 3), np.uint8)
    for j, cell in enumerate(cells):
        if cell is None:
            continue
        w = int(words[(cell[2] * Y + cell[1]) * X + cell[0]])
        if w >> 24:
            out[j] = (w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF)
    return out
