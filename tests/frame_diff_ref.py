"""CPU reference of the frame differences (include/tsdf_amd.h, "frame differences"), rule by rule in numpy: integers in int64 / uint64,
components by an explicit flood fill.  The device result is one unique set of bytes; this gives the same bytes."""
import numpy as np

NO_FRAME, NO_MODEL, SAME, FARTHER, NEARER = 0, 1, 2, 3, 4
NO_BLOB = 0xFFFFFFFF
BLOB_DTYPE = np.dtype([("label", np.uint32), ("size", np.uint32), ("lo", np.uint32, 2), ("hi", np.uint32, 2), ("min_depth", np.uint32),
                       ("max_depth", np.uint32), ("sum_x", np.uint64), ("sum_y", np.uint64), ("sum_depth", np.uint64)])


def tolerance(model, tolerance_mm, quadratic):
    """Rule 1: tolerance + ((quadratic * m * m) >> 32) in 64 bits, saturated to 65535.  (Python integers: nothing overflows.)"""
    m = np.asarray(model).astype(object)
    tol = int(tolerance_mm) + ((int(quadratic) * m * m) >> 32)
    return np.minimum(tol, 65535).astype(np.int64)


def states(frame, model, tolerance_mm, quadratic):
    """(H, W) uint8 states, the first rule that holds."""
    f, m = np.asarray(frame).astype(np.int64), np.asarray(model).astype(np.int64)
    tol = tolerance(model, tolerance_mm, quadratic)
    s = np.full(f.shape, SAME, np.uint8)
    s[f > m + tol] = FARTHER
    s[f + tol < m] = NEARER
    s[(f > 0) & (m == 0)] = NO_MODEL
    s[f == 0] = NO_FRAME
    return s


def counts(state_image):
    return np.bincount(np.asarray(state_image).reshape(-1), minlength=5).astype(np.uint64)


def neighbours(x, y, width, height, connectivity):
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dx or dy) and (connectivity == 8 or abs(dx) + abs(dy) == 1) and 0 <= x + dx < width and 0 <= y + dy < height:
                yield x + dx, y + dy


def cluster(listed, frame, connectivity, depth_step, min_pixels):
    """listed: (H, W) bool; frame: (H, W) depths.  -> (pixels (n,) uint32 ascending ids, labels (n,) uint32 = the smallest list index
    of the pixel's blob, all rows in ascending label, the rows kept: size >= max(min_pixels, 1))."""
    assert connectivity in (4, 8)
    listed = np.asarray(listed, bool)
    h, w = listed.shape
    depth = np.asarray(frame).astype(np.int64)
    pixels = np.flatnonzero(listed.reshape(-1)).astype(np.uint32)
    index = {int(p): i for i, p in enumerate(pixels)}
    labels = np.full(pixels.size, NO_BLOB, np.uint32)
    rows = []
    for i, p in enumerate(pixels):   # ascending: the first unlabelled index of a blob is its smallest
        if labels[i] != NO_BLOB:
            continue
        labels[i] = i
        stack, members = [int(p)], []
        while stack:
            q = stack.pop()
            members.append(q)
            qx, qy = q % w, q // w
            for nx, ny in neighbours(qx, qy, w, h, connectivity):
                j = index.get(ny * w + nx)
                if j is not None and labels[j] == NO_BLOB and abs(int(depth[ny, nx]) - int(depth[qy, qx])) <= depth_step:
                    labels[j] = i
                    stack.append(ny * w + nx)
        mem = np.array(members, np.int64)
        xs, ys, ds = mem % w, mem // w, depth.reshape(-1)[mem]
        row = np.zeros((), BLOB_DTYPE)
        row["label"], row["size"] = i, mem.size
        row["lo"], row["hi"] = (xs.min(), ys.min()), (xs.max(), ys.max())
        row["min_depth"], row["max_depth"] = ds.min(), ds.max()
        row["sum_x"], row["sum_y"], row["sum_depth"] = xs.sum(), ys.sum(), ds.sum()
        rows.append(row)
    rows = np.array(rows, BLOB_DTYPE) if rows else np.zeros(0, BLOB_DTYPE)
    kept = rows[rows["size"] >= max(int(min_pixels), 1)]
    return pixels, labels, rows, kept


def blob_index(shape, pixels, labels, kept):
    """Rule 3: the row of the kept blob of every listed pixel, NO_BLOB elsewhere."""
    row_of = {int(l): r for r, l in enumerate(kept["label"])}
    out = np.full(shape[0] * shape[1], NO_BLOB, np.uint32)
    for p, l in zip(pixels, labels):
        out[int(p)] = row_of.get(int(l), NO_BLOB)
    return out.reshape(shape)


def dilate(kept_pixels, radius):
    """mask[p] = 1 iff a kept pixel lies within Chebyshev distance `radius`, the window clipped at the border: the two separable
    passes, each an OR over shifted copies."""
    k = np.asarray(kept_pixels, bool)
    h, w = k.shape
    rows = np.zeros_like(k)
    for d in range(-radius, radius + 1):
        lo, hi = max(0, d), min(w, w + d)
        if lo < hi:
            rows[:, lo - d:hi - d] |= k[:, lo:hi]
    out = np.zeros_like(k)
    for d in range(-radius, radius + 1):
        lo, hi = max(0, d), min(h, h + d)
        if lo < hi:
            out[lo - d:hi - d, :] |= rows[lo:hi, :]
    return out.astype(np.uint8)


def run(frame, model, tolerance_mm=50, quadratic=0, connectivity=8, depth_step=50, min_pixels=64, dilate_px=4):
    """Everything for one pair of (H, W) images, as a dict of the arrays the device calls give."""
    frame, model = np.asarray(frame, np.uint16), np.asarray(model, np.uint16)
    s = states(frame, model, tolerance_mm, quadratic)
    pixels, labels, rows, kept = cluster(s == NEARER, frame, connectivity, depth_step, min_pixels)
    bi = blob_index(frame.shape, pixels, labels, kept)
    mask = dilate(bi != NO_BLOB, dilate_px)
    return {"states": s, "counts": counts(s), "pixels": pixels, "labels": labels, "rows": rows, "blobs": kept, "blob_index": bi, "mask": mask,
            "frame_out": np.where(mask != 0, 0, frame).astype(np.uint16)}
