"""CPU reference of the mesh renderer (include/tsdf_amd.h, "mesh rendering"): rules 1 - 8 in numpy, integers in int64 and every fp32
operation as one numpy float32 operation, in the order the header writes them.  The device must match every target byte for byte."""
import numpy as np

F = np.float32
MISS = 0xFFFFFFFF
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
LARGE_BOX = 256
CULL_BACK = 1


def project(V, inv_pose, k, near, far):
    """Rules 1 and 2: (X, Y int64, r float32, usable bool) per vertex."""
    V = np.ascontiguousarray(V, F).reshape(-1, 3)
    m = np.asarray(inv_pose, F).reshape(4, 4).T          # column-major in, m[i, j] = row i, column j
    k = np.asarray(k, F).reshape(-1)
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    with np.errstate(all="ignore"):
        row = lambda i: ((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3]
        w = row(3)
        cx, cy, cz = row(0) / w, row(1) / w, row(2) / w
        r = F(1.0) / cz
        sx = k[0] * (cx / cz) + k[6]
        sy = k[4] * (cy / cz) + k[7]
        usable = (np.isfinite(cx) & np.isfinite(cy) & np.isfinite(cz) & (cz >= F(near)) & (cz <= F(far)) &
                  (np.abs(sx) <= F(1048576.0)) & (np.abs(sy) <= F(1048576.0)))
        X = np.where(usable, np.rint(sx * F(256.0)), 0).astype(np.int64)
        Y = np.where(usable, np.rint(sy * F(256.0)), 0).astype(np.int64)
    return X, Y, r.astype(F), usable


def wired(I):
    """(n, 3) corners per triangle in the order (I[3t], I[3t+2], I[3t+1])."""
    return np.asarray(I, np.int64).reshape(-1, 3)[:, [0, 2, 1]]


def area2(X, Y, c):
    return (X[c[..., 1]] - X[c[..., 0]]) * (Y[c[..., 2]] - Y[c[..., 0]]) - (X[c[..., 2]] - X[c[..., 0]]) * (Y[c[..., 1]] - Y[c[..., 0]])


def edges(X, Y, c, a2):
    """Rule 4: a, b, cc (each [..., 3]) of the sign-normalised edge functions, and top_left [..., 3]."""
    s = np.where(a2 < 0, -1, 1).astype(np.int64)
    frm, to = c[..., [1, 2, 0]], c[..., [2, 0, 1]]
    ax, ay, bx, by = X[frm], Y[frm], X[to], Y[to]
    s3 = s[..., None]
    a = -s3 * (by - ay)
    b = s3 * (bx - ax)
    cc = s3 * ((by - ay) * ax - (bx - ax) * ay)
    return a, b, cc, (a > 0) | ((a == 0) & (b > 0))


def box(X, Y, c, width, height):
    """The clipped pixel box (x0, y0, x1, y1) inclusive of one triangle, or None."""
    xs, ys = X[c], Y[c]
    x0, x1 = max(0, -((-int(xs.min())) // 256)), min(width - 1, int(xs.max()) // 256)
    y0, y1 = max(0, -((-int(ys.min())) // 256)), min(height - 1, int(ys.max()) // 256)
    return None if x0 > x1 or y0 > y1 else (x0, y0, x1, y1)


def depth_of(e1, e2, area, r0, r1, r2):
    """Rule 5: (z, b1, b2) in float32."""
    with np.errstate(all="ignore"):
        b1 = np.asarray(e1, np.int64).astype(F) / np.asarray(area, np.int64).astype(F)
        b2 = np.asarray(e2, np.int64).astype(F) / np.asarray(area, np.int64).astype(F)
        rr = r0 + (b1 * (r1 - r0) + b2 * (r2 - r0))
        return F(1.0) / rr, b1, b2


def covered(e, top_left):
    return np.all((e > 0) | ((e == 0) & top_left), axis=-1)


def unit(n):
    with np.errstate(all="ignore"):
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        good = np.isfinite(n).all(axis=1) & (length != 0)
        out = n / length[:, None]
    out[~good] = np.nan
    return out.astype(F)


def render(V, I, width, height, inv_pose, k, near, far, flags=0, normals=None, colours=None, large_box=LARGE_BOX):
    """All targets and the info of one render: {"triangle", "z", "depth", "vertices", "normals", "rgb" (None without colours), "info",
    "coverage" (how many live triangles cover each pixel, before the depth test)}."""
    V = np.ascontiguousarray(V, F).reshape(-1, 3)
    I = np.ascontiguousarray(np.asarray(I).reshape(-1), np.uint32)
    n_pixels, n_triangles = width * height, I.size // 3
    near, far = F(near), F(far)
    X, Y, r, usable = project(V, inv_pose, k, near, far)
    keys = np.full((height, width), ALL_ONES, np.uint64)
    coverage = np.zeros((height, width), np.int64)
    info = {"n_triangles": n_triangles, "n_live": 0, "n_dropped": 0, "n_large": 0, "n_pixels_hit": 0, "bad_index": False}
    C = wired(I)
    for t in range(n_triangles):
        c = C[t]
        if (c >= len(V)).any():
            info["bad_index"] = True
            continue
        if not usable[c].all():
            info["n_dropped"] += 1
            continue
        a2 = area2(X, Y, c)
        if a2 == 0 or ((flags & CULL_BACK) and a2 > 0):
            continue
        info["n_live"] += 1
        bx = box(X, Y, c, width, height)
        if bx is None:
            continue
        x0, y0, x1, y1 = bx
        if (x1 - x0 + 1) * (y1 - y0 + 1) > large_box:
            info["n_large"] += 1
        a, b, cc, tl = edges(X, Y, c, a2)
        jj, ii = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
        e = a * (ii[..., None] * 256) + b * (jj[..., None] * 256) + cc
        cov = covered(e, tl)
        coverage[y0:y1 + 1, x0:x1 + 1] += cov
        z, _, _ = depth_of(e[..., 1], e[..., 2], abs(int(a2)), r[c[0]], r[c[1]], r[c[2]])
        frag = cov & np.isfinite(z) & (z >= near) & (z <= far)
        key = (z.astype(F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
        part = keys[y0:y1 + 1, x0:x1 + 1]
        np.minimum(part, np.where(frag, key, ALL_ONES), out=part)
    return resolve(keys.reshape(-1), V, C, X, Y, r, width, normals, colours, info, coverage)


def resolve(keys, V, C, X, Y, r, width, normals, colours, info, coverage=None):
    """Rule 7 from the keys."""
    n = keys.size
    hit = keys != ALL_ONES
    tri = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    z = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F), F(np.nan)).astype(F)
    with np.errstate(all="ignore"):
        zr = np.trunc(z)
        rounded = np.where(z - zr >= F(0.5), zr + F(1.0), zr)     # roundf for z > 0: z - trunc(z) is exact
        depth = np.where(hit & (rounded > 0) & (rounded < 65536), rounded, 0).astype(np.uint16)
    vertices = np.full((n, 3), np.nan, F)
    out_normals = np.full((n, 3), np.nan, F)
    rgb = np.zeros((n, 3), np.uint8)
    p = np.nonzero(hit)[0]
    if p.size:
        c = C[tri[p].astype(np.int64)]
        a2 = area2(X, Y, c)
        a, b, cc, _ = edges(X, Y, c, a2)
        i, j = (p % width).astype(np.int64), (p // width).astype(np.int64)
        e = a * (i[:, None] * 256) + b * (j[:, None] * 256) + cc
        area = np.abs(a2)
        with np.errstate(all="ignore"):
            b1, b2 = e[:, 1].astype(F) / area.astype(F), e[:, 2].astype(F) / area.astype(F)
            q1, q2 = (b1 * r[c[:, 1]]) * z[p], (b2 * r[c[:, 2]]) * z[p]
            mix = lambda A: (A[c[:, 0]] + (q1[:, None] * (A[c[:, 1]] - A[c[:, 0]]) + q2[:, None] * (A[c[:, 2]] - A[c[:, 0]]))).astype(F)
            vertices[p] = mix(V)
            if normals is not None:
                out_normals[p] = unit(mix(np.ascontiguousarray(normals, F).reshape(-1, 3)))
            else:
                u, w = V[c[:, 1]] - V[c[:, 0]], V[c[:, 2]] - V[c[:, 0]]
                cross = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
                out_normals[p] = unit(cross.astype(F))
            if colours is not None:
                f = mix(np.ascontiguousarray(colours, np.uint8).reshape(-1, 3).astype(F)) + F(0.5)
                f = np.where(f > 0, np.where(f > 255, F(255.0), f), F(0.0))
                rgb[p] = f.astype(np.uint8)
    info = dict(info)
    info["n_pixels_hit"] = int(hit.sum())
    return {"triangle": tri, "z": z, "depth": depth, "vertices": vertices, "normals": out_normals, "rgb": rgb if colours is not None else None,
            "info": info, "coverage": coverage}


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
