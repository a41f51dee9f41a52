"""The pixel boxes of the cell-parallel ray cast (tsdf_amd/csrc/cell_boxes.hpp), on the CPU: tsdf_selftest_cell_boxes runs the very
expressions a brick's turn of cast_cells_kernel compiles.  A box is a bound -- the pixels whose rays can have a sample in the (grown)
cell -- so it may be too wide, which costs pairs, and never too narrow, which loses a hit:

* it holds every integer pixel of the image inside the hull of the cell's eight corners projected in double precision (of the part
  of the cell at or in front of z_clip, where the view's samples lie; the bounding rectangle of that hull, which asks no less);
* it holds the box the earlier expressions gave (the centre through the world coordinates and three rows of the pose with separately
  rounded products: restated here in numpy's float32), wherever that one passes the same test;
* what it is wider by is the widened margin and nothing else: it lies inside the earlier box grown by that margin's worth.

Six cameras over a grid with partial bricks and anisotropic voxels and over 512^3; 20 000 random cells each."""
import ctypes as C

import numpy as np
import pytest

from tsdf_amd import _capi

F = np.float32
N_CELLS = 20000

GRIDS = {
    "24x20x28": dict(size=(24, 20, 28), phys=(3000.0, 3000.0, 3000.0), offset=(-300.0, 250.0, 100.0)),
    "512^3": dict(size=(512, 512, 512), phys=(3000.0, 3000.0, 3000.0), offset=(0.0, 0.0, 0.0)),
}
# position and target relative to the grid's origin (mm; "near": the z position is set 4.5 voxels in front of the z = 0 face),
# intrinsics (fx, fy, cx, cy, skew), image size, scale of the pose's 3 x 3 block
CAMERAS = {
    "standard": dict(at=(1500, 1300, -600), look=(1500, 1400, 1900), K=(525.0, 525.0, 320.0, 240.0, 0.0), size=(640, 480), block=1.0),
    "skew_anisotropic": dict(at=(-900, 1500, 900), look=(1500, 1400, 1900), K=(300.0, 800.0, 320.0, 100.0, 40.0), size=(640, 480), block=1.0),
    "principal_point_off_image": dict(at=(1500, 1300, -700), look=(900, 1400, 1900), K=(525.0, 525.0, -150.0, 240.0, 0.0), size=(640, 480), block=1.0),
    "tele": dict(at=(1500, 1300, -2500), look=(1500, 1400, 1900), K=(2500.0, 2500.0, 320.0, 240.0, 0.0), size=(640, 480), block=1.0),
    "quarter_scale_pose": dict(at=(1400, 1300, -900), look=(1500, 1400, 1900), K=(525.0, 525.0, 320.0, 240.0, 0.0), size=(640, 480), block=0.25),
    "near": dict(at=(1500, 1400, None), look=(3000, 1400, 600), K=(525.0, 525.0, 320.0, 240.0, 0.0), size=(640, 480), block=1.0),
}


def _view(grid, cam):
    """EntryParams as view_projection / choose_cell_cast form them: world -> camera rows, the intrinsics' rows, z_clip, z_near."""
    size = np.array(grid["size"], np.uint32)
    vs = (np.array(grid["phys"], F) / size.astype(F)).astype(F)
    off = np.array(grid["offset"], F)
    at = np.array(cam["at"], np.float64)
    if cam["at"][2] is None:
        at = np.array([cam["at"][0], cam["at"][1], -4.5 * float(vs.max())])
    at = at + off
    look = np.array(cam["look"], np.float64) + off
    z = look - at
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    block = cam["block"] * np.stack([x, y, z], axis=1)        # camera -> world, columns the camera's axes
    inv = np.linalg.inv(block)
    r = np.concatenate([inv, (-inv @ at)[:, None]], axis=1).astype(F)
    fx, fy, cx, cy, skew = cam["K"]
    k = np.array([[fx, skew, cx], [0.0, fy, cy]], F)
    w, h = cam["size"]
    # z_clip: half the distance to the grid over the longest direction vector of the image (choose_cell_cast)
    lo, hi = off.astype(np.float64), off.astype(np.float64) + np.array(grid["phys"])
    outside = float(np.linalg.norm(np.maximum(0.0, np.maximum(lo - at, at - hi))))
    kinv = np.linalg.inv(np.array([[fx, skew, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]))
    dmax = max(np.linalg.norm(block @ kinv @ np.array([px, py, 1.0])) for px, py in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (0.5 * w, 0.5 * h)))
    z_clip = F(0.5 * outside / dmax) if outside >= 4.0 * float(vs.max()) else F(0.0)
    z_near = max(z_clip, F(0.25) * vs.min())
    return dict(size=size, vs=vs, off=off, r=r, k=k, w=w, h=h, z_clip=F(z_clip), z_near=F(z_near))


def _selftest(v, cells, corners_only):
    n = len(cells)
    boxes, seen = np.zeros((n, 4), np.int32), np.zeros(n, np.uint8)
    r, k, cells = np.ascontiguousarray(v["r"]), np.ascontiguousarray(v["k"]), np.ascontiguousarray(cells, np.uint32)
    rc = _capi.lib.tsdf_selftest_cell_boxes(r.ctypes.data, k.ctypes.data, v["vs"].ctypes.data, v["off"].ctypes.data, v["size"].ctypes.data,
                                            v["w"], v["h"], C.c_float(float(v["z_clip"])), C.c_float(float(v["z_near"])), n, cells.ctypes.data,
                                            int(corners_only), boxes.ctypes.data, seen.ctypes.data)
    assert rc == 0
    return boxes, seen


def _eps(size):
    return max(F(1.0e-3), F(2.0e-6) * F(size.max()))


def _hull(v, cells):
    """Per cell, in double precision: the rectangle of integer pixels of the image that the part of the grown cell at or in front of
    z_clip projects over -- {u0, u1, v0, v1} inclusive, and whether there is one."""
    e = float(_eps(v["size"]))
    r, k, vs, off = (v[n].astype(np.float64) for n in ("r", "k", "vs", "off"))
    zc = float(v["z_clip"])
    assert zc > 0.0
    corner = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)], np.float64)              # (8, 3)
    lo = cells.astype(np.float64)[:, None, :] + 0.5 - e + corner[None] * (1.0 + 2.0 * e)            # voxel units
    cam = (lo * vs + off) @ r[:, :3].T + r[:, 3]                                                     # (n, 8, 3)
    pts, ok = [cam], [cam[..., 2] >= zc]
    for i in range(8):
        for a in range(3):
            j = i | (1 << a)
            if j == i:
                continue
            di, dj = cam[:, i, 2] - zc, cam[:, j, 2] - zc
            cut = di * dj < 0.0
            t = np.where(cut, di / np.where(cut, di - dj, 1.0), 0.0)
            p = cam[:, i] + t[:, None] * (cam[:, j] - cam[:, i])
            p[:, 2] = np.where(cut, zc, 1.0)
            pts.append(p[:, None]); ok.append(cut[:, None])
    pts, ok = np.concatenate(pts, axis=1), np.concatenate(ok, axis=1)
    depth = np.where(ok, pts[..., 2], 1.0)
    u = (pts @ k[0]) / depth
    w_ = (pts @ k[1]) / depth
    umin, umax = np.where(ok, u, np.inf).min(1), np.where(ok, u, -np.inf).max(1)
    vmin, vmax = np.where(ok, w_, np.inf).min(1), np.where(ok, w_, -np.inf).max(1)
    with np.errstate(invalid="ignore"):
        u0, u1 = np.maximum(np.ceil(umin), 0), np.minimum(np.floor(umax), v["w"] - 1)
        v0, v1 = np.maximum(np.ceil(vmin), 0), np.minimum(np.floor(vmax), v["h"] - 1)
    some = ok.any(1) & (u0 <= u1) & (v0 <= v1)
    return np.stack([u0, u1, v0, v1], 1), some


def _earlier_form(v, cells, corner_boxes, corner_seen, extra=None):
    """The box by the expressions this form replaced, every operation rounded to float32 in their order (reciprocals correctly
    rounded, as on the host).  extra: a per-cell (u, v) widening of the margin, in pixels."""
    r, k, vs, off, e = v["r"], v["k"], v["vs"], v["off"], _eps(v["size"])
    lx, ly, lz = (cells[:, a].astype(F) for a in range(3))
    one, half = F(1.0), F(0.5)
    wx, wy, wz = (lx + one) * vs[0] + off[0], (ly + one) * vs[1] + off[1], (lz + one) * vs[2] + off[2]
    row = lambda j: ((r[j, 0] * wx + r[j, 1] * wy) + r[j, 2] * wz) + r[j, 3]
    ccx, ccy, ccz = row(0), row(1), row(2)
    ext = (one + F(2.0) * e) * vs
    nu, nv, nz = [], [], []
    for a in range(3):
        cxa, cya, cza = r[0, a] * ext[a], r[1, a] * ext[a], r[2, a] * ext[a]
        nu.append((k[0, 0] * cxa + k[0, 1] * cya) + k[0, 2] * cza)
        nv.append((k[1, 0] * cxa + k[1, 1] * cya) + k[1, 2] * cza)
        nz.append(cza)
    half_dz = half * ((abs(nz[0]) + abs(nz[1])) + abs(nz[2]))
    zmin = ccz - half_dz
    front = zmin > v["z_near"]
    with np.errstate(all="ignore"):
        rz, rm = one / ccz, one / zmin
        uc = ((k[0, 0] * ccx + k[0, 1] * ccy) + k[0, 2] * ccz) * rz
        vc = ((k[1, 0] * ccx + k[1, 1] * ccy) + k[1, 2] * ccz) * rz
        su = half * ((np.abs(nu[0] - uc * nz[0]) + np.abs(nu[1] - uc * nz[1])) + np.abs(nu[2] - uc * nz[2]))
        sv = half * ((np.abs(nv[0] - vc * nz[0]) + np.abs(nv[1] - vc * nz[1])) + np.abs(nv[2] - vc * nz[2]))
        hu, hv = su * rm * F(1.0001) + F(0.05), sv * rm * F(1.0001) + F(0.05)
        if extra is not None:
            hu, hv = hu + extra[0](uc, rm), hv + extra[1](vc, rm)
        a0, a1 = np.maximum(np.ceil(uc - hu), F(0.0)), np.minimum(np.floor(uc + hu), F(v["w"] - 1))
        b0, b1 = np.maximum(np.ceil(vc - hv), F(0.0)), np.minimum(np.floor(vc + hv), F(v["h"] - 1))
        some = (a0 <= a1) & (b0 <= b1)
    box = np.zeros((len(cells), 4), np.int64)
    box[some] = np.stack([a0, b0, a1 - a0 + 1, b1 - b0 + 1], 1)[some].astype(np.int64)
    # at or behind z_near: the corners' bound, the same expressions then and now
    box[~front] = corner_boxes[~front]
    some = np.where(front, some, corner_seen != 0)
    box[~some] = 0
    return box, some, front


def _holds(box, some, rect, rect_some):
    """box (u0, v0, w, h) holds the rectangle (u0, u1, v0, v1) wherever there is one."""
    inside = some & (box[:, 0] <= rect[:, 0]) & (box[:, 0] + box[:, 2] - 1 >= rect[:, 1]) & (box[:, 1] <= rect[:, 2]) & (box[:, 1] + box[:, 3] - 1 >= rect[:, 3])
    return inside | ~rect_some


def _grow_terms(v):
    """cell_box_consts' grow terms, restated in double: pixels x depth per unit of 1 / D_min (without the factor `scale`)."""
    r, k, vs, off = (v[n].astype(np.float64) for n in ("r", "k", "vs", "off"))
    size = v["size"].astype(np.float64)
    m = r[:, :3] * vs
    t = r[:, :3] @ (off + vs) + r[:, 3]
    a_ = np.abs(r[:, :3]) @ (np.abs(off) + (size + 1.0) * vs) + np.abs(r[:, 3])
    rows = np.concatenate([k, [[0.0, 0.0, 1.0]]])
    b = np.abs(rows @ t) + np.abs(rows @ m) @ size
    old = np.abs(k) @ a_
    u = 2.0 ** -24
    return u * (5.0 * b[0] + 11.0 * old[0]), u * (5.0 * b[1] + 11.0 * old[1]), u * (13.0 * b[2] + 11.0 * a_[2])


@pytest.mark.parametrize("grid_name", list(GRIDS))
@pytest.mark.parametrize("cam_name", list(CAMERAS))
def test_cell_boxes_hold_the_hull_and_the_earlier_box(grid_name, cam_name):
    v = _view(GRIDS[grid_name], CAMERAS[cam_name])
    rng = np.random.default_rng(sum(map(ord, grid_name + cam_name)))
    cells = np.stack([rng.integers(0, int(s) - 1, N_CELLS) for s in v["size"]], 1).astype(np.uint32)
    new, new_seen = _selftest(v, cells, 0)
    new_near, new_seen = (new_seen & 2) != 0, new_seen & 1
    corners, corners_seen = _selftest(v, cells, 1)
    corners_seen = corners_seen & 1
    new, corners = new.astype(np.int64), corners.astype(np.int64)
    rect, rect_some = _hull(v, cells)
    old, old_some, front = _earlier_form(v, cells, corners, corners_seen)

    ok_new = _holds(new, new_seen != 0, rect, rect_some)
    ok_old = _holds(old, old_some, rect, rect_some)
    area_new, area_old = int((new[:, 2] * new[:, 3]).sum()), int((old[:, 2] * old[:, 3]).sum())
    print("%s, %s: z_clip %.3f z_near %.3f; %d cells with pixels in reach, %d by the corners' bound; box area %d (earlier form %d, %+.3f %%); "
          "hull not held: %d now, %d by the earlier form" % (grid_name, cam_name, v["z_clip"], v["z_near"], int(rect_some.sum()), int(new_near.sum()),
                                                             area_new, area_old, 100.0 * (area_new - area_old) / max(area_old, 1), int((~ok_new).sum()), int((~ok_old).sum())))
    assert rect_some.sum() > 100, "the camera sees too little of the sample"
    if cam_name == "near":
        assert new_near.sum() > 0 and (~new_near).sum() > 0, "both bounds are to be taken"
    bad = np.flatnonzero(~ok_new)
    assert bad.size == 0, "cell %s: box %s does not hold the hull's pixels %s" % (cells[bad[0]], new[bad[0]], rect[bad[0]])

    # the earlier form's box, wherever that one held the hull
    old_rect = np.stack([old[:, 0], old[:, 0] + old[:, 2] - 1, old[:, 1], old[:, 1] + old[:, 3] - 1], 1)
    inside = _holds(new, new_seen != 0, old_rect, old_some & ok_old)
    bad = np.flatnonzero(~inside)
    assert bad.size == 0, "cell %s: box %s does not hold the earlier form's %s" % (cells[bad[0]], new[bad[0]], old[bad[0]])

    # ... and wider by the margin alone: inside the earlier form's box with the grow terms (and 2e-3 px for the roundings of either
    # form) added to its margin, for the cells both forms bound in front of z_near
    gu, gv, gz = _grow_terms(v)
    scale = 1.0001 * 1.001
    wider = (lambda c, rm: ((gu + np.abs(c.astype(np.float64)) * gz) * rm * scale + 2.0e-3).astype(F),
             lambda c, rm: ((gv + np.abs(c.astype(np.float64)) * gz) * rm * scale + 2.0e-3).astype(F))
    grown, grown_some, _ = _earlier_form(v, cells, corners, corners_seen, extra=wider)
    both = front & ~new_near & (new_seen != 0)
    new_rect = np.stack([new[:, 0], new[:, 0] + new[:, 2] - 1, new[:, 1], new[:, 1] + new[:, 3] - 1], 1)
    inside = _holds(grown, grown_some, new_rect, both)
    bad = np.flatnonzero(~inside)
    assert bad.size == 0, "cell %s: box %s is wider than the earlier form's with the new margin, %s" % (cells[bad[0]], new[bad[0]], grown[bad[0]])
