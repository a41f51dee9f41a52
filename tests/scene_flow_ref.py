"""CPU reference of the scene-flow step (include/tsdf_amd.h, "scene flow"): numpy, fp32, every operation written out in the order the
header states.  Inputs are an indexed mesh (V, I) with the sorted lattice-edge keys of V (tests/mesh_ref.py: indexed() or
used_edge_keys(), V is in key order) and the grid; an edge's two end voxels are its key.  Two update functions: apply() is the
header's gather, scatter_serial() the reference's update_deformation_field (src/SceneFusion/SceneFusion_krnl.cu:211-232) run by one
thread at a time in soup order.  No expectations live here."""
import numpy as np

F32 = np.float32
NONE = -1


def _m3(a, r, c):
    return F32(np.asarray(a, F32).reshape(-1)[(c - 1) * 3 + (r - 1)])      # column-major, as Eigen's data()


def _m4(a, r, c):
    return F32(np.asarray(a, F32).reshape(-1)[(c - 1) * 4 + (r - 1)])


def correspond(oracle, P, depth, flow, width, height, pose, inv_pose, k, kinv, threshold):
    """Per row of P (n, 3): its pixel index y * width + x, or NONE (find_mesh_vertex_correspondences :74-114, plus the finite-flow
    rule).  Also returns the mask of vertices that pass everything but the finite-flow rule."""
    P = np.ascontiguousarray(P, F32).reshape(-1, 3)
    depth = np.asarray(depth, np.uint16).reshape(-1)
    flow = np.asarray(flow, F32).reshape(-1, 3)
    pix = oracle.world_to_pixel_n(P, inv_pose, k).astype(np.int64)
    inside = (pix[:, 0] >= 0) & (pix[:, 0] < width) & (pix[:, 1] >= 0) & (pix[:, 1] < height)
    at = np.where(inside, pix[:, 1] * width + pix[:, 0], 0)
    d = np.where(inside, depth[at], 0)
    with np.errstate(all="ignore"):
        fx, fy, fd = pix[:, 0].astype(F32), pix[:, 1].astype(F32), d.astype(F32)
        # pixel_to_world (src/Utilities/cuda_coordinate_transforms.cu:40-67): sums left to right, then the division by w
        cx = fd * ((_m3(kinv, 1, 1) * fx + _m3(kinv, 1, 2) * fy) + _m3(kinv, 1, 3))
        cy = fd * ((_m3(kinv, 2, 1) * fx + _m3(kinv, 2, 2) * fy) + _m3(kinv, 2, 3))
        cz = fd * ((_m3(kinv, 3, 1) * fx + _m3(kinv, 3, 2) * fy) + _m3(kinv, 3, 3))
        wz = ((_m4(pose, 3, 1) * cx + _m4(pose, 3, 2) * cy) + _m4(pose, 3, 3) * cz) + _m4(pose, 3, 4)
        w = ((_m4(pose, 4, 1) * cx + _m4(pose, 4, 2) * cy) + _m4(pose, 4, 3) * cz) + _m4(pose, 4, 4)
        near = np.abs(wz / w - P[:, 2]) < F32(threshold)
    seen = inside & (d > 0) & near
    finite = np.isfinite(flow[at]).all(axis=1)
    return np.where(seen & finite, at, NONE), seen


def edge_ends(keys, size):
    """(lower voxel, upper voxel, axis) of every key ((z Y + y) X + x) 3 + axis, as linear voxel indices x + y X + z X Y."""
    X, Y, _ = (int(v) for v in size)
    keys = np.asarray(keys, np.int64)
    lo, axis = keys // 3, keys % 3
    return lo, lo + np.array([1, X, X * Y], np.int64)[axis], axis


def multiplicity(I, n_vertices):
    return np.bincount(np.asarray(I, np.int64), minlength=n_vertices).astype(np.int64)


def counts(keys, I, size):
    """count[v]: the soup vertices on the edges that end in voxel v."""
    lo, hi, _ = edge_ends(keys, size)
    m = multiplicity(I, len(keys))
    c = np.zeros(int(size[0]) * int(size[1]) * int(size[2]), np.int64)
    np.add.at(c, lo, m)
    np.add.at(c, hi, m)
    return c


def apply(nodes, keys, I, pix, flow, size):
    """The header's update on a copy of nodes (voxels, 6): returns (nodes, the number of nodes written)."""
    nodes = np.array(nodes, F32).reshape(-1, 6)
    flow = np.asarray(flow, F32).reshape(-1, 3)
    lo, hi, axis = edge_ends(keys, size)
    m = multiplicity(I, len(keys))
    count = counts(keys, I, size)
    acc = np.zeros((len(nodes), 3), F32)
    moved = np.zeros(len(nodes), bool)
    corr = np.asarray(pix) != NONE
    for slot in range(6):                      # -x, +x, -y, +y, -z, +z: a voxel has at most one edge per slot
        sel = (axis == slot // 2) & corr
        vox = (lo if slot % 2 else hi)[sel]    # the edge towards +a belongs to its lower end, the one towards -a to its upper end
        assert len(np.unique(vox)) == len(vox)
        acc[vox] = acc[vox] + m[sel].astype(F32)[:, None] * flow[np.asarray(pix)[sel]]
        moved[vox] = True
    s = F32(1.0) / count[moved].astype(F32)
    nodes[moved, :3] = nodes[moved, :3] + s[:, None] * acc[moved]
    return nodes, int(moved.sum())


def scatter_serial(nodes, keys, I, pix, flow, size):
    """update_deformation_field with one thread at a time, in soup order: every corresponding soup vertex adds scale * flow to both
    of its voxels, scale = 1.0f / count.  Also returns, per voxel and component, the sum of |terms| (the initial translation and
    every scale * flow added) for the tolerance of a comparison."""
    nodes = np.array(nodes, F32).reshape(-1, 6)
    flow = np.asarray(flow, F32).reshape(-1, 3)
    lo, hi, _ = edge_ends(keys, size)
    count = counts(keys, I, size)
    magnitude = np.abs(nodes[:, :3]).astype(np.float64)
    for e in np.asarray(I, np.int64):
        if pix[e] == NONE:
            continue
        f = flow[pix[e]]
        for v in (lo[e], hi[e]):
            term = (F32(1.0) / F32(count[v])) * f
            nodes[v, :3] = nodes[v, :3] + term
            magnitude[v] += np.abs(term)
    return nodes, magnitude
