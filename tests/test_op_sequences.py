"""GPU: the writers of a volume in arbitrary order.  Each of the 32 seeded sequences of tests/op_sequences.py drives one
tsdf_amd.TSDFVolume (and the source volume of its fuses) side by side with the composed CPU model (tests/volume_model.py), and
everything is compared bit for bit, without a tolerance:

  * after every writer and every switch: distances, weights, the colour words when enabled, colour_enabled(), the class words when
    enabled, classes_enabled(), weight_cap(), and the updated-voxel count where the call returns one (the counters, behind a class
    frame);
  * at every observer: ray-cast vertices and normals against the oracle on the model's arrays, extract_surface against the oracle's
    marching cubes, the lazy brick flags at least their definition and the rebuilt ones (reach included) equal to it, a snapshot
    against tests/snapshot_ref.py at the storage the volume has at that moment;
  * a refused call: ValueError (TSDF_ERR_INVALID) with its message, and the whole state as it was;
  * at the end: a twin -- a new volume given the model's final arrays by upload -- casts, meshes and flags like the sequenced volume,
    and one more depth frame into both leaves them equal to the model again: a stale prepared list, bound or flag shows on the next
    write.

What no accessor shows -- the weight bound and storage, the dirty marks of the brick flags, a brick list culled ahead, the ray
caster's scratch -- is what the writers share; a writer that breaks it passes its own tests and fails here, behind another one.
A failure names the seed and the step and prints the ops up to it (python -m tests.op_sequences SEED prints them all).

Cost on an MI355X host, oracle work included: the whole file 14.5 s, of which 12.2 s are the first import of torch and the start of its
context in seed 2, the first to prepare a brick list (a suite that has used torch before does not pay it); every other seed 0.02 -
0.15 s, the slowest seeds 7 and 0 at 0.15 s.
"""
import numpy as np
import pytest

import tsdf_amd
from tests import op_sequences as S
from tests import snapshot_ref
from tests.helpers import Cam, assert_same_floats
from tests.volume_model import ModelRun
from tsdf_amd import _capi

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
DEPTH_TILE = 16          # TSDF_DEPTH_TILE (include/tsdf_amd.h)
REFUSALS = {"remove": "tsdf_deintegrate: the volume has a weight cap", "rays_colour": "tsdf_integrate_rays_colour: colour is not enabled",
            "restore_other": "tsdf_volume_restore: the snapshot is of a 8 x 8 x 8 grid",
            "depth_weighted_colour": "tsdf_integrate_weighted: colour is not enabled",
            "depth_classes_rgb": "tsdf_integrate_classes: rgb given but colour is not enabled",
            "depth_classes_nodes": "tsdf_integrate_classes: not supported once the deformation nodes are explicit"}
_SEEN = {"seeds": set(), "modes": {}, "casts": {True: 0, False: 0}}


def tile_maxima(depth, width, height):
    """The largest value of every 16 x 16 pixel tile, tile (tx, ty) at ty * ceil(width / 16) + tx."""
    tx, ty = (width + DEPTH_TILE - 1) // DEPTH_TILE, (height + DEPTH_TILE - 1) // DEPTH_TILE
    padded = np.zeros((ty * DEPTH_TILE, tx * DEPTH_TILE), np.uint16)
    padded[:height, :width] = np.asarray(depth, np.uint16).reshape(height, width)
    return np.ascontiguousarray(padded.reshape(ty, DEPTH_TILE, tx, DEPTH_TILE).max(axis=(1, 3))).reshape(-1)


def make_volume(spec):
    v = tsdf_amd.TSDFVolume(spec["dims"], spec["phys"])
    if spec["offset"] is not None:
        v.offset(*spec["offset"])          # (without a clear: offset_at_clear stays zero, as in the model)
    return v


class Sequenced:
    """One sequence on the library and on the model."""

    def __init__(self, oracle, seed, variant=0):
        self.seed = seed
        self.info, (self.width, self.height), self.ops = S.sequence(seed, variant)
        self.run = ModelRun(oracle, self.info, (self.width, self.height))
        self.model = self.run.model
        self.gv = make_volume(self.info)
        self.src = make_volume(self.info["source"])
        self.src.set_distance_data(self.info["source"]["dist"])
        self.src.set_weight_data(self.info["source"]["weight"])
        self.snaps = []
        self.counting = False
        self.dims = tuple(self.info["dims"])
        assert F32(self.gv.truncation_distance()) == self.model.trunc() and np.array_equal(self.gv.voxel_size(), self.model.ov.voxel_size())

    def close(self):
        for o in self.snaps + [self.gv, self.src]:
            o.close()

    # ---- comparisons
    def library_state(self, v=None):
        v = self.gv if v is None else v
        return (v.get_distance_data(), v.get_weight_data(), v.get_colour_data() if v.colour_enabled() else None, v.weight_cap(), v.weight_storage(),
                v.get_class_data() if v.classes_enabled() else None)

    def same_as_model(self, what, v=None):
        v = self.gv if v is None else v
        m = self.model
        assert_same_floats(v.get_weight_data(), m.weight, what + ": weights")
        assert_same_floats(v.get_distance_data(), m.dist, what + ": distances")
        assert v.colour_enabled() == (m.colour is not None), what + ": colour enabled"
        if m.colour is not None:
            got = v.get_colour_data()
            bad = np.flatnonzero(got != m.colour)
            assert not bad.size, "%s: %d colour words differ, first at %d: %#x vs %#x" % (what, bad.size, bad[0], got[bad[0]], m.colour[bad[0]])
        assert v.classes_enabled() == (m.classes is not None), what + ": classes enabled"
        if m.classes is not None:
            got = v.get_class_data()
            bad = np.flatnonzero(got != m.classes)
            assert not bad.size, "%s: %d class words differ, first at %d: %#x vs %#x" % (what, bad.size, bad[0], got[bad[0]], m.classes[bad[0]])
        assert v.weight_cap() == m.cap, what + ": weight cap"
        bits = v.weight_storage()[0]
        _SEEN["modes"][bits] = _SEEN["modes"].get(bits, 0) + 1

    # ---- one op on both sides
    def step(self, op, what):
        kind, gv, w, h = op[0], self.gv, self.width, self.height
        if kind == "depth_prepared":
            return self.prepared(op, what)
        if kind == "classes_prepared":
            return self.classes_prepared(op, what)
        if kind == "refused":
            return self.refused(op[1], what)
        want = self.run.apply(op)
        if kind == "depth":
            gv.integrate(op[1], w, h, Cam(*op[2]))
        elif kind == "depth_colour":
            gv.integrate_colour(op[1], op[2], w, h, Cam(*op[3]))
        elif kind == "depth_classes":
            gv.integrate_classes(op[1], op[2], w, h, Cam(*op[5]), confidence=op[3], rgb=op[4])
            if self.counting:
                assert gv.last_updated_voxels() == want, what + ": updated voxels"
        elif kind == "classes":
            gv.enable_classes(op[1])
        elif kind == "upload_classes":
            gv.set_class_data(op[1])
        elif kind == "nodes":
            assert gv.deformation()
        elif kind == "pin":
            assert gv.weight_data() and gv.weight_storage() == (32, True), what
        elif kind == "counting":
            gv.set_counting(op[1])
            self.counting = bool(op[1])
        elif kind == "image":
            self.width, self.height = op[1]
        elif kind == "depth_weighted":
            gv.integrate_weighted(op[1], op[2], w, h, Cam(*op[3]))
        elif kind == "depth_weighted_colour":
            gv.integrate_weighted(op[1], op[2], w, h, Cam(*op[4]), rgb=op[3])
        elif kind == "remove":
            gv.deintegrate(op[1], w, h, Cam(*op[2]))
        elif kind == "rays":
            assert gv.integrate_rays(op[1], op[2], band_only=op[3], min_range=op[4], max_range=op[5]) == want, what + ": updated voxels"
        elif kind == "rays_colour":
            assert gv.integrate_rays(op[1], op[2], band_only=op[4], min_range=op[5], max_range=op[6], rgb=op[3]) == want, what + ": updated voxels"
        elif kind == "fuse":
            assert gv.fuse(self.src, op[1]) == want, what + ": fused voxels"
        elif kind == "restore":
            gv.restore(self.snaps[op[1]])
        elif kind == "upload":
            if op[1] is not None:
                gv.set_distance_data(op[1])
            if op[2] is not None:
                gv.set_weight_data(op[2])
            if op[3] is not None:
                gv.set_colour_data(op[3])
        elif kind == "clear":
            gv.clear()
        elif kind == "cap":
            gv.set_weight_cap(op[1])
        elif kind == "colour":
            gv.enable_colour(op[1])
        elif kind == "storage":
            # widening is allowed at any time and narrowing never: which of the two this is depends on what the writers before it did
            if op[1] >= gv.weight_storage()[0]:
                gv.set_weight_storage(op[1])
                assert gv.weight_storage()[0] == op[1], what
            else:
                with pytest.raises(ValueError, match="the storage can only be widened"):
                    gv.set_weight_storage(op[1])
        elif kind == "raycast":
            V, N = gv.raycast(w, h, Cam(*op[1]))
            _SEEN["casts"][gv.last_raycast_cell_parallel()] += 1
            assert_same_floats(V, want[0], what + ": vertices")
            assert_same_floats(N, want[1], what + ": normals")
            return
        elif kind == "surface":
            assert_same_floats(gv.extract_surface(), want, what + ": surface")
            return
        elif kind == "flags":
            fine, cell, reach = gv.occupancy_data(force_rebuild=op[1])
            if op[1]:
                assert np.array_equal(fine, want[0]) and np.array_equal(cell, want[1]), what + ": rebuilt flags"
                assert np.array_equal(reach, want[2]), what + ": reach"
            else:
                assert np.all(fine >= want[0]) and np.all(cell >= want[1]), what + ": lazy flags below their definition"
            return
        elif kind == "snapshot":
            snap = gv.snapshot()
            self.snaps.append(snap)
            bits = gv.weight_storage()[0]
            ids, d, wt, c = snapshot_ref.take(self.model.dist, self.model.weight, self.dims, self.model.trunc(), bits, self.model.colour)
            gi, gd, gw, gc = snap.download()
            assert np.array_equal(gi, ids), what + ": brick ids"
            assert_same_floats(gd, d, what + ": brick distances")
            assert gw.dtype == wt.dtype and gw.tobytes() == wt.tobytes(), what + ": brick weights"
            assert (gc is None) == (c is None) and (c is None or np.array_equal(gc, c)), what + ": brick colours"
            # (the model's own snapshot holds the same bricks, its weights as fp32)
            assert np.array_equal(want["ids"], ids) and np.array_equal(want["weight"], wt.astype(F32))
            return
        else:
            raise ValueError(kind)
        self.same_as_model(what)

    def prepared(self, op, what):
        """integrate_prepare_device on a side stream, the op in between, then integrate_device with the same arguments."""
        import torch
        gv, w, h = self.gv, self.width, self.height
        cam = Cam(*op[2])
        depth = torch.from_numpy(np.ascontiguousarray(op[1], np.uint16).view(np.int16).copy()).cuda()
        tiles = torch.from_numpy(tile_maxima(op[1], w, h).view(np.int16).copy()).cuda()
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        gv.synchronize()
        gv.integrate_prepare_device(depth.data_ptr(), w, h, cam, tiles.data_ptr(), side.cuda_stream)
        side.synchronize()
        if op[3] is not None:
            self.step(op[3], what + ", the %s in between" % op[3][0])
        self.model.integrate(op[1], w, h, cam)
        gv.integrate_device(depth.data_ptr(), w, h, cam, tile_max_ptr=tiles.data_ptr())
        gv.synchronize()
        self.same_as_model(what)

    def classes_prepared(self, op, what):
        """integrate_prepare_device for a frame (on the default stream, waited for), then integrate_classes_device with that frame's
        depth pointer and camera -- it holds no tile maxima, so the list is not its own and it culls for itself -- then the
        integrate_device the list was prepared for, which finds it used up and culls too: the frame is fused twice, the vote cast once.
        The images live in allocations of the library's own (tsdf_device_alloc)."""
        import ctypes as C
        gv, w, h, lib = self.gv, self.width, self.height, _capi.lib
        _, d, k, s, cam4 = op
        cam = Cam(*cam4)
        held = []

        def dev(a, dtype):
            a = np.ascontiguousarray(a, dtype).reshape(-1)
            p = C.c_void_p()
            _capi.check(lib.tsdf_device_alloc(max(a.nbytes, 4), C.byref(p)))
            held.append(p)
            _capi.check(lib.tsdf_device_upload(p, a.ctypes.data, a.nbytes))
            return p.value

        try:
            depth, classes, tiles = dev(d, np.uint16), dev(k, np.uint16), dev(tile_maxima(d, w, h), np.uint16)
            conf = dev(s, np.uint8) if s is not None else None
            gv.synchronize()
            gv.integrate_prepare_device(depth, w, h, cam, tiles, 0)
            _capi.check(lib.tsdf_stream_synchronize(None))
            self.run.apply(("depth_classes", d, k, s, None, cam4))
            gv.integrate_classes_device(depth, classes, w, h, cam, confidence_ptr=conf)
            gv.synchronize()
            self.same_as_model(what + ", the class call")
            self.model.integrate(d, w, h, cam)
            gv.integrate_device(depth, w, h, cam, tile_max_ptr=tiles)
            gv.synchronize()
            self.same_as_model(what)
        finally:
            for p in held:
                lib.tsdf_device_free(p)

    def refused(self, op, what):
        gv = self.gv
        before = self.library_state()
        self.run.apply(("refused", op))          # (the model refuses it too, and stays as it was)
        other = snap = None
        reason = op[0]
        if reason == "depth_classes":
            reason = "depth_classes_rgb" if op[4] is not None and not gv.colour_enabled() else "depth_classes_nodes"
        with pytest.raises(ValueError, match=REFUSALS[reason]):
            if op[0] == "depth_classes":
                gv.integrate_classes(op[1], op[2], self.width, self.height, Cam(*op[5]), confidence=op[3], rgb=op[4])
            elif op[0] == "remove":
                gv.deintegrate(op[1], self.width, self.height, Cam(*op[2]))
            elif op[0] == "rays_colour":
                gv.integrate_rays(op[1], op[2], band_only=op[4], min_range=op[5], max_range=op[6], rgb=op[3])
            elif op[0] == "depth_weighted_colour":
                gv.integrate_weighted(op[1], op[2], self.width, self.height, Cam(*op[4]), rgb=op[3])
            else:
                other = tsdf_amd.TSDFVolume(op[1], (200.0, 200.0, 200.0))
                other.set_weight_data(np.ones(other.resident_voxels(), F32))
                snap = other.snapshot()
                gv.restore(snap)
        assert REFUSALS[reason] in _capi.last_error(), what
        for o in (snap, other):
            if o is not None:
                o.close()
        after = self.library_state()
        for a, b, name in zip(before, after, ("distances", "weights", "colours", "cap", "storage", "class words")):
            assert (a is None and b is None) or np.array_equal(np.asarray(a).view(U32) if isinstance(a, np.ndarray) else a,
                                                               np.asarray(b).view(U32) if isinstance(b, np.ndarray) else b), what + ": " + name
        self.same_as_model(what)

    # ---- the end of a sequence
    def twin(self):
        """A new volume given the model's final arrays by upload, with the same cap and colour."""
        m = self.model
        t = make_volume(self.info)
        if any(self.gv.info().offset_at_clear):
            t.clear()                    # (the sequence cleared the volume at its offset: clear() is what bakes it in)
        assert tuple(t.info().offset_at_clear) == tuple(self.gv.info().offset_at_clear)
        if m.colour is not None:
            t.enable_colour()
            t.set_colour_data(m.colour)
        if m.classes is not None:
            t.enable_classes()
            t.set_class_data(m.classes)
        t.set_weight_cap(m.cap)
        t.set_distance_data(m.dist)
        t.set_weight_data(m.weight)
        return t

    def pictures(self, v):
        out = []
        for cam in self.info["cameras"]:
            out += list(v.raycast(self.width, self.height, Cam(*cam)))
        out.append(v.extract_surface())
        mesh = v.extract_mesh()
        out += [mesh.vertices, mesh.indices]
        mesh.close()
        out += list(v.occupancy_data(force_rebuild=True))
        return out

    def finish(self):
        what = "seed %d, the end" % self.seed
        t = self.twin()
        names = ("vertices 0", "normals 0", "vertices 1", "normals 1", "surface", "mesh vertices", "mesh indices", "fine", "cell", "reach")
        for name, a, b in zip(names, self.pictures(self.gv), self.pictures(t)):
            assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s of the twin has another shape" % (what, name)
            if a.dtype == np.float32:
                assert_same_floats(a, b, "%s: %s against the twin" % (what, name))
            else:
                assert np.array_equal(a, b), "%s: %s against the twin" % (what, name)
        depth, cam = self.info["last_frame"]
        self.model.integrate(depth, self.width, self.height, Cam(*cam))
        for v, who in ((self.gv, "the sequenced volume"), (t, "the twin")):
            v.integrate(depth, self.width, self.height, Cam(*cam))
            self.same_as_model("%s: one more frame into %s" % (what, who), v)
        t.close()


def drive(oracle, seed, ops=None, variant=0):
    """A whole sequence (or `ops` in place of the seed's own); a failure carries the seed, the step and the ops up to it."""
    q = Sequenced(oracle, seed, variant)
    if ops is not None:
        q.ops = ops
    try:
        for i, op in enumerate(q.ops):
            try:
                q.step(op, "seed %d, step %d (%s)" % (seed, i, op[0]))
            except Exception as e:
                raise AssertionError("seed %d, step %d: %s: %s\nthe ops up to it:\n%s" % (seed, i, type(e).__name__, e, S.describe(q.ops, i + 1))) from e
        try:
            q.finish()
        except Exception as e:
            raise AssertionError("seed %d, after the last step: %s: %s\nthe ops:\n%s" % (seed, type(e).__name__, e, S.describe(q.ops))) from e
    finally:
        q.close()


@pytest.mark.parametrize("seed", S.SEEDS)
def test_a_sequence_of_writers_leaves_the_models_state(oracle, seed):
    drive(oracle, seed)
    _SEEN["seeds"].add(seed)


def test_every_weight_storage_was_met_and_which_ray_casts_ran():
    """Reports, across the seeds, the comparisons made in each storage mode and the ray casts by kernel family.  The cell-parallel cast
    is the chooser's to pick or not: it is reported, never forced."""
    if len(_SEEN["seeds"]) < len(S.SEEDS):
        pytest.skip("needs the whole sweep")
    print("\nop sequences: state comparisons by weight storage %s; ray casts: %d cell-parallel, %d march"
          % (dict(sorted(_SEEN["modes"].items())), _SEEN["casts"][True], _SEEN["casts"][False]))
    assert set(_SEEN["modes"]) == {8, 16, 32}, _SEEN["modes"]


# ---- what the sequences found ---------------------------------------------------------------------------------------------------------
def stale_rim_sequence():
    """The shortest form of what a sweep over other data of the same sequences met behind a removal (seed 10 on the 72 x 12 x 40 grid):
    brick (1, 2, 4) lies beside the boundary brick (0, 2, 4) and holds one voxel, within two voxels of it, that is safely positive but
    not flat.  Its own flag is clear, the boundary brick's is set.  A frame that only ever saw free space there is fused first (it
    stores no distance: the scratch of the incremental rebuild exists, nothing is marked) and taken out afterwards: the voxel returns
    to +trunc and no brick is in reach of anything but cleared voxels."""
    info, image, _ = S.sequence(0)
    dims = info["dims"]
    rng = np.random.default_rng(5)
    cam, far = S._view(rng, (dims, info["phys"], info["offset"]), image)
    frame = (np.full(image[0] * image[1], int(4 * far), np.uint16), S.cam4(cam))
    trunc = S._truncation(dims, info["phys"])
    dist = np.full(dims[0] * dims[1] * dims[2], trunc, F32)
    dist[5 + dims[0] * (10 + dims[1] * 17)] = F32(0.5) * trunc
    return [("depth",) + frame, ("upload", dist, None, None), ("flags", True), ("remove",) + frame, ("flags", True)]


def test_a_rebuild_clears_the_flag_of_a_boundary_brick_when_the_brick_beside_it_turns_flat(oracle):
    """The incremental rebuild of the brick flags skipped every brick whose own flag is clear -- also the ones beside a boundary brick,
    whose rim bits that neighbour reads -- so the boundary brick stayed flagged after the values beside it had returned to the flat band:
    a superset, harmless to a picture, but not the definition a rebuild promises (tests/test_occupancy.py).  Fixed in
    occupancy_scan_kernel (tsdf_amd/csrc/volume.hip)."""
    ops = stale_rim_sequence()
    run = ModelRun(oracle, *S.sequence(0)[:2])
    assert run.apply(ops[0]) >= 16
    run.apply(ops[1])
    fine, _, _ = run.apply(ops[2])
    assert fine[4, 2, 0] == 1 and fine[4, 2, 1] == 0          # (the boundary brick by its rim rule; the brick that holds the voxel not)
    assert run.apply(ops[3]) >= 16
    assert not run.apply(ops[4])[0].any() and np.all(run.model.dist == run.model.trunc())
    drive(oracle, 0, ops=ops)
