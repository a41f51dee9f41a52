"""One CPU model of a whole volume: every writer, switch and observer of tsdf_amd.TSDFVolume on plain (dist, weight, colour, class) arrays, each
delegated to the reference that already pins that operation on its own -- oracle/ for integrate, ray cast and marching cubes,
weight_cap_ref, colour_ref, deintegrate_ref, weighted_ref, rays_integrate_ref, rays_colour_ref, fuse_ref, snapshot_ref, classes_ref, and
the flag definition of tests/test_occupancy.py.  No arithmetic of its own: what is new is only that the references act on ONE state, in any
order (tests/op_sequences.py, tests/test_op_sequences.py; tests/weighted_sequences.py, tests/test_weighted_fuzz.py;
tests/class_sequences.py, tests/test_class_fuzz.py).  The class words belong to the class writers alone: a class integrate votes, clear
zeroes, an upload sets them, and every other writer -- restore included -- leaves them as they are.  How the weights
are stored must not show in a single bit, so the model has no storage.  `mutant=` switches in one plausible defect at a time
(tests/test_op_sequences_host.py and tests/test_weighted_fuzz_host.py show that the sequences see each).
Test infrastructure only."""
import numpy as np

from tests import classes_ref, colour_ref, deintegrate_ref, fuse_ref, rays_colour_ref, rays_integrate_ref, snapshot_ref, weighted_ref
from tests.field_ref import geometry as field_geometry
from tests.weight_cap_ref import oracle_step

F32, U32 = np.float32, np.uint32
MUTANTS = ("counts_wrap_at_256", "restore_keeps_colour", "rays_ignore_cap", "remove_keeps_distance",
           # switched in only inside integrate_weighted (tests/test_weighted_fuzz_host.py shows that its sequences and cases see each)
           "weighted_cap_clamps_divisor", "weighted_invalid_pixel_colours", "weighted_next_pixel",
           # switched in only where class words are enabled (tests/test_op_sequences_host.py shows that the class sequences see each)
           "restore_zeroes_classes", "remove_takes_votes_back", "classes_vote_in_free_space")
WEIGHTED_MUTANTS = MUTANTS[4:7]
CLASS_MUTANTS = MUTANTS[7:]


class Refused(Exception):
    """The call is on a refusal list of include/tsdf_amd.h: the model's state is as it was."""


class VolumeModel:
    def __init__(self, O, dims, phys, offset=None, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.O, self.mutant = O, mutant
        self.ov = O.Volume(dims, phys)
        if offset is not None:
            self.ov.offset(*offset)          # (set without a clear, as the ray and fuse tests do: offset_at_clear stays zero)
        self.colour = None                   # uint32 words, or None while colour is not enabled
        self.classes = None                  # uint32 {class, votes} words, or None while classes are not enabled
        self.explicit_nodes = False          # deformation() was called: the nodes are materialised (a class integrate is refused)
        self.cap = 0
        self.last_stores = None              # distance stores of the last integrate_weighted

    # ---- the state
    @property
    def dist(self):
        return self.ov.dist

    @property
    def weight(self):
        return self.ov.weight

    def dims(self):
        return tuple(int(s) for s in self.ov.size())

    def trunc(self):
        return F32(self.ov.truncation_distance())

    def state(self):
        """Copies of (dist, weight, colour or None, cap, class words or None)."""
        return (self.dist.copy(), self.weight.copy(), None if self.colour is None else self.colour.copy(), self.cap,
                None if self.classes is None else self.classes.copy())

    def _colour_geometry(self):
        g = self.ov.g
        return (self.dims(), np.array(g.vs, F32), np.array(g.offset, F32), np.array(g.offset_at_clear, F32), self.trunc())

    # ---- writers: each returns the number of voxels the call updated (what the library's call reports, where it reports one)
    def integrate(self, depth, width, height, cam):
        before = self.weight.view(U32).copy()
        oracle_step(self.O, self.ov, depth, cam, self.cap, width, height)
        return int((self.weight.view(U32) != before).sum())

    def integrate_colour(self, depth, rgb, width, height, cam):
        if self.colour is None:
            raise Refused("colour integrate on a volume without colour enabled")
        self.colour = colour_ref.integrate_colour(self.O, self.colour, self._colour_geometry(), depth, rgb, width, height, cam)[0]
        return self.integrate(depth, width, height, cam)

    def integrate_classes(self, depth, classes, confidence, rgb, width, height, cam):
        """tsdf_integrate_classes: the plain (or, with rgb, the colour) integrate plus tests/classes_ref.py's vote.  The vote reads the
        geometry, the images and the old words only: which of the two comes first makes no difference."""
        if self.classes is None:
            raise Refused("tsdf_integrate_classes: classes are not enabled on this volume")
        if self.explicit_nodes:
            raise Refused("tsdf_integrate_classes: not supported once the deformation nodes are explicit")
        if rgb is not None and self.colour is None:
            raise Refused("tsdf_integrate_classes: rgb given but colour is not enabled on this volume")
        geom = self._colour_geometry()
        if self.mutant == "classes_vote_in_free_space":
            geom = geom[:4] + (F32(np.inf),)
        self.classes, updated, _ = classes_ref.integrate_classes(self.O, self.classes, geom, depth, classes, confidence, width, height, cam)
        if rgb is None:
            self.integrate(depth, width, height, cam)
        else:
            self.integrate_colour(depth, rgb, width, height, cam)
        return int(updated.sum())            # (the distance update's set: what the counter counts, whether or not a cap holds the weight)

    def integrate_weighted(self, depth, weights, width, height, cam, rgb=None):
        """tsdf_integrate_weighted: tests/weighted_ref.py's frame and blend, tests/colour_ref.py on the masked image."""
        if rgb is not None and self.colour is None:
            raise Refused("tsdf_integrate_weighted: colour is not enabled on this volume")
        p_image = np.asarray(weights, F32).reshape(-1)
        in_set, tsdf, pidx = weighted_ref.frame(self.O, self.ov, depth, p_image, cam, width, height)
        if self.mutant == "weighted_next_pixel":             # the weight of pixel (px + 1, py), clamped to the row
            pidx = (pidx // width) * width + np.minimum(pidx % width + 1, width - 1)
        keep_d, keep_w = self.dist.copy(), self.weight.copy()
        p = p_image[pidx]
        updated, self.last_stores = weighted_ref.blend(self.ov, in_set, tsdf, p, self.cap)
        if self.mutant == "weighted_cap_clamps_divisor" and self.cap:
            with np.errstate(all="ignore"):
                nw = (keep_w + p).astype(F32)
                clamped = in_set & (nw > F32(self.cap))
                d = (((keep_d * keep_w).astype(F32) + (tsdf * p).astype(F32)).astype(F32) / F32(self.cap)).astype(F32)
            self.dist[clamped] = d[clamped]
        if rgb is not None:
            image = np.asarray(depth, np.uint16).reshape(-1) if self.mutant == "weighted_invalid_pixel_colours" else weighted_ref.masked_depth(depth, p_image)
            self.colour = colour_ref.integrate_colour(self.O, self.colour, self._colour_geometry(), image, rgb, width, height, cam)[0]
        return updated

    def deintegrate(self, depth, width, height, cam):
        if self.cap:
            raise Refused("tsdf_deintegrate: the volume has a weight cap")
        in_set, tsdf = deintegrate_ref.frame_set(self.O, self.ov, depth, cam, width, height)
        keep = self.dist.copy()
        updated, _ = deintegrate_ref.remove(self.ov, in_set, tsdf)
        if self.mutant == "remove_keeps_distance":
            gone = in_set & (self.weight == 0)
            self.dist[gone] = keep[gone]
        if self.mutant == "remove_takes_votes_back" and self.classes is not None:
            self.classes = np.where(in_set & (self.weight == 0), U32(0), self.classes)
        return updated

    def integrate_rays(self, origins, points, rgb=None, band_only=False, min_range=0.0, max_range=np.inf):
        if rgb is not None and self.colour is None:
            raise Refused("tsdf_integrate_rays_colour: colour is not enabled on this volume")
        geom = rays_integrate_ref.geometry(self.ov)
        flags = rays_integrate_ref.BAND_ONLY if band_only else 0
        cap = 0 if self.mutant == "rays_ignore_cap" else self.cap
        top = self.weight.max()
        if rgb is None:
            d, w, upd, _ = rays_integrate_ref.integrate(geom, self.dist, self.weight, origins, points, min_range, max_range, flags, cap)
        else:
            d, w, upd, words, _, _ = rays_colour_ref.integrate(geom, self.dist, self.weight, self.colour, origins, points, rgb, min_range,
                                                               max_range, flags, cap)
            self.colour = words
        self._store(d, w, upd, top)
        return int(upd.sum())

    def fuse(self, src, m=None):
        top = self.weight.max()
        d, w, upd = fuse_ref.fuse(self.O, field_geometry(self.ov), self.trunc(), self.dist, self.weight, field_geometry(src.ov), src.dist,
                                  src.weight, m, cap=self.cap)
        self._store(d, w, upd, top)
        return int(upd.sum())

    def _store(self, d, w, upd, top_before):
        if self.mutant == "counts_wrap_at_256" and top_before <= 255:
            w = np.where(upd, np.mod(w, F32(256.0)), w).astype(F32)
        self.ov.set_distance_data(d)
        self.ov.set_weight_data(w)

    def snapshot(self):
        """What tsdf_volume_snapshot keeps, with the weights as fp32 (the storage of the moment is the library's business): a dict."""
        ids, d, w, c = snapshot_ref.take(self.dist, self.weight, self.dims(), self.trunc(), 32, self.colour)
        return {"size": self.dims(), "fill": self.trunc(), "ids": ids, "dist": d, "weight": w, "colour": c}

    def restore(self, s):
        if tuple(s["size"]) != self.dims():
            raise Refused("tsdf_volume_restore: the snapshot is of another grid")
        d, w, c = snapshot_ref.put(s["ids"], s["dist"], s["weight"], s["colour"], s["size"], s["fill"])
        self.ov.set_distance_data(d)
        self.ov.set_weight_data(w)
        if self.mutant == "restore_zeroes_classes" and self.classes is not None:
            self.classes = np.zeros_like(self.classes)
        if self.mutant == "restore_keeps_colour":
            return
        if c is not None:
            self.colour = c                                  # a snapshot with colour enables it
        elif self.colour is not None:
            self.colour = np.zeros_like(self.colour)         # one without zeroes an enabled array

    def clear(self):
        self.ov.clear()
        if self.colour is not None:
            self.colour = np.zeros_like(self.colour)
        if self.classes is not None:
            self.classes = np.zeros_like(self.classes)

    def set_distance_data(self, d):
        self.ov.set_distance_data(d)

    def set_weight_data(self, w):
        self.ov.set_weight_data(w)

    def set_colour_data(self, c):
        if self.colour is None:
            raise Refused("colour data access on a volume without colour enabled")
        self.colour = np.array(c, U32).reshape(-1)
        assert self.colour.size == self.dist.size

    def set_class_data(self, c):
        if self.classes is None:
            raise Refused("class data access on a volume without classes enabled")
        self.classes = np.array(c, U32).reshape(-1)
        assert self.classes.size == self.dist.size

    # ---- switches
    def enable_classes(self, on=True):
        if not on:
            self.classes = None
        elif self.classes is None:
            self.classes = np.zeros(self.dist.size, U32)

    def materialise_nodes(self):
        """deformation(): the regular grid as explicit nodes -- the same centres, so every writer that takes nodes writes the same bits."""
        self.explicit_nodes = True

    def enable_colour(self, on=True):
        if not on:
            self.colour = None
        elif self.colour is None:
            self.colour = np.zeros(self.dist.size, U32)

    def set_weight_cap(self, cap):
        self.cap = int(cap)

    def set_weight_storage(self, bits):
        pass

    # ---- observers
    def raycast(self, cam, width, height):
        return self.ov.raycast(width, height, cam.pose(), cam.kinv(), nthreads=self.O.max_threads())

    def surface(self):
        return self.O.marching_cubes(self.dist, self.dims(), self.ov.voxel_size(), self.ov.offset(), nthreads=self.O.max_threads())

    def flags(self):
        """(fine, cell, reach) as the ray caster's brick flags are defined."""
        from tests.test_occupancy import _expected, _expected_reach
        tau = F32(0.01) * self.trunc()
        fine, cell = _expected(self.dist, self.dims(), tau, trunc=self.trunc())
        return fine, cell, _expected_reach(fine)


class ModelRun:
    """One sequence of tests/op_sequences.py on the model: the volume, the source of its fuses and the snapshots taken so far."""

    def __init__(self, O, info, image, mutant=None):
        from tests.helpers import Cam
        self.Cam = Cam
        self.model = VolumeModel(O, info["dims"], info["phys"], info["offset"], mutant)
        s = info["source"]
        self.source = VolumeModel(O, s["dims"], s["phys"], s["offset"])
        self.source.set_distance_data(s["dist"])
        self.source.set_weight_data(s["weight"])
        self.width, self.height = image
        self.snapshots = []

    def apply(self, op):
        """-> the updated-voxel count of a writer, the result of an observer, None for a switch.  A "depth_prepared" applies the op in
        between first: the prepare call writes nothing.  A refused op raises Refused and leaves the state as it was."""
        m, kind, w, h = self.model, op[0], self.width, self.height
        if kind == "depth":
            return m.integrate(op[1], w, h, self.Cam(*op[2]))
        if kind == "depth_prepared":
            if op[3] is not None:
                self.apply(op[3])
            return m.integrate(op[1], w, h, self.Cam(*op[2]))
        if kind == "depth_colour":
            return m.integrate_colour(op[1], op[2], w, h, self.Cam(*op[3]))
        if kind == "depth_classes":
            return m.integrate_classes(op[1], op[2], op[3], op[4], w, h, self.Cam(*op[5]))
        if kind == "classes":
            return m.enable_classes(op[1])
        if kind == "upload_classes":
            return m.set_class_data(op[1])
        if kind == "nodes":
            return m.materialise_nodes()
        if kind in ("counting", "pin"):
            return None                      # (the counters and the storage are the library's: the model counts every writer and has no storage)
        if kind == "image":
            self.width, self.height = op[1]  # the size of every image from here on
            return None
        if kind == "depth_weighted":
            return m.integrate_weighted(op[1], op[2], w, h, self.Cam(*op[3]))
        if kind == "depth_weighted_colour":
            return m.integrate_weighted(op[1], op[2], w, h, self.Cam(*op[4]), op[3])
        if kind == "remove":
            return m.deintegrate(op[1], w, h, self.Cam(*op[2]))
        if kind == "rays":
            return m.integrate_rays(op[1], op[2], None, op[3], op[4], op[5])
        if kind == "rays_colour":
            return m.integrate_rays(op[1], op[2], op[3], op[4], op[5], op[6])
        if kind == "fuse":
            return m.fuse(self.source, op[1])
        if kind == "restore":
            return m.restore(self.snapshots[op[1]])
        if kind == "restore_other":
            return m.restore({"size": tuple(op[1])})
        if kind == "upload":
            if op[1] is not None:
                m.set_distance_data(op[1])
            if op[2] is not None:
                m.set_weight_data(op[2])
            if op[3] is not None:
                m.set_colour_data(op[3])
            return None
        if kind == "clear":
            return m.clear()
        if kind == "cap":
            return m.set_weight_cap(op[1])
        if kind == "storage":
            return m.set_weight_storage(op[1])
        if kind == "colour":
            return m.enable_colour(op[1])
        if kind == "raycast":
            return m.raycast(self.Cam(*op[1]), w, h)
        if kind == "surface":
            return m.surface()
        if kind == "flags":
            return m.flags()
        if kind == "snapshot":
            self.snapshots.append(m.snapshot())
            return self.snapshots[-1]
        if kind == "refused":
            before = m.state()
            try:
                self.apply(op[1])
            except Refused:
                after = m.state()
                assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(before[:3] + before[4:], after[:3] + after[4:]))
                assert before[3] == after[3]
                return None
            raise AssertionError("the model does not refuse %r" % (op[1][0],))
        raise ValueError(kind)
