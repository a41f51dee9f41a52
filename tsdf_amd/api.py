"""Python mirror of the reference's class surface for the hot path, over the C ABI.

Names, argument meaning and error behaviour follow src/include/TSDFVolume.hpp,
GPURaycaster.hpp and BilateralFilter.hpp of the reference so that tests read like the
reference's own.  Matrices are column-major float32 vectors (what Eigen's .data() yields).
Every call runs the HIP kernels in tsdf_amd/lib/libtsdf_hip.so; there is no CPU path.
"""
import ctypes as C
import os
import struct

import numpy as np

from . import _capi
from ._capi import check, lib


def _mat(a, n):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    if a.size != n:
        raise ValueError("expected %d matrix elements, got %d" % (n, a.size))
    return a


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def direction_lengths(directions):
    """fp32 lengths of (n, 3) float32 directions: sqrt((x x + y y) + z z), every operation rounded to float32."""
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def unit_directions(directions):
    """Each of (n, 3) float32 directions divided by its fp32 length (direction_lengths); a zero or non-finite direction comes out
    non-finite, which a ray query answers with a miss."""
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(d / direction_lengths(d)[:, None], dtype=np.float32)


def _camera_matrices(camera):
    """pose, inverse_pose, k, kinv of anything shaped like the reference's Camera (src/include/Camera.hpp)."""
    return (_mat(camera.pose(), 16), _mat(camera.inverse_pose(), 16), _mat(camera.k(), 9), _mat(camera.kinv(), 9))


class TSDFVolume:
    """src/include/TSDFVolume.hpp:21-304.  `slab=(z_begin, z_end)` makes this object one Z-slab of the
    grid (multi-GPU sharding); the default is the whole volume."""

    def __init__(self, size=(64, 64, 64), physical_size=(3000.0, 3000.0, 3000.0), slab=None):
        self._h = C.c_void_p()
        sx, sy, sz = (int(s) for s in size)
        if min(sx, sy, sz) < 0:
            raise ValueError("Attempt to construct TSDFVolume with zero or negative size")
        px, py, pz = (float(p) for p in physical_size)
        if slab is None:
            check(lib.tsdf_volume_create(sx, sy, sz, px, py, pz, C.byref(self._h)))
        else:
            check(lib.tsdf_volume_create_slab(sx, sy, sz, px, py, pz, int(slab[0]), int(slab[1]), C.byref(self._h)))

    def close(self):
        if lib is not None and getattr(self, "_h", None) is not None and self._h.value:   # (lib is None during interpreter shutdown)
            for ref in getattr(self, "_dependents", ()):      # pipelines built on this volume hold its stream: they go first
                dep = ref()
                if dep is not None:
                    dep.close()
            lib.tsdf_volume_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    # ---- geometry accessors (TSDFVolume.hpp:120-153)
    def info(self):
        i = _capi.VolumeInfo()
        check(lib.tsdf_volume_get_info(self._h, C.byref(i)))
        return i

    def size(self):
        return tuple(self.info().size)

    def voxel_size(self):
        return np.array(self.info().voxel_size, np.float32)

    def physical_size(self):
        return np.array(self.info().physical_size, np.float32)

    def truncation_distance(self):
        return float(self.info().truncation_distance)

    def offset(self, *o):
        """offset() -> current offset; offset(ox, oy, oz) sets it (without re-initialising the deformation grid)."""
        if o:
            check(lib.tsdf_volume_set_offset(self._h, float(o[0]), float(o[1]), float(o[2])))
            return None
        return np.array(self.info().offset, np.float32)

    def set_global_transform(self, rotation, translation):
        """m_global_rotation (three angles) / m_global_translation, used by deform_mesh and stored in .tsdf files."""
        i = self.info()
        off = np.array(i.offset, np.float32)
        r = np.ascontiguousarray(rotation, np.float32)
        t = np.ascontiguousarray(translation, np.float32)
        check(lib.tsdf_volume_set_header(self._h, _fp(off), float(i.truncation_distance), float(i.max_weight), _fp(t), _fp(r)))

    def resident_planes(self):
        i = self.info()
        return int(i.z_store_begin), int(i.z_store_end)

    def owned_planes(self):
        i = self.info()
        return int(i.z_begin), int(i.z_end)

    def resident_voxels(self):
        i = self.info()
        return int(i.size[0]) * int(i.size[1]) * int(i.z_store_end - i.z_store_begin)

    def index(self, x, y, z):
        sx, sy, _ = self.size()
        return x + y * sx + z * sx * sy

    def clear(self):
        check(lib.tsdf_volume_clear(self._h))
        check(lib.tsdf_volume_synchronize(self._h))

    def set_stream(self, hip_stream):
        check(lib.tsdf_volume_set_stream(self._h, C.c_void_p(int(hip_stream) if hip_stream else 0)))

    def stream_ptr(self):
        """The HIP stream (as an integer, 0 = the null stream) the volume's kernels are enqueued on now."""
        p = C.c_void_p()
        check(lib.tsdf_volume_stream(self._h, C.byref(p)))
        return p.value or 0

    def synchronize(self):
        check(lib.tsdf_volume_synchronize(self._h))

    # ---- data access (TSDFVolume.hpp:165-203): device pointers, blocking uploads
    def distance_data(self):
        p = C.c_void_p()
        check(lib.tsdf_volume_distances(self._h, C.byref(p)))
        return p.value

    def weight_data(self):
        p = C.c_void_p()
        check(lib.tsdf_volume_weights(self._h, C.byref(p)))
        return p.value

    def weight_storage(self):
        """(bits per stored weight: 8 / 16 = packed counts, 32 = the reference's fp32 array; pinned to fp32 by weight_data())"""
        bits, pinned = C.c_int(), C.c_int()
        check(lib.tsdf_volume_weight_storage(self._h, C.byref(bits), C.byref(pinned)))
        return bits.value, bool(pinned.value)

    def last_raycast_cell_parallel(self):
        """True when the volume's last ray cast took the cell-parallel kernels (scheduling only: the same bits as the march)."""
        k = C.c_int()
        check(lib.tsdf_volume_last_raycast_kind(self._h, C.byref(k)))
        return bool(k.value)

    def last_cell_list(self):
        """Tasks the last cell-parallel cast listed (diagnostics; waits for the volume's stream)."""
        n = C.c_uint32()
        check(lib.tsdf_volume_last_cell_list(self._h, C.byref(n)))
        return int(n.value)

    def set_weight_storage(self, bits):
        """Widen the weight storage now (8 -> 16 -> 32 bits, values unchanged) instead of when a count is about to overflow."""
        check(lib.tsdf_volume_set_weight_storage(self._h, int(bits)))

    def set_weight_cap(self, cap):
        """Cap the weight integrate stores at `cap` (1 .. 65535; 0 = off, the default): a running average that follows a scene that
        changes, and -- up to 255 -- counts that stay in 8 bits for ever.  The blend's divisor is never clamped (include/tsdf_amd.h)."""
        cap = int(cap)
        if cap < 0 or cap > 0xFFFFFFFF:
            raise ValueError("set_weight_cap: the cap is 0 (off) or 1 .. 65535")
        check(lib.tsdf_volume_set_weight_cap(self._h, cap))

    def weight_cap(self):
        c = C.c_uint32()
        check(lib.tsdf_volume_weight_cap(self._h, C.byref(c)))
        return int(c.value)

    def deformation(self):
        p = C.c_void_p()
        check(lib.tsdf_volume_deformation(self._h, C.byref(p)))
        return p.value

    def _host(self, a, per_voxel=1):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        if a.size != self.resident_voxels() * per_voxel:
            raise ValueError("expected %d floats, got %d" % (self.resident_voxels() * per_voxel, a.size))
        return a

    def set_distance_data(self, distance_data):
        a = self._host(distance_data)
        check(lib.tsdf_volume_set_distance_data(self._h, a.ctypes.data))

    def set_weight_data(self, weight_data):
        a = self._host(weight_data)
        check(lib.tsdf_volume_set_weight_data(self._h, a.ctypes.data))

    def set_deformation(self, nodes):
        """nodes: (voxels, 6) float32 = translation xyz + rotation xyz (DeformationNode, TSDFVolume.hpp:23-26)."""
        a = self._host(nodes, 6)
        check(lib.tsdf_volume_set_deformation(self._h, a.ctypes.data))

    def get_deformation(self):
        """The deformation nodes as (voxels, 6) float32 (tsdf_volume_get_deformation_planes over the resident planes): what
        set_deformation takes; the regular grid while the nodes are implicit.  Blocking."""
        z0, z1 = self.resident_planes()
        a = np.empty((self.resident_voxels(), 6), np.float32)
        check(lib.tsdf_volume_get_deformation_planes(self._h, 0, z1 - z0, a.ctypes.data))
        return a

    def extract_surface(self):
        """extract_surface on the device (tsdf_volume_marching_cubes): (3*T, 3) float32 vertices, triangle t = rows 3t,
        3t+1, 3t+2, cubes in the reference's order -- the same array as marching_cubes() on the downloaded distances."""
        table = marching_cubes_table()
        n = C.c_uint64(0)
        check(lib.tsdf_volume_marching_cubes(self._h, table.ctypes.data, C.byref(n), None, 0))
        out = np.empty((n.value, 3), np.float32)
        if n.value:
            check(lib.tsdf_volume_marching_cubes(self._h, table.ctypes.data, C.byref(n), out.ctypes.data, n.value))
        return out

    def deform_mesh(self, points):
        """TSDFVolume::deform_mesh (src/TSDF/TSDFVolume.cu:265-291): points (n,3) float32 -> deformed copy."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3).copy()
        check(lib.tsdf_volume_deform_points(self._h, p.shape[0], p.ctypes.data))
        return p

    def get_distance_data(self):
        a = np.empty(self.resident_voxels(), np.float32)
        check(lib.tsdf_volume_get_distance_data(self._h, a.ctypes.data))
        return a

    def get_weight_data(self):
        a = np.empty(self.resident_voxels(), np.float32)
        check(lib.tsdf_volume_get_weight_data(self._h, a.ctypes.data))
        return a

    # ---- integrate (TSDFVolume.hpp:238-246)
    def integrate(self, depth_map, width, height, camera):
        """Blocking; depth_map is a host uint16 array of width*height mm values (0 = invalid)."""
        if depth_map is None:
            raise AssertionError("depth_map")        # the reference asserts (TSDFVolume.cu:862)
        d = np.ascontiguousarray(depth_map, dtype=np.uint16).reshape(-1)
        if d.size != width * height:
            raise ValueError("depth map has %d pixels, expected %d" % (d.size, width * height))
        pose, ipose, k, kinv = _camera_matrices(camera)
        check(lib.tsdf_integrate(self._h, d.ctypes.data, width, height, _fp(pose), _fp(ipose), _fp(k), _fp(kinv)))

    def integrate_device(self, depth_ptr, width, height, camera, tile_max_ptr=None):
        """Asynchronous on the volume's stream; depth_ptr is a device pointer to width*height uint16.  tile_max_ptr: the
        16 x 16 pixel tile maxima of that image when the caller holds them (BilateralFilter.filter_device(tile_max_ptr=...))."""
        pose, ipose, k, kinv = _camera_matrices(camera)
        if tile_max_ptr:
            check(lib.tsdf_integrate_device_tiles(self._h, C.c_void_p(int(depth_ptr)), width, height, _fp(pose), _fp(ipose),
                                                  _fp(k), _fp(kinv), C.c_void_p(int(tile_max_ptr))))
        else:
            check(lib.tsdf_integrate_device(self._h, C.c_void_p(int(depth_ptr)), width, height, _fp(pose), _fp(ipose),
                                            _fp(k), _fp(kinv)))

    def deintegrate(self, depth_map, width, height, camera):
        """Take a frame back out (include/tsdf_amd.h, "de-integration"): the depth map and camera of an earlier integrate().  Blocking.
        Refused on a volume with a weight cap."""
        if depth_map is None:
            raise AssertionError("depth_map")
        d = np.ascontiguousarray(depth_map, dtype=np.uint16).reshape(-1)
        if d.size != width * height:
            raise ValueError("depth map has %d pixels, expected %d" % (d.size, width * height))
        pose, ipose, k, kinv = _camera_matrices(camera)
        check(lib.tsdf_deintegrate(self._h, d.ctypes.data, width, height, _fp(pose), _fp(ipose), _fp(k), _fp(kinv)))

    def deintegrate_device(self, depth_ptr, width, height, camera):
        """deintegrate() of a device image (width*height uint16), asynchronous on the volume's stream."""
        pose, ipose, k, kinv = _camera_matrices(camera)
        check(lib.tsdf_deintegrate_device(self._h, C.c_void_p(int(depth_ptr)), width, height, _fp(pose), _fp(ipose), _fp(k), _fp(kinv)))

    # ---- weighted integration (include/tsdf_amd.h, "weighted integration"; not in the reference's class)
    def integrate_weighted(self, depth_map, weights, width, height, camera, rgb=None):
        """integrate() with one float32 weight per pixel: a pixel whose weight is not finite and > 0 counts as a pixel without depth.
        `rgb` (uint8, width*height*3) adds the colour update on a colour volume.  The volume goes to fp32 weights.  Blocking."""
        d = np.ascontiguousarray(depth_map, dtype=np.uint16).reshape(-1)
        if weights is None:
            raise ValueError("integrate_weighted: weights is None")
        p = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if d.size != width * height or p.size != width * height:
            raise ValueError("expected %d depth pixels and as many weights, got %d and %d" % (width * height, d.size, p.size))
        c = None
        if rgb is not None:
            c = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1)
            if c.size != 3 * width * height:
                raise ValueError("expected %d colour bytes, got %d" % (3 * width * height, c.size))
        pose, ipose, k, kinv = _camera_matrices(camera)
        check(lib.tsdf_integrate_weighted(self._h, d.ctypes.data, p.ctypes.data, c.ctypes.data if c is not None else None, width, height,
                                          _fp(pose), _fp(ipose), _fp(k), _fp(kinv)))

    def integrate_weighted_device(self, depth_ptr, weights_ptr, width, height, camera, rgb_ptr=None):
        """Asynchronous on the volume's stream; device pointers to width*height uint16, width*height float32 and (optionally)
        width*height*3 uint8."""
        pose, ipose, k, kinv = _camera_matrices(camera)
        check(lib.tsdf_integrate_weighted_device(self._h, C.c_void_p(int(depth_ptr)) if depth_ptr else None,
                                                 C.c_void_p(int(weights_ptr)) if weights_ptr else None,
                                                 C.c_void_p(int(rgb_ptr)) if rgb_ptr else None, width, height, _fp(pose), _fp(ipose), _fp(k), _fp(kinv)))

    def integrate_prepare_device(self, depth_ptr, width, height, camera, tile_max_ptr, stream):
        """The brick culling of integrate_device(depth_ptr, ..., tile_max_ptr=...) ahead of time, on `stream` (see
        tsdf_integrate_prepare_device_tiles); the matching integrate_device call then launches the integrate kernel alone."""
        pose, ipose, k, kinv = _camera_matrices(camera)
        check(lib.tsdf_integrate_prepare_device_tiles(self._h, C.c_void_p(int(depth_ptr)), width, height, _fp(pose), _fp(ipose),
                                                      _fp(k), _fp(kinv), C.c_void_p(int(tile_max_ptr)), C.c_void_p(int(stream))))

    # ---- colour fusion (include/tsdf_amd.h, "colour fusion"; not in the reference's class)
    def enable_colour(self, enabled=True):
        """Allocate the {r, g, b, n} dword per voxel, zeroed (False: free it).  Refused on a Z-slab."""
        check(lib.tsdf_volume_enable_colour(self._h, 1 if enabled else 0))
        self.synchronize()

    def colour_enabled(self):
        e = C.c_int()
        check(lib.tsdf_volume_colour_enabled(self._h, C.byref(e)))
        return bool(e.value)

    def colour_data(self):
        """Device pointer to the colour dwords."""
        p = C.c_void_p()
        check(lib.tsdf_volume_colours(self._h, C.byref(p)))
        return p.value

    def get_colour_data(self):
        """uint32 per resident voxel: r | g << 8 | b << 16 | n << 24."""
        a = np.empty(self.resident_voxels(), np.uint32)
        check(lib.tsdf_volume_get_colour_data(self._h, a.ctypes.data))
        return a

    def set_colour_data(self, colour_data):
        a = np.ascontiguousarray(colour_data, dtype=np.uint32).reshape(-1)
        if a.size != self.resident_voxels():
            raise ValueError("expected %d colour words, got %d" % (self.resident_voxels(), a.size))
        check(lib.tsdf_volume_set_colour_data(self._h, a.ctypes.data))

    def integrate_colour(self, depth_map, rgb, width, height, camera):
        """integrate() plus the colour of rgb (uint8, width*height*3 interleaved RGB, registered to the depth map); blocking."""
        d = np.ascontiguousarray(depth_map, dtype=np.uint16).reshape(-1)
        c = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1)
        if d.size != width * height or c.size != 3 * width * height:
            raise ValueError("expected %d depth pixels and %d colour bytes, got %d and %d" % (width * height, 3 * width * height, d.size, c.size))
        pose, ipose, k, kinv = _camera_matrices(camera)
        check(lib.tsdf_integrate_colour(self._h, d.ctypes.data, c.ctypes.data, width, height, _fp(pose), _fp(ipose), _fp(k), _fp(kinv)))

    def integrate_colour_device(self, depth_ptr, rgb_ptr, width, height, camera):
        """Asynchronous on the volume's stream; device pointers to width*height uint16 and width*height*3 uint8."""
        pose, ipose, k, kinv = _camera_matrices(camera)
        check(lib.tsdf_integrate_colour_device(self._h, C.c_void_p(int(depth_ptr)), C.c_void_p(int(rgb_ptr)), width, height, _fp(pose),
                                               _fp(ipose), _fp(k), _fp(kinv)))

    def sample_colours_device(self, n, points_ptr, rgb_ptr, stream=None):
        """n points (3 float32 each) -> 3 uint8 each, device pointers; on `stream` (default: the volume's)."""
        s = self.stream_ptr() if stream is None else stream
        check(lib.tsdf_volume_sample_colours_device(self._h, int(n), C.c_void_p(int(points_ptr)), C.c_void_p(int(rgb_ptr)),
                                                    C.c_void_p(int(s) if s else 0)))

    def sample_colours(self, points):
        """(n, 3) float32 world points (mm) -> (n, 3) uint8: the colour of the voxel each lies in, (0, 0, 0) for NaN, off-grid
        and unobserved voxels."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(p), 3), np.uint8)
        if not len(p):
            if not self.colour_enabled():
                raise ValueError("sample_colours: colour is not enabled on this volume")
            return out
        dp, dc = C.c_void_p(), C.c_void_p()
        check(lib.tsdf_device_alloc(p.nbytes, C.byref(dp)))
        try:
            check(lib.tsdf_device_alloc(out.nbytes, C.byref(dc)))
            check(lib.tsdf_device_upload(dp, p.ctypes.data, p.nbytes))
            self.sample_colours_device(len(p), dp.value, dc.value)
            self.synchronize()
            check(lib.tsdf_device_download(out.ctypes.data, dc, out.nbytes))
        finally:
            lib.tsdf_device_free(dp)
            if dc.value:
                lib.tsdf_device_free(dc)
        return out

    def extract_coloured_surface(self):
        """extract_surface() and the colour of every vertex (sample_colours): (vertices (3T, 3) float32, colours (3T, 3) uint8)."""
        V = self.extract_surface()
        return V, self.sample_colours(V)

    # ---- class fusion (include/tsdf_amd.h, "class fusion"; not in the reference's class)
    def enable_classes(self, enabled=True):
        """Allocate the {class, votes} dword per voxel, zeroed (False: free it).  Refused on a Z-slab."""
        check(lib.tsdf_volume_enable_classes(self._h, 1 if enabled else 0))
        self.synchronize()

    def classes_enabled(self):
        e = C.c_int()
        check(lib.tsdf_volume_classes_enabled(self._h, C.byref(e)))
        return bool(e.value)

    def class_data(self):
        """Device pointer to the class dwords."""
        p = C.c_void_p()
        check(lib.tsdf_volume_classes(self._h, C.byref(p)))
        return p.value

    def get_class_data(self):
        """uint32 per resident voxel: class | votes << 16; 0 where nothing was voted."""
        a = np.empty(self.resident_voxels(), np.uint32)
        check(lib.tsdf_volume_get_class_data(self._h, a.ctypes.data))
        return a

    def set_class_data(self, class_data):
        a = np.ascontiguousarray(class_data, dtype=np.uint32).reshape(-1)
        if a.size != self.resident_voxels():
            raise ValueError("expected %d class words, got %d" % (self.resident_voxels(), a.size))
        check(lib.tsdf_volume_set_class_data(self._h, a.ctypes.data))

    def integrate_classes(self, depth_map, classes, width, height, camera, confidence=None, rgb=None):
        """integrate() plus the vote of classes (uint16 per pixel, CLASS_VOID = no class, registered to the depth map) with the
        strength confidence (uint8 per pixel; None: 1 everywhere); rgb (uint8, width*height*3) adds integrate_colour()'s colour
        update on a colour volume.  Blocking."""
        d = np.ascontiguousarray(depth_map, dtype=np.uint16).reshape(-1)
        c = np.ascontiguousarray(classes, dtype=np.uint16).reshape(-1)
        if d.size != width * height or c.size != width * height:
            raise ValueError("expected %d depth pixels and %d classes, got %d and %d" % (width * height, width * height, d.size, c.size))
        s = r = None
        if confidence is not None:
            s = np.ascontiguousarray(confidence, dtype=np.uint8).reshape(-1)
            if s.size != width * height:
                raise ValueError("expected %d confidences, got %d" % (width * height, s.size))
        if rgb is not None:
            r = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1)
            if r.size != 3 * width * height:
                raise ValueError("expected %d colour bytes, got %d" % (3 * width * height, r.size))
        pose, ipose, k, kinv = _camera_matrices(camera)
        check(lib.tsdf_integrate_classes(self._h, d.ctypes.data, r.ctypes.data if r is not None else None, c.ctypes.data,
                                         s.ctypes.data if s is not None else None, width, height, _fp(pose), _fp(ipose), _fp(k), _fp(kinv)))

    def integrate_classes_device(self, depth_ptr, classes_ptr, width, height, camera, confidence_ptr=None, rgb_ptr=None):
        """Asynchronous on the volume's stream; device pointers to width*height uint16 depths and classes, optionally width*height
        uint8 confidences and width*height*3 uint8 colours."""
        ptr = lambda p: C.c_void_p(int(p)) if p else None
        pose, ipose, k, kinv = _camera_matrices(camera)
        check(lib.tsdf_integrate_classes_device(self._h, ptr(depth_ptr), ptr(rgb_ptr), ptr(classes_ptr), ptr(confidence_ptr), width, height,
                                                _fp(pose), _fp(ipose), _fp(k), _fp(kinv)))

    def sample_classes_device(self, n, points_ptr, classes_ptr, votes_ptr=None, stream=None):
        """n points (3 float32 each) -> a uint16 class and (optionally) a uint16 vote count each, device pointers; on `stream`
        (default: the volume's)."""
        s = self.stream_ptr() if stream is None else stream
        check(lib.tsdf_volume_sample_classes_device(self._h, int(n), C.c_void_p(int(points_ptr)) if points_ptr else None,
                                                    C.c_void_p(int(classes_ptr)) if classes_ptr else None,
                                                    C.c_void_p(int(votes_ptr)) if votes_ptr else None, C.c_void_p(int(s) if s else 0)))

    def sample_classes(self, points):
        """(n, 3) float32 world points (mm) -> (classes (n,) uint16, votes (n,) uint16): the class of the voxel each lies in and its
        votes, (CLASS_VOID, 0) for NaN, off-grid and unclassified voxels."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.empty((2, len(p)), np.uint16)
        if not len(p):
            if not self.classes_enabled():
                raise ValueError("sample_classes: classes are not enabled on this volume")
            return out[0], out[1]
        dp, dc = C.c_void_p(), C.c_void_p()
        check(lib.tsdf_device_alloc(p.nbytes, C.byref(dp)))
        try:
            check(lib.tsdf_device_alloc(out.nbytes, C.byref(dc)))
            check(lib.tsdf_device_upload(dp, p.ctypes.data, p.nbytes))
            self.sample_classes_device(len(p), dp.value, dc.value, dc.value + out[0].nbytes)
            self.synchronize()
            check(lib.tsdf_device_download(out.ctypes.data, dc, out.nbytes))
        finally:
            lib.tsdf_device_free(dp)
            if dc.value:
                lib.tsdf_device_free(dc)
        return out[0], out[1]

    def class_counts(self, n_classes, min_votes=1):
        """(n_classes,) uint64: the resident voxels whose class is k and whose votes are at least max(min_votes, 1)."""
        n = int(n_classes)
        if not 1 <= n <= 65535:
            raise ValueError("class_counts: n_classes %d is not in 1..65535" % n)
        out = np.empty(n, np.uint64)
        check(lib.tsdf_volume_class_counts(self._h, n, int(min_votes), out.ctypes.data))
        return out

    def extract_classed_surface(self):
        """extract_surface() and the class of every vertex (sample_classes): (vertices (3T, 3) float32, classes (3T,) uint16)."""
        V = self.extract_surface()
        return V, self.sample_classes(V)[0]

    # ---- field queries (include/tsdf_amd.h, "field queries"; not in the reference's class)
    def sample_field_device(self, n, points_ptr, distance_ptr=None, gradient_ptr=None, weight_ptr=None, unit_gradient=False,
                            stream=None):
        """n points (3 float32 each, device) -> distance (n float32), gradient (3 n), weight (n): device pointers, any of the three
        may be None; on `stream` (default: the volume's).  Points are in the frame of ray-cast and mesh vertices (the current
        offset)."""
        s = self.stream_ptr() if stream is None else stream
        ptr = lambda p: C.c_void_p(int(p)) if p else None
        check(lib.tsdf_volume_sample_field_device(self._h, int(n), ptr(points_ptr), ptr(distance_ptr), ptr(gradient_ptr),
                                                  ptr(weight_ptr), _capi.TSDF_FIELD_UNIT_GRADIENT if unit_gradient else 0,
                                                  C.c_void_p(int(s) if s else 0)))

    def sample_field(self, points, gradient=True, weight=True, unit_gradient=False):
        """(n, 3) float32 world points (mm) -> (distance (n,), gradient (n, 3) or None, weight (n,) or None), float32: the trilinear
        distance the ray cast samples (NaN outside the grid), its central-difference gradient (NaN triple within a voxel of a face;
        unit_gradient: normalised -- it points out of the surface) and the weight of the voxel the point lies in (0 outside)."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        # (one row more than asked for: the pointer of an empty array may be null, which the C ABI reads as "not asked for")
        d = np.empty(n + 1, np.float32)
        g = np.empty((n + 1, 3), np.float32) if gradient else None
        w = np.empty(n + 1, np.float32) if weight else None
        check(lib.tsdf_volume_sample_field(self._h, n, p.ctypes.data if n else None, d.ctypes.data,
                                           g.ctypes.data if gradient else None, w.ctypes.data if weight else None,
                                           _capi.TSDF_FIELD_UNIT_GRADIENT if unit_gradient else 0))
        return d[:n], g[:n] if gradient else None, w[:n] if weight else None

    def extract_surface_with_normals(self):
        """extract_surface() and the unit gradient of the field at every vertex (sample_field): (vertices (3T, 3), normals (3T, 3)),
        float32; a normal is the NaN triple within a voxel of the grid's faces."""
        V = self.extract_surface()
        return V, self.sample_field(V, weight=False, unit_gradient=True)[1]

    # ---- indexed mesh (include/tsdf_amd.h, "indexed mesh"; not in the reference's class)
    def extract_mesh(self, box=None, normals=False, colours=False, into=None):
        """The surface as an indexed mesh that stays on the device (tsdf_volume_extract_mesh): one vertex per lattice edge the surface
        crosses, one index per vertex of extract_surface()'s soup, vertices[indices] being that soup bit for bit.  box = (x0, y0, z0,
        x1, y1, z1) marches the cubes rooted in [x0, x1) x [y0, y1) x [z0, z1) only (ends clipped to the grid); normals / colours: the
        unit gradient (sample_field) / the colour (sample_colours) at every shared vertex.  `into`: a Mesh to reuse -- its device
        arrays are kept and only grow.  Returns the Mesh."""
        mesh = Mesh() if into is None else into
        b = None
        if box is not None:
            b = (C.c_uint32 * 6)(*[int(v) for v in box])
        flags = (_capi.TSDF_MESH_NORMALS if normals else 0) | (_capi.TSDF_MESH_COLOURS if colours else 0)
        table = marching_cubes_table()
        check(lib.tsdf_volume_extract_mesh(self._h, table.ctypes.data, b, flags, mesh._h))
        return mesh

    # ---- scene flow (include/tsdf_amd.h, "scene flow"; the device part of the reference's process_frames)
    def _scene_flow(self, call, depth, flow, width, height, camera, threshold, deformed, mesh, *tail):
        own = mesh is None
        if own:
            mesh = self.extract_mesh()
        info = _capi.SceneFlowInfo()
        pose, ipose, k, kinv = _camera_matrices(camera)
        try:
            check(call(self._h, mesh._h, depth, flow, width, height, _fp(pose), _fp(ipose), _fp(k), _fp(kinv), float(threshold),
                       _capi.TSDF_SCENE_FLOW_DEFORMED if deformed else 0, C.byref(info), *tail))
        finally:
            if own:
                mesh.close()
        return {"n_vertices": int(info.n_vertices), "n_correspondences": int(info.n_correspondences),
                "n_nodes_moved": int(info.n_nodes_moved)}

    def apply_scene_flow(self, depth, flow, camera, threshold=10.0, deformed=False, mesh=None):
        """One frame of the reference's scene fusion (tsdf_volume_apply_scene_flow): the mesh vertices the depth frame (height x width
        uint16, 0 = invalid) sees take the scene flow (height x width x 3 float32, world units) at their pixel, and it is added,
        weighted by how many triangle corners lie on each edge, to the translations of the deformation nodes of the two voxels that
        bracket each vertex -- deterministically.  threshold: how far (along z) the depth's point may lie from the vertex; deformed:
        the vertices go through the current deformation before they are projected (the later frames of a sequence).  mesh: a Mesh
        holding extract_mesh() of this volume's whole grid (None: extracted into a private one).  Blocking.  Returns
        {n_vertices, n_correspondences, n_nodes_moved}."""
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        if d.ndim != 2:
            raise ValueError("the depth image must be (height, width)")
        height, width = d.shape
        f = np.ascontiguousarray(flow, dtype=np.float32)
        if f.shape != (height, width, 3):
            raise ValueError("the scene flow must be (%d, %d, 3), got %r" % (height, width, f.shape))
        return self._scene_flow(lib.tsdf_volume_apply_scene_flow, d.ctypes.data, f.ctypes.data, width, height, camera, threshold,
                                deformed, mesh)

    def apply_scene_flow_device(self, depth_ptr, flow_ptr, width, height, camera, threshold=10.0, deformed=False, mesh=None, stream=None):
        """apply_scene_flow on device images (width * height uint16, 3 * width * height float32), enqueued on `stream` (None: the
        volume's); blocks for the counts."""
        s = self.stream_ptr() if stream is None else stream
        return self._scene_flow(lib.tsdf_volume_apply_scene_flow_device, C.c_void_p(int(depth_ptr)), C.c_void_p(int(flow_ptr)), width,
                                height, camera, threshold, deformed, mesh, C.c_void_p(int(s) if s else 0))

    # ---- distance field (include/tsdf_amd.h, "distance field"; not in the reference's class)
    def compute_esdf(self, max_distance=float("inf"), fill_unknown=False, into=None):
        """The Euclidean signed distance field (tsdf_volume_compute_esdf): per voxel the distance (mm) to the nearest site -- an observed
        voxel with an observed 6-neighbour of the other sign -- negative behind the surface, capped at max_distance (inf: no cap), NaN
        where unobserved (fill_unknown: the positive distance).  It stays on the device.  `into`: an ESDF to reuse -- its arrays are
        kept and only grow.  Returns the ESDF."""
        esdf = ESDF() if into is None else into
        check(lib.tsdf_volume_compute_esdf(self._h, float(max_distance), _capi.TSDF_ESDF_FILL_UNKNOWN if fill_unknown else 0, esdf._h))
        return esdf

    # ---- exploration (include/tsdf_amd.h, "exploration"; not in the reference's class)
    def find_frontiers(self, into=None):
        """The free voxels with an unobserved face neighbour inside the grid (tsdf_volume_find_frontiers), as an ascending list of voxel
        ids that stays on the device, with the whole-grid counts of unknown, free and occupied voxels.  `into`: an Explorer to reuse
        -- its arrays are kept and only grow.  Returns the Explorer."""
        explorer = Explorer() if into is None else into
        check(lib.tsdf_volume_find_frontiers(self._h, 0, explorer._h))
        return explorer

    def view_gain_device(self, explorer, n, origins_ptr, directions_ptr, t_max_ptr=None, unknown_ptr=None, free_ptr=None, stop_ptr=None,
                         keep=False, gain=True):
        """n rays (origins and directions 3 float32 each, t_max n float32 or None; device) -> unknown (n uint32), free (n uint32), stop
        (n uint8): device pointers, any may be None.  gain: wait for the volume's stream and return the number of distinct unknown
        voxels marked in `explorer` (None otherwise: asynchronous); keep: add to the marks of earlier calls."""
        ptr = lambda p: C.c_void_p(int(p)) if p else None
        g = C.c_uint64(0)
        check(lib.tsdf_volume_view_gain_device(self._h, explorer._h, int(n), ptr(origins_ptr), ptr(directions_ptr), ptr(t_max_ptr),
                                               _capi.TSDF_GAIN_KEEP_MASK if keep else 0, ptr(unknown_ptr), ptr(free_ptr), ptr(stop_ptr),
                                               C.byref(g) if gain else None))
        return int(g.value) if gain else None

    def view_gain(self, origins, directions, t_max=None, explorer=None, keep=False):
        """(n, 3) float32 origins and directions (world mm; the direction is used as given, t_max (n,) is in units of it) -> (gain,
        unknown (n,) uint32, free (n,) uint32, stop (n,) uint8): each ray is walked voxel by voxel until it leaves the grid, passes
        t_max (stop 1) or meets an occupied voxel (stop 2); unknown / free count the voxels it passed in either state, gain the
        distinct unknown voxels all rays passed (stop 0: the ray was skipped).  explorer: the Explorer whose mask takes the marks (None:
        a private one); keep: add to the marks of earlier calls with that explorer, so gain is that of the union."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        if len(d) != n:
            raise ValueError("view_gain: %d origins, %d directions" % (n, len(d)))
        m = None
        if t_max is not None:
            m = np.ascontiguousarray(t_max, dtype=np.float32).reshape(-1)
            if len(m) != n:
                raise ValueError("view_gain: %d rays, %d range limits" % (n, len(m)))
        own = explorer is None
        if own:
            explorer = Explorer()
        # (one element more than asked for: the pointer of an empty array may be null, which the C ABI reads as "not asked for")
        u, f, s = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint8)
        g = C.c_uint64(0)
        try:
            check(lib.tsdf_volume_view_gain(self._h, explorer._h, n, o.ctypes.data if n else None, d.ctypes.data if n else None,
                                            m.ctypes.data if (m is not None and n) else None, _capi.TSDF_GAIN_KEEP_MASK if keep else 0,
                                            u.ctypes.data, f.ctypes.data, s.ctypes.data, C.byref(g)))
        finally:
            if own:
                explorer.close()
        return int(g.value), u[:n], f[:n], s[:n]

    # ---- reachability (include/tsdf_amd.h, "reachability"; not in the reference's class)
    def reach(self, seeds, connectivity=26, esdf=None, clearance=0.0, max_cost=0, through_unknown=False, into=None):
        """The travel cost from `seeds` ((n, 3) float32 world points, mm) to every voxel through free voxels (through_unknown: unobserved
        ones too) whose ESDF value is at least `clearance` (esdf: an ESDF of this volume; None: no clearance), in steps of 10 / 14 / 17
        for face / edge / corner neighbours (connectivity 6: faces only) that never cut a corner; max_cost: values above it are
        REACH_UNREACHED (0: no cap).  It stays on the device; the call returns when the field is final.  `into`: a Reach to reuse -- its
        arrays are kept and only grow.  Returns the Reach."""
        p = np.ascontiguousarray(seeds, dtype=np.float32).reshape(-1, 3)
        reach = Reach() if into is None else into
        check(lib.tsdf_volume_compute_reach(self._h, len(p), p.ctypes.data if len(p) else None, int(connectivity),
                                            esdf._h if esdf is not None else None, float(clearance), int(max_cost),
                                            _capi.TSDF_REACH_THROUGH_UNKNOWN if through_unknown else 0, reach._h))
        return reach

    # ---- column maps (include/tsdf_amd.h, "column maps"; not in the reference's class)
    def column_map(self, axis=2, band=None, reversed=False, esdf=None, into=None):
        """Every column of voxels along `axis` (0, 1, 2 for x, y, z) reduced to one row of a 2-D map over the two other axes
        (tsdf_volume_project_columns): counts of unknown / free / occupied voxels, the highest and lowest occupied voxel (top, bottom),
        the free run above the top (headroom), the sub-voxel height of the surface there and, with `esdf` (an ESDF of this volume), the
        smallest distance to a surface anywhere in the column.  band: (lo, hi) voxel indices on the axis, None for all of it;
        reversed: "up" is towards smaller indices.  It stays on the device and the call does not wait.  `into`: a ColumnMap to reuse
        -- its arrays are kept and only grow.  Returns the ColumnMap."""
        lo, hi = (0, 0) if band is None else (int(band[0]), int(band[1]))
        if band is not None and hi == 0:
            raise ValueError("column_map: the band (%d, %d) is empty" % (lo, hi))   # (hi == 0 is the C ABI's "to the axis' end")
        cmap = ColumnMap() if into is None else into
        flags = _capi.TSDF_COLUMNS_REVERSED if reversed else 0
        check(lib.tsdf_volume_project_columns(self._h, int(axis), lo, hi, esdf._h if esdf is not None else None, flags, cmap._h))
        return cmap

    # ---- class objects (include/tsdf_amd.h, "class objects"; not in the reference's class)
    def find_objects(self, min_votes=1, classes=None, connectivity=26, min_size=1, into=None):
        """The connected pieces of each fused class (tsdf_volume_find_objects): the voxels whose word has at least max(min_votes, 1)
        votes and a class in `classes` (an iterable of admitted ids; None: every class) are listed, neighbours at `connectivity` (6 or
        26) of the SAME class are joined, and the table lists the objects of at least min_size voxels.  Everything stays on the
        device.  `into`: an Objects to reuse -- its arrays are kept and only grow.  Returns the Objects."""
        select, n_select = None, 0
        if classes is not None:
            ids = sorted({int(c) for c in classes})
            if ids and not 0 <= ids[0] <= ids[-1] <= 65534:
                raise ValueError("find_objects: class ids are 0..65534, got %d .. %d" % (ids[0], ids[-1]))
            select = np.zeros(ids[-1] + 1 if ids else 1, np.uint8)   # (an empty selection admits nothing: one zero byte)
            select[ids] = 1
            n_select = len(select)
        objects = Objects() if into is None else into
        check(lib.tsdf_volume_find_objects(self._h, int(min_votes), select.ctypes.data if select is not None else None, n_select,
                                           int(connectivity), int(min_size), 0, objects._h))
        return objects

    # ---- sparse snapshots (include/tsdf_amd.h, "sparse snapshot"; not in the reference's class)
    def _file_header(self):
        """The fields of the .tsdf header as the volume reports them now."""
        i = self.info()
        return {"physical_size": tuple(i.physical_size), "offset": tuple(i.offset), "truncation_distance": float(i.truncation_distance),
                "max_weight": float(i.max_weight), "global_translation": tuple(i.global_translation),
                "global_rotation": tuple(i.global_rotation)}

    def snapshot(self, into=None):
        """The live bricks of the volume -- those of 8^3 voxels that hold anything but what clear() leaves -- as compact device arrays
        (tsdf_volume_snapshot).  Nothing of the volume is written.  `into`: a Snapshot to reuse -- its arrays are kept and only grow.
        Returns the Snapshot."""
        snap = Snapshot() if into is None else into
        check(lib.tsdf_volume_snapshot(self._h, 0, snap._h))
        snap.header = self._file_header()
        return snap

    def restore(self, snapshot, shift=(0, 0, 0), keep_others=False):
        """Put a Snapshot of a grid of this size back (tsdf_volume_restore): every accessor then reports the state the snapshot was
        taken from, bit for bit.  The offset and the other header fields, the weight cap and the stream are not touched.
        With a `shift` in bricks or `keep_others` (tsdf_volume_restore_shifted; include/tsdf_amd.h, "rolling volume"): brick b of the
        volume takes brick b - shift of the snapshot, whose grid may be of another size; with `keep_others` the voxels of bricks that are
        not written keep their bits instead of being cleared."""
        shift = tuple(int(s) for s in shift)
        if shift == (0, 0, 0) and not keep_others:
            check(lib.tsdf_volume_restore(self._h, snapshot._h))
        else:
            check(lib.tsdf_volume_restore_shifted(self._h, snapshot._h, (C.c_int32 * 3)(*shift),
                                                  _capi.TSDF_RESTORE_KEEP_OTHERS if keep_others else 0))

    def shift(self, box_shift, work=None, leaving=None):
        """Move the volume's box by `box_shift` bricks of 8^3 voxels in the world; the content stays where it is in the world
        (tsdf_volume_shift).  `work`: a Snapshot to use for the round trip (its arrays are kept and only grow); `leaving`: a Snapshot to
        fill with the bricks that fall out, at the old offset -- one is made if None.  Returns `leaving`."""
        own = work is None
        work = Snapshot() if own else work
        leaving = Snapshot() if leaving is None else leaving
        try:
            check(lib.tsdf_volume_shift(self._h, (C.c_int32 * 3)(*(int(s) for s in box_shift)), work._h, leaving._h))
        finally:
            if own:
                work.close()
        leaving.header = None
        return leaving

    def save_sparse(self, path):
        """Write the volume's live bricks and header to a .tsdfs file.  Deformation nodes are not stored."""
        if self.info().deformation_materialised:
            raise ValueError("save_sparse: the volume has a materialised deformation-node array, which a .tsdfs file does not carry")
        snap = self.snapshot()
        try:
            snap.save(path)
        finally:
            snap.close()

    @classmethod
    def load_sparse(cls, path):
        """A new volume of the size, physical size and header of a .tsdfs file, holding its state."""
        snap = Snapshot.load(path)
        try:
            h = snap.header
            vol = cls(size=tuple(int(v) for v in snap.info.size), physical_size=h["physical_size"])
            f3 = lambda v: _fp(np.array(v, np.float32))
            check(lib.tsdf_volume_set_header(vol._h, f3(h["offset"]), h["truncation_distance"], h["max_weight"], f3(h["global_translation"]),
                                             f3(h["global_rotation"])))
            vol.restore(snap)
            vol.synchronize()
        finally:
            snap.close()
        return vol

    # ---- ray queries (include/tsdf_amd.h, "ray queries"; not in the reference's class)
    def cast_rays_device(self, n, origins_ptr, directions_ptr, t_max_ptr, points_ptr, t_ptr, normals_ptr, colours_ptr=None):
        """n rays (origins and directions 3 float32 each, t_max n float32 or None; device) -> points (3 n), t (n), normals (3 n): device
        pointers, any of the three outputs may be None, not all.  colours_ptr (3 n bytes, device): also the colour of the voxel each
        hit lies in, (0, 0, 0) on a miss; needs colour enabled and the points.  Asynchronous on the volume's stream."""
        ptr = lambda p: C.c_void_p(int(p)) if p else None
        if colours_ptr is None:
            check(lib.tsdf_volume_cast_rays_device(self._h, int(n), ptr(origins_ptr), ptr(directions_ptr), ptr(t_max_ptr),
                                                   ptr(points_ptr), ptr(t_ptr), ptr(normals_ptr)))
        else:
            check(lib.tsdf_volume_cast_rays_colour_device(self._h, int(n), ptr(origins_ptr), ptr(directions_ptr), ptr(t_max_ptr),
                                                          ptr(points_ptr), ptr(t_ptr), ptr(normals_ptr), ptr(colours_ptr)))

    def cast_rays(self, origins, directions, t_max=None, normals=False, normalise=False, colours=False):
        """(n, 3) float32 origins and directions (world mm, the frame of ray-cast and mesh vertices) -> (points (n, 3), t (n,)[,
        normals (n, 3)]), float32: where each ray first meets the surface, marched as the image cast marches a pixel's ray -- the
        direction is used as given, t is the hit's ray parameter in units of it -- NaN on a miss.  t_max (n,): a hit counts only if
        t <= t_max.  normals: the unit gradient of the field at the hit.  normalise: divide each direction by its fp32 length first,
        so t is in millimetres.  colours: the (n, 3) uint8 colour of the voxel each hit lies in ((0, 0, 0) on a miss) is appended to
        the tuple; needs colour enabled."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        if len(d) != n:
            raise ValueError("cast_rays: %d origins, %d directions" % (n, len(d)))
        if normalise:
            d = unit_directions(d)
        m = None
        if t_max is not None:
            m = np.ascontiguousarray(t_max, dtype=np.float32).reshape(-1)
            if len(m) != n:
                raise ValueError("cast_rays: %d rays, %d range limits" % (n, len(m)))
        # (one row more than asked for: the pointer of an empty array may be null, which the C ABI reads as "not asked for")
        p = np.empty((n + 1, 3), np.float32)
        t = np.empty(n + 1, np.float32)
        g = np.empty((n + 1, 3), np.float32) if normals else None
        args = (self._h, n, o.ctypes.data if n else None, d.ctypes.data if n else None, m.ctypes.data if (m is not None and n) else None,
                p.ctypes.data, t.ctypes.data, g.ctypes.data if normals else None)
        out = (p[:n], t[:n], g[:n]) if normals else (p[:n], t[:n])
        if not colours:
            check(lib.tsdf_volume_cast_rays(*args))
            return out
        c = np.zeros((n + 1, 3), np.uint8)
        check(lib.tsdf_volume_cast_rays_colour(*args, c.ctypes.data))
        return out + (c[:n],)

    def visible(self, a, b):
        """(n, 3) points a and b -> bool (n,): True where no surface lies between them -- the ray from a along the normalised b - a
        (fp32) with t_max = |b - a| hits nothing.  (a == b, or a non-finite point: a decreed miss, True.)"""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
        d = b - a
        _, t = self.cast_rays(a, d, t_max=direction_lengths(d), normalise=True)
        return np.isnan(t)

    # ---- field alignment (include/tsdf_amd.h, "field alignment"; not in the reference's class)
    def align_points(self, points, T0=None, iterations=10, gate=None, intensity=None, colour_gate=None, colour_weight=None):
        """The rigid pose that puts (n, 3) float32 points on this volume's surface: `iterations` Gauss-Newton steps on the squared
        field distance from T0 (4 x 4, points' frame -> the frame of mesh and ray-cast vertices; default identity), points further
        than `gate` (default: the truncation distance) from the surface left out.  -> (T 4 x 4 float64, residual, inliers) of the
        last step; inliers == 0 means the chain ended blind.  Raises ValueError on the refusals.  `intensity` ((n,) float32, NaN: none):
        with the colour term (FieldAligner.run); residual and inliers are then pairs (geometric, colour)."""
        if intensity is None:
            return FieldAligner().run(self, [(points, int(iterations))], T0, gate)
        return FieldAligner().run(self, [(points, int(iterations))], T0, gate, intensity=[intensity], colour_gate=colour_gate,
                                  colour_weight=colour_weight)

    # ---- colour alignment (include/tsdf_amd.h, "colour alignment"; not in the reference's class)
    def sample_intensity_device(self, n, points_ptr, intensity_ptr=None, gradient_ptr=None, stream=None):
        """n points (3 float32 each, device) -> intensity (n float32), gradient (3 n): device pointers, either may be None; on `stream`
        (default: the volume's).  Points are in the frame of sample_field."""
        s = self.stream_ptr() if stream is None else stream
        ptr = lambda p: C.c_void_p(int(p)) if p else None
        check(lib.tsdf_volume_sample_intensity_device(self._h, int(n), ptr(points_ptr), ptr(intensity_ptr), ptr(gradient_ptr),
                                                      C.c_void_p(int(s) if s else 0)))

    def sample_intensity(self, points, gradient=True):
        """(n, 3) float32 world points (mm) -> (intensity (n,), gradient (n, 3) or None), float32: the trilinear intensity
        Y = (77 r + 150 g + 29 b) / 256 of the fused colours in the cell sample_field's distance comes from and the exact derivative of
        that interpolant; NaN outside the grid and where one of the eight voxels was never observed in colour."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        c = np.empty(n + 1, np.float32)     # (one more than asked for: see sample_field)
        g = np.empty((n + 1, 3), np.float32) if gradient else None
        check(lib.tsdf_volume_sample_intensity(self._h, n, p.ctypes.data if n else None, c.ctypes.data, g.ctypes.data if gradient else None))
        return c[:n], g[:n] if gradient else None

    def register(self, src, T0=None, iterations=10, gate=None):
        """Volume-to-volume registration: align the mesh vertices of `src` (another TSDFVolume) to this volume's field from T0.
        -> (T src -> this volume, residual, inliers); the inverse of T is the dst_to_src that fuse(src, ...) takes."""
        return self.align_points(src.extract_surface(), T0, iterations, gate)

    # ---- volume fusion (include/tsdf_amd.h, "volume fusion"; not in the reference's class)
    def fuse(self, src, dst_to_src=None):
        """Resample the field of `src` (another TSDFVolume) onto this volume's grid through the rigid transform dst_to_src (4 x 4,
        column-major like a pose; default: identity) and blend it in, weights added.  -> the number of voxels updated.  Grids, voxel
        sizes, offsets and truncation distances may differ; src is not changed.  Raises ValueError on the refusals."""
        m = _mat(np.eye(4, dtype=np.float32) if dst_to_src is None else dst_to_src, 16)
        n = C.c_uint64()
        check(lib.tsdf_volume_fuse(self._h, src._h, _fp(m), C.byref(n)))
        return int(n.value)

    def last_fuse_bricks(self):
        """(listed, total) 64 x 4 x 32-voxel bricks of the last fuse() into this volume: what its cull kept, and all of them."""
        listed, total = C.c_uint32(), C.c_uint32()
        check(lib.tsdf_volume_last_fuse_bricks(self._h, C.byref(listed), C.byref(total)))
        return int(listed.value), int(total.value)

    # ---- ray integration (include/tsdf_amd.h, "ray integration"; not in the reference's class)
    def integrate_rays_device(self, n, origins_ptr, n_origins, points_ptr, band_only=False, min_range=0.0, max_range=float("inf"),
                              rgb=None):
        """n rays on the device: origins (3 float32 each; n_origins = 1 for one sensor position, or n) and end points (3 n float32).
        rgb: a device pointer to 3 n bytes, the colour of every point, fused into a colour-enabled volume with the distances.
        Asynchronous on the volume's stream; nothing is returned."""
        ptr = lambda p: C.c_void_p(int(p)) if p else None
        flags = _capi.TSDF_RAYS_BAND_ONLY if band_only else 0
        if rgb is None:
            check(lib.tsdf_integrate_rays_device(self._h, int(n), ptr(origins_ptr), int(n_origins), ptr(points_ptr), float(min_range),
                                                 float(max_range), flags, None))
        else:
            check(lib.tsdf_integrate_rays_colour_device(self._h, int(n), ptr(origins_ptr), int(n_origins), ptr(points_ptr), ptr(rgb),
                                                        float(min_range), float(max_range), flags, None))

    def integrate_rays(self, origins, points, band_only=False, min_range=0.0, max_range=float("inf"), rgb=None):
        """Fuse a LiDAR scan or a point cloud: (n, 3) float32 end points (world mm, the frame of ray-cast and mesh vertices) measured from
        `origins`, (3,) for one sensor position or (n, 3).  Every voxel the rays cross takes the mean of their observations as ONE
        observation (weight + 1), free space in front of the points included; band_only: only within the truncation distance of each
        point.  Rays shorter than min_range or longer than max_range are left out.  rgb: (n, 3) uint8, the colour of every point: the
        voxels within the truncation distance of a point also take the mean colour of their rays as one colour observation (the volume
        needs colour enabled).  -> the number of voxels updated.  Raises ValueError on the refusals."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        o = np.ascontiguousarray(origins, dtype=np.float32)
        if o.ndim == 1 and o.size == 3:
            o = o.reshape(1, 3)
        if o.ndim != 2 or o.shape[1] != 3:
            raise ValueError("integrate_rays: origins must be (3,) or (n, 3), got shape %s" % (o.shape,))
        n = len(p)
        updated = C.c_uint64()
        flags = _capi.TSDF_RAYS_BAND_ONLY if band_only else 0
        if rgb is None:
            check(lib.tsdf_integrate_rays(self._h, n, o.ctypes.data if n else None, len(o), p.ctypes.data if n else None, float(min_range),
                                          float(max_range), flags, C.byref(updated)))
            return int(updated.value)
        c = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1, 3)
        if len(c) != n:
            raise ValueError("integrate_rays: %d points, %d colours" % (n, len(c)))
        check(lib.tsdf_integrate_rays_colour(self._h, n, o.ctypes.data if n else None, len(o), p.ctypes.data if n else None,
                                             c.ctypes.data if n else None, float(min_range), float(max_range), flags, C.byref(updated)))
        return int(updated.value)

    def release_ray_scratch(self):
        """Free the scratch integrate_rays keeps between calls (8 bytes per voxel, 16 more once colours were fused); the next call
        allocates it again."""
        check(lib.tsdf_volume_release_ray_scratch(self._h))

    def ray_scratch_bytes(self):
        """Bytes of scratch integrate_rays holds on the device right now (0 before the first call and after release_ray_scratch)."""
        n = C.c_uint64()
        check(lib.tsdf_volume_ray_scratch_bytes(self._h, C.byref(n)))
        return int(n.value)

    def occupancy(self):
        """(occupied, total) bricks of the ray caster's empty-space summary."""
        o, t = C.c_uint64(), C.c_uint64()
        check(lib.tsdf_volume_occupancy(self._h, C.byref(o), C.byref(t)))
        return int(o.value), int(t.value)

    def occupancy_data(self, force_rebuild=False):
        """(fine, cell, reach) uint8 arrays of shape (nbz, nby, nbx): the ray caster's brick flags (diagnostics)."""
        X, Y, Z = self.size()
        shape = ((Z + 3) // 4, (Y + 3) // 4, (X + 3) // 4)
        out = [np.empty(shape, np.uint8) for _ in range(3)]
        check(lib.tsdf_volume_get_occupancy_data(self._h, 1 if force_rebuild else 0, *[a.ctypes.data for a in out]))
        return tuple(out)

    def set_timing(self, enabled):
        """HIP-event timing of integrate_kernel / process_ray_kernel launches on the volume's stream: True = every
        launch, an integer n > 1 = every n-th launch, False / 0 = off."""
        check(lib.tsdf_volume_set_timing(self._h, int(enabled)))

    def kernel_time(self, which):
        """(launches, average ms) of which = 'integrate' | 'raycast' | 'raycast_tail' since set_timing(True)."""
        n, ms = C.c_uint32(), C.c_float()
        check(lib.tsdf_volume_kernel_time(self._h, {"integrate": 0, "raycast": 1, "raycast_tail": 2}[which], C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def set_counting(self, enabled):
        check(lib.tsdf_volume_set_counting(self._h, 1 if enabled else 0))

    def last_updated_voxels(self):
        c = C.c_uint64()
        check(lib.tsdf_volume_last_updated_voxels(self._h, C.byref(c)))
        return int(c.value)

    def last_distance_stores(self):
        """Distances the last integrate with counting on wrote (<= last_updated_voxels(): unchanged bits are not stored)."""
        c = C.c_uint64()
        check(lib.tsdf_volume_last_distance_stores(self._h, C.byref(c)))
        return int(c.value)

    # ---- raycast (TSDFVolume.hpp:260): forwards to GPURaycaster like TSDFVolume.cu:1054-1058
    def raycast(self, width, height, camera):
        return GPURaycaster(width, height).raycast(self, camera)


class GPURaycaster:
    """src/include/GPURaycaster.hpp:19-41 (+ Raycaster.hpp:17-39)."""

    def __init__(self, width=640, height=480):
        self.m_width = int(width) & 0xFFFF    # uint16_t members in the reference
        self.m_height = int(height) & 0xFFFF

    def raycast(self, volume, camera):
        """-> (vertices, normals), each (width*height, 3) float32; misses are NaN rows."""
        pose, _, _, kinv = _camera_matrices(camera)
        n = self.m_width * self.m_height
        V = np.empty((n, 3), np.float32)
        N = np.empty((n, 3), np.float32)
        check(lib.tsdf_raycast(volume._h, self.m_width, self.m_height, _fp(pose), _fp(kinv), V.ctypes.data,
                               N.ctypes.data))
        return V, N

    def raycast_colour(self, volume, camera):
        """raycast() plus the colour of the voxel every vertex lies in: (vertices, normals, rgb (width*height, 3) uint8); misses
        and unobserved voxels are (0, 0, 0).  The volume must have colour enabled."""
        pose, _, _, kinv = _camera_matrices(camera)
        n = self.m_width * self.m_height
        V = np.empty((n, 3), np.float32)
        N = np.empty((n, 3), np.float32)
        rgb = np.empty((n, 3), np.uint8)
        check(lib.tsdf_raycast_colour(volume._h, self.m_width, self.m_height, _fp(pose), _fp(kinv), V.ctypes.data, N.ctypes.data,
                                      rgb.ctypes.data))
        return V, N, rgb

    def raycast_colour_device(self, volume, camera, vertices_ptr, normals_ptr, rgb_ptr):
        pose, _, _, kinv = _camera_matrices(camera)
        check(lib.tsdf_raycast_colour_device(volume._h, self.m_width, self.m_height, _fp(pose), _fp(kinv), C.c_void_p(int(vertices_ptr)),
                                             C.c_void_p(int(normals_ptr)) if normals_ptr else None, C.c_void_p(int(rgb_ptr))))

    def raycast_classes(self, volume, camera):
        """raycast() plus the class of the voxel every vertex lies in: (vertices, normals, classes (width*height,) uint16, votes
        (width*height,) uint16); misses and unclassified voxels are (CLASS_VOID, 0).  The volume must have classes enabled."""
        pose, _, _, kinv = _camera_matrices(camera)
        n = self.m_width * self.m_height
        V = np.empty((n, 3), np.float32)
        N = np.empty((n, 3), np.float32)
        classes = np.empty(n, np.uint16)
        votes = np.empty(n, np.uint16)
        check(lib.tsdf_raycast_classes(volume._h, self.m_width, self.m_height, _fp(pose), _fp(kinv), V.ctypes.data, N.ctypes.data,
                                       classes.ctypes.data, votes.ctypes.data))
        return V, N, classes, votes

    def raycast_classes_device(self, volume, camera, vertices_ptr, normals_ptr, classes_ptr, votes_ptr=None):
        pose, _, _, kinv = _camera_matrices(camera)
        ptr = lambda p: C.c_void_p(int(p)) if p else None
        check(lib.tsdf_raycast_classes_device(volume._h, self.m_width, self.m_height, _fp(pose), _fp(kinv), ptr(vertices_ptr),
                                              ptr(normals_ptr), ptr(classes_ptr), ptr(votes_ptr)))

    def raycast_gradient_normals(self, volume, camera):
        """raycast() with the unit gradient of the fused field at every vertex in place of the cross-product normals (NaN along
        every silhouette and beside every miss): -> (vertices, normals); the vertices are raycast()'s, a miss is a NaN row in both."""
        n = self.m_width * self.m_height
        V = np.empty((n, 3), np.float32)
        N = np.empty((n, 3), np.float32)
        if not n:
            return V, N
        dv = C.c_void_p()
        check(lib.tsdf_device_alloc(2 * V.nbytes, C.byref(dv)))
        try:
            self.raycast_gradient_normals_device(volume, camera, dv.value, dv.value + V.nbytes)
            volume.synchronize()
            check(lib.tsdf_device_download(V.ctypes.data, dv, V.nbytes))
            check(lib.tsdf_device_download(N.ctypes.data, C.c_void_p(dv.value + V.nbytes), N.nbytes))
        finally:
            volume.synchronize()
            lib.tsdf_device_free(dv)
        return V, N

    def raycast_gradient_normals_device(self, volume, camera, vertices_ptr, normals_ptr):
        """The same on device buffers (3 * width * height float32 each), asynchronous on the volume's stream."""
        pose, _, _, kinv = _camera_matrices(camera)
        check(lib.tsdf_raycast_gradient_normals_device(volume._h, self.m_width, self.m_height, _fp(pose), _fp(kinv),
                                                       C.c_void_p(int(vertices_ptr)), C.c_void_p(int(normals_ptr))))

    def get_vertices(self, volume, camera):
        pose, _, _, kinv = _camera_matrices(camera)
        V = np.empty((self.m_width * self.m_height, 3), np.float32)
        check(lib.tsdf_raycast(volume._h, self.m_width, self.m_height, _fp(pose), _fp(kinv), V.ctypes.data, None))
        return V

    def raycast_device(self, volume, camera, vertices_ptr, normals_ptr=None):
        pose, _, _, kinv = _camera_matrices(camera)
        check(lib.tsdf_raycast_device(volume._h, self.m_width, self.m_height, _fp(pose), _fp(kinv),
                                      C.c_void_p(int(vertices_ptr)),
                                      C.c_void_p(int(normals_ptr)) if normals_ptr else None))

    def render_to_depth_device(self, volume, camera, depth_ptr, vertices_ptr=None):
        """GPURaycaster::render_to_depth_image on device buffers: uint16 mm per pixel (0 = no hit), the vertex map too when asked for."""
        pose, ipose, _, kinv = _camera_matrices(camera)
        check(lib.tsdf_raycast_depth_device(volume._h, self.m_width, self.m_height, _fp(pose), _fp(ipose), _fp(kinv),
                                            C.c_void_p(int(depth_ptr)), C.c_void_p(int(vertices_ptr)) if vertices_ptr else None))

    def raycast_slab_device(self, volume, camera, hits_ptr):
        pose, _, _, kinv = _camera_matrices(camera)
        check(lib.tsdf_raycast_slab_device(volume._h, self.m_width, self.m_height, _fp(pose), _fp(kinv),
                                           C.c_void_p(int(hits_ptr))))

    def stats(self, volume, camera, per_ray_work=False):
        """Roofline diagnostics of one raycast: samples S, distinct voxels touched T, hits."""
        pose, _, _, kinv = _camera_matrices(camera)
        s, t, h = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib.tsdf_raycast_stats(volume._h, self.m_width, self.m_height, _fp(pose), _fp(kinv), C.byref(s),
                                     C.byref(t), C.byref(h)))
        e = C.c_uint64()
        per_ray = np.empty((self.m_width * self.m_height, 3), np.float32) if per_ray_work else None
        check(lib.tsdf_raycast_evaluated_samples(volume._h, self.m_width, self.m_height, _fp(pose), _fp(kinv), C.byref(e),
                                                 per_ray.ctypes.data if per_ray is not None else None))
        out = {"samples": int(s.value), "touched": int(t.value), "hits": int(h.value), "evaluated": int(e.value)}
        if per_ray is not None:
            out["per_ray"] = per_ray      # columns: samples evaluated, loop trips, reference sample count
        return out


def compute_normals_device(width, height, vertices_ptr, normals_ptr, stream=0):
    check(lib.tsdf_normals_device(width, height, C.c_void_p(int(vertices_ptr)), C.c_void_p(int(normals_ptr)),
                                  C.c_void_p(int(stream) if stream else 0)))


def vertices_to_depth_device(width, height, vertices_ptr, camera, depth_ptr, stream=0):
    """The per-pixel part of GPURaycaster::render_to_depth_image on device buffers (uint16 mm, 0 = no hit)."""
    ip = _mat(camera.inverse_pose(), 16)
    check(lib.tsdf_vertices_to_depth_device(width, height, C.c_void_p(int(vertices_ptr)), ip.ctypes.data,
                                            C.c_void_p(int(depth_ptr)), C.c_void_p(int(stream) if stream else 0)))


#: bytes of one slab hit record {uint32 k, float t} (struct tsdf_hit_record)
HIT_RECORD_BYTES = 8


def merge_hits_device(volume, hits_all_ptr, n_slabs, width, height, camera, vertices_ptr, stream=0):
    """Min-k select over the gathered slab records ((n_slabs, W*H) x {k, t}); the vertex of a pixel is formed from the winning
    record's refined ray parameter and the pixel's own ray (`camera`; `volume`: any slab of the grid, for its offset / size)."""
    pose, _, _, kinv = _camera_matrices(camera)
    check(lib.tsdf_merge_hits_device(volume._h, C.c_void_p(int(hits_all_ptr)), n_slabs, width, height, _fp(pose), _fp(kinv),
                                     C.c_void_p(int(vertices_ptr)), C.c_void_p(int(stream) if stream else 0)))


def merge_hits_normals_device(volume, hits_all_ptr, n_slabs, width, height, camera, vertices_ptr, normals_ptr, stream=0):
    """The same select and the normals of the merged map, one launch."""
    pose, _, _, kinv = _camera_matrices(camera)
    check(lib.tsdf_merge_hits_normals_device(volume._h, C.c_void_p(int(hits_all_ptr)), n_slabs, width, height, _fp(pose), _fp(kinv),
                                             C.c_void_p(int(vertices_ptr)), C.c_void_p(int(normals_ptr)),
                                             C.c_void_p(int(stream) if stream else 0)))


class BilateralFilter:
    """src/include/BilateralFilter.hpp:12-35.  filter() works in place on a host image, as the reference does."""

    def __init__(self, sigma_colour, sigma_space):
        self._h = C.c_void_p()
        check(lib.tsdf_bilateral_create(float(sigma_colour), float(sigma_space), C.byref(self._h)))

    def close(self):
        if lib is not None and getattr(self, "_h", None) is not None and self._h.value:   # (lib is None during interpreter shutdown)
            lib.tsdf_bilateral_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def filter(self, image, width, height):
        if not isinstance(image, np.ndarray) or image.dtype not in (np.uint8, np.uint16) or \
                not image.flags["C_CONTIGUOUS"]:
            raise ValueError("image must be a C-contiguous uint8 or uint16 numpy array")
        if image.size != width * height:
            raise ValueError("image has %d pixels, expected %d" % (image.size, width * height))
        fn = lib.tsdf_bilateral_filter_u8 if image.dtype == np.uint8 else lib.tsdf_bilateral_filter_u16
        check(fn(self._h, image.ctypes.data, width, height))

    def filter_device(self, in_ptr, out_ptr, width, height, bits=16, stream=0, tile_max_ptr=None):
        """tile_max_ptr (16 bit only): device array of ceil(width / 16) * ceil(height / 16) uint16 that receives the largest
        filtered value of every 16 x 16 pixel tile, for TSDFVolume.integrate_device(tile_max_ptr=...)."""
        if tile_max_ptr:
            if bits != 16:
                raise ValueError("tile maxima are produced by the 16-bit filter only")
            check(lib.tsdf_bilateral_filter_u16_device_tiles(self._h, C.c_void_p(int(in_ptr)), C.c_void_p(int(out_ptr)), width, height,
                                                             C.c_void_p(int(tile_max_ptr)), C.c_void_p(int(stream) if stream else 0)))
            return
        fn = lib.tsdf_bilateral_filter_u8_device if bits == 8 else lib.tsdf_bilateral_filter_u16_device
        check(fn(self._h, C.c_void_p(int(in_ptr)), C.c_void_p(int(out_ptr)), width, height,
                 C.c_void_p(int(stream) if stream else 0)))


def marching_cubes(distances, size, voxel_size, offset=(0.0, 0.0, 0.0)):
    """Host marching cubes of the class surface (MarkAndSweepMC.cpp, what extract_surface runs on a volume's distances):
    distances indexed x + y*X + z*X*Y -> (3*T, 3) float32 vertices, triangle t = rows 3t, 3t+1, 3t+2 (the reference then
    wires them (i, i+2, i+1))."""
    X, Y, Z = (int(v) for v in size)
    d = np.ascontiguousarray(distances, dtype=np.float32).reshape(-1)
    if d.size != X * Y * Z:
        raise ValueError("expected %d distances, got %d" % (X * Y * Z, d.size))
    vs = np.ascontiguousarray(voxel_size, dtype=np.float32)
    off = np.ascontiguousarray(offset, dtype=np.float32)
    n = _capi.host.tsdf_host_marching_cubes_c(d.ctypes.data, X, Y, Z, vs.ctypes.data, off.ctypes.data, None, 0)
    out = np.empty((n, 3), np.float32)
    _capi.host.tsdf_host_marching_cubes_c(d.ctypes.data, X, Y, Z, vs.ctypes.data, off.ctypes.data, out.ctypes.data, n)
    return out


def load_block_tsdf(file_name):
    """BlockTSDFLoader::load_from_file (text TSDF format) -> (complete, size xyz, physical size xyz, distances, weights)."""
    size = np.zeros(3, np.uint32)
    phys = np.zeros(3, np.float32)
    path = str(file_name).encode()
    ok = _capi.host.tsdf_host_block_loader_parse(path, size.ctypes.data, phys.ctypes.data, None, None, 0)
    n = int(size[0]) * int(size[1]) * int(size[2])
    d, w = np.zeros(n, np.float32), np.zeros(n, np.float32)
    if n:
        ok = _capi.host.tsdf_host_block_loader_parse(path, size.ctypes.data, phys.ctypes.data, d.ctypes.data, w.ctypes.data, n)
    return bool(ok), tuple(int(v) for v in size), tuple(float(v) for v in phys), d, w


def marching_cubes_table():
    """The generated 256 x 32 triangle table (edge numbers, -1 terminated rows)."""
    t = np.empty((256, 32), np.int8)
    _capi.host.tsdf_host_mc_table(t.ctypes.data)
    return t


class _Handle:
    """What the handles that live beside a volume share: creation, destruction, the info struct and the scratch size.  A subclass
    names its C functions by their stem (`_c`: tsdf_<_c>_create, _destroy, _get_info, _scratch_bytes) and its info struct (`_Info`)."""

    _c = None
    _Info = None

    def __init__(self):
        self._h = C.c_void_p()
        check(getattr(lib, "tsdf_%s_create" % self._c)(C.byref(self._h)))

    def close(self):
        if lib is not None and getattr(self, "_h", None) is not None and self._h.value:
            getattr(lib, "tsdf_%s_destroy" % self._c)(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _get_info(self):
        i = self._Info()
        check(getattr(lib, "tsdf_%s_get_info" % self._c)(self._h, C.byref(i)))
        return i

    @property
    def scratch_bytes(self):
        """Device bytes the handle holds besides the arrays it hands out (include/tsdf_amd.h, tsdf_*_scratch_bytes, says which)."""
        n = C.c_uint64(0)
        check(getattr(lib, "tsdf_%s_scratch_bytes" % self._c)(self._h, C.byref(n)))
        return int(n.value)


class Mesh(_Handle):
    """tsdf_mesh (include/tsdf_amd.h, "indexed mesh"): the device arrays of an indexed mesh and the scratch of its extraction, kept
    between extractions (TSDFVolume.extract_mesh(into=mesh)).  The array properties are blocking downloads."""

    _c, _Info = "mesh", _capi.MeshInfo

    def info(self):
        return self._get_info()

    @property
    def n_vertices(self):
        return int(self.info().n_vertices)

    @property
    def n_indices(self):
        return int(self.info().n_indices)

    @property
    def box(self):
        """The marched box as clipped to the grid: (x0, y0, z0, x1, y1, z1)."""
        return tuple(int(v) for v in self.info().box)

    def _download(self, which, shape, dtype):
        # (one element more than the mesh has: the pointer of an empty array may be null, which the C ABI reads as "not asked for")
        out = np.empty(int(np.prod(shape)) + 1, dtype)
        args = [None] * 4
        args[which] = out.ctypes.data
        check(lib.tsdf_mesh_download(self._h, *args))
        return out[:-1].reshape(shape)

    @property
    def vertices(self):
        """(n_vertices, 3) float32, sorted by lattice-edge key."""
        return self._download(0, (self.n_vertices, 3), np.float32)

    @property
    def indices(self):
        """(n_indices,) uint32, one per soup vertex in soup order."""
        return self._download(1, (self.n_indices,), np.uint32)

    @property
    def normals(self):
        """(n_vertices, 3) float32; ValueError unless the mesh was extracted with normals."""
        return self._download(2, (self.n_vertices, 3), np.float32)

    @property
    def colours(self):
        """(n_vertices, 3) uint8; ValueError unless the mesh was extracted with colours."""
        return self._download(3, (self.n_vertices, 3), np.uint8)

    def sample_classes(self, volume):
        """(n_vertices,) uint16: the class volume.sample_classes gives at every vertex, sampled device to device on the mesh's vertex
        buffer (CLASS_VOID where the voxel is unclassified).  The volume must have classes enabled."""
        n = self.n_vertices
        out = np.empty(n, np.uint16)
        if not n:
            if not volume.classes_enabled():
                raise ValueError("sample_classes: classes are not enabled on this volume")
            return out
        vertices = self.device_buffers()[0]
        dc = C.c_void_p()
        check(lib.tsdf_device_alloc(out.nbytes, C.byref(dc)))
        try:
            volume.sample_classes_device(n, vertices, dc.value)
            volume.synchronize()
            check(lib.tsdf_device_download(out.ctypes.data, dc, out.nbytes))
        finally:
            lib.tsdf_device_free(dc)
        return out

    def triangles(self):
        """(n_indices / 3, 3) uint32, wired as extract_surface wires its soup: triangle t = (I[3t], I[3t+2], I[3t+1])."""
        return np.ascontiguousarray(self.indices.reshape(-1, 3)[:, [0, 2, 1]])

    def device_buffers(self):
        """(vertices, indices, normals, colours) as raw device pointers (0: the mesh lacks the array, or is empty); valid until the
        next extraction into this mesh.  Waits for the extraction's kernels."""
        p = [C.c_void_p() for _ in range(4)]
        check(lib.tsdf_mesh_buffers(self._h, *[C.byref(q) for q in p]))
        return tuple(int(q.value or 0) for q in p)

    # ---- mesh components (include/tsdf_amd.h, "mesh components")
    def label_components(self, stream=0):
        """Label the connected pieces of the mesh on the device (tsdf_mesh_label_components): returns {n_components, n_triangles,
        largest_triangles, largest_label}.  The labels and sizes stay in the handle until the next extraction or filter into it."""
        i = _capi.ComponentsInfo()
        check(lib.tsdf_mesh_label_components(self._h, C.byref(i), C.c_void_p(int(stream) if stream else 0)))
        return _components_info(i)

    def _component_download(self, which):
        out = np.empty(self.n_vertices + 1, np.uint32)   # (see _download)
        args = [None, None]
        args[which] = out.ctypes.data
        check(lib.tsdf_mesh_component_download(self._h, *args))
        return out[:-1]

    @property
    def labels(self):
        """(n_vertices,) uint32: the smallest vertex index of each vertex's component; ValueError unless the mesh was labelled."""
        return self._component_download(0)

    @property
    def component_triangles(self):
        """(n_vertices,) uint32: the triangles of each vertex's component; ValueError unless the mesh was labelled."""
        return self._component_download(1)

    def component_buffers(self):
        """(labels, component_triangles) as raw device pointers (0 for an empty mesh); valid until the next extraction or filter into
        this mesh.  ValueError unless the mesh was labelled."""
        p = [C.c_void_p() for _ in range(2)]
        check(lib.tsdf_mesh_component_buffers(self._h, *[C.byref(q) for q in p]))
        return tuple(int(q.value or 0) for q in p)

    def filter_components(self, min_triangles=0, keep_largest=False, into=None, stream=0):
        """The mesh without its small pieces, on the device (tsdf_mesh_filter_components): the components with at least
        `min_triangles` triangles -- with `keep_largest`, the largest one only, if it has that many -- as a Mesh of the kept vertices and
        triples in their order, indices remapped, normals and colours carried along.  Labels this mesh first if need be.  `into`: a
        Mesh to reuse (not this one)."""
        dst = Mesh() if into is None else into
        flags = _capi.TSDF_MESH_KEEP_LARGEST if keep_largest else 0
        check(lib.tsdf_mesh_filter_components(self._h, int(min_triangles), flags, dst._h, C.c_void_p(int(stream) if stream else 0)))
        return dst

    # ---- mesh simplification (include/tsdf_amd.h, "mesh simplification")
    def simplify(self, cell_size, into=None, stream=0):
        """A level of detail of the mesh, on the device (tsdf_mesh_simplify): the vertices of each cubic cell of side `cell_size` (mm)
        become one vertex -- the mean of their positions, normals and colours -- and the triples left with fewer than three corners are
        dropped.  Returns a Mesh (`into`: one to reuse, not this one); vertices no triple names any more stay until
        filter_components(1) removes them.  A tiny cell welds exactly coincident vertices and changes nothing else."""
        dst = Mesh() if into is None else into
        check(lib.tsdf_mesh_simplify(self._h, float(cell_size), 0, dst._h, C.c_void_p(int(stream) if stream else 0)))
        return dst

    # ---- mesh smoothing (include/tsdf_amd.h, "mesh smoothing")
    def smooth(self, iterations=10, lam=0.5, mu=-0.53, pin_boundary=False, normals=False, into=None, stream=0):
        """The mesh smoothed on the device (tsdf_mesh_smooth): `iterations` times a pass with factor `lam`, then one with `mu` (Taubin's
        pair: the second undoes the shrinking of the first; mu=0 is the plain Laplacian).  `pin_boundary` keeps the bytes of the open
        border, so meshes extracted in neighbouring boxes still fit; `normals` computes area-weighted normals from the smoothed faces
        (otherwise the source's normals are carried along).  Indices and colours are carried along.  Returns a Mesh (`into`: one to
        reuse, not this one)."""
        dst = Mesh() if into is None else into
        check(lib.tsdf_mesh_smooth(self._h, int(iterations), float(lam), float(mu), _smooth_flags(pin_boundary, normals), dst._h,
                                   C.c_void_p(int(stream) if stream else 0)))
        return dst

    def compute_normals(self, stream=0):
        """Area-weighted vertex normals from the mesh's own faces (tsdf_mesh_compute_normals): they replace the normals the mesh has, or
        give it some -- after a simplification or for arrays that came without.  Returns the mesh."""
        check(lib.tsdf_mesh_compute_normals(self._h, C.c_void_p(int(stream) if stream else 0)))
        return self

    # ---- mesh rendering (include/tsdf_amd.h, "mesh rendering")
    def render(self, inv_pose, k, size, near=1.0, far=65535.0, cull_back=False, targets=("depth",), into=None):
        """The mesh seen from a pinhole camera (tsdf_mesh_render): `inv_pose` (16) and `k` (9) column-major, `size` = (width, height),
        only triangles with all corners in [near, far] are drawn.  `targets`: any of RENDER_TARGETS.  Returns a dict of host arrays in
        pixel order -- triangle (n,) uint32, z (n,) float32, depth (n,) uint16, vertices / normals (n, 3) float32, rgb (n, 3) uint8 --
        and "info".  `into`: a Renderer to reuse.  Blocking."""
        renderer = Renderer() if into is None else into
        try:
            return renderer.render(self, inv_pose, k, size, near, far, cull_back, targets)
        finally:
            if into is None:
                renderer.close()


#: the maps a render can fill: name -> (dtype, values per pixel)
RENDER_TARGETS = {"triangle": (np.uint32, 1), "z": (np.float32, 1), "depth": (np.uint16, 1), "vertices": (np.float32, 3),
                  "normals": (np.float32, 3), "rgb": (np.uint8, 3)}
RENDER_CULL_BACK = _capi.TSDF_RENDER_CULL_BACK
RENDER_MISS = _capi.TSDF_RENDER_MISS


def _render_info(i):
    return {"n_triangles": int(i.n_triangles), "n_live": int(i.n_live), "n_dropped": int(i.n_dropped), "n_large": int(i.n_large),
            "n_pixels_hit": int(i.n_pixels_hit)}


def _render_targets(pointers):
    unknown = set(pointers) - set(RENDER_TARGETS)
    if unknown:
        raise ValueError("unknown render targets %s (known: %s)" % (sorted(unknown), ", ".join(RENDER_TARGETS)))
    return _capi.RenderTargets(**{name: C.c_void_p(int(p) if p else 0) for name, p in pointers.items()})


class Renderer(_Handle):
    """tsdf_render (include/tsdf_amd.h, "mesh rendering"): the scratch of the mesh renderer -- 8 bytes per pixel, 16 per shared vertex, 4
    per triangle -- kept between renders, so a warm one allocates nothing."""

    _c, _Info = "render", _capi.RenderInfo

    def info(self):
        """The counts of the last render (waits for it): n_triangles, n_live, n_dropped, n_large, n_pixels_hit.  ValueError if the
        render met an index that is not below n_vertices."""
        return _render_info(self._get_info())

    def set_large_box(self, pixels=_capi.TSDF_RENDER_LARGE_BOX):
        """Scheduling only (tsdf_render_set_large_box): a live triangle whose clipped box holds more pixels than this is rasterised by a
        whole wave; None: never."""
        check(lib.tsdf_render_set_large_box(self._h, 0xFFFFFFFF if pixels is None else int(pixels)))

    def _view(self, inv_pose, k, size, cull_back):
        width, height = (int(v) for v in size)
        return width, height, _mat(inv_pose, 16), _mat(k, 9), (_capi.TSDF_RENDER_CULL_BACK if cull_back else 0)

    def render_device(self, mesh, inv_pose, k, size, near, far, cull_back=False, targets=None, info=False, stream=0):
        """tsdf_mesh_render_device: the Mesh `mesh` into device pointers (`targets`: name -> pointer), enqueued on `stream` behind the
        mesh's pending work.  With `info` the call waits and returns the counts, otherwise None."""
        width, height, ip, km, flags = self._view(inv_pose, k, size, cull_back)
        t, i = _render_targets(targets or {}), _capi.RenderInfo()
        check(lib.tsdf_mesh_render_device(self._h, mesh._h, width, height, _fp(ip), _fp(km), float(near), float(far), flags, C.byref(t),
                                          C.byref(i) if info else None, C.c_void_p(int(stream) if stream else 0)))
        return _render_info(i) if info else None

    def render_arrays_device(self, n_vertices, n_indices, vertices_ptr, indices_ptr, inv_pose, k, size, near, far, cull_back=False, targets=None,
                             normals_ptr=0, colours_ptr=0, info=False, stream=0):
        """tsdf_render_mesh_device: plain device arrays (float32 x 3 vertices, uint32 indices, float32 x 3 normals or 0, uint8 x 3
        colours or 0) into device pointers."""
        width, height, ip, km, flags = self._view(inv_pose, k, size, cull_back)
        vp = lambda p: C.c_void_p(int(p) if p else 0)
        t, i = _render_targets(targets or {}), _capi.RenderInfo()
        check(lib.tsdf_render_mesh_device(self._h, int(n_vertices), int(n_indices), vp(vertices_ptr), vp(indices_ptr), vp(normals_ptr), vp(colours_ptr),
                                          width, height, _fp(ip), _fp(km), float(near), float(far), flags, C.byref(t), C.byref(i) if info else None,
                                          vp(stream)))
        return _render_info(i) if info else None

    def render(self, mesh, inv_pose, k, size, near=1.0, far=65535.0, cull_back=False, targets=("depth",)):
        """tsdf_mesh_render: the Mesh `mesh` into host arrays, blocking; see Mesh.render."""
        width, height, ip, km, flags = self._view(inv_pose, k, size, cull_back)
        n = max(width * height, 0)
        out = {name: np.empty((n, RENDER_TARGETS[name][1]) if RENDER_TARGETS[name][1] > 1 else (n,), RENDER_TARGETS[name][0])
               for name in targets if name in RENDER_TARGETS}
        t, i = _render_targets({name: (out[name].ctypes.data if name in out else 1) for name in targets}), _capi.RenderInfo()
        check(lib.tsdf_mesh_render(self._h, mesh._h, width, height, _fp(ip), _fp(km), float(near), float(far), flags, C.byref(t), C.byref(i)))
        out["info"] = _render_info(i)
        return out


def render_mesh_device(renderer, n_vertices, n_indices, vertices_ptr, indices_ptr, inv_pose, k, size, near, far, cull_back=False, targets=None,
                       normals_ptr=0, colours_ptr=0, info=False, stream=0):
    """tsdf_render_mesh_device on device pointers with the Renderer `renderer` (Renderer.render_arrays_device)."""
    return renderer.render_arrays_device(n_vertices, n_indices, vertices_ptr, indices_ptr, inv_pose, k, size, near, far, cull_back, targets, normals_ptr,
                                         colours_ptr, info, stream)


def render_mesh(vertices, indices, inv_pose, k, size, near=1.0, far=65535.0, cull_back=False, targets=("depth",), normals=None, colours=None,
                into=None):
    """Host arrays rendered on the device (upload, tsdf_render_mesh_device, download): (n, 3) float32 vertices, 3 m indices, optionally
    (n, 3) float32 normals and (n, 3) uint8 colours -> the dict Mesh.render returns.  `into`: a Renderer to reuse."""
    V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    I = np.ascontiguousarray(np.asarray(indices).reshape(-1), np.uint32)
    N = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    RGB = None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(-1, 3)
    for a, what in ((N, "normals"), (RGB, "colours")):
        if a is not None and len(a) != len(V):
            raise ValueError("%d %s for %d vertices" % (len(a), what, len(V)))
    _render_targets({name: 0 for name in targets})
    width, height = (int(v) for v in size)
    n = max(width * height, 0)
    out = {name: np.empty((n, RENDER_TARGETS[name][1]) if RENDER_TARGETS[name][1] > 1 else (n,), RENDER_TARGETS[name][0]) for name in targets}
    renderer = Renderer() if into is None else into
    try:
        with _DeviceArray(V) as dv, _DeviceArray(I) as di, _DeviceArray(nbytes=4) as none:
            with _DeviceArray(N if N is not None and len(V) else None, 0) as dn, _DeviceArray(RGB if RGB is not None and len(V) else None, 0) as dc:
                given = lambda a, d: 0 if a is None else (d.ptr.value or none.ptr.value)      # (see simplify_mesh)
                buffers = {name: _DeviceArray(nbytes=max(a.nbytes, 4)) for name, a in out.items()}
                try:
                    for b in buffers.values():
                        b.__enter__()
                    out["info"] = renderer.render_arrays_device(len(V), I.size, dv.ptr.value, di.ptr.value, inv_pose, k, (width, height), near, far, cull_back,
                                                                {name: b.ptr.value for name, b in buffers.items()}, given(N, dn), given(RGB, dc), info=True)
                    for name, b in buffers.items():
                        if out[name].nbytes:
                            check(lib.tsdf_device_download(out[name].ctypes.data, b.ptr, out[name].nbytes))
                finally:
                    for b in buffers.values():
                        b.__exit__()
        return out
    finally:
        if into is None:
            renderer.close()


class ESDF(_Handle):
    """tsdf_esdf (include/tsdf_amd.h, "distance field"): the device array of a distance field, its scratch and the geometry it was
    computed for, kept between computations (TSDFVolume.compute_esdf(into=esdf)).  Sampling needs no volume."""

    _c, _Info = "esdf", _capi.EsdfInfo

    @property
    def info(self):
        """tsdf_esdf_info: size, flags, voxel_size, offset, max_distance, n_sites.  Waits for the computation."""
        return self._get_info()

    @property
    def n_sites(self):
        return int(self.info.n_sites)

    @property
    def distances(self):
        """(X * Y * Z,) float32 in index order x + y X + z X Y, shaped like TSDFVolume.get_distance_data(); a blocking download."""
        sx, sy, sz = (int(v) for v in self.info.size)
        out = np.empty(sx * sy * sz + 1, np.float32)   # (one element more: the pointer of an empty array may be null)
        check(lib.tsdf_esdf_download(self._h, out.ctypes.data))
        return out[:-1]

    def device_buffer(self):
        """The raw device pointer of the array (0 before the first computation); valid until the next computation into this handle."""
        p = C.c_void_p()
        check(lib.tsdf_esdf_buffer(self._h, C.byref(p)))
        return int(p.value or 0)

    def sample_device(self, n, points_ptr, distance_ptr=None, gradient_ptr=None, unit=False, stream=None):
        """n points (3 float32 each, device) -> distance (n float32), gradient (3 n): device pointers, either may be None; on `stream`
        (default: the null stream), ordered behind the computation."""
        ptr = lambda p: C.c_void_p(int(p)) if p else None
        check(lib.tsdf_esdf_sample_device(self._h, int(n), ptr(points_ptr), ptr(distance_ptr), ptr(gradient_ptr),
                                          _capi.TSDF_FIELD_UNIT_GRADIENT if unit else 0, C.c_void_p(int(stream) if stream else 0)))

    def sample(self, points, gradient=False, unit=False):
        """(n, 3) float32 world points (mm, the frame of ray-cast and mesh vertices when computed) -> the trilinear distance (n,), or
        (distance, gradient (n, 3)) with gradient=True (unit: normalised).  NaN outside the grid and next to unobserved voxels."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        d = np.empty(n + 1, np.float32)
        g = np.empty((n + 1, 3), np.float32) if gradient else None
        check(lib.tsdf_esdf_sample(self._h, n, p.ctypes.data if n else None, d.ctypes.data, g.ctypes.data if gradient else None,
                                   _capi.TSDF_FIELD_UNIT_GRADIENT if unit else 0))
        return (d[:n], g[:n]) if gradient else d[:n]


#: one row of Explorer.clusters: struct tsdf_frontier_cluster (56 bytes)
CLUSTER_DTYPE = np.dtype([("label", np.uint32), ("size", np.uint32), ("lo", np.uint32, 3), ("hi", np.uint32, 3), ("sum", np.uint64, 3)])


def _voxel_coordinates(ids, size):
    """(n,) voxel ids (z * Y + y) * X + x of a grid of `size` -> (n, 3) uint32 (x, y, z)."""
    sx, sy, _ = (int(v) for v in size)
    ids = ids.astype(np.uint64)
    return np.stack([ids % sx, (ids // sx) % sy, ids // (sx * sy)], axis=1).astype(np.uint32)


def _row_centroids(rows, info):
    """Table rows with `sum` and `size`, and the info with their geometry -> (n, 3) float64 world centroids (mm)."""
    vs, off = np.array(info.voxel_size, np.float64), np.array(info.offset, np.float64)
    return (rows["sum"].astype(np.float64) / np.maximum(rows["size"], 1)[:, None] + 0.5) * vs + off


class Explorer(_Handle):
    """tsdf_explorer (include/tsdf_amd.h, "exploration"): the frontier voxels of a volume (TSDFVolume.find_frontiers(into=explorer)),
    their clusters (cluster()) and the mask of unknown voxels that view-gain rays have passed (TSDFVolume.view_gain(explorer=...)), on
    the device, with the geometry they belong to.  Nothing here needs the volume."""

    _c, _Info = "explorer", _capi.ExplorerInfo

    @property
    def info(self):
        """tsdf_explorer_info: size, connectivity, voxel_size, offset, n_unknown, n_free, n_occupied, n_frontiers, n_clusters,
        n_listed_clusters."""
        return self._get_info()

    @property
    def voxels(self):
        """(n_frontiers,) uint32: the ids (z * Y + y) * X + x of the frontier voxels, ascending; a blocking download."""
        n = int(self.info.n_frontiers)
        out = np.empty(n + 1, np.uint32)   # (one element more: the pointer of an empty array may be null)
        check(lib.tsdf_explorer_frontier_download(self._h, out.ctypes.data))
        return out[:n]

    @property
    def coordinates(self):
        """(n_frontiers, 3) uint32: (x, y, z) of the frontier voxels."""
        return _voxel_coordinates(self.voxels, self.info.size)

    @property
    def points(self):
        """(n_frontiers, 3) float32: the world centres (mm) of the frontier voxels, offset + (coordinate + 0.5) * voxel_size."""
        i = self.info
        vs, off = np.array(i.voxel_size, np.float32), np.array(i.offset, np.float32)
        return ((self.coordinates.astype(np.float32) + np.float32(0.5)) * vs + off).astype(np.float32)

    def cluster(self, connectivity=26, min_size=1, stream=0):
        """Label the connected sets of frontier voxels (tsdf_explorer_cluster_frontiers): connectivity 6 (faces) or 26 (faces, edges,
        corners); the table lists the clusters of at least min_size voxels.  Returns the explorer."""
        check(lib.tsdf_explorer_cluster_frontiers(self._h, int(connectivity), int(min_size), C.c_void_p(int(stream) if stream else 0)))
        return self

    def _download_clusters(self):
        i = self.info
        labels = np.empty(int(i.n_frontiers) + 1, np.uint32)
        rows = np.zeros(int(i.n_listed_clusters) + 1, CLUSTER_DTYPE)
        check(lib.tsdf_explorer_cluster_download(self._h, labels.ctypes.data, rows.ctypes.data))
        return labels[:-1], rows[:-1]

    @property
    def labels(self):
        """(n_frontiers,) uint32: per listed voxel the smallest list index of its cluster."""
        return self._download_clusters()[0]

    @property
    def clusters(self):
        """(n_listed_clusters,) CLUSTER_DTYPE rows in ascending label: label, size, lo / hi (the inclusive voxel box), sum (the integer
        coordinate sums)."""
        return self._download_clusters()[1]

    @property
    def centroids(self):
        """(n_listed_clusters, 3) float64: the world centroid (mm) of every listed cluster, offset + (sum / size + 0.5) * voxel_size."""
        return _row_centroids(self.clusters, self.info)

    def device_buffers(self):
        """Raw device pointers {voxels, masks, bases, labels, clusters} (0 where empty or not clustered); valid until the next call
        that fills them."""
        v, m, b = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib.tsdf_explorer_frontier_buffers(self._h, C.byref(v), C.byref(m), C.byref(b)))
        out = {"voxels": int(v.value or 0), "masks": int(m.value or 0), "bases": int(b.value or 0), "labels": 0, "clusters": 0}
        if self.info.connectivity:
            l, r = C.c_void_p(), C.c_void_p()
            check(lib.tsdf_explorer_cluster_buffers(self._h, C.byref(l), C.byref(r)))
            out["labels"], out["clusters"] = int(l.value or 0), int(r.value or 0)
        return out


#: one row of FrameDiff.blobs: struct tsdf_diff_blob (56 bytes)
DIFF_BLOB_DTYPE = np.dtype([("label", np.uint32), ("size", np.uint32), ("lo", np.uint32, 2), ("hi", np.uint32, 2), ("min_depth", np.uint32),
                            ("max_depth", np.uint32), ("sum_x", np.uint64), ("sum_y", np.uint64), ("sum_depth", np.uint64)])
DIFF_NO_FRAME, DIFF_NO_MODEL, DIFF_SAME, DIFF_FARTHER, DIFF_NEARER = 0, 1, 2, 3, 4
DIFF_NO_BLOB = 0xFFFFFFFF
#: starting values of dynamic rejection, unvalidated on real data
DIFF_DEFAULTS = dict(tolerance=50, quadratic=0, connectivity=8, depth_step=50, min_pixels=64, dilate=4)


class FrameDiff(_Handle):
    """tsdf_frame_diff (include/tsdf_amd.h, "frame differences"): a depth frame compared with the model's depth image (compare), the
    pixels in front of the model clustered into blobs (cluster), and the dilated mask of the blobs kept (mask), on the device."""

    _c, _Info = "frame_diff", _capi.FrameDiffInfo
    #: the state image of the last compare(states=True), else None
    states = None

    @property
    def info(self):
        """tsdf_frame_diff_info: width, height, tolerance, quadratic, connectivity, depth_step, min_pixels, counts[5], n_blobs,
        n_kept_blobs."""
        return self._get_info()

    def compare_device(self, frame_ptr, model_ptr, width, height, tolerance=50, quadratic=0, states_ptr=0, stream=0):
        """tsdf_frame_diff_compare_device on device pointers (uint16 mm images; states: uint8 per pixel, or 0).  Returns self."""
        vp = lambda p: C.c_void_p(int(p) if p else 0)
        params = _capi.DiffParams(int(tolerance), int(quadratic))
        check(lib.tsdf_frame_diff_compare_device(self._h, vp(frame_ptr), vp(model_ptr), int(width), int(height), C.byref(params), vp(states_ptr),
                                                 vp(stream)))
        return self

    def compare(self, frame, model, tolerance=50, quadratic=0, states=False):
        """Host images (H, W) uint16; with states=True the (H, W) uint8 state image is kept in self.states.  Returns self."""
        f = np.ascontiguousarray(frame, np.uint16)
        m = np.ascontiguousarray(model, np.uint16)
        if f.ndim != 2 or f.shape != m.shape:
            raise ValueError("compare: frame and model are (height, width) images of one shape, got %r and %r" % (f.shape, m.shape))
        h, w = f.shape
        self.states = None
        if not states:
            with _DeviceArray(f) as df, _DeviceArray(m) as dm:
                return self.compare_device(df.ptr.value, dm.ptr.value, w, h, tolerance, quadratic)
        out = np.empty((h, w), np.uint8)
        with _DeviceArray(f) as df, _DeviceArray(m) as dm, _DeviceArray(nbytes=max(out.nbytes, 1)) as ds:
            self.compare_device(df.ptr.value, dm.ptr.value, w, h, tolerance, quadratic, ds.ptr.value)
            if out.nbytes:
                check(lib.tsdf_device_download(out.ctypes.data, ds.ptr, out.nbytes))
        self.states = out
        return self

    @property
    def counts(self):
        """(5,) uint64: the pixels in each state, indexed by DIFF_NO_FRAME .. DIFF_NEARER."""
        return np.array(list(self.info.counts), np.uint64)

    def cluster(self, connectivity=8, depth_step=50, min_pixels=64, stream=0):
        """tsdf_frame_diff_cluster: connectivity 4 or 8; listed neighbours whose frame depths differ by at most depth_step are joined; the
        table lists the blobs of at least max(min_pixels, 1) pixels.  Returns self."""
        check(lib.tsdf_frame_diff_cluster(self._h, int(connectivity), int(depth_step), int(min_pixels), C.c_void_p(int(stream) if stream else 0)))
        return self

    def _download(self):
        i = self.info
        n = int(i.counts[DIFF_NEARER])
        pixels, labels = np.empty(n + 1, np.uint32), np.empty(n + 1, np.uint32)
        rows = np.zeros(int(i.n_kept_blobs) + 1, DIFF_BLOB_DTYPE)
        check(lib.tsdf_frame_diff_download(self._h, pixels.ctypes.data, labels.ctypes.data, rows.ctypes.data))
        return pixels[:n], labels[:n], rows[:-1]

    @property
    def pixels(self):
        """(n_nearer,) uint32: the ids y * width + x of the listed pixels, ascending."""
        return self._download()[0]

    @property
    def labels(self):
        """(n_nearer,) uint32: per listed pixel the smallest list index of its blob."""
        return self._download()[1]

    @property
    def blobs(self):
        """(n_kept_blobs,) DIFF_BLOB_DTYPE rows in ascending label."""
        return self._download()[2]

    def device_buffers(self):
        """Raw device pointers {pixels, masks, bases, labels, blobs} (0 where empty); valid until the next call that fills them."""
        p = [C.c_void_p() for _ in range(5)]
        check(lib.tsdf_frame_diff_buffers(self._h, *[C.byref(x) for x in p]))
        return dict(zip(("pixels", "masks", "bases", "labels", "blobs"), (int(x.value or 0) for x in p)))

    def mask_device(self, dilate=4, mask_ptr=0, blob_index_ptr=0, frame_in_ptr=0, frame_out_ptr=0, stream=0):
        """tsdf_frame_diff_mask_device on device pointers (any may be 0; frame_in and frame_out together).  Asynchronous on `stream`."""
        vp = lambda p: C.c_void_p(int(p) if p else 0)
        check(lib.tsdf_frame_diff_mask_device(self._h, int(dilate), vp(mask_ptr), vp(blob_index_ptr), vp(frame_in_ptr), vp(frame_out_ptr), vp(stream)))
        return self

    def mask(self, dilate=4, frame=None, blob_index=False):
        """The (H, W) uint8 mask of the kept blobs dilated by `dilate` pixels; with `frame` ((H, W) uint16) also the frame with the masked
        pixels set to 0; with blob_index=True also the (H, W) uint32 instance image.  Returns the mask, or a tuple in that order."""
        i = self.info
        h, w = int(i.height), int(i.width)
        m = np.empty((h, w), np.uint8)
        b = np.empty((h, w), np.uint32) if blob_index else None
        f = None
        if frame is not None:
            f = np.ascontiguousarray(frame, np.uint16)
            if f.shape != (h, w):
                raise ValueError("mask: the frame is (%d, %d), the comparison was of (%d, %d)" % (f.shape + (h, w)))
            f = f.copy()
        with _DeviceArray(nbytes=max(m.nbytes, 1)) as dm, _DeviceArray(nbytes=4 * max(m.size, 1) if blob_index else 0) as db, \
                _DeviceArray(f if f is not None else None, nbytes=0) as df:
            self.mask_device(dilate, dm.ptr.value, db.ptr.value, df.ptr.value, df.ptr.value)
            self.device_buffers()   # (waits for the handle's pending work)
            if m.nbytes:
                check(lib.tsdf_device_download(m.ctypes.data, dm.ptr, m.nbytes))
                if b is not None:
                    check(lib.tsdf_device_download(b.ctypes.data, db.ptr, b.nbytes))
                if f is not None:
                    check(lib.tsdf_device_download(f.ctypes.data, df.ptr, f.nbytes))
        out = (m,) + ((f,) if f is not None else ()) + ((b,) if b is not None else ())
        return out[0] if len(out) == 1 else out


#: one row of Reach.rank: struct tsdf_reach_cluster (16 bytes)
REACH_CLUSTER_DTYPE = np.dtype([("label", np.uint32), ("cost", np.uint32), ("voxel", np.uint32), ("reserved", np.uint32)])
#: the cost of a voxel that no admissible path reaches, or none within max_cost
REACH_UNREACHED = _capi.TSDF_REACH_UNREACHED
REACH_COST_FACE, REACH_COST_EDGE, REACH_COST_CORNER = _capi.TSDF_REACH_COST_FACE, _capi.TSDF_REACH_COST_EDGE, _capi.TSDF_REACH_COST_CORNER
TSDF_REACH_THROUGH_UNKNOWN = _capi.TSDF_REACH_THROUGH_UNKNOWN


class Reach(_Handle):
    """tsdf_reach (include/tsdf_amd.h, "reachability"): the travel cost from a set of seeds to every voxel of a volume
    (TSDFVolume.reach(into=reach)), on the device, with the geometry it belongs to.  Lookup, paths and ranking need no volume."""

    _c, _Info = "reach", _capi.ReachInfo

    @property
    def info(self):
        """tsdf_reach_info: size, connectivity, voxel_size, offset, flags, clearance, max_cost, max_cost_reached, n_traversable,
        n_reached, n_seed_voxels, rounds (a diagnostic: it may differ from run to run)."""
        return self._get_info()

    @property
    def costs(self):
        """(X * Y * Z,) uint32 by voxel id (z * Y + y) * X + x: the cost, REACH_UNREACHED where there is none; a blocking download."""
        sx, sy, sz = (int(v) for v in self.info.size)
        out = np.empty(sx * sy * sz + 1, np.uint32)   # (one element more: the pointer of an empty array may be null)
        check(lib.tsdf_reach_download(self._h, out.ctypes.data))
        return out[:-1]

    def device_buffer(self):
        """The raw device pointer of the cost array (0 before the first computation); valid until the next computation into this handle."""
        p = C.c_void_p()
        check(lib.tsdf_reach_buffer(self._h, C.byref(p)))
        return int(p.value or 0)

    def lookup_device(self, n, points_ptr, costs_ptr, stream=None):
        """n points (3 float32 each, device) -> n uint32 costs (device), on `stream` (default: the null stream)."""
        ptr = lambda p: C.c_void_p(int(p)) if p else None
        check(lib.tsdf_reach_lookup_device(self._h, int(n), ptr(points_ptr), ptr(costs_ptr), C.c_void_p(int(stream) if stream else 0)))

    def lookup(self, points):
        """(n, 3) float32 world points (mm) -> (n,) uint32: the cost of the voxel each lies in, REACH_UNREACHED off the grid."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        out = np.empty(n + 1, np.uint32)
        check(lib.tsdf_reach_lookup(self._h, n, p.ctypes.data if n else None, out.ctypes.data))
        return out[:n]

    def paths(self, goals, max_len=None, rows=None):
        """(n, 3) float32 goal points -> the voxel path of each back to a seed, goal first.  max_len None: a list of n uint32 id arrays,
        each as long as its path (empty for a goal off the grid or not reached).  With max_len: (lengths (n,) uint32, rows (n, max_len)
        uint32) -- a length is that of the whole path even where the row holds only its first max_len ids; `rows`: the array to write
        into (what a path does not fill is left as it was; default: filled with REACH_UNREACHED)."""
        p = np.ascontiguousarray(goals, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        want = 1 if max_len is None else int(max_len)
        while True:
            lengths = np.zeros(n + 1, np.uint32)
            if rows is not None and max_len is not None:
                table = np.ascontiguousarray(rows, dtype=np.uint32).reshape(n, want)
            else:
                table = np.full((n, want), REACH_UNREACHED, np.uint32)
            buf = table if table.size else np.zeros(1, np.uint32)
            check(lib.tsdf_reach_paths(self._h, n, p.ctypes.data if n else None, want, lengths.ctypes.data, buf.ctypes.data))
            lengths = lengths[:n]
            if max_len is not None:
                return lengths, table
            longest = int(lengths.max()) if n else 0
            if longest <= want:
                return [table[i, :int(lengths[i])].copy() for i in range(n)]
            want = longest   # (a second call with rows as long as the longest path)

    def rank(self, explorer):
        """(n_listed_clusters,) REACH_CLUSTER_DTYPE rows in the order of explorer.clusters: label, cost and voxel -- the smallest (cost,
        voxel id) among the cluster's voxels; (REACH_UNREACHED, 0xFFFFFFFF) where none was reached."""
        out = np.zeros(int(explorer.info.n_listed_clusters) + 1, REACH_CLUSTER_DTYPE)
        check(lib.tsdf_reach_rank_frontiers(self._h, explorer._h, out.ctypes.data))
        return out[:-1]

    def rank_device(self, explorer, rows_ptr, stream=None):
        """The same into n_listed_clusters 16-byte rows on the device, on `stream`."""
        check(lib.tsdf_reach_rank_frontiers_device(self._h, explorer._h, C.c_void_p(int(rows_ptr)) if rows_ptr else None,
                                                   C.c_void_p(int(stream) if stream else 0)))

    def voxel_centres(self, ids):
        """(n,) voxel ids -> (n, 3) float32 world centres (mm), offset + (coordinate + 0.5) * voxel_size: what paths() takes as goals."""
        i = self.info
        vs, off = np.array(i.voxel_size, np.float32), np.array(i.offset, np.float32)
        c = _voxel_coordinates(np.asarray(ids, np.uint32).reshape(-1), i.size)
        return ((c.astype(np.float32) + np.float32(0.5)) * vs + off).astype(np.float32)


#: one row of ColumnMap.columns: struct tsdf_column (32 bytes)
COLUMN_DTYPE = np.dtype([("n_unknown", np.uint32), ("n_free", np.uint32), ("n_occupied", np.uint32), ("top", np.int32), ("bottom", np.int32),
                         ("headroom", np.uint32), ("height", np.float32), ("min_distance", np.float32)])
CELL_NO_GROUND, CELL_TRAVERSABLE, CELL_BLOCKED = _capi.TSDF_CELL_NO_GROUND, _capi.TSDF_CELL_TRAVERSABLE, _capi.TSDF_CELL_BLOCKED


class ColumnMap(_Handle):
    """tsdf_columns (include/tsdf_amd.h, "column maps"): the rows of a 2-D map of a volume's columns along one axis
    (TSDFVolume.column_map(into=cmap)), on the device, with the geometry they belong to.  Classification and downloads need no volume."""

    _c, _Info = "columns", _capi.ColumnsInfo

    @property
    def info(self):
        """tsdf_columns_info: size, axis, voxel_size, offset, lo, hi, flags, has_esdf, map_size (U, V), map_axes, the totals n_unknown,
        n_free, n_occupied, n_ground and, after classify, n_no_ground, n_traversable, n_blocked, max_step, min_headroom.  Waits for
        the handle's pending work."""
        return self._get_info()

    @property
    def columns(self):
        """(V, U) COLUMN_DTYPE: the row of cell (u, v) at [v, u]; a blocking download."""
        u, v = (int(n) for n in self.info.map_size)
        out = np.zeros(u * v + 1, COLUMN_DTYPE)   # (one element more: the pointer of an empty array may be null)
        check(lib.tsdf_columns_download(self._h, out.ctypes.data))
        return out[:-1].reshape(v, u)

    def device_buffer(self):
        """The raw device pointer of the rows (cell order, 32 bytes each); valid until the next projection into this handle."""
        p = C.c_void_p()
        check(lib.tsdf_columns_buffer(self._h, C.byref(p)))
        return int(p.value or 0)

    def classify_device(self, max_step, min_headroom, cells_ptr, stream=None):
        """One uint8 per cell (CELL_NO_GROUND / CELL_TRAVERSABLE / CELL_BLOCKED) into U * V device bytes, on `stream` (default: the
        null stream), ordered behind the projection."""
        check(lib.tsdf_columns_classify_device(self._h, int(max_step), int(min_headroom), 0, C.c_void_p(int(cells_ptr)) if cells_ptr else None,
                                               C.c_void_p(int(stream) if stream else 0)))

    def classify(self, max_step, min_headroom):
        """(V, U) uint8: CELL_NO_GROUND where the column holds no occupied voxel; CELL_BLOCKED where the headroom is below
        min_headroom or a 4-neighbour with ground has a top more than max_step voxels away; CELL_TRAVERSABLE otherwise."""
        u, v = (int(n) for n in self.info.map_size)
        out = np.zeros(u * v + 1, np.uint8)
        check(lib.tsdf_columns_classify(self._h, int(max_step), int(min_headroom), 0, out.ctypes.data))
        return out[:-1].reshape(v, u)

    def height_world(self, columns=None):
        """(V, U) float32: the world coordinate (mm) of the surface on the map's axis, offset + (lo + height) * voxel_size forward,
        offset + (hi - height) * voxel_size reversed, in fp32; NaN where a cell has no ground.  columns: rows already downloaded."""
        i = self.info
        rows = self.columns if columns is None else columns
        f32 = np.float32
        off, vs = f32(i.offset[i.axis]), f32(i.voxel_size[i.axis])
        if i.flags & _capi.TSDF_COLUMNS_REVERSED:
            return (off + (f32(i.hi) - rows["height"]) * vs).astype(f32)
        return (off + (f32(i.lo) + rows["height"]) * vs).astype(f32)


#: one row of Objects.objects: struct tsdf_class_object (72 bytes)
OBJECT_DTYPE = np.dtype([("label", np.uint32), ("size", np.uint32), ("lo", np.uint32, 3), ("hi", np.uint32, 3), ("sum", np.uint64, 3),
                         ("votes", np.uint64), ("class_id", np.uint32), ("reserved", np.uint32)])
#: what Objects.lookup gives for a point in no listed object
OBJECT_NONE = _capi.TSDF_OBJECT_NONE


class Objects(_Handle):
    """tsdf_objects (include/tsdf_amd.h, "class objects"): the labelled voxels of a volume, the connected pieces of each class among
    them and their table (TSDFVolume.find_objects(into=objects)), on the device, with the geometry they belong to; lookup() resolves
    world points to table rows.  Nothing here needs the volume."""

    _c, _Info = "objects", _capi.ObjectsInfo

    @property
    def info(self):
        """tsdf_objects_info: size, connectivity, voxel_size, offset, min_votes, min_size, n_labelled, n_objects, n_listed_objects."""
        return self._get_info()

    def _download(self, voxels=False, labels=False, rows=False):
        # (one element more than asked for: the pointer of an empty array may be null, which the C ABI reads as "not asked for")
        i = self.info
        v = np.empty(int(i.n_labelled) + 1, np.uint32) if voxels else None
        l = np.empty(int(i.n_labelled) + 1, np.uint32) if labels else None
        r = np.zeros(int(i.n_listed_objects) + 1, OBJECT_DTYPE) if rows else None
        ptr = lambda a: a.ctypes.data if a is not None else None
        check(lib.tsdf_objects_download(self._h, ptr(v), ptr(l), ptr(r)))
        return tuple(a[:-1] if a is not None else None for a in (v, l, r))

    @property
    def voxels(self):
        """(n_labelled,) uint32: the ids (z * Y + y) * X + x of the labelled voxels, ascending; a blocking download."""
        return self._download(voxels=True)[0]

    @property
    def coordinates(self):
        """(n_labelled, 3) uint32: (x, y, z) of the labelled voxels."""
        return _voxel_coordinates(self.voxels, self.info.size)

    @property
    def labels(self):
        """(n_labelled,) uint32: per listed voxel the smallest list index of its object."""
        return self._download(labels=True)[1]

    @property
    def objects(self):
        """(n_listed_objects,) OBJECT_DTYPE rows in ascending label: label, size, lo / hi (the inclusive voxel box), sum (the integer
        coordinate sums), votes (the sum of the members' votes), class_id."""
        return self._download(rows=True)[2]

    @property
    def centroids(self):
        """(n_listed_objects, 3) float64: the world centroid (mm) of every listed object, offset + (sum / size + 0.5) * voxel_size."""
        return _row_centroids(self.objects, self.info)

    @property
    def boxes(self):
        """(n_listed_objects, 6) uint32: (x0, y0, z0, x1, y1, z1) per listed object, lower corner inclusive and upper exclusive -- the
        box argument of TSDFVolume.extract_mesh."""
        rows = self.objects
        return np.concatenate([rows["lo"], rows["hi"] + np.uint32(1)], axis=1).astype(np.uint32)

    def lookup_device(self, n, points_ptr, rows_ptr, stream=0):
        """n points (3 float32 each, device) -> n uint32 table rows (device), OBJECT_NONE where the point lies in no listed object;
        asynchronous on `stream`, behind the handle's pending work."""
        check(lib.tsdf_objects_lookup_device(self._h, int(n), C.c_void_p(int(points_ptr)) if points_ptr else None,
                                             C.c_void_p(int(rows_ptr)) if rows_ptr else None, C.c_void_p(int(stream) if stream else 0)))

    def lookup(self, points):
        """(n, 3) float32 world points (mm, the frame of TSDFVolume.sample_classes) -> (n,) uint32: the row in `objects` of the object
        whose voxel each point lies in, OBJECT_NONE for NaN, off-grid and unlisted voxels and objects below min_size.  Blocking."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.empty(len(p) + 1, np.uint32)
        check(lib.tsdf_objects_lookup(self._h, len(p), p.ctypes.data if len(p) else None, out.ctypes.data))
        return out[:-1]

    def device_buffers(self):
        """Raw device pointers {voxels, masks, bases, labels, objects} (0 where empty); valid until the next call that fills them."""
        p = [C.c_void_p() for _ in range(5)]
        check(lib.tsdf_objects_buffers(self._h, *[C.byref(q) for q in p]))
        return {k: int(q.value or 0) for k, q in zip(("voxels", "masks", "bases", "labels", "objects"), p)}


def pixel_rays(camera, width, height, step=1):
    """The rays of every step-th pixel of a width x height pinhole view, for TSDFVolume.view_gain and cast_rays: (origins, directions),
    (n, 3) float32 each, rows first.  The origin is the camera's position; the direction of pixel (u, v) is R (K^-1 (u, v, 1)) in float32,
    not normalised -- t is the camera depth, as in the image cast."""
    pose, _, _, kinv = _camera_matrices(camera)
    P, Ki = pose.reshape(4, 4).T, kinv.reshape(3, 3).T
    step = max(int(step), 1)
    v, u = np.meshgrid(np.arange(0, int(height), step, dtype=np.float32), np.arange(0, int(width), step, dtype=np.float32), indexing="ij")
    pix = np.stack([u.reshape(-1), v.reshape(-1), np.ones(u.size, np.float32)], axis=1)
    d = ((pix @ Ki.T).astype(np.float32) @ P[:3, :3].T).astype(np.float32)
    o = np.broadcast_to(P[:3, 3].astype(np.float32), d.shape)
    return np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)


SPARSE_MAGIC = b"TSDFSPR1"
_SPARSE_HEADER = "<3I3f3fff3f3f" "IIIIfIQ"   # the 68-byte header of .tsdf, then brick, flags, weight_bits, weight_bound, fill, 0, n_bricks
_WEIGHT_DTYPES = {8: np.uint8, 16: np.uint16, 32: np.float32}


def _check_snapshot_layout(who, size, weight_bits, n_bricks):
    """What tsdf_snapshot_upload checks of a header, without a device; returns the grid's brick count."""
    if not all(1 <= int(s) <= 65535 for s in size):
        raise ValueError("%s: size %s is not in 1 .. 65535" % (who, tuple(int(s) for s in size)))
    if weight_bits not in _WEIGHT_DTYPES:
        raise ValueError("%s: weight_bits = %d is not 8, 16 or 32" % (who, weight_bits))
    total = 1
    for s in size:
        total *= (int(s) + 7) // 8
    if n_bricks > total:
        raise ValueError("%s: n_bricks = %d, the grid has %d bricks" % (who, n_bricks, total))
    return total


def _check_snapshot_ids(who, ids, total):
    if len(ids) and (int(ids[-1]) >= total or np.any(ids[1:] <= ids[:-1])):
        raise ValueError("%s: brick ids are not strictly ascending and below the brick count %d" % (who, total))


def write_sparse_file(path, size, header, weight_bound, fill_distance, ids, distances, weights, colours=None):
    """Write a .tsdfs file from host arrays (what Snapshot.download() returns); nothing is checked and no device is touched.
    `header`: the .tsdf fields physical_size, offset, truncation_distance, max_weight, global_translation, global_rotation."""
    weights = np.asarray(weights)
    bits = 8 * weights.dtype.itemsize
    with open(path, "wb") as f:
        f.write(SPARSE_MAGIC)
        f.write(struct.pack(_SPARSE_HEADER, *(int(s) for s in size), *header["physical_size"], *header["offset"], header["truncation_distance"],
                            header["max_weight"], *header["global_translation"], *header["global_rotation"], _capi.TSDF_SNAPSHOT_BRICK,
                            _capi.TSDF_SNAPSHOT_COLOUR if colours is not None else 0, bits, int(weight_bound), float(fill_distance), 0, len(ids)))
        for a, dtype in ((ids, np.uint32), (distances, np.float32), (weights, weights.dtype), (colours, np.uint32)):
            if a is not None:
                np.ascontiguousarray(a, np.dtype(dtype).newbyteorder("<")).tofile(f)


def read_sparse_file(path):
    """Parse and validate a .tsdfs file without touching a device: (header dict, SnapshotInfo, ids, distances, weights, colours or
    None).  The magic, the brick size, the sizes, weight_bits, n_bricks against the grid and the file's length against what the header
    implies are checked before anything is allocated; then the ids (strictly ascending, below the brick count).  ValueError otherwise."""
    who = "read_sparse_file(%s)" % path
    n_head = len(SPARSE_MAGIC) + struct.calcsize(_SPARSE_HEADER)
    length = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(n_head)
        if len(head) < n_head or head[:8] != SPARSE_MAGIC:
            raise ValueError("%s: not a .tsdfs file (magic %r, %d bytes)" % (who, head[:8], length))
        v = struct.unpack(_SPARSE_HEADER, head[8:])
        size, brick, flags, weight_bits, weight_bound, fill, n_bricks = v[0:3], v[17], v[18], v[19], v[20], v[21], v[23]
        if brick != _capi.TSDF_SNAPSHOT_BRICK:
            raise ValueError("%s: brick size %d, expected %d" % (who, brick, _capi.TSDF_SNAPSHOT_BRICK))
        if flags & ~_capi.TSDF_SNAPSHOT_COLOUR:
            raise ValueError("%s: unknown flags %#x" % (who, flags))
        total = _check_snapshot_layout(who, size, weight_bits, n_bricks)
        colour = bool(flags & _capi.TSDF_SNAPSHOT_COLOUR)
        expect = n_head + n_bricks * (4 + 512 * (4 + weight_bits // 8 + (4 if colour else 0)))
        if length != expect:
            raise ValueError("%s: the file has %d bytes, its header implies %d" % (who, length, expect))
        ids = np.fromfile(f, np.uint32, n_bricks)
        _check_snapshot_ids(who, ids, total)
        dist = np.fromfile(f, np.float32, 512 * n_bricks)
        weights = np.fromfile(f, _WEIGHT_DTYPES[weight_bits], 512 * n_bricks)
        colours = np.fromfile(f, np.uint32, 512 * n_bricks) if colour else None
    header = {"physical_size": v[3:6], "offset": v[6:9], "truncation_distance": v[9], "max_weight": v[10], "global_translation": v[11:14],
              "global_rotation": v[14:17]}
    info = _capi.SnapshotInfo()
    info.size[:] = size
    info.flags, info.weight_bits, info.weight_bound, info.fill_distance, info.n_bricks = flags, weight_bits, weight_bound, fill, n_bricks
    info.voxel_size[:] = [np.float32(p) / np.float32(s) for p, s in zip(v[3:6], size)]
    info.offset[:] = v[6:9]
    return header, info, ids, dist, weights, colours


class Snapshot(_Handle):
    """tsdf_snapshot (include/tsdf_amd.h, "sparse snapshot"): the live bricks of a volume as compact device arrays -- ids, distances,
    weights in the volume's own element type, colour words -- with the scratch that fills them, kept between snapshots
    (TSDFVolume.snapshot(into=snap)).  `header`: the .tsdf header fields that go into a file (set by TSDFVolume.snapshot and load)."""

    _c, _Info = "snapshot", _capi.SnapshotInfo

    def __init__(self):
        self.header = None
        super().__init__()

    @property
    def info(self):
        """tsdf_snapshot_info: size, bricks, flags, weight_bits, weight_bound, fill_distance, voxel_size, offset, n_bricks, bytes."""
        return self._get_info()

    @property
    def n_bricks(self):
        return int(self.info.n_bricks)

    def download(self):
        """(ids (n,) uint32, distances (n, 512) float32, weights (n, 512) uint8 / uint16 / float32, colours (n, 512) uint32 or None):
        one blocking download."""
        i = self.info
        n, colour = int(i.n_bricks), bool(i.flags & _capi.TSDF_SNAPSHOT_COLOUR)
        ids = np.empty(n + 1, np.uint32)   # (one element more: the pointer of an empty array may be null)
        dist = np.empty((n + 1, 512), np.float32)
        weights = np.empty((n + 1, 512), _WEIGHT_DTYPES[int(i.weight_bits) or 32])
        colours = np.empty((n + 1, 512), np.uint32) if colour else None
        check(lib.tsdf_snapshot_download(self._h, ids.ctypes.data, dist.ctypes.data, weights.ctypes.data, colours.ctypes.data if colour else None))
        return ids[:n], dist[:n], weights[:n], colours[:n] if colour else None

    @property
    def bricks(self):
        return self.download()[0]

    @property
    def distances(self):
        return self.download()[1]

    @property
    def weights(self):
        return self.download()[2]

    @property
    def colours(self):
        return self.download()[3]

    def device_buffers(self):
        """(ids, distances, weights, colours) as raw device pointers (0 where there is none); valid until the handle is filled again."""
        p = [C.c_void_p() for _ in range(4)]
        check(lib.tsdf_snapshot_buffers(self._h, *(C.byref(q) for q in p)))
        return tuple(int(q.value or 0) for q in p)

    def select(self, lo, hi, outside=False, into=None):
        """The Snapshot of those bricks whose brick coordinates lie inside the box [lo, hi) -- with `outside`, outside it
        (tsdf_snapshot_select).  Ids, geometry and storage are this snapshot's.  `into`: a Snapshot to reuse (not this one)."""
        dst = Snapshot() if into is None else into
        i3 = lambda v: (C.c_int32 * 3)(*(int(x) for x in v))
        check(lib.tsdf_snapshot_select(self._h, i3(lo), i3(hi), _capi.TSDF_SELECT_OUTSIDE if outside else 0, dst._h))
        dst.header = self.header
        return dst

    @classmethod
    def from_arrays(cls, size, bricks, distances, weights, colours=None, fill_distance=0.0, voxel_size=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0),
                    header=None, into=None):
        """A Snapshot from host arrays (tsdf_snapshot_upload): what download() returns, or a file holds.  The element type of `weights`
        (uint8, uint16 or float32) is the snapshot's weight_bits.  The arrays are checked on the host first."""
        weights = np.asarray(weights)
        bits = {np.dtype(np.uint8): 8, np.dtype(np.uint16): 16, np.dtype(np.float32): 32}.get(weights.dtype)
        if bits is None:
            raise ValueError("Snapshot.from_arrays: weights must be uint8, uint16 or float32, not %s" % weights.dtype)
        ids = np.ascontiguousarray(bricks, np.uint32).reshape(-1)
        n = len(ids)
        total = _check_snapshot_layout("Snapshot.from_arrays", size, bits, n)
        _check_snapshot_ids("Snapshot.from_arrays", ids, total)
        dist = np.ascontiguousarray(distances, np.float32).reshape(-1)
        weights = np.ascontiguousarray(weights).reshape(-1)
        col = None if colours is None else np.ascontiguousarray(colours, np.uint32).reshape(-1)
        for name, a in (("distances", dist), ("weights", weights), ("colours", col)):
            if a is not None and a.size != 512 * n:
                raise ValueError("Snapshot.from_arrays: %s has %d elements, expected %d" % (name, a.size, 512 * n))
        info = _capi.SnapshotInfo()
        info.size[:] = [int(s) for s in size]
        info.flags = _capi.TSDF_SNAPSHOT_COLOUR if col is not None else 0
        info.weight_bits, info.fill_distance, info.n_bricks = bits, float(fill_distance), n
        info.voxel_size[:] = [float(v) for v in voxel_size]
        info.offset[:] = [float(v) for v in offset]
        snap = cls() if into is None else into
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        check(lib.tsdf_snapshot_upload(snap._h, C.byref(info), ptr(ids), ptr(dist), ptr(weights), ptr(col)))
        snap.header = header
        return snap

    def save(self, path):
        """Write a .tsdfs file: little-endian, no padding; "TSDFSPR1", the 68-byte header of .tsdf, brick = 8, flags,
        weight_bits, weight_bound, fill_distance, 0, n_bricks, then the id, distance, weight and colour arrays.  The .tsdf fields come
        from `header`; without one they are made from the snapshot's own geometry."""
        i = self.info
        size = [int(s) for s in i.size]
        h = self.header or {"physical_size": tuple(float(np.float32(v) * np.float32(s)) for v, s in zip(i.voxel_size, size)),
                            "offset": tuple(i.offset), "truncation_distance": float(i.fill_distance), "max_weight": 0.0,
                            "global_translation": (0.0, 0.0, 0.0), "global_rotation": (0.0, 0.0, 0.0)}
        ids, dist, weights, colours = self.download()
        write_sparse_file(path, size, h, int(i.weight_bound), float(i.fill_distance), ids, dist, weights, colours)

    @classmethod
    def load(cls, path, into=None):
        """A Snapshot from a .tsdfs file, validated on the host first (read_sparse_file); `header` holds the file's .tsdf fields."""
        header, info, ids, dist, weights, colours = read_sparse_file(path)
        return cls.from_arrays(tuple(info.size), ids, dist, weights, colours, fill_distance=info.fill_distance, voxel_size=tuple(info.voxel_size),
                               offset=tuple(info.offset), header=header, into=into)


class _DeviceArray:
    """A device copy of a host array for the length of a `with` block (tsdf_device_alloc / upload / free)."""

    def __init__(self, host=None, nbytes=None):
        self.host = host
        self.nbytes = int(host.nbytes if host is not None else nbytes)
        self.ptr = C.c_void_p()

    def __enter__(self):
        if self.nbytes:
            check(lib.tsdf_device_alloc(self.nbytes, C.byref(self.ptr)))
            if self.host is not None:
                try:
                    check(lib.tsdf_device_upload(self.ptr, self.host.ctypes.data, self.nbytes))
                except Exception:
                    lib.tsdf_device_free(self.ptr)
                    raise
        return self

    def __exit__(self, *a):
        if self.ptr.value:
            lib.tsdf_device_free(self.ptr)
            self.ptr = C.c_void_p()


def _components_info(i):
    return {"n_components": int(i.n_components), "n_triangles": int(i.n_triangles), "largest_triangles": int(i.largest_triangles),
            "largest_label": int(i.largest_label)}


def label_components_device(n_vertices, n_indices, indices_ptr, labels_ptr, component_triangles_ptr=0, stream=0):
    """tsdf_label_components_device on device pointers (uint32 arrays: n_indices indices, n_vertices labels and -- or 0 -- n_vertices
    sizes): blocking; returns the info dict.  ValueError for an index that is not below n_vertices."""
    i = _capi.ComponentsInfo()
    vp = lambda p: C.c_void_p(int(p) if p else 0)
    check(lib.tsdf_label_components_device(int(n_vertices), int(n_indices), vp(indices_ptr), vp(labels_ptr), vp(component_triangles_ptr),
                                           C.byref(i), vp(stream)))
    return _components_info(i)


def label_components(n_vertices, indices):
    """The connected components of the graph whose index triples are `indices` (any integer array of 3 n values below n_vertices), on
    the device: (labels (n_vertices,) uint32, sizes (n_vertices,) uint32, info)."""
    I = np.ascontiguousarray(np.asarray(indices).reshape(-1), np.uint32)
    n = int(n_vertices)
    labels, sizes = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    with _DeviceArray(I) as di, _DeviceArray(nbytes=4 * max(n, 1)) as dl, _DeviceArray(nbytes=4 * max(n, 1)) as dt:
        info = label_components_device(n, I.size, di.ptr.value, dl.ptr.value, dt.ptr.value)
        if n:
            check(lib.tsdf_device_download(labels.ctypes.data, dl.ptr, labels.nbytes))
            check(lib.tsdf_device_download(sizes.ctypes.data, dt.ptr, sizes.nbytes))
    return labels, sizes, info


def simplify_mesh_device(n_vertices, n_indices, vertices_ptr, indices_ptr, cell_size, into, normals_ptr=0, colours_ptr=0, stream=0):
    """tsdf_simplify_mesh_device on device pointers (float32 x 3 vertices, uint32 indices, float32 x 3 normals or 0, uint8 x 3 colours
    or 0) into the Mesh `into`, which is returned.  ValueError for an index that is not below n_vertices."""
    vp = lambda p: C.c_void_p(int(p) if p else 0)
    check(lib.tsdf_simplify_mesh_device(int(n_vertices), int(n_indices), vp(vertices_ptr), vp(indices_ptr), vp(normals_ptr), vp(colours_ptr),
                                        float(cell_size), 0, into._h, vp(stream)))
    return into


def simplify_mesh(vertices, indices, cell_size, normals=None, colours=None):
    """Vertex clustering of host arrays on the device (upload, tsdf_simplify_mesh_device, download): (n, 3) float32 vertices, 3 m
    indices, optionally (n, 3) float32 normals and (n, 3) uint8 colours -> (vertices, indices, normals or None, colours or None)."""
    V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    I = np.ascontiguousarray(np.asarray(indices).reshape(-1), np.uint32)
    N = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    RGB = None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(-1, 3)
    for a, what in ((N, "normals"), (RGB, "colours")):
        if a is not None and len(a) != len(V):
            raise ValueError("%d %s for %d vertices" % (len(a), what, len(V)))
    dst = Mesh()
    try:
        with _DeviceArray(V) as dv, _DeviceArray(I) as di, _DeviceArray(nbytes=4) as none:
            with _DeviceArray(N if N is not None and len(V) else None, 0) as dn, _DeviceArray(RGB if RGB is not None and len(V) else None, 0) as dc:
                # (an empty array given is still "given": any non-null pointer says so, nothing is read through it)
                given = lambda a, d: 0 if a is None else (d.ptr.value or none.ptr.value)
                simplify_mesh_device(len(V), I.size, dv.ptr.value, di.ptr.value, cell_size, dst, given(N, dn), given(RGB, dc))
                return dst.vertices, dst.indices, None if N is None else dst.normals, None if RGB is None else dst.colours
    finally:
        dst.close()


def _smooth_flags(pin_boundary, normals):
    return (_capi.TSDF_SMOOTH_PIN_BOUNDARY if pin_boundary else 0) | (_capi.TSDF_SMOOTH_NORMALS if normals else 0)


def smooth_mesh_device(n_vertices, n_indices, vertices_ptr, indices_ptr, into, iterations=10, lam=0.5, mu=-0.53, pin_boundary=False,
                       face_normals=False, normals_ptr=0, colours_ptr=0, stream=0):
    """tsdf_smooth_mesh_device on device pointers (float32 x 3 vertices, uint32 indices, float32 x 3 normals or 0, uint8 x 3 colours or
    0) into the Mesh `into`, which is returned.  ValueError for an index that is not below n_vertices."""
    vp = lambda p: C.c_void_p(int(p) if p else 0)
    check(lib.tsdf_smooth_mesh_device(int(n_vertices), int(n_indices), vp(vertices_ptr), vp(indices_ptr), vp(normals_ptr), vp(colours_ptr),
                                      int(iterations), float(lam), float(mu), _smooth_flags(pin_boundary, face_normals), into._h, vp(stream)))
    return into


def smooth_mesh(vertices, indices, iterations=10, lam=0.5, mu=-0.53, pin_boundary=False, face_normals=False, normals=None, colours=None):
    """Taubin smoothing of host arrays on the device (upload, tsdf_smooth_mesh_device, download): (n, 3) float32 vertices, 3 m indices,
    optionally (n, 3) float32 normals and (n, 3) uint8 colours -> (vertices, indices, normals or None, colours or None); with
    `face_normals` the normals are those of the smoothed faces, whether or not any were given."""
    V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    I = np.ascontiguousarray(np.asarray(indices).reshape(-1), np.uint32)
    N = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    RGB = None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(-1, 3)
    for a, what in ((N, "normals"), (RGB, "colours")):
        if a is not None and len(a) != len(V):
            raise ValueError("%d %s for %d vertices" % (len(a), what, len(V)))
    dst = Mesh()
    try:
        with _DeviceArray(V) as dv, _DeviceArray(I) as di, _DeviceArray(nbytes=4) as none:
            with _DeviceArray(N if N is not None and len(V) else None, 0) as dn, _DeviceArray(RGB if RGB is not None and len(V) else None, 0) as dc:
                given = lambda a, d: 0 if a is None else (d.ptr.value or none.ptr.value)      # (see simplify_mesh)
                smooth_mesh_device(len(V), I.size, dv.ptr.value, di.ptr.value, dst, iterations, lam, mu, pin_boundary, face_normals,
                                   given(N, dn), given(RGB, dc))
                return dst.vertices, dst.indices, dst.normals if N is not None or face_normals else None, None if RGB is None else dst.colours
    finally:
        dst.close()


def vertex_normals(vertices, indices):
    """Area-weighted vertex normals of host arrays, computed on the device (tsdf_vertex_normals_device): (n, 3) float32, the NaN triple
    where no face gives a direction.  Triangle t is (I[3t], I[3t+2], I[3t+1]), as Mesh.triangles() wires it."""
    V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    I = np.ascontiguousarray(np.asarray(indices).reshape(-1), np.uint32)
    out = np.empty((len(V), 3), np.float32)
    with _DeviceArray(V) as dv, _DeviceArray(I) as di, _DeviceArray(nbytes=out.nbytes) as dn:
        check(lib.tsdf_vertex_normals_device(len(V), I.size, dv.ptr, di.ptr, dn.ptr, None))
        if len(V):
            check(lib.tsdf_device_download(out.ctypes.data, dn.ptr, out.nbytes))
    return out


def _pose16(T):
    """4 x 4 (normal indexing; None: identity) -> column-major float64[16]."""
    T = np.eye(4) if T is None else np.asarray(T, np.float64)
    if T.shape != (4, 4):
        raise ValueError("expected a 4 x 4 pose, got shape %s" % (T.shape,))
    return np.ascontiguousarray(T.T.reshape(-1))


#: Defaults of the colour term ("colour alignment").  The sweep of the CPU reference on two synthetic scenes hardly tells the weights
#: apart, and the one noisy-depth sequence tracked on a GPU ends nearer the truth than without colour at 0.001 and 0.01 and farther
#: at 0.1 and 1: hence 0.01.  Measured on nothing else: they are scene-dependent.  COLOUR_GATE is in intensity units
#: (0 .. 255), COLOUR_WEIGHT in mm^2 per intensity^2 -- it trades a squared distance residual against a squared brightness residual.
COLOUR_GATE = 64.0
COLOUR_WEIGHT = 0.01


class FieldAligner:
    """tsdf_aligner (include/tsdf_amd.h, "field alignment"): Gauss-Newton alignment of point sets to a volume's field.  Every call
    runs on the volume's stream."""

    MAX_STAGES = 8

    def __init__(self):
        self._h = C.c_void_p()
        check(lib.tsdf_aligner_create(C.byref(self._h)))

    def close(self):
        if lib is not None and getattr(self, "_h", None) is not None and self._h.value:   # (lib is None during interpreter shutdown)
            lib.tsdf_aligner_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _on(self, volume, gate):
        s = volume.stream_ptr()
        check(lib.tsdf_aligner_set_stream(self._h, C.c_void_p(int(s) if s else 0)))
        return float(volume.truncation_distance() if gate is None else gate)

    def step_device(self, volume, n, points_ptr, T=None, gate=None, rows_ptr=None):
        """One step's sums at T over n device points: (A 6x6, b 6, residual, inliers), float32; rows_ptr: 7 n floats or None."""
        gate = self._on(volume, gate)
        Tc = _pose16(T)
        A, b, ri = np.zeros(36, np.float32), np.zeros(6, np.float32), np.zeros(2, np.float32)
        check(lib.tsdf_aligner_step(self._h, volume._h, int(n), C.c_void_p(int(points_ptr)) if points_ptr else None, Tc.ctypes.data, gate,
                                    A.ctypes.data, b.ctypes.data, ri.ctypes.data, C.c_void_p(int(rows_ptr)) if rows_ptr else None))
        return A.reshape(6, 6), b, float(ri[0]), float(ri[1])

    def _colour(self, colour_gate, colour_weight):
        return (float(COLOUR_GATE if colour_gate is None else colour_gate), float(COLOUR_WEIGHT if colour_weight is None else colour_weight))

    def step_colour_device(self, volume, n, points_ptr, intensity_ptr, T=None, gate=None, colour_gate=None, colour_weight=None, rows_ptr=None):
        """tsdf_aligner_step_colour over n device points and intensities: (A 6x6, b 6 of the combined system, (residual, colour
        residual), (inliers, colour inliers)); rows_ptr: 14 n floats or None."""
        gate = self._on(volume, gate)
        cg, cw = self._colour(colour_gate, colour_weight)
        Tc = _pose16(T)
        A, b, ri = np.zeros(36, np.float32), np.zeros(6, np.float32), np.zeros(4, np.float32)
        ptr = lambda p: C.c_void_p(int(p)) if p else None
        check(lib.tsdf_aligner_step_colour(self._h, volume._h, int(n), ptr(points_ptr), ptr(intensity_ptr), Tc.ctypes.data, gate, cg, cw,
                                           A.ctypes.data, b.ctypes.data, ri.ctypes.data, ptr(rows_ptr)))
        return A.reshape(6, 6), b, (float(ri[0]), float(ri[2])), (float(ri[1]), float(ri[3]))

    def run_colour_device(self, volume, stages, T0=None, gate=None, colour_gate=None, colour_weight=None):
        """stages: up to 8 (points_ptr, intensity_ptr, n, iterations) run as one chain -> (T 4x4 float64, (residual, colour residual),
        (inliers, colour inliers)) of the last step."""
        gate = self._on(volume, gate)
        cg, cw = self._colour(colour_gate, colour_weight)
        st = (_capi.AlignColourStage * max(1, len(stages)))()
        for i, (ptr, iptr, n, it) in enumerate(stages):
            st[i].device_points, st[i].device_intensity = (int(ptr) if ptr else None), (int(iptr) if iptr else None)
            st[i].n, st[i].iterations = int(n), int(it)
        Tc = _pose16(T0)
        res, inl = np.zeros(2, np.float32), np.zeros(2, np.float32)
        check(lib.tsdf_aligner_run_colour(self._h, volume._h, len(stages), st, gate, cg, cw, Tc.ctypes.data, res.ctypes.data, inl.ctypes.data))
        return Tc.reshape(4, 4).T.copy(), (float(res[0]), float(res[1])), (float(inl[0]), float(inl[1]))

    def step(self, volume, points, T=None, gate=None, rows=False, intensity=None, colour_gate=None, colour_weight=None):
        """(n, 3) float32 host points -> (A, b, residual, inliers) and, with rows=True, the (n, 7) rows (NaN rows for outliers).
        `intensity` ((n,) float32; NaN: a point without colour): the step with the colour term ("colour alignment") -- A and b are the
        combined system, residual and inliers pairs (geometric, colour), the rows (n, 14): both rows of every point.  colour_gate,
        colour_weight: see COLOUR_GATE, COLOUR_WEIGHT."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        if intensity is not None:
            y = np.ascontiguousarray(intensity, dtype=np.float32).reshape(-1)
            if len(y) != n:
                raise ValueError("expected %d intensities, got %d" % (n, len(y)))
            out = np.empty((n, 14), np.float32)
            with _DeviceArray(p) as dp, _DeviceArray(y) as dy, _DeviceArray(nbytes=out.nbytes if rows else 0) as dr:
                res = self.step_colour_device(volume, n, dp.ptr.value, dy.ptr.value, T, gate, colour_gate, colour_weight, dr.ptr.value)
                if rows and n:
                    check(lib.tsdf_device_download(out.ctypes.data, dr.ptr, out.nbytes))
            return res + (out,) if rows else res
        out = np.empty((n, 7), np.float32)
        with _DeviceArray(p) as dp, _DeviceArray(nbytes=out.nbytes if rows else 0) as dr:
            res = self.step_device(volume, n, dp.ptr.value, T, gate, dr.ptr.value)
            if rows and n:
                check(lib.tsdf_device_download(out.ctypes.data, dr.ptr, out.nbytes))
        return res + (out,) if rows else res

    def run_device(self, volume, stages, T0=None, gate=None):
        """stages: up to 8 (points_ptr, n, iterations) run as one chain -> (T 4x4 float64, residual, inliers) of the last step."""
        gate = self._on(volume, gate)
        st = (_capi.AlignStage * max(1, len(stages)))()
        for i, (ptr, n, it) in enumerate(stages):
            st[i].device_points, st[i].n, st[i].iterations = (int(ptr) if ptr else None), int(n), int(it)
        Tc = _pose16(T0)
        res, inl = C.c_float(), C.c_float()
        check(lib.tsdf_aligner_run(self._h, volume._h, len(stages), st, gate, Tc.ctypes.data, C.byref(res), C.byref(inl)))
        return Tc.reshape(4, 4).T.copy(), float(res.value), float(inl.value)

    def run(self, volume, stages, T0=None, gate=None, intensity=None, colour_gate=None, colour_weight=None):
        """stages: up to 8 ((n, 3) float32 host points, iterations).  `intensity`: one (n,) float32 array per stage -- the chain with
        the colour term (run_colour_device); residual and inliers are then pairs (geometric, colour)."""
        import contextlib
        hosts = [(np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3), int(it)) for p, it in stages]
        if intensity is not None:
            ys = [np.ascontiguousarray(y, dtype=np.float32).reshape(-1) for y in intensity]
            if len(ys) != len(hosts) or any(len(y) != len(p) for y, (p, _) in zip(ys, hosts)):
                raise ValueError("run: one intensity per point of every stage is needed")
            with contextlib.ExitStack() as stack:
                dev = [(stack.enter_context(_DeviceArray(p)).ptr.value, stack.enter_context(_DeviceArray(y)).ptr.value, len(p), it)
                       for (p, it), y in zip(hosts, ys)]
                return self.run_colour_device(volume, dev, T0, gate, colour_gate, colour_weight)
        with contextlib.ExitStack() as stack:
            dev = [(stack.enter_context(_DeviceArray(p)).ptr.value, len(p), it) for p, it in hosts]
            return self.run_device(volume, dev, T0, gate)


def depth_to_points_device(width, height, depth_ptr, kinv, step, depth_cutoff, points_ptr, stream=0):
    """tsdf_depth_to_points_device: every step-th pixel of a uint16 depth image (mm) -> ceil(width / step) * ceil(height / step)
    camera-frame points on the device; asynchronous on `stream`."""
    check(lib.tsdf_depth_to_points_device(int(width), int(height), C.c_void_p(int(depth_ptr)) if depth_ptr else None, _fp(_mat(kinv, 9)),
                                          int(step), float(depth_cutoff), C.c_void_p(int(points_ptr)) if points_ptr else None,
                                          C.c_void_p(int(stream) if stream else 0)))


def depth_to_points(depth, width, height, kinv, step=1, depth_cutoff=float("inf")):
    """Host uint16 depth image (mm) -> (ceil(height / step), ceil(width / step), 3) float32 camera-frame points of every step-th
    pixel; the NaN triple for depth 0 or depth > depth_cutoff (mm)."""
    d = np.ascontiguousarray(depth, dtype=np.uint16).reshape(-1)
    width, height, step = int(width), int(height), int(step)
    if d.size != width * height:
        raise ValueError("depth has %d pixels, expected %d" % (d.size, width * height))
    if step <= 0:
        raise ValueError("depth_to_points: step is 0")
    out = np.empty((-(-height // step), -(-width // step), 3), np.float32)
    with _DeviceArray(d) as dd, _DeviceArray(nbytes=out.nbytes) as dp:
        depth_to_points_device(width, height, dd.ptr.value, kinv, step, depth_cutoff, dp.ptr.value)
        check(lib.tsdf_stream_synchronize(None))
        check(lib.tsdf_device_download(out.ctypes.data, dp.ptr, out.nbytes))
    return out


#: tsdf_depth_weights flags (include/tsdf_amd.h, "weighted integration")
WEIGHTS_INVERSE_SQUARE, WEIGHTS_COSINE = _capi.TSDF_WEIGHTS_INVERSE_SQUARE, _capi.TSDF_WEIGHTS_COSINE
CLASS_VOID = _capi.TSDF_CLASS_VOID   # a pixel, or a sample, without a class


def depth_weights_device(width, height, depth_ptr, kinv, flags, z_ref, weights_ptr, stream=0):
    """tsdf_depth_weights_device: the standard weight models of a uint16 depth image on the device -> width * height float32;
    asynchronous on `stream`."""
    check(lib.tsdf_depth_weights_device(int(width), int(height), C.c_void_p(int(depth_ptr)) if depth_ptr else None, _fp(_mat(kinv, 9)),
                                        int(flags), float(z_ref), C.c_void_p(int(weights_ptr)) if weights_ptr else None,
                                        C.c_void_p(int(stream) if stream else 0)))


def depth_weights(depth, width, height, kinv, flags=0, z_ref=0.0):
    """Host uint16 depth image -> (height, width) float32 weights: 0 where the depth is 0, else the product of the factors `flags`
    selects (WEIGHTS_INVERSE_SQUARE: min(1, (z_ref / depth)^2); WEIGHTS_COSINE: the cosine of the incidence angle, 0 on silhouettes)."""
    d = np.ascontiguousarray(depth, dtype=np.uint16).reshape(-1)
    width, height = int(width), int(height)
    if d.size != width * height:
        raise ValueError("depth has %d pixels, expected %d" % (d.size, width * height))
    out = np.empty((height, width), np.float32)
    check(lib.tsdf_depth_weights(width, height, d.ctypes.data, _fp(_mat(kinv, 9)), int(flags), float(z_ref), out.ctypes.data))
    return out


def rgb_to_intensity_device(width, height, rgb_ptr, step, intensity_ptr, stream=0):
    """tsdf_rgb_to_intensity_device: every step-th pixel of an RGB frame (3 bytes a pixel) -> its intensity, in the order and count of
    depth_to_points_device's points; asynchronous on `stream`."""
    check(lib.tsdf_rgb_to_intensity_device(int(width), int(height), C.c_void_p(int(rgb_ptr)) if rgb_ptr else None, int(step),
                                           C.c_void_p(int(intensity_ptr)) if intensity_ptr else None, C.c_void_p(int(stream) if stream else 0)))


def rgb_to_intensity(rgb, width, height, step=1):
    """Host RGB frame (uint8, width * height * 3) -> (ceil(height / step), ceil(width / step)) float32: Y = (77 r + 150 g + 29 b) / 256
    of every step-th pixel, pairing up with depth_to_points at the same step."""
    c = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1)
    width, height, step = int(width), int(height), int(step)
    if c.size != 3 * width * height:
        raise ValueError("rgb has %d bytes, expected %d" % (c.size, 3 * width * height))
    if step <= 0:
        raise ValueError("rgb_to_intensity: step is 0")
    out = np.empty((-(-height // step), -(-width // step)), np.float32)
    with _DeviceArray(c) as dc, _DeviceArray(nbytes=out.nbytes) as dy:
        rgb_to_intensity_device(width, height, dc.ptr.value, step, dy.ptr.value)
        check(lib.tsdf_stream_synchronize(None))
        check(lib.tsdf_device_download(out.ctypes.data, dy.ptr, out.nbytes))
    return out


class ICPOdometry:
    """third_party/ICP_CUDA/ICPOdometry.h of the reference: projective point-to-plane ICP between a model depth image
    (initICPModel) and the current one (initICP), three pyramid levels, 4/5/10 iterations."""

    def __init__(self, width, height, cx, cy, fx, fy, dist_thresh=0.10, angle_thresh=None):
        import math
        if angle_thresh is None:   # sinf(20.f * 3.14159254f / 180.f), ICPOdometry.h:27
            angle_thresh = float(np.float32(math.sin(np.float32(20.0) * np.float32(3.14159254) / np.float32(180.0))))
        self.width, self.height = int(width), int(height)
        self._h = C.c_void_p()
        check(lib.tsdf_icp_create(self.width, self.height, float(cx), float(cy), float(fx), float(fy), float(dist_thresh),
                                  float(angle_thresh), C.byref(self._h)))
        self.last_error, self.last_inliers = 0.0, float(width * height)

    def close(self):
        if lib is not None and getattr(self, "_h", None) is not None and self._h.value:   # (lib is None during interpreter shutdown)
            lib.tsdf_icp_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def set_stream(self, hip_stream):
        check(lib.tsdf_icp_set_stream(self._h, C.c_void_p(int(hip_stream) if hip_stream else 0)))

    def _depth(self, depth):
        d = np.ascontiguousarray(depth, dtype=np.uint16).reshape(-1)
        if d.size != self.width * self.height:
            raise ValueError("depth has %d pixels, expected %d" % (d.size, self.width * self.height))
        return d

    def init_icp(self, depth, depth_cutoff=20.0):
        d = self._depth(depth)
        check(lib.tsdf_icp_init(self._h, 0, d.ctypes.data, float(depth_cutoff)))

    def init_icp_model(self, depth, depth_cutoff=20.0):
        d = self._depth(depth)
        check(lib.tsdf_icp_init(self._h, 1, d.ctypes.data, float(depth_cutoff)))

    def init_icp_device(self, depth_ptr, model=False, depth_cutoff=20.0):
        check(lib.tsdf_icp_init_device(self._h, 1 if model else 0, C.c_void_p(int(depth_ptr)), float(depth_cutoff)))

    def estimate_step(self, level, R, t):
        """R 3x3 (normal indexing), t 3 -> (A 6x6, b 6, residual, inliers) of one Gauss-Newton step at `level`."""
        Rc = np.ascontiguousarray(np.asarray(R, np.float32).T.reshape(-1))   # column-major
        tc = np.ascontiguousarray(t, np.float32).reshape(-1)
        A, b, ri = np.zeros(36, np.float32), np.zeros(6, np.float32), np.zeros(2, np.float32)
        check(lib.tsdf_icp_estimate_step(self._h, int(level), Rc.ctypes.data, tc.ctypes.data, A.ctypes.data, b.ctypes.data,
                                         ri.ctypes.data))
        return A.reshape(6, 6), b, float(ri[0]), float(ri[1])

    def get_incremental_transformation(self, T=None):
        """T_prev_curr (4x4 float64, identity by default) refined in place of the reference's Sophus::SE3d argument."""
        Tc = np.ascontiguousarray((np.eye(4) if T is None else np.asarray(T, np.float64)).T.reshape(-1))
        err, inl = C.c_float(), C.c_float()
        check(lib.tsdf_icp_get_incremental_transformation(self._h, Tc.ctypes.data, C.byref(err), C.byref(inl)))
        self.last_error, self.last_inliers = float(err.value), float(inl.value)
        return Tc.reshape(4, 4).T.copy()

    def get_map(self, which, level):
        """which in vmap_prev | nmap_prev | vmap_curr | nmap_curr -> (3*rows, cols) float32 (planar)."""
        rows, cols = self.height >> level, self.width >> level
        m = np.empty((3 * rows, cols), np.float32)
        check(lib.tsdf_icp_get_map(self._h, {"vmap_prev": 0, "nmap_prev": 1, "vmap_curr": 2, "nmap_curr": 3}[which], int(level),
                                   m.ctypes.data))
        return m

    def get_depth_level(self, level):
        d = np.empty((self.height >> level, self.width >> level), np.uint16)
        check(lib.tsdf_icp_get_depth_level(self._h, int(level), d.ctypes.data))
        return d


class Camera:
    """The C++ Camera of the host library (same surface as src/include/Camera.hpp of the reference).
    Matrices come back as column-major float32 vectors, i.e. what Eigen's .data() yields."""

    def __init__(self, focal_x, focal_y, centre_x, centre_y):
        self._h = _capi.host.tsdf_camera_create(float(focal_x), float(focal_y), float(centre_x), float(centre_y))
        self._refresh()

    @staticmethod
    def default_depth_camera():
        return Camera(591.1, 590.1, 331.0, 234.6)   # Camera.hpp:41-44

    def __del__(self):
        host = getattr(_capi, "host", None) if _capi is not None else None   # (None during interpreter shutdown)
        if getattr(self, "_h", None) and host is not None:
            host.tsdf_camera_destroy(self._h)
            self._h = None

    def _refresh(self):
        self._k, self._kinv = np.zeros(9, np.float32), np.zeros(9, np.float32)
        self._pose, self._ipose = np.zeros(16, np.float32), np.zeros(16, np.float32)
        _capi.host.tsdf_camera_get(self._h, _fp(self._k), _fp(self._kinv), _fp(self._pose), _fp(self._ipose))

    def k(self):
        return self._k

    def kinv(self):
        return self._kinv

    def pose(self):
        return self._pose

    def inverse_pose(self):
        return self._ipose

    def set_pose(self, pose):
        """pose: 16 floats column-major (or a 7-vector tx ty tz qx qy qz qw in TUM order)."""
        p = np.ascontiguousarray(pose, dtype=np.float32).reshape(-1)
        if p.size == 7:
            _capi.host.tsdf_camera_set_pose_tum(self._h, _fp(p))
        else:
            _capi.host.tsdf_camera_set_pose(self._h, _fp(_mat(p, 16)))
        self._refresh()

    def set_pose_rows(self, rows):
        """pose given as a 4x4 in the usual row-major maths notation."""
        self.set_pose(np.ascontiguousarray(np.asarray(rows, np.float32).reshape(4, 4).T).reshape(-1))

    def move_to(self, wx, wy, wz):
        _capi.host.tsdf_camera_move_to(self._h, float(wx), float(wy), float(wz))
        self._refresh()

    def look_at(self, wx, wy, wz):
        _capi.host.tsdf_camera_look_at(self._h, float(wx), float(wy), float(wz))
        self._refresh()

    def position(self):
        return self._pose[12:15].copy()

    def _v3(self, fn, w):
        a = _mat(w, 3)
        out = np.zeros(3, np.float32)
        fn(self._h, _fp(a), _fp(out))
        return out

    def world_to_camera(self, w):
        return self._v3(_capi.host.tsdf_camera_world_to_camera, w)

    def camera_to_world(self, c):
        return self._v3(_capi.host.tsdf_camera_camera_to_world, c)

    def world_to_pixel(self, w):
        out = (C.c_int * 2)()
        _capi.host.tsdf_camera_world_to_pixel(self._h, _fp(_mat(w, 3)), out)
        return int(out[0]), int(out[1])

    def pixel_to_image_plane(self, x, y):
        out = np.zeros(2, np.float32)
        _capi.host.tsdf_camera_pixel_to_image_plane(self._h, int(x), int(y), _fp(out))
        return out

    def image_plane_to_pixel(self, p):
        out = (C.c_int * 2)()
        _capi.host.tsdf_camera_image_plane_to_pixel(self._h, _fp(_mat(p, 2)), out)
        return int(out[0]), int(out[1])


def load_tum_directory(directory):
    """Every frame of a TUM-layout directory through the host library's TUMDataLoader (the loader tools/kinfu_stream.cpp and
    the reference's kinfu.cpp use): [(depth uint16 (H*W,) in millimetres, Camera at the frame's ground-truth pose)], (W, H)."""
    def opened():
        h = _capi.host.tsdf_host_tum_open(str(directory).encode())
        if not h:
            raise ValueError("%s does not have the TUM layout (depth/*.png + ground_truth.txt)" % directory)
        return h

    size, pose = (C.c_uint * 2)(), np.zeros(16, np.float32)
    h = opened()       # the first frame's size (nothing is copied without a buffer)
    got = _capi.host.tsdf_host_tum_next(h, None, 0, size, _fp(pose))
    _capi.host.tsdf_host_tum_close(h)
    if got < 0:
        raise ValueError("%s: the first record's depth image is missing or unreadable" % directory)
    if not got:
        return [], (0, 0)
    w, hh = int(size[0]), int(size[1])
    buf, frames = np.zeros(w * hh, np.uint16), []
    h = opened()
    try:
        while True:
            got = _capi.host.tsdf_host_tum_next(h, buf.ctypes.data, buf.size, size, _fp(pose))
            if got == 0:
                break
            if got < 0:     # (a truncated stream would silently become another workload)
                raise ValueError("%s: record %d of ground_truth.txt has no readable depth image" % (directory, len(frames)))
            if (int(size[0]), int(size[1])) != (w, hh):
                raise ValueError("depth images of different sizes in %s" % directory)
            cam = Camera.default_depth_camera()
            cam.set_pose(pose)
            frames.append((buf.copy(), cam))
    finally:
        _capi.host.tsdf_host_tum_close(h)
    return frames, (w, hh)
