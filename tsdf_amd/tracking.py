"""Frame-to-model tracking: the kinfu loop with ICP poses instead of ground truth (BASELINE configs[4]).

The reference has the two halves -- src/Tools/kinfu.cpp integrates a TUM sequence with the ground-truth poses,
src/Tools/tsdf_icp.cpp aligns one depth image to a rendering of a volume (GPURaycaster::render_to_depth_image +
ICPOdometry) -- the library composes them per frame, device resident (tsdf_amd/csrc/pipeline.hip: tsdf_tracker_*):

    filtered  = BilateralFilter(depth), initICP(filtered)          (second, lower-priority stream)
    model     = render_to_depth_image(volume, pose[i-1])           (ray cast + vertices_to_depth, beside the line above)
    T         = ICPOdometry(model = model, current = filtered)     (current-camera -> model-camera, metres)
    pose[i]   = pose[i-1] * T                                      (translation back to millimetres; here, with the Camera class)
    volume.integrate(filtered, pose[i])

With method="field" the model image, its maps and ICP are replaced by field alignment (include/tsdf_amd.h, "field alignment"): the
filtered frame's pixels become camera-frame points and the pose is refined directly against the volume's distance field from the
previous pose (tsdf_tracker_align_field); no ray cast.

This class is the ctypes mirror of those entry points plus the pose composition; torch only wraps the tracker's streams.
"""
import ctypes as C

import numpy as np

from . import api
from ._capi import check, lib
from .pipeline import OVERLAP, _matrices


class FrameToModelTracker:
    def __init__(self, volume, width=640, height=480, camera=None, sigma_colour=30.0, sigma_space=4.5, depth_cutoff=20.0, overlap=True, window=0,
                 method="icp", colour_weight=0.0, colour_gate=None, weighting=None, reject_dynamic=None):
        import torch
        if method not in ("icp", "field"):
            raise ValueError("method is 'icp' or 'field', got %r" % (method,))
        colour_weight = float(colour_weight)
        if not (colour_weight >= 0.0 and colour_weight < float("inf")):
            raise ValueError("colour_weight must be finite and >= 0, got %r" % (colour_weight,))
        if colour_weight > 0.0 and method != "field":
            raise ValueError("colour_weight needs method='field' (the colour term belongs to field alignment)")
        self.method = method
        # > 0: frames processed with rgb are aligned with the colour term (include/tsdf_amd.h, "colour alignment") from the second on
        self.colour_weight = colour_weight
        self.colour_gate = float(api.COLOUR_GATE if colour_gate is None else colour_gate)
        self.last_colour_error, self.last_colour_inliers = 0.0, 0.0
        self.torch = torch
        self.volume = volume
        self.width, self.height = int(width), int(height)
        self.camera = camera or api.Camera.default_depth_camera()
        k = self.camera.k()          # column-major 3x3: fx = k[0], fy = k[4], cx = k[6], cy = k[7]
        self.icp = api.ICPOdometry(self.width, self.height, float(k[6]), float(k[7]), float(k[0]), float(k[4]))
        if not sigma_colour:
            raise ValueError("tracking needs the bilateral filter (raw one-pixel normals fail the ICP angle gate)")
        self.bilateral = api.BilateralFilter(sigma_colour, sigma_space)
        self.depth_cutoff = float(depth_cutoff)
        self._h = C.c_void_p()
        check(lib.tsdf_tracker_create(volume._h, self.bilateral._h, self.icp._h, self.width, self.height, self.depth_cutoff,
                                      OVERLAP if overlap else 0, C.byref(self._h)))
        import weakref
        volume._dependents = list(getattr(volume, "_dependents", ())) + [weakref.ref(self)]
        m, s = C.c_void_p(), C.c_void_p()
        check(lib.tsdf_tracker_streams(self._h, C.byref(m), C.byref(s)))
        self.stream = torch.cuda.ExternalStream(m.value, device=torch.device("cuda", torch.cuda.current_device()))
        if window:
            self.set_window(window)
        if weighting is not None:
            self.set_weighting(*weighting)
        if reject_dynamic is not None:
            self.set_dynamic_rejection(**dict(reject_dynamic))
        self.frames = 0
        self.last_error, self.last_inliers = 0.0, 0.0
        self.last_T = None          # the last incremental transformation (4x4, metres) as ICPOdometry returned it

    def close(self):
        if lib is not None and getattr(self, "_h", None) is not None and self._h.value:   # (lib is None during interpreter shutdown)
            lib.tsdf_tracker_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def set_window(self, n):
        """Keep only the last `n` frames in the volume (0: every frame, the default): each integrate past the n-th takes the oldest
        kept frame back out (tsdf_tracker_set_window).  Refused on a volume with a weight cap."""
        n = int(n)
        if n < 0 or n > 0xFFFFFFFF:
            raise ValueError("set_window: the window is 0 (off) or a number of frames")
        check(lib.tsdf_tracker_set_window(self._h, n))

    def window(self):
        n = C.c_uint32()
        check(lib.tsdf_tracker_window(self._h, C.byref(n)))
        return int(n.value)

    def set_weighting(self, flags, z_ref=0.0):
        """Integrate every frame with the weights of a standard model (include/tsdf_amd.h, "weighted integration"): `flags` a combination
        of api.WEIGHTS_INVERSE_SQUARE / api.WEIGHTS_COSINE (0: off, the default), `z_ref` in depth units.  Refused together with a window."""
        check(lib.tsdf_tracker_set_weighting(self._h, int(flags), float(z_ref)))

    def weighting(self):
        """(flags, z_ref) of set_weighting; (0, 0.0) when off."""
        f, z = C.c_uint32(), C.c_float()
        check(lib.tsdf_tracker_weighting(self._h, C.byref(f), C.byref(z)))
        return int(f.value), float(z.value)

    def set_dynamic_rejection(self, on=True, **params):
        """Keep what moves out of the fusion (include/tsdf_amd.h, "the tracked loop", tsdf_tracker_set_dynamic_rejection): every integrate
        renders the model's depth at its camera, compares the filtered frame with it, clusters the pixels in front of the model and
        fuses the frame with the kept blobs' dilated mask set to 0.  params: tolerance, quadratic, connectivity, depth_step, min_pixels,
        dilate (defaults: api.DIFF_DEFAULTS, starting values).  on=False (or set_dynamic_rejection(None)): off, the default."""
        if not on:
            if params:
                raise ValueError("set_dynamic_rejection: parameters given while turning it off")
            check(lib.tsdf_tracker_set_dynamic_rejection(self._h, None))
            return
        unknown = set(params) - set(api.DIFF_DEFAULTS)
        if unknown:
            raise ValueError("set_dynamic_rejection: unknown parameters %s" % sorted(unknown))
        p = dict(api.DIFF_DEFAULTS, **params)
        r = api._capi.DiffRejection(int(p["tolerance"]), int(p["quadratic"]), int(p["connectivity"]), int(p["depth_step"]), int(p["min_pixels"]),
                                    int(p["dilate"]))
        check(lib.tsdf_tracker_set_dynamic_rejection(self._h, C.byref(r)))

    def dynamic_rejection(self):
        """The parameters of set_dynamic_rejection as a dict, or None when off."""
        on, r = C.c_int(), api._capi.DiffRejection()
        check(lib.tsdf_tracker_dynamic_rejection(self._h, C.byref(on), C.byref(r)))
        return {k: int(getattr(r, k)) for k in api.DIFF_DEFAULTS} if on.value else None

    def last_rejection(self, mask=True):
        """(counts (5,) uint64 by state, kept blobs, mask (height, width) uint8 or None) of the last integrated frame."""
        counts, blobs, ptr = (C.c_uint64 * 5)(), C.c_uint64(), C.c_void_p()
        check(lib.tsdf_tracker_last_rejection(self._h, C.byref(counts), C.byref(blobs), C.byref(ptr)))
        m = None
        if mask:
            m = np.empty((self.height, self.width), np.uint8)
            check(lib.tsdf_device_download(m.ctypes.data, ptr, m.nbytes))
        return np.array(list(counts), np.uint64), int(blobs.value), m

    def pose(self):
        """Current camera pose, 4x4 float64 (camera -> world, millimetres)."""
        return self.camera.pose().astype(np.float64).reshape(4, 4).T.copy()

    def process_device(self, depth_ptr, initial_pose=None, rgb_ptr=None):
        """One frame (uint16 millimetres on the device; it must stay valid until the call returns ... and until the frame has been
        filtered: synchronize() or the next call).  The first frame is placed at `initial_pose` (4x4, camera -> world, mm; default:
        the camera's current pose) and only integrated.  `rgb_ptr` (device, 3 * width * height uint8 registered to the depth
        image, valid until the frame has been integrated): the frame is integrated with its colour (the volume must have colour
        enabled).  Returns the pose used for the frame."""
        check(lib.tsdf_tracker_filter(self._h, C.c_void_p(int(depth_ptr))))
        if self.frames == 0:
            if initial_pose is not None:
                self.camera.set_pose_rows(np.asarray(initial_pose, np.float64))
        elif self.method == "field":
            Tc = np.ascontiguousarray(self.pose().T.reshape(-1))     # column-major double: the previous pose is the prediction
            kinv = np.ascontiguousarray(self.camera.kinv(), np.float32).reshape(-1)
            if self.colour_weight > 0.0 and rgb_ptr is not None:
                res2, inl2 = np.zeros(2, np.float32), np.zeros(2, np.float32)
                check(lib.tsdf_tracker_align_field_colour(self._h, kinv.ctypes.data, C.c_void_p(int(rgb_ptr)) if rgb_ptr else None, self.colour_gate,
                                                          self.colour_weight, Tc.ctypes.data, res2.ctypes.data, inl2.ctypes.data))
                self.last_error, self.last_inliers = float(res2[0]), float(inl2[0])
                self.last_colour_error, self.last_colour_inliers = float(res2[1]), float(inl2[1])   # sum of e^2, colour inliers
            else:
                res, inl = C.c_float(), C.c_float()
                check(lib.tsdf_tracker_align_field(self._h, kinv.ctypes.data, Tc.ctypes.data, C.byref(res), C.byref(inl)))
                self.last_error, self.last_inliers = float(res.value), float(inl.value)   # sum of squared distances (mm^2), inliers
                self.last_colour_error, self.last_colour_inliers = 0.0, 0.0               # (a frame without rgb, or weight 0: no colour term)
            self.last_T = None
            self.camera.set_pose_rows(Tc.reshape(4, 4).T.copy())
        else:
            prev = _matrices(self.camera)
            Tc = np.ascontiguousarray(np.eye(4).T.reshape(-1))      # column-major double, identity start
            err, inl = C.c_float(), C.c_float()
            check(lib.tsdf_tracker_align(self._h, C.byref(prev), Tc.ctypes.data, C.byref(err), C.byref(inl)))
            T = Tc.reshape(4, 4).T.copy()                            # current camera -> previous camera, metres
            self.last_T = T.copy()
            T[:3, 3] *= 1000.0
            self.last_error, self.last_inliers = float(err.value), float(inl.value)
            self.icp.last_error, self.icp.last_inliers = self.last_error, self.last_inliers
            self.camera.set_pose_rows(self.pose() @ T)
        cam = _matrices(self.camera)
        if rgb_ptr is None:
            check(lib.tsdf_tracker_integrate(self._h, C.byref(cam)))
        else:
            check(lib.tsdf_tracker_integrate_colour(self._h, C.byref(cam), C.c_void_p(int(rgb_ptr)) if rgb_ptr else None))
        self.frames += 1
        return self.pose()

    def synchronize(self):
        check(lib.tsdf_tracker_synchronize(self._h))

    def last_icp_inputs(self):
        """(model depth, filtered current depth) of the last tracked frame as host uint16 arrays: the pair ICPOdometry was
        given, for checking its answer elsewhere."""
        self.synchronize()
        m, f = C.c_void_p(), C.c_void_p()
        check(lib.tsdf_tracker_buffers(self._h, C.byref(m), C.byref(f)))
        n = self.width * self.height
        out = []
        for p in (m, f):
            a = np.empty(n, np.uint16)
            check(lib.tsdf_device_download(a.ctypes.data, p, n * 2))
            out.append(a)
        return tuple(out)

    def process(self, depth, initial_pose=None, rgb=None):
        """Host depth image (uint16 mm); `rgb`: its host colour image (uint8, width * height * 3), or None."""
        d = self.torch.from_numpy(np.ascontiguousarray(depth, dtype=np.uint16).reshape(-1).view(np.int16)).cuda()
        c = None
        if rgb is not None:
            c = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1)
            if c.size != 3 * self.width * self.height:
                raise ValueError("expected %d colour bytes, got %d" % (3 * self.width * self.height, c.size))
            c = self.torch.from_numpy(c).cuda()
        self.torch.cuda.current_stream().synchronize()
        pose = self.process_device(d.data_ptr(), initial_pose, rgb_ptr=c.data_ptr() if c is not None else None)
        self.synchronize()           # (the temporary upload is released on return)
        return pose
