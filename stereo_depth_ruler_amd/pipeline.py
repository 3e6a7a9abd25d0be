"""Device pipelines for the reference's two per-frame loops, built from the engine's C ABI:

* ``LiveLoop`` -- stereo_vision/src/stereo_displayer.cpp:145-185 (``show_disparity_overlay``):
  side-by-side BGR frame -> split + StereoRectifier::rectify -> StereoDisparity::computeDisparity
  (BGR2GRAY, INTER_AREA 0.5x, left 3WAY + right matcher, WLS, /16) -> computeDepth, and with
  ``display=True`` the loop's display outputs (show_depthMap, show_disparityMap, the JET overlay
  on the half-size rectified left view; :164-173), frames of a batch in order through the EMAs.
  With ``ruler=`` the loop's two-point measurement (onMouseMeasure, :24-63) runs on the same stream.
* ``CloudEmit`` -- point_cloud/src/pcd_write.cpp:81-130 (``save_and_display_pointcloud``):
  side-by-side BGR frame -> split -> BGR2GRAY -> StereoSGBM::compute -> /16 ->
  reprojectImageTo3D(handleMissing) -> convertCVMatToPCL(left) -> VoxelGrid.

Both take device-resident frames (torch uint8 (F, H, 2W, 3)), enqueue on the given stream and keep
all scratch per instance, so several instances can keep frames in flight on separate streams.
The CPU is never used for pixels; a missing libsdr.so raises.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import FUSE_MEAN, check, lib
from .display import Display
from .ruler import Ruler
from .sgbm import MODE_SGBM_3WAY, StereoSGBM, _Q, createRightMatcher, set_handle_stream, torch
from .ximgproc import createDisparityWLSFilter


def _vp(x):
    return ctypes.c_void_p(x)


class LiveLoop:
    """The reference app's per-frame loop on one device (see module docstring)."""

    def __init__(self, rectifier, Q, batch: int, device: int = 0, args=None, display: bool = False,
                 ruler=None):
        """ruler (opt-in): a Ruler, or a dict of Ruler keywords (Q and min_disp = minDisparity - 1
        are filled in): the loop then also keeps the WLS confidence map and gains measure()."""
        self.rect = rectifier
        self.W, self.H = rectifier.W, rectifier.H
        self.Q = np.asarray(Q, np.float64)
        self.batch = int(batch)
        self.dev = torch.device("cuda", device)
        args = args or (0, 80, 5, 8 * 5 * 5 * 3, 32 * 5 * 5 * 3, 1, 63, 12, 200, 2, MODE_SGBM_3WAY)
        self.left = StereoSGBM.create(*args, device=device)          # stereo_disparity.cpp:5-9
        self.right = createRightMatcher(self.left)                     # :10
        self.wls = createDisparityWLSFilter(self.left)                 # :11
        self.wls.setLambda(8000.0)                                     # :12
        self.wls.setSigmaColor(1.1)                                    # :13
        h2, w2 = self.H // 2, self.W // 2
        self.h2, self.w2 = h2, w2
        z = dict(device=self.dev)
        self.small_l = torch.empty((batch, h2, w2), dtype=torch.uint8, **z)
        self.small_r = torch.empty_like(self.small_l)
        self.disp = torch.empty((batch, h2, w2), dtype=torch.float32, **z)     # computeDisparity()
        self.filtered = torch.empty((batch, h2, w2), dtype=torch.int16, **z)
        self.depth = torch.empty((batch, h2, w2, 3), dtype=torch.float32, **z)  # computeDepth()
        self.display = Display(device) if display else None
        self.ruler, self.conf = None, None
        if ruler is not None:
            if not isinstance(ruler, Ruler):
                kw = dict(ruler)
                kw.setdefault("min_disp", float(self.left.getMinDisparity() - 1))
                kw.setdefault("device", device)
                ruler = Ruler(self.Q, **kw)
            self.ruler = ruler
            self.conf = torch.empty((batch, h2, w2), dtype=torch.float32, **z)  # getConfidenceMap()
        if display:
            self.left_rect = torch.empty((batch, self.H, self.W, 3), dtype=torch.uint8, **z)
            self.vis = torch.empty((batch, h2, w2), dtype=torch.uint8, **z)           # show_disparityMap
            self.depth_vis = torch.empty((batch, h2, w2, 3), dtype=torch.uint8, **z)  # show_depthMap
            self.overlay = torch.empty((batch, h2, w2, 3), dtype=torch.uint8, **z)    # overlay

    def matcher(self):
        return self.left

    def enqueue(self, sbs, stream, ingest_events=None):
        """sbs: uint8 (batch, H, 2W, 3) on the device; everything runs on `stream`.
        ingest_events (optional): two torch.cuda.Event recorded on `stream` around the ingest
        (split + rectify + gray + INTER_AREA), for per-kernel timing."""
        s = _vp(stream.cuda_stream)
        L = lib()
        check(L.sdr_rectifier_set_stream(self.rect._h, s))
        disp_on = self.display is not None
        if ingest_events:
            ingest_events[0].record(stream)
        check(L.sdr_rectify_sbs_device(self.rect._h, sbs.data_ptr(), self.W * 6, self.W * 6 * self.H,
                                       self.batch, self.left_rect.data_ptr() if disp_on else None, None,
                                       self.small_l.data_ptr(), self.small_r.data_ptr()))
        if ingest_events:
            ingest_events[1].record(stream)
        set_handle_stream(self.left._h, self.left._device, stream)
        # computeDisparity + computeDepth: reprojectImageTo3D(half-res disparity, full-res Q)
        # (stereo_disparity.cpp:76-80), fused into the WLS filter's epilogue
        check(L.sdr_stereo_class_depth_device(self.left._h, self.right._h, self.wls._h,
                                              self.small_l.data_ptr(), self.small_r.data_ptr(),
                                              self.w2, self.h2, self.batch, self.disp.data_ptr(),
                                              self.filtered.data_ptr(),
                                              self.conf.data_ptr() if self.conf is not None else None,
                                              _Q(self.Q),
                                              self.depth.data_ptr()))
        if disp_on:  # stereo_displayer.cpp:164-173
            d, F, w2, h2 = self.display, self.batch, self.w2, self.h2
            check(L.sdr_display_set_stream(d._h, s))
            check(L.sdr_show_depth_map_device(d._h, self.depth.data_ptr(), w2, h2, 3, F, None, None,
                                              self.depth_vis.data_ptr(), None))
            check(L.sdr_show_disparity_map_device(d._h, self.disp.data_ptr(), w2, h2, w2, w2 * h2, F,
                                                  self.left.getNumDisparities(), self.vis.data_ptr()))
            check(L.sdr_disparity_overlay_device(d._h, self.vis.data_ptr(), self.left_rect.data_ptr(),
                                                 self.W * 3, self.W * 3 * self.H, w2, h2, F, None, None,
                                                 self.overlay.data_ptr()))
        return self.filtered

    def measure(self, segments, stream, profile_cap=None, profile_out=None):
        """onMouseMeasure (stereo_displayer.cpp:24-63) on the frames the last enqueue left in
        `disp`, with their confidence map, enqueued on `stream` (the stream of that enqueue: no
        synchronise in between, host segments included).  Returns Ruler.measure_device's
        (records, profile) tensors; profile_cap / profile_out as there."""
        if self.ruler is None:
            raise RuntimeError("LiveLoop was built without ruler=")
        return self.ruler.measure_device(self.disp, segments, conf=self.conf, stream=stream,
                                         profile_cap=profile_cap, profile_out=profile_out)

    def fit_plane(self, regions, stream, iterations: int = 3, inlier_px: float = 1.0, min_inliers: int = 16):
        """Ruler.fit_plane_device on the frames the last enqueue left in `disp`, with their
        confidence map, enqueued on `stream` like measure(): the (K, 128) records tensor."""
        if self.ruler is None:
            raise RuntimeError("LiveLoop was built without ruler=")
        return self.ruler.fit_plane_device(self.disp, regions, conf=self.conf, iterations=iterations,
                                           inlier_px=inlier_px, min_inliers=min_inliers, stream=stream)

    def find_planes(self, region, stream, max_planes: int = 4, hypotheses: int = 256, seed: int = 0,
                    iterations: int = 3, inlier_px: float = 1.0, min_inliers: int = 64, labels: bool = False,
                    labels_out=None):
        """Ruler.find_planes_device on the frames the last enqueue left in `disp`, with their
        confidence map, enqueued on `stream` like fit_plane(): the (planes, count, rounds, labels)
        tensors.  region: (frame, x0, y0, x1, y1) / (x0, y0, x1, y1), None: all of frame 0."""
        if self.ruler is None:
            raise RuntimeError("LiveLoop was built without ruler=")
        return self.ruler.find_planes_device(self.disp, region, conf=self.conf, max_planes=max_planes,
                                             hypotheses=hypotheses, seed=seed, iterations=iterations,
                                             inlier_px=inlier_px, min_inliers=min_inliers, labels=labels,
                                             stream=stream, labels_out=labels_out)

    def plane_distance(self, planes, points, stream):
        """Ruler.plane_distance_device on the same frames: `planes` the tensor fit_plane returned
        (or host records), the (K, 32) distances tensor, no synchronise in between."""
        if self.ruler is None:
            raise RuntimeError("LiveLoop was built without ruler=")
        return self.ruler.plane_distance_device(self.disp, planes, points, conf=self.conf, stream=stream)

    def relief(self, planes, regions, stream, labels=None, quantiles=(50, 500, 950), band: float = 0.0):
        """Ruler.relief_device on the same frames: `planes` (and `labels`) the tensors find_planes or
        fit_plane returned (or host records), regions rows {frame, x0, y0, x1, y1, plane, label}: the
        (K, 128) relief records tensor, no synchronise in between.  A label map of one frame (what
        find_planes writes) serves a batch of one frame; a batch takes a (batch, H, W) map."""
        if self.ruler is None:
            raise RuntimeError("LiveLoop was built without ruler=")
        return self.ruler.relief_device(self.disp, planes, regions, labels=labels, conf=self.conf,
                                        quantiles=quantiles, band=band, stream=stream)

    def footprint(self, planes, regions, stream, labels=None, cell: float = 4.0, grid: int = 512, support: int = 4,
                  h_range=None):
        """Ruler.footprint_device on the same frames, chained like relief(): the (K, 256) footprint
        records tensor, no synchronise in between."""
        if self.ruler is None:
            raise RuntimeError("LiveLoop was built without ruler=")
        return self.ruler.footprint_device(self.disp, planes, regions, labels=labels, conf=self.conf, cell=cell,
                                           grid=grid, support=support, h_range=h_range, stream=stream)

    def find_objects(self, planes, region, stream, labels=None, h_range=(10.0, 1048576.0), max_diff: float = 1.0,
                     connectivity: int = 8, min_pixels: int = 64, max_objects: int = 16, labels_out=True):
        """Ruler.find_objects_device on the same frames, chained like relief(): the (objects, scan,
        labels) tensors, no synchronise in between; the labels feed relief() and footprint()."""
        if self.ruler is None:
            raise RuntimeError("LiveLoop was built without ruler=")
        return self.ruler.find_objects_device(self.disp, planes, region, labels=labels, conf=self.conf,
                                              h_range=h_range, max_diff=max_diff, connectivity=connectivity,
                                              min_pixels=min_pixels, max_objects=max_objects, stream=stream,
                                              labels_out=labels_out)

    def clearance(self, planes, pairs, stream, labels, h_range=None):
        """Ruler.clearance_device on the same frames, chained like relief(): `labels` the tensor
        find_objects returned, pairs rows {frame, x0, y0, x1, y1, plane, label_a, label_b}: the
        (K, 128) clearance records tensor, no synchronise in between."""
        if self.ruler is None:
            raise RuntimeError("LiveLoop was built without ruler=")
        return self.ruler.clearance_device(self.disp, planes, pairs, labels, conf=self.conf, h_range=h_range,
                                           stream=stream)

    def fuse(self, stream, tol: float = 1.0, min_count: int = 2, mode: int = FUSE_MEAN, support: bool = False,
             spread: bool = False):
        """Ruler.fuse_device on the `batch` frames the last enqueue left in `disp`, with their
        confidence maps, enqueued on `stream` like measure(), no synchronise in between: one map of a
        still scene's last frames (the reference measures after the `f` freeze,
        stereo_displayer.cpp:191-196), as the (fused, record[, support][, spread]) tensors.  Pass the
        result to `loop.ruler.<call>_device(fused, ..., conf=None, stream=stream)`: the confidence
        gate has been applied frame by frame, and the per-frame `conf` tensor must not be passed
        again (it has `batch` frames, the fused map one).  The other methods keep reading `disp`."""
        if self.ruler is None:
            raise RuntimeError("LiveLoop was built without ruler=")
        return self.ruler.fuse_device(self.disp, conf=self.conf, tol=tol, min_count=min_count, mode=mode,
                                      support=support, spread=spread, stream=stream)

    def close(self):
        for o in (self.left, self.right, self.wls, self.display):
            if o is not None:
                o.close()


class CloudEmit:
    """pcd_write.cpp's single-frame path as a batched device pipeline (see module docstring)."""

    def __init__(self, W, H, args, batch: int, Q, leaf=0.005, device: int = 0):
        self.W, self.H, self.batch = int(W), int(H), int(batch)
        self.Q = np.asarray(Q, np.float64)
        self.leaf = float(leaf)
        self.dev = torch.device("cuda", device)
        self.m = StereoSGBM.create(*args, device=device)
        z = dict(device=self.dev)
        self.gray_l = torch.empty((batch, H, W), dtype=torch.uint8, **z)
        self.gray_r = torch.empty_like(self.gray_l)
        self.disp = torch.empty((batch, H, W), dtype=torch.int16, **z)
        self.xyz = torch.empty((batch, H, W, 3), dtype=torch.float32, **z)
        self.points = torch.empty((batch, H * W, 4), dtype=torch.float32, **z)
        self.filtered = torch.empty((batch, H * W, 4), dtype=torch.float32, **z)
        self.counts = [0] * batch
        self.passthrough = [False] * batch

    def matcher(self):
        return self.m

    def enqueue(self, sbs, stream, voxel=True):
        """sbs: uint8 (batch, H, 2W, 3) on the device.  The voxel grid returns host counts, so that
        stage synchronises `stream` once per frame; voxel=False leaves it to voxel(), which a
        caller running several pipelines can call after enqueueing the next one's frames, so the
        GPU has work queued while the host waits."""
        s = _vp(stream.cuda_stream)
        L = lib()
        W, H, F = self.W, self.H, self.batch
        row = 2 * W * 3
        # frame(Rect(0, 0, W, H)) / frame(Rect(W, 0, W, H)) -> cvtColor(BGR2GRAY)  (pcd_write.cpp:83-89)
        check(L.sdr_bgr2gray_device(sbs.data_ptr(), W, H, row, self.gray_l.data_ptr(), W, F, s))
        check(L.sdr_bgr2gray_device(sbs.data_ptr() + W * 3, W, H, row, self.gray_r.data_ptr(), W, F, s))
        # sgbm->compute -> convertTo(1/16) -> reprojectImageTo3D(handleMissing)  (:111-116)
        set_handle_stream(self.m._h, self.m._device, stream)
        check(L.sdr_sgbm_compute_reproject_device(self.m._h, self.gray_l.data_ptr(), self.gray_r.data_ptr(),
                                                  W, H, W, W * H, F, self.disp.data_ptr(), _Q(self.Q), 1,
                                                  self.xyz.data_ptr()))
        # convertCVMatToPCL(pointCloud_CV, left)  (:119)
        check(L.sdr_xyz_to_cloud_device(self.xyz.data_ptr(), sbs.data_ptr(), row, row * H, W, H, F,
                                        self.points.data_ptr(), s))
        if voxel:
            self.voxel(stream)
        return self.disp

    def voxel(self, stream):
        """VoxelGrid 5 mm (:122-130) of the frames the last enqueue left in `points`, on the stream
        that enqueued them (synchronous: the counts are host values)."""
        s = _vp(stream.cuda_stream)
        L = lib()
        W, H = self.W, self.H
        cnt, pt = ctypes.c_int(), ctypes.c_int()
        for f in range(self.batch):
            check(L.sdr_voxel_grid_device(self.points[f].data_ptr(), W * H, self.leaf, self.leaf,
                                          self.leaf, self.filtered[f].data_ptr(), ctypes.byref(cnt),
                                          ctypes.byref(pt), s))
            self.counts[f], self.passthrough[f] = cnt.value, bool(pt.value)

    def close(self):
        self.m.close()
