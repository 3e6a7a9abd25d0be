"""The ruler: the reference's two-point measurement (StereoDisplayer::onMouseMeasure,
stereo_vision/src/stereo_displayer.cpp:24-63) and its CSV log (save_csvFile, :74-102) on the HIP
engine (csrc/sdr_ruler.hip; the plane fit, the plane search and the point query: csrc/sdr_plane.hip;
the definition is in include/sdr/sdr.h).

* ``Ruler.measure_xyz(depth_map, segments)`` is the reference's own: the computeDepth map read at
  the two pixels, ``cv::norm`` of the difference.
* ``Ruler.measure(disparity, segments, conf=None)`` measures from the disparity map: each endpoint
  is the lower median of the valid disparities in a (2r+1)^2 window, reprojected through Q; with
  ``profile=True`` every pixel of the segment is sampled and the record reports the depth profile
  (valid samples, longest hole, Z range, largest Z step), which shows whether both endpoints lie on
  one surface.  ``radius=0, min_count=1`` equals the reference's lookup on finite pixels.
* ``Ruler.fit_plane(disparity, regions)`` fits a plane to the disparities of each rectangle (exact
  integer moments, a coarse-to-fine inlier refit) and ``Ruler.plane_distance(disparity, planes,
  points)`` gives the signed distance of sampled points to those planes, positive towards the
  camera: heights above a table, steps, distances from a wall.
* ``Ruler.relief(disparity, planes, regions, labels=None)`` measures a whole surface against a plane:
  the heights of a rectangle's pixels (optionally only those with one label of ``find_planes``' map)
  above a plane record, as counts, extremes, exact means and order statistics (a radix selection on
  the device, csrc/sdr_relief.hip, on the region rule of csrc/sdr_region.hpp): the height of a box
  above the table, the depth of a step.
* ``Ruler.footprint(disparity, planes, regions, labels=None)`` measures a surface IN a plane: the
  pixels of a rectangle (optionally one label, optionally a band of heights) binned on square cells
  of the plane, stray cells dropped by a 3 x 3 support rule, and the minimum-area bounding rectangle
  over 90 whole-degree directions (csrc/sdr_footprint.hip): the length and width of a box on a
  table at whatever angle it lies, with its four 3-D corners.
* ``Ruler.find_objects(disparity, planes, region, labels=None)`` finds the things that stand on a
  plane: the connected sets of a rectangle's pixels in a band of heights above a plane record whose
  disparities step by at most ``max_diff`` from pixel to pixel (tiles labelled in LDS, a lock-free
  union-find across tile borders, csrc/sdr_objects.hip), the largest first, as records (pixels,
  bounding box, centroid sums, height sums and extremes) and as a label map that ``relief`` and
  ``footprint`` take: a mug, a ball or a box seen corner-on gets a label though it is no plane.
* ``Ruler.clearance(disparity, planes, pairs, labels)`` measures the gap between two of those things:
  the smallest 3-D distance between a point of one label and a point of another, each pixel's point
  the ruler's sample taken over its own label's pixels (``radius``, ``min_count``), found by all pairs
  block against block with an exact prune on the blocks' bounds (csrc/sdr_clearance.hip), with the two
  pixels and points where it is attained and its parts along and across the floor's normal.
* ``Ruler.fuse(stack)`` makes one map of a still scene's last frames (the frames before the
  reference's ``f`` freeze): per pixel the valid values within ``tol`` of their median, averaged, and
  a hole where the frames are too few or disagree (csrc/sdr_fuse.hip).  Every call above takes the
  result as its disparity.
* ``Ruler.find_planes(disparity, region=None)`` finds a region's dominant planes without a prior (a
  box on a table in front of a wall): rounds of seeded three-point hypotheses scored in exact
  integer arithmetic on the pixels no earlier plane has claimed, the winner refitted as
  ``fit_plane`` does; the records feed ``plane_distance``, a label map says which pixel lies on
  which plane.

A segment is ``(frame, x0, y0, x1, y1)`` (or ``(x0, y0, x1, y1)`` on frame 0), in pixels of the
map.  The walk rounds ties towards +x / +y: from P1 to P0 it visits the same pixels in reverse, so
a record does not depend on the direction (but for p0 / p1), while the walk of a mirrored segment is
not the mirror image.

numpy inputs go through the synchronous host ABI; torch CUDA tensors stay on the device.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

from ._lib import (DISP_F32, DISP_S16, FUSE_MEAN, FUSE_MEDIAN, ClearanceParams, FootprintParams, FuseParams, ObjectParams,
                   PlaneParams, PlaneSearchParams, ReliefParams, RulerParams, SDRError, check, lib)
from .sgbm import _Q, _is_cuda, torch

MEASUREMENT_DTYPE = np.dtype([
    ("p0", "<f4", (3,)), ("p1", "<f4", (3,)), ("d0", "<f4"), ("d1", "<f4"), ("distance", "<f8"),
    ("n0", "<i4"), ("n1", "<i4"), ("path_samples", "<i4"), ("path_valid", "<i4"),
    ("max_gap", "<i4"), ("z_min", "<f4"), ("z_max", "<f4"), ("max_dz", "<f4"), ("flags", "<u4"),
    ("reserved", "<i4")])
assert MEASUREMENT_DTYPE.itemsize == 80

# sdr_measurement.flags (SDR_MEAS_*)
P0_VALID, P1_VALID, OUT_OF_RANGE, PROFILE_TRUNCATED = 1, 2, 4, 8

PLANE_DTYPE = np.dtype([
    ("coef", "<f8", (3,)), ("normal", "<f8", (3,)), ("offset", "<f8"), ("centroid", "<f8", (3,)),
    ("rms_px", "<f8"), ("max_abs_px", "<f4"), ("x0", "<i4"), ("y0", "<i4"), ("frame", "<i4"),
    ("area", "<i4"), ("n_valid", "<i4"), ("n_inliers", "<i4"), ("fits", "<i4"), ("flags", "<u4"),
    ("reserved", "<i4")])
assert PLANE_DTYPE.itemsize == 128
PLANE_DISTANCE_DTYPE = np.dtype([
    ("p", "<f4", (3,)), ("d", "<f4"), ("distance", "<f8"), ("n", "<i4"), ("flags", "<u4")])
assert PLANE_DISTANCE_DTYPE.itemsize == 32

# sdr_plane.flags (SDR_PLANE_*) and sdr_plane_distance.flags (SDR_PDIST_*)
PLANE_OK, PLANE_DEGENERATE, PLANE_NONFINITE, PLANE_OUT_OF_RANGE = 1, 2, 4, 8
PDIST_VALID, PDIST_OUT_OF_RANGE, PDIST_NO_PLANE = 1, 2, 4

# sdr_plane_search_round and its stop codes (SDR_SEARCH_*)
PLANE_SEARCH_ROUND_DTYPE = np.dtype([("hypothesis", "<i4"), ("score", "<i4"), ("voids", "<i4"), ("stop", "<u4")])
assert PLANE_SEARCH_ROUND_DTYPE.itemsize == 16
(SEARCH_RAN, SEARCH_NO_HYPOTHESIS, SEARCH_LOW_SCORE, SEARCH_REFIT_DEGENERATE, SEARCH_FEW_INLIERS,
 SEARCH_NOT_RUN) = range(6)


# sdr_relief and its flags (SDR_RELIEF_*)
RELIEF_DTYPE = np.dtype([
    ("q", "<f4", (8,)), ("h_min", "<f4"), ("h_max", "<f4"), ("mean", "<f8"), ("mean_above", "<f8"),
    ("sum256", "<i8"), ("sum256_above", "<i8"), ("area", "<i4"), ("n_masked", "<i4"), ("n_valid", "<i4"),
    ("n", "<i4"), ("n_above", "<i4"), ("n_below", "<i4"), ("n_rejected", "<i4"), ("frame", "<i4"),
    ("plane", "<i4"), ("label", "<i4"), ("flags", "<u4"), ("reserved", "<i4", (3,))])
assert RELIEF_DTYPE.itemsize == 128
RELIEF_VALID, RELIEF_OUT_OF_RANGE, RELIEF_NO_PLANE, RELIEF_EMPTY = 1, 2, 4, 8


# sdr_footprint and its flags (SDR_FOOTPRINT_*)
FOOTPRINT_DTYPE = np.dtype([
    ("side", "<f8", (2,)), ("fill", "<f8"), ("corner", "<f8", (4, 3)), ("basis_s", "<f8", (3,)),
    ("basis_t", "<f8", (3,)), ("i0", "<i8"), ("j0", "<i8"), ("angle_deg", "<i4"), ("span_s", "<i4"),
    ("span_t", "<i4"), ("area", "<i4"), ("n_masked", "<i4"), ("n_valid", "<i4"), ("n", "<i4"),
    ("n_outside", "<i4"), ("n_cells_raw", "<i4"), ("n_cells", "<i4"), ("frame", "<i4"), ("plane", "<i4"),
    ("label", "<i4"), ("flags", "<u4"), ("reserved", "<i4", (4,))])
assert FOOTPRINT_DTYPE.itemsize == 256
FOOTPRINT_VALID, FOOTPRINT_OUT_OF_RANGE, FOOTPRINT_NO_PLANE, FOOTPRINT_EMPTY, FOOTPRINT_CLIPPED = 1, 2, 4, 8, 16


# sdr_object, sdr_object_scan and their flags (SDR_OBJECT_*, SDR_OBJECTS_*)
OBJECT_DTYPE = np.dtype([
    ("n", "<i4"), ("root", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("sum_x", "<i8"),
    ("sum_y", "<i8"), ("sum256", "<i8"), ("h_min", "<f4"), ("h_max", "<f4"), ("flags", "<u4"), ("reserved", "<i4")])
assert OBJECT_DTYPE.itemsize == 64
OBJECT_SCAN_DTYPE = np.dtype([
    ("flags", "<u4"), ("area", "<i4"), ("n_masked", "<i4"), ("n_valid", "<i4"), ("n", "<i4"),
    ("n_components", "<i4"), ("n_kept", "<i4"), ("count", "<i4"), ("largest_dropped", "<i4"), ("frame", "<i4"),
    ("plane", "<i4"), ("label", "<i4"), ("reserved", "<i4", (4,))])
assert OBJECT_SCAN_DTYPE.itemsize == 64
OBJECTS_VALID, OBJECTS_OUT_OF_RANGE, OBJECTS_NO_PLANE, OBJECTS_EMPTY, OBJECTS_TRUNCATED = 1, 2, 4, 8, 16
OBJECT_VALID, OBJECT_CUT = 1, 2


# sdr_clearance and its flags (SDR_CLEARANCE_*)
CLEARANCE_DTYPE = np.dtype([
    ("distance", "<f8"), ("along", "<f8"), ("across", "<f8"), ("p_a", "<f4", (3,)), ("p_b", "<f4", (3,)),
    ("d_a", "<f4"), ("d_b", "<f4"), ("xa", "<i4"), ("ya", "<i4"), ("xb", "<i4"), ("yb", "<i4"), ("area", "<i4"),
    ("n_a", "<i4"), ("n_b", "<i4"), ("m_a", "<i4"), ("m_b", "<i4"), ("frame", "<i4"), ("plane", "<i4"),
    ("label_a", "<i4"), ("label_b", "<i4"), ("flags", "<u4"), ("reserved", "<i4", (4,))])
assert CLEARANCE_DTYPE.itemsize == 128
CLEARANCE_VALID, CLEARANCE_OUT_OF_RANGE, CLEARANCE_NO_PLANE, CLEARANCE_EMPTY = 1, 2, 4, 8


# sdr_fusion: the record of a fused stack (its modes: FUSE_MEAN, FUSE_MEDIAN)
FUSION_DTYPE = np.dtype([
    ("frames", "<i4"), ("width", "<i4"), ("height", "<i4"), ("mode", "<i4"), ("n_fused", "<i4"), ("n_empty", "<i4"),
    ("n_sparse", "<i4"), ("n_unstable", "<i4"), ("n_filled", "<i4"), ("n_replaced", "<i4"), ("sum_support", "<i8"),
    ("n_disagree", "<i8"), ("reserved", "<i8")])
assert FUSION_DTYPE.itemsize == 64


def footprint_length_width(records):
    """(length, width) = (max, min) of each FOOTPRINT_DTYPE record's sides (NaN without a rectangle)."""
    side = np.asarray(records)["side"]
    return side.max(axis=-1), side.min(axis=-1)


def as_relief_queries(regions) -> np.ndarray:
    """(K, 8) int32 {frame, x0, y0, x1, y1, plane, label, 0} from rows of 7
    {frame, x0, y0, x1, y1, plane, label}, of 6 (label -1) or of 5 (plane 0, label -1) / one tuple."""
    r = np.asarray(regions)
    if r.size == 0:
        return np.zeros((0, 8), np.int32)
    if r.ndim == 1:
        r = r[None, :]
    if r.ndim != 2 or r.shape[1] not in (5, 6, 7):
        raise SDRError(-1, "regions must be (K, 7) {frame, x0, y0, x1, y1, plane, label}, (K, 6) or (K, 5)")
    if r.dtype.kind not in "iu":
        raise SDRError(-1, "regions must be integers")
    q = np.zeros((r.shape[0], 8), np.int32)
    q[:, 6] = -1
    q[:, :r.shape[1]] = r
    return q


def as_clearance_queries(pairs) -> np.ndarray:
    """(K, 8) int32 {frame, x0, y0, x1, y1, plane, label_a, label_b} from rows of 8 / one tuple."""
    r = np.asarray(pairs)
    if r.size == 0:
        return np.zeros((0, 8), np.int32)
    if r.ndim == 1:
        r = r[None, :]
    if r.ndim != 2 or r.shape[1] != 8:
        raise SDRError(-1, "pairs must be (K, 8) {frame, x0, y0, x1, y1, plane, label_a, label_b}")
    if r.dtype.kind not in "iu":
        raise SDRError(-1, "pairs must be integers")
    return np.ascontiguousarray(r, dtype=np.int32)


def as_queries(points) -> np.ndarray:
    """(K, 4) int32 {frame, x, y, plane} from (K, 4) / (K, 3) {x, y, plane} on frame 0 / one tuple."""
    q = np.asarray(points)
    if q.size == 0:
        return np.zeros((0, 4), np.int32)
    if q.ndim == 1:
        q = q[None, :]
    if q.ndim != 2 or q.shape[1] not in (3, 4):
        raise SDRError(-1, "points must be (K, 4) {frame, x, y, plane} or (K, 3) {x, y, plane}")
    if q.shape[1] == 3:
        q = np.concatenate([np.zeros((q.shape[0], 1), q.dtype), q], axis=1)
    return np.ascontiguousarray(q, dtype=np.int32)


def plane_angle_deg(a, b) -> float:
    """Angle between the normals of two PLANE_DTYPE records, in degrees (a host dot product)."""
    c = float(np.dot(np.asarray(a["normal"], np.float64), np.asarray(b["normal"], np.float64)))
    return float(np.degrees(np.arccos(min(1.0, abs(c)))))


def as_segments(segments) -> np.ndarray:
    """(K, 5) int32 {frame, x0, y0, x1, y1} from (K, 5) / (K, 4) / a single 4- or 5-tuple."""
    s = np.asarray(segments)
    if s.size == 0:
        return np.zeros((0, 5), np.int32)
    if s.ndim == 1:
        s = s[None, :]
    if s.ndim != 2 or s.shape[1] not in (4, 5):
        raise SDRError(-1, "segments must be (K, 5) {frame, x0, y0, x1, y1} or (K, 4) {x0, y0, x1, y1}")
    if s.shape[1] == 4:
        s = np.concatenate([np.zeros((s.shape[0], 1), s.dtype), s], axis=1)
    return np.ascontiguousarray(s, dtype=np.int32)


# the query rows of the device calls: (host converter, name in messages, int32 columns)
_RECTANGLES = (as_segments, "regions", 5)
_POINTS = (as_queries, "points", 4)
_REGIONS = (as_relief_queries, "regions", 8)
_PAIRS = (as_clearance_queries, "pairs", 8)
_NO_LABELS = object()  # an entry that takes no label map


def _frames3(a, what):
    """a as (F, H, W)."""
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise SDRError(-1, f"{what} must be (H, W) or (F, H, W)")
    return a


def _on_device(index: int):
    """The host-pointer calls run on the thread's current device: make it `index` for the call."""
    if torch is not None and torch.cuda.is_available():
        return torch.cuda.device(index)
    return contextlib.nullcontext()


def _host_planes(planes) -> np.ndarray:
    """Plane records (PLANE_DTYPE, or a tensor of them) as a host PLANE_DTYPE array."""
    if _is_cuda(planes):
        planes = planes.cpu().numpy()
    return np.ascontiguousarray(planes).reshape(-1).view(np.uint8).view(PLANE_DTYPE)


def _device_planes(planes, dev):
    """Plane records as a contiguous uint8 tensor (P, 128) on `dev`; None for no record."""
    if _is_cuda(planes):
        if planes.dtype != torch.uint8 or planes.numel() % 128:
            raise SDRError(-5, "device planes must be a uint8 tensor (P, 128)")
        return planes.contiguous()
    host = np.ascontiguousarray(planes).reshape(-1).view(np.uint8).reshape(-1, 128)
    return torch.from_numpy(host.copy()).to(dev) if host.shape[0] else None


def _host_labels(labels, shape):
    """A label map (host or tensor, or None) as a contiguous host uint8 array of `shape` (F, H, W)."""
    if labels is None:
        return None
    if _is_cuda(labels):
        labels = labels.cpu().numpy()
    lab = np.asarray(labels)
    if lab.dtype != np.uint8:
        raise SDRError(-5, "labels must be uint8")
    lab = np.ascontiguousarray(_frames3(lab, "labels"))
    if lab.shape != shape:
        raise SDRError(-1, "labels must have the disparity's shape")
    return lab


def _device_labels(labels, d, dev):
    """A label map (host or tensor, or None) as a contiguous uint8 tensor of d's size on `dev`."""
    if labels is None:
        return None
    lab = labels if _is_cuda(labels) else torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    if lab.dtype != torch.uint8 or lab.numel() != d.numel():
        raise SDRError(-5, "labels must be a uint8 map of the disparity's shape")
    return lab.contiguous()


class _SegmentStaging:
    """Host segments reach the device without a wait on the stream: a ring of page-locked slots,
    each copied from with a non-blocking transfer on the measurement's stream and guarded by an
    event recorded behind that transfer.  A slot is reused only after its event has completed,
    which the host waits for only when `slots` uploads are still in flight."""

    def __init__(self, slots: int = 8, cols: int = 5):
        self._ring = [None] * slots
        self._next = 0
        self._cols = cols

    def upload(self, host: np.ndarray, dev, stream):
        K = host.shape[0]
        if K == 0:
            return torch.empty((0, self._cols), dtype=torch.int32, device=dev)
        i = self._next
        self._next = (i + 1) % len(self._ring)
        slot = self._ring[i]
        if slot is not None:
            slot[1].synchronize()  # the slot's last transfer has left the buffer
        if slot is None or slot[0].shape[0] < K:
            slot = (torch.empty((max(K, 64), self._cols), dtype=torch.int32, pin_memory=True), torch.cuda.Event())
            self._ring[i] = slot
        buf, ev = slot
        buf[:K].copy_(torch.from_numpy(host))
        with torch.cuda.stream(stream):
            out = buf[:K].to(dev, non_blocking=True)
            ev.record(stream)
        return out


def _records(buf: np.ndarray) -> np.ndarray:
    return buf.reshape(-1).view(MEASUREMENT_DTYPE)


class Ruler:
    def __init__(self, Q, radius: int = 0, min_count: int = 1, min_disp: float = -1.0,
                 conf_min: float = 0.0, profile: bool = False, device: int = 0):
        self.Q = np.asarray(Q, dtype=np.float64).reshape(4, 4).copy()
        self.radius, self.min_count = int(radius), int(min_count)
        self.min_disp, self.conf_min = float(min_disp), float(conf_min)
        self.profile = bool(profile)
        self.device = int(device)
        self._staging = {}  # (device index, columns) -> _SegmentStaging

    def _upload_segments(self, host: np.ndarray, dev, stream):
        key = (dev.index, host.shape[1])
        st = self._staging.get(key)
        if st is None:
            st = self._staging[key] = _SegmentStaging(cols=host.shape[1])
        return st.upload(host, dev, stream)

    def _params(self, cap: int) -> RulerParams:
        return RulerParams(self.radius, self.min_count, self.min_disp, self.conf_min,
                           int(self.profile), int(cap))

    # ---- disparity mode ----
    def measure(self, disparity, segments, conf=None):
        """Records (a MEASUREMENT_DTYPE array of K), and with profile=True also the profile,
        float32 (K, cap, 4) rows {X, Y, Z, d_med} (NaN rows: invalid samples and rows past a
        segment's samples), cap the longest segment's sample count."""
        if _is_cuda(disparity):
            rec, prof = self.measure_device(disparity, segments, conf)
            out = _records(rec.cpu().numpy())
            return (out, prof.cpu().numpy()) if self.profile else out
        d, c, a = self._host_maps(disparity, conf)
        F, H, W = d.shape
        segs = as_segments(segments)
        K = segs.shape[0]
        cap = self._cap(segs, W, H, F)
        rec = np.zeros(K, MEASUREMENT_DTYPE)
        prof = np.full((K, cap, 4), np.nan, np.float32) if self.profile else None
        p = self._params(cap)
        with _on_device(self.device):
            rc = lib().sdr_measure_disp(*a, _Q(self.Q), ctypes.byref(p), segs.ctypes.data if K else None, K,
                                        rec.ctypes.data if K else None,
                                        prof.ctypes.data if prof is not None and prof.size else None)
        check(rc)
        return (rec, prof) if self.profile else rec

    @staticmethod
    def _cap(segs: np.ndarray, W: int, H: int, F: int) -> int:
        """Samples of the longest in-range segment."""
        if segs.shape[0] == 0:
            return 0
        f, x0, y0, x1, y1 = segs.T.astype(np.int64)
        ok = (f >= 0) & (f < F) & (x0 >= 0) & (x0 < W) & (x1 >= 0) & (x1 < W) & \
             (y0 >= 0) & (y0 < H) & (y1 >= 0) & (y1 < H)
        n = np.maximum(np.abs(x1 - x0), np.abs(y1 - y0)) + 1
        return int(n[ok].max()) if ok.any() else 0

    def measure_device(self, disparity, segments, conf=None, stream=None, profile_cap=None,
                       profile_out=None):
        """Enqueues the measurement of a CUDA disparity tensor (H, W) / (F, H, W), float32 or
        int16 with unit stride along W, on `stream` (default: the current stream) and returns
        (records, profile) without synchronising: records is a uint8 tensor (K, 80) (view its
        host copy as MEASUREMENT_DTYPE), profile a float32 tensor (K, cap, 4) or None.
        segments: host (K, 5) / (K, 4), uploaded through page-locked staging by a non-blocking
        copy on `stream` (the host does not wait for the stream's earlier work), or a CUDA int32
        tensor (K, 5) (then profile_cap defaults to max(W, H)).  profile_cap: rows a segment of the profile (0: the record's profile fields
        only).  profile_out: a (K, cap, 4) tensor to write the profile into."""
        if not _is_cuda(disparity):
            raise SDRError(-5, "measure_device expects a CUDA float32 or int16 tensor")
        dev = disparity.device
        s = stream if stream is not None else torch.cuda.current_stream(dev.index)
        with torch.cuda.stream(s):
            d, conf, a = self._device_maps(disparity, conf)  # copies, if any, on `s`, ahead of the kernel
            F, H, W = d.shape
            if _is_cuda(segments):
                if segments.dtype != torch.int32 or segments.dim() != 2 or segments.shape[1] != 5:
                    raise SDRError(-5, "device segments must be an int32 tensor (K, 5)")
                segs = segments.contiguous()
                cap = max(W, H)
            else:
                host = as_segments(segments)
                cap = self._cap(host, W, H, F)
                segs = self._upload_segments(host, dev, s)
            K = segs.shape[0]
            if profile_cap is not None:
                cap = int(profile_cap)
            rec = torch.empty((K, 80), dtype=torch.uint8, device=dev)
            prof = None
            if self.profile:
                if profile_out is not None:
                    if (not _is_cuda(profile_out) or profile_out.dtype != torch.float32
                            or not profile_out.is_contiguous() or profile_out.dim() != 3
                            or profile_out.shape[0] != K or profile_out.shape[2] != 4):
                        raise SDRError(-5, "profile_out must be a contiguous CUDA float32 tensor (K, cap, 4)")
                    prof, cap = profile_out, profile_out.shape[1]
                else:
                    prof = torch.full((K, cap, 4), float("nan"), dtype=torch.float32, device=dev)
            p = self._params(cap)
            check(lib().sdr_measure_disp_device(
                *a, _Q(self.Q), ctypes.byref(p), segs.data_ptr() if K else None, K, rec.data_ptr() if K else None,
                prof.data_ptr() if prof is not None and prof.numel() else None, ctypes.c_void_p(s.cuda_stream)))
        return rec, prof

    # ---- the maps of the disparity-mode calls ----
    @staticmethod
    def _host_maps(disparity, conf):
        """(d (F, H, W), conf or None, the host ABI's argument run (disp, disp_type, stride,
        frame_stride, W, H, F, conf)) of host maps."""
        d = np.asarray(disparity)
        if d.dtype not in (np.float32, np.int16):
            raise SDRError(-5, "disparity must be float32 (px) or int16 (1/16 px)")
        d = _frames3(d, "disparity")
        if d.strides[2] != d.itemsize or d.strides[1] % d.itemsize or d.strides[0] % d.itemsize \
                or min(d.strides) <= 0:
            d = np.ascontiguousarray(d)
        F, H, W = d.shape
        c = None
        if conf is not None:
            c = np.ascontiguousarray(_frames3(np.asarray(conf, dtype=np.float32), "conf"))
            if c.shape != d.shape:
                raise SDRError(-1, "conf must have the disparity's shape")
        rs = d.strides[1] // d.itemsize
        return d, c, (d.ctypes.data, DISP_F32 if d.dtype == np.float32 else DISP_S16, rs,
                      rs * H if F == 1 else d.strides[0] // d.itemsize, W, H, F,
                      c.ctypes.data if c is not None else None)

    @staticmethod
    def _device_maps(disparity, conf):
        """(d (F, H, W), conf or None, the device ABI's argument run as _host_maps gives the host's)
        of CUDA maps, made contiguous on the current stream."""
        d = disparity
        if not _is_cuda(d) or d.dtype not in (torch.float32, torch.int16):
            raise SDRError(-5, "expected a CUDA float32 or int16 disparity tensor")
        if d.dim() == 2:
            d = d.unsqueeze(0)
        if d.dim() != 3:
            raise SDRError(-1, "disparity must be (H, W) or (F, H, W)")
        if d.stride(2) != 1 or d.stride(1) < d.shape[2] or d.stride(0) < d.stride(1):
            d = d.contiguous()
        if conf is not None:
            if not _is_cuda(conf) or conf.dtype != torch.float32 or conf.numel() != d.numel():
                raise SDRError(-5, "conf must be a CUDA float32 tensor of the disparity's shape")
            conf = conf.contiguous()
        F, H, W = d.shape
        return d, conf, (d.data_ptr(), DISP_F32 if d.dtype == torch.float32 else DISP_S16, d.stride(1),
                         d.stride(1) * H if F == 1 else d.stride(0), W, H, F,
                         conf.data_ptr() if conf is not None else None)

    # ---- against a surface: plane fit and point-to-plane distance ----
    def _plane_params(self, iterations, inlier_px, min_inliers) -> PlaneParams:
        return PlaneParams(int(iterations), int(min_inliers), float(inlier_px), self.min_disp, self.conf_min)

    def fit_plane(self, disparity, regions, conf=None, iterations: int = 3, inlier_px: float = 1.0,
                  min_inliers: int = 16):
        """Robust plane fits (sdr.h, "the ruler against a surface") of K rectangles
        (frame, x0, y0, x1, y1) / (x0, y0, x1, y1), corners in any order: a PLANE_DTYPE array."""
        if _is_cuda(disparity):
            rec = self.fit_plane_device(disparity, regions, conf, iterations, inlier_px, min_inliers)
            return rec.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
        d, c, a = self._host_maps(disparity, conf)
        regs = as_segments(regions)
        K = regs.shape[0]
        rec = np.zeros(K, PLANE_DTYPE)
        p = self._plane_params(iterations, inlier_px, min_inliers)
        with _on_device(self.device):
            rc = lib().sdr_fit_planes(*a, _Q(self.Q), ctypes.byref(p), regs.ctypes.data if K else None, K,
                                      rec.ctypes.data if K else None)
        check(rc)
        return rec

    def fit_plane_device(self, disparity, regions, conf=None, iterations: int = 3, inlier_px: float = 1.0,
                         min_inliers: int = 16, stream=None):
        """Enqueues the fits on `stream` (default: the current stream) and returns the records as
        a uint8 tensor (K, 128) without synchronising (view its host copy as PLANE_DTYPE, or hand
        it to plane_distance_device).  regions: host (K, 5) / (K, 4) or a CUDA int32 (K, 5)."""
        if not _is_cuda(disparity):
            raise SDRError(-5, "fit_plane_device expects a CUDA float32 or int16 tensor")
        dev = disparity.device
        s = stream if stream is not None else torch.cuda.current_stream(dev.index)
        with torch.cuda.stream(s):
            d, conf, a = self._device_maps(disparity, conf)
            regs = self._device_rows(regions, _RECTANGLES, dev, s)
            K = regs.shape[0]
            rec = torch.empty((K, 128), dtype=torch.uint8, device=dev)
            p = self._plane_params(iterations, inlier_px, min_inliers)
            check(lib().sdr_fit_planes_device(*a, _Q(self.Q), ctypes.byref(p), regs.data_ptr() if K else None, K,
                                              rec.data_ptr() if K else None, ctypes.c_void_p(s.cuda_stream)))
        return rec

    # ---- the dominant planes of a region (sdr.h, "the dominant planes of a region") ----
    def _search_params(self, max_planes, hypotheses, seed, iterations, inlier_px, min_inliers) -> PlaneSearchParams:
        seed = int(seed)
        if not 0 <= seed < 2 ** 32:
            raise SDRError(-1, "seed must be in 0..2^32-1")
        return PlaneSearchParams(self._plane_params(iterations, inlier_px, min_inliers), int(max_planes),
                                 int(hypotheses), seed)

    @staticmethod
    def _search_region(region, W, H) -> np.ndarray:
        if region is None:
            return np.array([[0, 0, 0, W - 1, H - 1]], np.int32)
        reg = as_segments(region)
        if reg.shape[0] != 1:
            raise SDRError(-1, "find_planes takes one region")
        return reg

    def find_planes(self, disparity, region=None, conf=None, max_planes: int = 4, hypotheses: int = 256,
                    seed: int = 0, iterations: int = 3, inlier_px: float = 1.0, min_inliers: int = 64,
                    labels: bool = False):
        """The dominant planes of one rectangle, the largest first, without a prior: a seeded search
        (three-point hypotheses scored on the pixels no earlier plane has claimed, the winner
        refitted as fit_plane does).  region: (frame, x0, y0, x1, y1) / (x0, y0, x1, y1), None: the
        whole map of frame 0.  Returns the planes found as a PLANE_DTYPE array (at most
        max_planes), and with labels=True also the (H, W) uint8 map of the region's frame: the
        index of the plane a pixel lies on, 255 on none."""
        if _is_cuda(disparity):
            rec, count, _, lab = self.find_planes_device(disparity, region, conf, max_planes, hypotheses, seed,
                                                         iterations, inlier_px, min_inliers, labels=labels)
            n = int(count.cpu()[0])
            out = rec.cpu().numpy().reshape(-1).view(PLANE_DTYPE)[:n].copy()
            return (out, lab.cpu().numpy()) if labels else out
        out, count, _, lab = self.find_planes_full(disparity, region, conf, max_planes, hypotheses, seed, iterations,
                                                   inlier_px, min_inliers, labels=labels)
        return (out[:count].copy(), lab) if labels else out[:count].copy()

    def find_planes_full(self, disparity, region=None, conf=None, max_planes: int = 4, hypotheses: int = 256,
                         seed: int = 0, iterations: int = 3, inlier_px: float = 1.0, min_inliers: int = 64,
                         labels: bool = False):
        """find_planes on host maps with everything the search writes: (all max_planes records, count,
        the rounds as a PLANE_SEARCH_ROUND_DTYPE array, the labels or None)."""
        d, c, a = self._host_maps(disparity, conf)
        F, H, W = d.shape
        reg = self._search_region(region, W, H)
        p = self._search_params(max_planes, hypotheses, seed, iterations, inlier_px, min_inliers)
        n = max(int(max_planes), 0)
        rec = np.zeros(n, PLANE_DTYPE)
        rounds = np.zeros(n, PLANE_SEARCH_ROUND_DTYPE)
        count = np.zeros(1, np.int32)
        lab = np.full((H, W), 255, np.uint8) if labels else None
        with _on_device(self.device):
            rc = lib().sdr_find_planes(*a, _Q(self.Q), ctypes.byref(p), reg.ctypes.data, rec.ctypes.data if n else None,
                                       count.ctypes.data, rounds.ctypes.data if n else None,
                                       lab.ctypes.data if lab is not None else None)
        check(rc)
        return rec, int(count[0]), rounds, lab

    def find_planes_device(self, disparity, region=None, conf=None, max_planes: int = 4, hypotheses: int = 256,
                           seed: int = 0, iterations: int = 3, inlier_px: float = 1.0, min_inliers: int = 64,
                           labels: bool = False, stream=None, labels_out=None):
        """Enqueues the search on `stream` (default: the current stream) without synchronising and
        returns (planes uint8 (max_planes, 128), count int32 (1,), rounds int32 (max_planes, 4),
        labels uint8 (H, W) or None).  The planes tensor feeds plane_distance_device unchanged
        (records past count are not PLANE_OK).  region: host, or a CUDA int32 (1, 5); labels_out: a
        contiguous CUDA uint8 (H, W) tensor to write the labels into."""
        if not _is_cuda(disparity):
            raise SDRError(-5, "find_planes_device expects a CUDA float32 or int16 tensor")
        dev = disparity.device
        s = stream if stream is not None else torch.cuda.current_stream(dev.index)
        with torch.cuda.stream(s):
            d, conf, a = self._device_maps(disparity, conf)
            F, H, W = d.shape
            p = self._search_params(max_planes, hypotheses, seed, iterations, inlier_px, min_inliers)
            if _is_cuda(region):
                if region.dtype != torch.int32 or region.dim() != 2 or tuple(region.shape) != (1, 5):
                    raise SDRError(-5, "a device region must be an int32 tensor (1, 5)")
                reg = region.contiguous()
            else:
                reg = self._upload_segments(self._search_region(region, W, H), dev, s)
            n = max(int(max_planes), 0)
            rec = torch.empty((n, 128), dtype=torch.uint8, device=dev)
            count = torch.empty((1,), dtype=torch.int32, device=dev)
            rounds = torch.empty((n, 4), dtype=torch.int32, device=dev)
            lab = None
            if labels_out is not None:
                if (not _is_cuda(labels_out) or labels_out.dtype != torch.uint8 or not labels_out.is_contiguous()
                        or tuple(labels_out.shape) != (H, W)):
                    raise SDRError(-5, "labels_out must be a contiguous CUDA uint8 tensor (H, W)")
                lab = labels_out
            elif labels:
                lab = torch.empty((H, W), dtype=torch.uint8, device=dev)
            check(lib().sdr_find_planes_device(
                *a, _Q(self.Q), ctypes.byref(p), reg.data_ptr(), rec.data_ptr() if n else None, count.data_ptr(),
                rounds.data_ptr() if n else None, lab.data_ptr() if lab is not None else None,
                ctypes.c_void_p(s.cuda_stream)))
        return rec, count, rounds, lab

    # ---- queries against plane records: the point query, the relief, the footprint ----
    def _plane_queries(self, entry, params, dtype, disparity, planes, rows, kind, conf, labels=_NO_LABELS):
        """The host-pointer form of an entry that takes maps, plane records and query rows: a `dtype`
        array of K.  params: makes the parameter struct; kind: the rows' (converter, name, width);
        labels: the label map or None of an entry that takes one."""
        p = params()
        pl = _host_planes(planes)
        d, c, a = self._host_maps(disparity, conf)
        lab_arg = ()
        if labels is not _NO_LABELS:
            lab = _host_labels(labels, d.shape)
            lab_arg = (lab.ctypes.data if lab is not None else None,)
        qs = kind[0](rows)
        K, P = qs.shape[0], pl.shape[0]
        out = np.zeros(K, dtype)
        with _on_device(self.device):
            rc = entry(*a, *lab_arg, _Q(self.Q), ctypes.byref(p), pl.ctypes.data if P else None, P,
                       qs.ctypes.data if K else None, K, out.ctypes.data if K else None)
        check(rc)
        return out

    def _plane_queries_device(self, name, entry, params, size, disparity, planes, rows, kind, conf, stream,
                              labels=_NO_LABELS):
        """The device form of _plane_queries: enqueues on `stream` (default: the current stream) and
        returns a uint8 tensor (K, size) without synchronising."""
        if not _is_cuda(disparity):
            raise SDRError(-5, f"{name} expects a CUDA float32 or int16 tensor")
        p = params()
        dev = disparity.device
        s = stream if stream is not None else torch.cuda.current_stream(dev.index)
        with torch.cuda.stream(s):
            d, conf, a = self._device_maps(disparity, conf)
            pl = _device_planes(planes, dev)
            P = pl.numel() // 128 if pl is not None else 0
            lab_arg = ()
            if labels is not _NO_LABELS:
                lab = _device_labels(labels, d, dev)
                lab_arg = (lab.data_ptr() if lab is not None else None,)
            qs = self._device_rows(rows, kind, dev, s)
            K = qs.shape[0]
            out = torch.empty((K, size), dtype=torch.uint8, device=dev)
            check(entry(*a, *lab_arg, _Q(self.Q), ctypes.byref(p), pl.data_ptr() if P else None, P,
                        qs.data_ptr() if K else None, K, out.data_ptr() if K else None,
                        ctypes.c_void_p(s.cuda_stream)))
        return out

    def _device_rows(self, rows, kind, dev, stream):
        """Query rows on the device: a CUDA int32 tensor of the kind's width as it is, host rows
        through the kind's converter and the page-locked staging."""
        as_rows, what, width = kind
        if not _is_cuda(rows):
            return self._upload_segments(as_rows(rows), dev, stream)
        if rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != width:
            raise SDRError(-5, f"device {what} must be an int32 tensor (K, {width})")
        return rows.contiguous()

    def _point_params(self) -> RulerParams:
        p = self._params(0)
        p.profile = 0
        return p

    def plane_distance(self, disparity, planes, points, conf=None):
        """Signed distances of sampled points to fitted planes: a PLANE_DISTANCE_DTYPE array of K.
        planes: PLANE_DTYPE records or fit_plane_device's tensor; points: (K, 4)
        {frame, x, y, plane} or (K, 3) {x, y, plane} on frame 0; each point is sampled with the
        ruler's radius and min_count."""
        if _is_cuda(disparity):
            out = self.plane_distance_device(disparity, planes, points, conf)
            return out.cpu().numpy().reshape(-1).view(PLANE_DISTANCE_DTYPE)
        return self._plane_queries(lib().sdr_plane_distance, self._point_params, PLANE_DISTANCE_DTYPE, disparity,
                                   planes, points, _POINTS, conf)

    def plane_distance_device(self, disparity, planes, points, conf=None, stream=None):
        """Enqueues the queries on `stream` and returns a uint8 tensor (K, 32) without
        synchronising.  planes: the uint8 tensor (P, 128) of fit_plane_device (a fit and its queries
        then chain on one stream with no host round trip) or host records; points: host (K, 4) /
        (K, 3) or a CUDA int32 (K, 4)."""
        return self._plane_queries_device("plane_distance_device", lib().sdr_plane_distance_device,
                                          self._point_params, 32, disparity, planes, points, _POINTS, conf, stream)

    # ---- the relief of a region (sdr.h, "the relief of a region") ----
    def _relief_params(self, quantiles, band) -> ReliefParams:
        qs = [int(v) for v in quantiles]
        if len(qs) > 8:
            raise SDRError(-1, "at most 8 quantiles")
        if any(v < 0 or v > 1000 for v in qs) or any(int(v) != v for v in quantiles):
            raise SDRError(-1, "quantiles are integers in 0..1000 (permille)")
        band = float(band)
        if not (np.isfinite(band) and band >= 0.0):
            raise SDRError(-1, "band must be finite and >= 0")
        p = ReliefParams(self.min_disp, self.conf_min, band, len(qs))
        for j, v in enumerate(qs):
            p.permille[j] = v
        return p

    def relief(self, disparity, planes, regions, labels=None, conf=None, quantiles=(50, 500, 950),
               band: float = 0.0):
        """The heights of K rectangles' pixels above plane records: a RELIEF_DTYPE array of K.
        planes: PLANE_DTYPE records or a device tensor of them; regions: rows
        {frame, x0, y0, x1, y1, plane, label} (rows of 5 or 6: plane 0, label -1 = no mask);
        labels: a uint8 (H, W) / (F, H, W) map as find_planes returns it, a query with label >= 0
        takes only the pixels that carry it; quantiles: up to 8 permille values, q[j] the element
        (n-1)*permille/1000 of the heights in ascending order; band: n_above / n_below count the
        heights beyond +-band (Q's units)."""
        if _is_cuda(disparity):
            out = self.relief_device(disparity, planes, regions, labels, conf, quantiles, band)
            return out.cpu().numpy().reshape(-1).view(RELIEF_DTYPE)
        return self._plane_queries(lib().sdr_plane_relief, lambda: self._relief_params(quantiles, band), RELIEF_DTYPE,
                                   disparity, planes, regions, _REGIONS, conf, labels)

    def relief_device(self, disparity, planes, regions, labels=None, conf=None, quantiles=(50, 500, 950),
                      band: float = 0.0, stream=None):
        """Enqueues the reliefs on `stream` (default: the current stream) and returns a uint8 tensor
        (K, 128) without synchronising (view its host copy as RELIEF_DTYPE).  planes and labels: as
        find_planes_device returns them (a search and its relief then chain on one stream with no
        host round trip) or host arrays; regions: host rows or a CUDA int32 (K, 8)."""
        return self._plane_queries_device("relief_device", lib().sdr_plane_relief_device,
                                          lambda: self._relief_params(quantiles, band), 128, disparity, planes,
                                          regions, _REGIONS, conf, stream, labels)

    # ---- the footprint of a region (sdr.h, "the footprint of a region") ----
    def _footprint_params(self, cell, grid, support, h_range) -> FootprintParams:
        lo, hi = (-1048576.0, 1048576.0) if h_range is None else (float(h_range[0]), float(h_range[1]))
        cell = float(cell)
        if not (np.isfinite(cell) and 0.0625 <= cell <= 65536.0):
            raise SDRError(-1, "cell must be finite and in 0.0625..65536")
        if int(grid) != grid or not 16 <= grid <= 1024:
            raise SDRError(-1, "grid must be an integer in 16..1024")
        if int(support) != support or not 1 <= support <= 255:
            raise SDRError(-1, "support must be an integer in 1..255")
        if np.isnan(lo) or np.isnan(hi) or lo > hi:
            raise SDRError(-1, "h_range must be (lo, hi) with lo <= hi, neither NaN")
        return FootprintParams(self.min_disp, self.conf_min, cell, lo, hi, int(grid), int(support))

    def footprint(self, disparity, planes, regions, labels=None, conf=None, cell: float = 4.0, grid: int = 512,
                  support: int = 4, h_range=None):
        """The oriented bounding rectangles of K rectangles' pixels in plane records' planes: a
        FOOTPRINT_DTYPE array of K.  planes, regions and labels: as relief() takes them; cell: the
        side of a grid cell in Q's units; grid: cells a side (members beyond it set
        FOOTPRINT_CLIPPED); support: the members a kept cell's 3 x 3 neighbourhood must hold;
        h_range: (lo, hi), only pixels whose height above the plane lies in it."""
        if _is_cuda(disparity):
            out = self.footprint_device(disparity, planes, regions, labels, conf, cell, grid, support, h_range)
            return out.cpu().numpy().reshape(-1).view(FOOTPRINT_DTYPE)
        return self._plane_queries(lib().sdr_plane_footprint,
                                   lambda: self._footprint_params(cell, grid, support, h_range), FOOTPRINT_DTYPE,
                                   disparity, planes, regions, _REGIONS, conf, labels)

    def footprint_device(self, disparity, planes, regions, labels=None, conf=None, cell: float = 4.0,
                         grid: int = 512, support: int = 4, h_range=None, stream=None):
        """Enqueues the footprints on `stream` (default: the current stream) and returns a uint8
        tensor (K, 256) without synchronising (view its host copy as FOOTPRINT_DTYPE).  The argument
        forms are relief_device's."""
        return self._plane_queries_device("footprint_device", lib().sdr_plane_footprint_device,
                                          lambda: self._footprint_params(cell, grid, support, h_range), 256, disparity,
                                          planes, regions, _REGIONS, conf, stream, labels)

    # ---- the objects of a region (sdr.h, "the objects of a region") ----
    def _object_params(self, h_range, max_diff, connectivity, min_pixels, max_objects) -> ObjectParams:
        lo, hi = float(h_range[0]), float(h_range[1])
        max_diff = float(max_diff)
        if np.isnan(lo) or np.isnan(hi) or lo > hi:
            raise SDRError(-1, "h_range must be (lo, hi) with lo <= hi, neither NaN")
        if not (np.isfinite(max_diff) and max_diff >= 0.0):
            raise SDRError(-1, "max_diff must be finite and >= 0")
        if connectivity not in (4, 8):
            raise SDRError(-1, "connectivity must be 4 or 8")
        if int(min_pixels) != min_pixels or not 1 <= min_pixels <= 2 ** 24:
            raise SDRError(-1, "min_pixels must be an integer in 1..2^24")
        if int(max_objects) != max_objects or not 1 <= max_objects <= 64:
            raise SDRError(-1, "max_objects must be an integer in 1..64")
        return ObjectParams(self.min_disp, self.conf_min, lo, hi, max_diff, int(connectivity), int(min_pixels),
                            int(max_objects))

    @staticmethod
    def _object_query(region) -> np.ndarray:
        q = as_relief_queries(region)
        if q.shape[0] != 1:
            raise SDRError(-1, "find_objects takes one region")
        return q

    def find_objects(self, disparity, planes, region, labels=None, conf=None, h_range=(10.0, 1048576.0),
                     max_diff: float = 1.0, connectivity: int = 8, min_pixels: int = 64, max_objects: int = 16,
                     labels_out: bool = True):
        """The things standing on a plane: the connected sets of one rectangle's pixels whose height
        above a plane record lies in h_range (Q's units) and whose disparities step by at most
        max_diff (px) between neighbours (connectivity 4 or 8), those of at least min_pixels pixels,
        the largest first, at most max_objects.  planes and labels: as relief() takes them; region:
        one row {frame, x0, y0, x1, y1, plane, label} (5 or 6 entries: plane 0, label -1); label 255
        with find_planes' map takes the pixels no plane claimed.  Returns (objects, scan, labels):
        the objects found as an OBJECT_DTYPE array, one OBJECT_SCAN_DTYPE record (counts, flags),
        and with labels_out the (H, W) uint8 map of the region's frame, k on object k's pixels and
        255 elsewhere, which relief() and footprint() take with label k (None without)."""
        if _is_cuda(disparity):
            rec, scan, lab = self.find_objects_device(disparity, planes, region, labels, conf, h_range, max_diff,
                                                      connectivity, min_pixels, max_objects, labels_out=labels_out)
            sc = scan.cpu().numpy().reshape(-1).view(OBJECT_SCAN_DTYPE)[0]
            out = rec.cpu().numpy().reshape(-1).view(OBJECT_DTYPE)[:int(sc["count"])].copy()
            return out, sc, (lab.cpu().numpy() if lab is not None else None)
        p = self._object_params(h_range, max_diff, connectivity, min_pixels, max_objects)
        pl = _host_planes(planes)
        d, c, a = self._host_maps(disparity, conf)
        F, H, W = d.shape
        lab_in = _host_labels(labels, d.shape)
        q = self._object_query(region)
        P = pl.shape[0]
        rec = np.zeros(int(max_objects), OBJECT_DTYPE)
        scan = np.zeros(1, OBJECT_SCAN_DTYPE)
        lab = np.empty((H, W), np.uint8) if labels_out else None
        with _on_device(self.device):
            rc = lib().sdr_find_objects(*a, lab_in.ctypes.data if lab_in is not None else None, _Q(self.Q),
                                        ctypes.byref(p), pl.ctypes.data if P else None, P, q.ctypes.data,
                                        rec.ctypes.data, scan.ctypes.data, lab.ctypes.data if lab is not None else None)
        check(rc)
        return rec[:int(scan["count"][0])].copy(), scan[0], lab

    def find_objects_device(self, disparity, planes, region, labels=None, conf=None, h_range=(10.0, 1048576.0),
                            max_diff: float = 1.0, connectivity: int = 8, min_pixels: int = 64, max_objects: int = 16,
                            stream=None, labels_out=None):
        """Enqueues the labelling on `stream` (default: the current stream) without synchronising and
        returns (objects uint8 (max_objects, 64), scan uint8 (64,), labels uint8 (H, W) or None):
        view the host copies as OBJECT_DTYPE and OBJECT_SCAN_DTYPE; the labels tensor feeds
        relief_device and footprint_device unchanged.  planes and labels: as find_planes_device
        returns them or host arrays; region: a host row or a CUDA int32 (1, 8); labels_out: True for
        a new label tensor, a contiguous CUDA uint8 (H, W) tensor to write into (not `labels`), or
        None / False for no label map."""
        if not _is_cuda(disparity):
            raise SDRError(-5, "find_objects_device expects a CUDA float32 or int16 tensor")
        p = self._object_params(h_range, max_diff, connectivity, min_pixels, max_objects)
        dev = disparity.device
        s = stream if stream is not None else torch.cuda.current_stream(dev.index)
        with torch.cuda.stream(s):
            d, conf, a = self._device_maps(disparity, conf)
            F, H, W = d.shape
            pl = _device_planes(planes, dev)
            P = pl.numel() // 128 if pl is not None else 0
            lab_in = _device_labels(labels, d, dev)
            if _is_cuda(region):
                if region.dtype != torch.int32 or tuple(region.shape) != (1, 8):
                    raise SDRError(-5, "a device region must be an int32 tensor (1, 8)")
                q = region.contiguous()
            else:
                q = self._upload_segments(self._object_query(region), dev, s)
            lab = None
            if labels_out is True:
                lab = torch.empty((H, W), dtype=torch.uint8, device=dev)
            elif labels_out is not None and labels_out is not False:
                if (not _is_cuda(labels_out) or labels_out.dtype != torch.uint8 or not labels_out.is_contiguous()
                        or tuple(labels_out.shape) != (H, W)):
                    raise SDRError(-5, "labels_out must be a contiguous CUDA uint8 tensor (H, W)")
                if lab_in is not None and labels_out.data_ptr() == lab_in.data_ptr():
                    raise SDRError(-1, "labels_out must not be the input label map")
                lab = labels_out
            rec = torch.empty((int(max_objects), 64), dtype=torch.uint8, device=dev)
            scan = torch.empty((64,), dtype=torch.uint8, device=dev)
            check(lib().sdr_find_objects_device(
                *a, lab_in.data_ptr() if lab_in is not None else None, _Q(self.Q), ctypes.byref(p),
                pl.data_ptr() if P else None, P, q.data_ptr(), rec.data_ptr(), scan.data_ptr(),
                lab.data_ptr() if lab is not None else None, ctypes.c_void_p(s.cuda_stream)))
        return rec, scan, lab

    # ---- the clearance of two labelled things (sdr.h, "the clearance of two labelled things") ----
    def _clearance_params(self, h_range) -> ClearanceParams:
        lo, hi = (-1048576.0, 1048576.0) if h_range is None else (float(h_range[0]), float(h_range[1]))
        if np.isnan(lo) or np.isnan(hi) or lo > hi:
            raise SDRError(-1, "h_range must be (lo, hi) with lo <= hi, neither NaN")
        if not 0 <= self.radius <= 4 or self.min_count < 1:
            raise SDRError(-1, "the clearance takes a ruler with radius in 0..4 and min_count >= 1")
        return ClearanceParams(self.min_disp, self.conf_min, lo, hi, self.radius, self.min_count)

    def clearance(self, disparity, planes, pairs, labels, conf=None, h_range=None):
        """The gaps between K pairs of labelled things: a CLEARANCE_DTYPE array of K.  planes: as
        relief() takes them; pairs: rows {frame, x0, y0, x1, y1, plane, label_a, label_b}; labels: the
        uint8 (H, W) / (F, H, W) map find_objects or find_planes returns (required).  Each pixel of a
        label has for its point the ruler's sample (radius, min_count) over the pixels of the same
        label; a record holds the smallest 3-D distance between a point of label_a and a point of
        label_b, the two pixels and points, and the distance's parts along the plane's normal and in
        the plane; h_range: (lo, hi), only pixels whose height above the plane lies in it."""
        if labels is None:
            raise SDRError(-1, "clearance needs a label map")
        if _is_cuda(disparity):
            out = self.clearance_device(disparity, planes, pairs, labels, conf, h_range)
            return out.cpu().numpy().reshape(-1).view(CLEARANCE_DTYPE)
        return self._plane_queries(lib().sdr_clearance, lambda: self._clearance_params(h_range), CLEARANCE_DTYPE,
                                   disparity, planes, pairs, _PAIRS, conf, labels)

    def clearance_device(self, disparity, planes, pairs, labels, conf=None, h_range=None, stream=None):
        """Enqueues the clearances on `stream` (default: the current stream) and returns a uint8
        tensor (K, 128) without synchronising (view its host copy as CLEARANCE_DTYPE).  planes and
        labels: as find_planes_device and find_objects_device return them (the floor, the objects and
        their gap then chain on one stream with no host round trip) or host arrays; pairs: host rows
        or a CUDA int32 (K, 8)."""
        if labels is None:
            raise SDRError(-1, "clearance needs a label map")
        return self._plane_queries_device("clearance_device", lib().sdr_clearance_device,
                                          lambda: self._clearance_params(h_range), 128, disparity, planes, pairs,
                                          _PAIRS, conf, stream, labels)

    # ---- the ruler over time (sdr.h, "the ruler over time") ----
    def _fuse_params(self, tol, min_count, mode, fill) -> FuseParams:
        fill = self.min_disp if fill is None else float(fill)
        return FuseParams(self.min_disp, self.conf_min, float(tol), fill, int(min_count), int(mode))

    def fuse(self, disparity, conf=None, tol: float = 1.0, min_count: int = 2, mode: int = FUSE_MEAN, fill=None,
             support: bool = False, spread: bool = False):
        """One disparity map from the (F, H, W) stack of a still scene's last frames (F <= 32): a
        pixel's valid values vote, those within `tol` px of their lower median agree, and with at
        least min_count of them the pixel is their ordered mean (FUSE_MEAN) or the median itself
        (FUSE_MEDIAN); any other pixel is `fill` (None: the ruler's min_disp, an invalid value).
        conf: the frames' confidence maps, gated by the ruler's conf_min frame by frame.  Returns
        (fused, record[, support][, spread]): fused float32 (1, H, W) in px, which every other
        call takes as its disparity (without conf: the gate has been applied), one FUSION_DTYPE
        record (the pixels fused, empty, sparse and unstable; the holes filled and the outliers
        replaced against the last frame), support uint8 (H, W) the agreeing values a pixel, spread
        float32 (H, W) their range (NaN where the pixel is not fused)."""
        if _is_cuda(disparity):
            outs = self.fuse_device(disparity, conf, tol, min_count, mode, fill, support, spread)
            rec = outs[1].cpu().numpy().view(FUSION_DTYPE)[0]
            return (outs[0].cpu().numpy(), rec) + tuple(o.cpu().numpy() for o in outs[2:])
        d, c, a = self._host_maps(disparity, conf)
        F, H, W = d.shape
        p = self._fuse_params(tol, min_count, mode, fill)
        out = np.empty((1, H, W), np.float32)
        rec = np.zeros(1, FUSION_DTYPE)
        sup = np.empty((H, W), np.uint8) if support else None
        spr = np.empty((H, W), np.float32) if spread else None
        with _on_device(self.device):
            rc = lib().sdr_fuse_disp(*a, ctypes.byref(p), out.ctypes.data, sup.ctypes.data if support else None,
                                     spr.ctypes.data if spread else None, rec.ctypes.data)
        check(rc)
        return (out, rec[0]) + ((sup,) if support else ()) + ((spr,) if spread else ())

    def fuse_device(self, disparity, conf=None, tol: float = 1.0, min_count: int = 2, mode: int = FUSE_MEAN,
                    fill=None, support: bool = False, spread: bool = False, stream=None, out=None):
        """Enqueues the fusion of a CUDA stack (F, H, W), float32 or int16, on `stream` (default: the
        current stream) and returns (fused, record[, support][, spread]) without synchronising:
        fused a float32 tensor (1, H, W) that goes straight into any *_device call of the ruler on
        the same stream (with conf=None), record a uint8 tensor (64,) (view its host copy as
        FUSION_DTYPE).  out: a contiguous CUDA float32 tensor of H * W elements to write the map
        into (not the stack)."""
        if not _is_cuda(disparity):
            raise SDRError(-5, "fuse_device expects a CUDA float32 or int16 tensor")
        dev = disparity.device
        s = stream if stream is not None else torch.cuda.current_stream(dev.index)
        with torch.cuda.stream(s):
            d, conf, a = self._device_maps(disparity, conf)
            F, H, W = d.shape
            if F > 1 and d.stride(0) < d.stride(1) * H:  # frames that interleave: the entry takes whole frames
                d, conf, a = self._device_maps(d.contiguous(), conf)
            p = self._fuse_params(tol, min_count, mode, fill)
            if out is not None:
                if (not _is_cuda(out) or out.dtype != torch.float32 or not out.is_contiguous()
                        or out.numel() != H * W or out.device != dev):
                    raise SDRError(-5, "out must be a contiguous CUDA float32 tensor of H * W elements")
                fused = out.view(1, H, W)
            else:
                fused = torch.empty((1, H, W), dtype=torch.float32, device=dev)
            rec = torch.empty((64,), dtype=torch.uint8, device=dev)
            sup = torch.empty((H, W), dtype=torch.uint8, device=dev) if support else None
            spr = torch.empty((H, W), dtype=torch.float32, device=dev) if spread else None
            check(lib().sdr_fuse_disp_device(*a, ctypes.byref(p), fused.data_ptr(), sup.data_ptr() if support else None,
                                             spr.data_ptr() if spread else None, rec.data_ptr(),
                                             ctypes.c_void_p(s.cuda_stream)))
        return (fused, rec) + ((sup,) if support else ()) + ((spr,) if spread else ())

    # ---- XYZ-map mode (the reference's measurement) ----
    def measure_xyz(self, depth_map, segments):
        """onMouseMeasure on a computeDepth map (H, W, 3) / (F, H, W, 3): records of K."""
        segs = as_segments(segments)
        K = segs.shape[0]
        if _is_cuda(depth_map):
            x = depth_map
            if x.dtype != torch.float32 or x.shape[-1] != 3 or x.dim() not in (3, 4):
                raise SDRError(-5, "depth_map must be float32 (H, W, 3) or (F, H, W, 3)")
            x = x.contiguous()
            if x.dim() == 3:
                x = x.unsqueeze(0)
            F, H, W, _ = x.shape
            st = torch.cuda.current_stream(x.device.index)
            sd = self._upload_segments(segs, x.device, st)
            rec = torch.empty((K, 80), dtype=torch.uint8, device=x.device)
            check(lib().sdr_measure_xyz_device(x.data_ptr(), W * 3, W * H * 3, W, H, F,
                                               sd.data_ptr() if K else None, K,
                                               rec.data_ptr() if K else None,
                                               ctypes.c_void_p(st.cuda_stream)))
            return _records(rec.cpu().numpy())
        x = np.asarray(depth_map)
        if x.dtype != np.float32 or x.shape[-1] != 3 or x.ndim not in (3, 4):
            raise SDRError(-5, "depth_map must be float32 (H, W, 3) or (F, H, W, 3)")
        x = np.ascontiguousarray(x)
        if x.ndim == 3:
            x = x[None]
        F, H, W, _ = x.shape
        rec = np.zeros(K, MEASUREMENT_DTYPE)
        with _on_device(self.device):
            rc = lib().sdr_measure_xyz(x.ctypes.data, W * 3, W * H * 3, W, H, F,
                                       segs.ctypes.data if K else None, K,
                                       rec.ctypes.data if K else None)
        check(rc)
        return rec


class MeasurementLog:
    """The reference's measurement_record list and save_csvFile (stereo_displayer.cpp:52, 74-102).
    A record carries 3-D points only, so add() also takes the segment's pixels."""

    def __init__(self):
        self.image_index = []
        self.segments = []
        self.records = []

    def __len__(self):
        return len(self.records)

    def add(self, image_index: int, rec, segment):
        """rec: one MEASUREMENT_DTYPE record; segment: (x0, y0, x1, y1) or (frame, x0, ...)."""
        seg = as_segments(segment)
        r = np.asarray(rec, dtype=MEASUREMENT_DTYPE).reshape(-1)
        if seg.shape[0] != 1 or r.shape[0] != 1:
            raise SDRError(-1, "add() takes one record and one segment")
        self.image_index.append(int(image_index))
        self.segments.append(seg[0])
        self.records.append(r[0])

    def to_csv(self, header: bool = True) -> str:
        n = len(self.records)
        idx = np.asarray(self.image_index, dtype=np.int32).reshape(n)
        segs = np.ascontiguousarray(np.asarray(self.segments, dtype=np.int32).reshape(n, 5))
        recs = np.asarray(self.records, dtype=MEASUREMENT_DTYPE).reshape(n)
        args = (idx.ctypes.data if n else None, segs.ctypes.data if n else None,
                recs.ctypes.data if n else None, n, int(bool(header)))
        size = lib().sdr_measurements_csv(*args, None, 0)
        if size < 0:
            check(size)
        buf = ctypes.create_string_buffer(size + 1)
        size = lib().sdr_measurements_csv(*args, buf, size + 1)
        if size < 0:
            check(size)
        return buf.raw[:size].decode()

    def save_csv(self, path, header: bool = True):
        """Appends (std::ios::app, as the reference does; it writes the header at every save)."""
        with open(path, "ab") as f:
            f.write(self.to_csv(header).encode())
