"""ctypes binding of the engine's C ABI (include/sdr/sdr.h -> lib/libsdr.so).

There is no CPU fallback: if the HIP library is missing, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsdr.so")

SDR_OK = 0
ERRORS = {
    -1: "SDR_ERR_ARG", -2: "SDR_ERR_NUMDISP", -3: "SDR_ERR_MODE", -4: "SDR_ERR_SIZE",
    -5: "SDR_ERR_TYPE", -6: "SDR_ERR_DEVICE", -7: "SDR_ERR_NOMEM", -8: "SDR_ERR_LIMIT",
}


class SDRError(RuntimeError):
    """Raised where cv::StereoSGBM / reprojectImageTo3D would throw cv::Exception."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class SgbmParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff",
        "preFilterCap", "uniquenessRatio", "speckleWindowSize", "speckleRange", "mode",
        "nstripes", "uniq_rule")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class WlsParams(ctypes.Structure):
    """sdr_wls_params (include/sdr/sdr.h)."""
    _fields_ = [("lambda_", ctypes.c_double), ("sigma_color", ctypes.c_double),
                ("lrc_thresh", ctypes.c_int), ("depth_discontinuity_radius", ctypes.c_int),
                ("roll_off", ctypes.c_float), ("lambda_attenuation", ctypes.c_double),
                ("num_iter", ctypes.c_int), ("left_offset", ctypes.c_int),
                ("right_offset", ctypes.c_int), ("top_offset", ctypes.c_int),
                ("bottom_offset", ctypes.c_int), ("min_disp", ctypes.c_int),
                ("fgs_solver", ctypes.c_int)]


FGS_PCR, FGS_THOMAS = 0, 1  # SDR_FGS_* (sdr_wls_params.fgs_solver)


FGS_KERNELS = {0: "none", 1: "lr", 2: "lrjob", 3: "th", 4: "pcr"}  # SDR_FGS_KERNEL_*


class FgsLaunch(ctypes.Structure):
    """sdr_fgs_launch: the kernel family and its lines a workgroup."""
    _fields_ = [("kernel", ctypes.c_int32), ("lines", ctypes.c_int32)]

    def as_tuple(self):
        return FGS_KERNELS[self.kernel], self.lines


class FgsPlan(ctypes.Structure):
    """sdr_fgs_plan (sdr_fgs_plan_query)."""
    _fields_ = [("row_pass", FgsLaunch), ("col_pass", FgsLaunch), ("row_job", FgsLaunch),
                ("col_job", FgsLaunch), ("cus", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def fgs_plan(w, h, nframes=1, nimg=2, num_iter=3, solver=FGS_THOMAS, cus=0):
    """The kernels an FGS call on w x h takes, as {"row_pass": (family, lines), "col_pass": ...,
    "row_job": ..., "col_job": ..., "cus": n}; cus = 0 asks the current device."""
    p = FgsPlan()
    check(lib().sdr_fgs_plan_query(int(w), int(h), int(nframes), int(nimg), int(num_iter),
                                   int(solver), int(cus), ctypes.byref(p)))
    plan = {k: getattr(p, k).as_tuple() for k in ("row_pass", "col_pass", "row_job", "col_job")}
    plan["cus"] = p.cus
    return plan


COST_KERNELS = {0: "none", 1: "k_cost", 2: "census", 3: "generic"}  # SDR_SGBM_COST_*
PATHS_KERNELS = {0: "none", 1: "k_paths", 2: "k_paths_tc"}              # SDR_SGBM_PATHS_*
SOUTH_KERNELS = {0: "none", 1: "k_south_wta", 2: "sweep"}               # SDR_SGBM_SOUTH_*
POST_ROUTES = {0: "none", 1: "speckle", 2: "median3_lr", 3: "median3_cols"}  # SDR_SGBM_POST_*


class SgbmLaunches(ctypes.Structure):
    """sdr_sgbm_launches (sdr_sgbm_plan_query, sdr_sgbm_last_plan)."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "cost_kernel", "cost_nr", "cost_k", "cost_cn", "paths_kernel", "paths_dpl", "paths_pad",
        "paths_r12", "south_kernel", "south_dpl", "south_pad", "south_np", "south_tc", "south_r12",
        "sweep_dw", "sweep_pad")] + \
               [("sweep_nslots", ctypes.c_int32 * 2), ("sweep_ntiles", ctypes.c_int32 * 2)] + \
               [(n, ctypes.c_int32) for n in ("post", "paths_chains", "south_chains", "cus", "cost_rows",
                                                "cost_bands")]

    def as_dict(self):
        """{"cost": (family, NR, K, CN), "paths": (family, DPL, PAD, R12), "south": ("k_south_wta",
        DPL, PAD, NP, TC, R12) or ("sweep", DW, PAD) or ("none",), "sweep_shape": ((nslots, ntiles)
        of the down pass, of the up pass), "post": route, "paths_chains", "south_chains", "cus",
        "cost_rows", "cost_bands" (the rows of a row band and the main bands of a one-pass cost
        launch; 0 from a plan query)}."""
        paths = (PATHS_KERNELS[self.paths_kernel],)
        if self.paths_kernel:
            paths += (self.paths_dpl, bool(self.paths_pad), bool(self.paths_r12))
        south = (SOUTH_KERNELS[self.south_kernel],)
        if self.south_kernel == 1:
            south += (self.south_dpl, bool(self.south_pad), self.south_np, bool(self.south_tc),
                      bool(self.south_r12))
        elif self.south_kernel == 2:
            south += (self.sweep_dw, bool(self.sweep_pad))
        return {"cost": (COST_KERNELS[self.cost_kernel], self.cost_nr, self.cost_k, self.cost_cn),
                "paths": paths, "south": south,
                "sweep_shape": tuple((self.sweep_nslots[i], self.sweep_ntiles[i]) for i in range(2)),
                "post": POST_ROUTES[self.post], "paths_chains": self.paths_chains,
                "south_chains": self.south_chains, "cus": self.cus, "cost_rows": self.cost_rows,
                "cost_bands": self.cost_bands}


def sgbm_plan(params, w, h, nframes=1, channels=1, cost=0, cus=0):
    """The kernels a matcher call of nframes frames of w x h takes under `params` (SgbmParams), as
    SgbmLaunches.as_dict(); cus = 0 asks the current device, any other value stays off the GPU."""
    out = SgbmLaunches()
    check(lib().sdr_sgbm_plan_query(ctypes.byref(params), int(cost), int(w), int(h), int(nframes),
                                    int(channels), int(cus), ctypes.byref(out)))
    return out.as_dict()


class SgbmRecords(ctypes.Structure):
    """sdr_sgbm_records (sdr_sgbm_records_query, sdr_sgbm_last_records)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("order", "r12", "nrec", "pix")] + \
               [(n, ctypes.c_int64) for n in ("xs", "ys", "frame", "slack", "reach")]

    def as_dict(self):
        """{"order": "row" or "col", "r12", "nrec", "pix", "xs", "ys", "frame", "slack", "reach"}
        (int16 elements; sdr.h)."""
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["order"] = "col" if self.order == 1 else "row"
        d["r12"] = bool(self.r12)
        return d


def sgbm_records(params, w, h, nframes=1, channels=1, cost=0, cus=0):
    """The path-cost records' layout of the call sgbm_plan describes, as SgbmRecords.as_dict()."""
    out = SgbmRecords()
    check(lib().sdr_sgbm_records_query(ctypes.byref(params), int(cost), int(w), int(h), int(nframes),
                                       int(channels), int(cus), ctypes.byref(out)))
    return out.as_dict()


class Segment(ctypes.Structure):
    """sdr_segment."""
    _fields_ = [(n, ctypes.c_int32) for n in ("frame", "x0", "y0", "x1", "y1")]


class RulerParams(ctypes.Structure):
    """sdr_ruler_params."""
    _fields_ = [("radius", ctypes.c_int32), ("min_count", ctypes.c_int32),
                ("min_disp", ctypes.c_float), ("conf_min", ctypes.c_float),
                ("profile", ctypes.c_int32), ("profile_cap", ctypes.c_int32)]


class Measurement(ctypes.Structure):
    """sdr_measurement (80 bytes)."""
    _fields_ = [("p0", ctypes.c_float * 3), ("p1", ctypes.c_float * 3), ("d0", ctypes.c_float),
                ("d1", ctypes.c_float), ("distance", ctypes.c_double), ("n0", ctypes.c_int32),
                ("n1", ctypes.c_int32), ("path_samples", ctypes.c_int32),
                ("path_valid", ctypes.c_int32), ("max_gap", ctypes.c_int32),
                ("z_min", ctypes.c_float), ("z_max", ctypes.c_float), ("max_dz", ctypes.c_float),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32)]


DISP_F32, DISP_S16 = 0, 1  # SDR_DISP_*


class PlaneParams(ctypes.Structure):
    """sdr_plane_params (32 bytes)."""
    _fields_ = [("iterations", ctypes.c_int32), ("min_inliers", ctypes.c_int32),
                ("inlier_px", ctypes.c_float), ("min_disp", ctypes.c_float),
                ("conf_min", ctypes.c_float), ("reserved", ctypes.c_int32 * 3)]


class Plane(ctypes.Structure):
    """sdr_plane (128 bytes)."""
    _fields_ = [("coef", ctypes.c_double * 3), ("normal", ctypes.c_double * 3),
                ("offset", ctypes.c_double), ("centroid", ctypes.c_double * 3),
                ("rms_px", ctypes.c_double), ("max_abs_px", ctypes.c_float),
                ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("frame", ctypes.c_int32),
                ("area", ctypes.c_int32), ("n_valid", ctypes.c_int32),
                ("n_inliers", ctypes.c_int32), ("fits", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32)]


class PlaneQuery(ctypes.Structure):
    """sdr_plane_query (16 bytes)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("frame", "x", "y", "plane")]


class PlaneDistance(ctypes.Structure):
    """sdr_plane_distance (32 bytes)."""
    _fields_ = [("p", ctypes.c_float * 3), ("d", ctypes.c_float), ("distance", ctypes.c_double),
                ("n", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class PlaneSearchParams(ctypes.Structure):
    """sdr_plane_search_params (64 bytes)."""
    _fields_ = [("fit", PlaneParams), ("max_planes", ctypes.c_int32), ("hypotheses", ctypes.c_int32),
                ("seed", ctypes.c_uint32), ("reserved", ctypes.c_int32 * 5)]


class PlaneSearchRound(ctypes.Structure):
    """sdr_plane_search_round (16 bytes)."""
    _fields_ = [("hypothesis", ctypes.c_int32), ("score", ctypes.c_int32), ("voids", ctypes.c_int32),
                ("stop", ctypes.c_uint32)]


class ReliefQuery(ctypes.Structure):
    """sdr_relief_query (32 bytes)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("frame", "x0", "y0", "x1", "y1", "plane", "label", "reserved")]


class ReliefParams(ctypes.Structure):
    """sdr_relief_params (64 bytes)."""
    _fields_ = [("min_disp", ctypes.c_float), ("conf_min", ctypes.c_float), ("band", ctypes.c_float),
                ("nq", ctypes.c_int32), ("permille", ctypes.c_int32 * 8), ("reserved", ctypes.c_int32 * 4)]


class Relief(ctypes.Structure):
    """sdr_relief (128 bytes)."""
    _fields_ = [("q", ctypes.c_float * 8), ("h_min", ctypes.c_float), ("h_max", ctypes.c_float),
                ("mean", ctypes.c_double), ("mean_above", ctypes.c_double),
                ("sum256", ctypes.c_int64), ("sum256_above", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("area", "n_masked", "n_valid", "n", "n_above", "n_below",
                                              "n_rejected", "frame", "plane", "label")] + \
               [("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32 * 3)]


class FootprintParams(ctypes.Structure):
    """sdr_footprint_params (64 bytes)."""
    _fields_ = [(n, ctypes.c_float) for n in ("min_disp", "conf_min", "cell", "h_lo", "h_hi")] + \
               [("grid", ctypes.c_int32), ("support", ctypes.c_int32), ("reserved", ctypes.c_int32 * 9)]


class Footprint(ctypes.Structure):
    """sdr_footprint (256 bytes)."""
    _fields_ = [("side", ctypes.c_double * 2), ("fill", ctypes.c_double), ("corner", (ctypes.c_double * 3) * 4),
                ("basis_s", ctypes.c_double * 3), ("basis_t", ctypes.c_double * 3),
                ("i0", ctypes.c_int64), ("j0", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("angle_deg", "span_s", "span_t", "area", "n_masked", "n_valid", "n",
                                              "n_outside", "n_cells_raw", "n_cells", "frame", "plane", "label")] + \
               [("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32 * 4)]


class ObjectParams(ctypes.Structure):
    """sdr_object_params (64 bytes)."""
    _fields_ = [(n, ctypes.c_float) for n in ("min_disp", "conf_min", "h_lo", "h_hi", "max_diff")] + \
               [(n, ctypes.c_int32) for n in ("connectivity", "min_pixels", "max_objects")] + \
               [("reserved", ctypes.c_int32 * 8)]


class Object(ctypes.Structure):
    """sdr_object (64 bytes)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("n", "root", "x0", "y0", "x1", "y1")] + \
               [(n, ctypes.c_int64) for n in ("sum_x", "sum_y", "sum256")] + \
               [("h_min", ctypes.c_float), ("h_max", ctypes.c_float), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_int32)]


class ObjectScan(ctypes.Structure):
    """sdr_object_scan (64 bytes)."""
    _fields_ = [("flags", ctypes.c_uint32)] + \
               [(n, ctypes.c_int32) for n in ("area", "n_masked", "n_valid", "n", "n_components", "n_kept", "count",
                                              "largest_dropped", "frame", "plane", "label")] + \
               [("reserved", ctypes.c_int32 * 4)]


class ClearanceQuery(ctypes.Structure):
    """sdr_clearance_query (32 bytes)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("frame", "x0", "y0", "x1", "y1", "plane", "label_a", "label_b")]


class ClearanceParams(ctypes.Structure):
    """sdr_clearance_params (64 bytes)."""
    _fields_ = [(n, ctypes.c_float) for n in ("min_disp", "conf_min", "h_lo", "h_hi")] + \
               [("radius", ctypes.c_int32), ("min_count", ctypes.c_int32), ("reserved", ctypes.c_int32 * 10)]


class Clearance(ctypes.Structure):
    """sdr_clearance (128 bytes)."""
    _fields_ = [("distance", ctypes.c_double), ("along", ctypes.c_double), ("across", ctypes.c_double),
                ("p_a", ctypes.c_float * 3), ("p_b", ctypes.c_float * 3), ("d_a", ctypes.c_float),
                ("d_b", ctypes.c_float)] + \
               [(n, ctypes.c_int32) for n in ("xa", "ya", "xb", "yb", "area", "n_a", "n_b", "m_a", "m_b", "frame",
                                              "plane", "label_a", "label_b")] + \
               [("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32 * 4)]


CLEARANCE_MAX_QUERIES = 64  # SDR_CLEARANCE_MAX_QUERIES
DEBUG_CLEARANCE_PRUNE = 1   # SDR_DEBUG_CLEARANCE_PRUNE (sdr_clearance_debug_knob)


class FuseParams(ctypes.Structure):
    """sdr_fuse_params (32 bytes)."""
    _fields_ = [(n, ctypes.c_float) for n in ("min_disp", "conf_min", "tol", "fill")] + \
               [("min_count", ctypes.c_int32), ("mode", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


class Fusion(ctypes.Structure):
    """sdr_fusion (64 bytes)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("frames", "width", "height", "mode", "n_fused", "n_empty", "n_sparse",
                                              "n_unstable", "n_filled", "n_replaced")] + \
               [(n, ctypes.c_int64) for n in ("sum_support", "n_disagree", "reserved")]


FUSE_MEAN, FUSE_MEDIAN = 0, 1  # SDR_FUSE_*
FUSE_MAX_FRAMES = 32           # SDR_FUSE_MAX_FRAMES


_lib = None
_path = LIB_PATH


def use_library(path: str) -> None:
    """Scripts only (experiment A/B, scripts/kbench.py): load `path` instead of lib/libsdr.so.
    Must be called before the first use of the engine."""
    global _path
    if _lib is not None:
        raise RuntimeError("the engine library is already loaded")
    _path = os.path.abspath(path)

# (name, restype, argtypes) for every function declared in include/sdr/sdr.h
_c = ctypes
_vp = _c.c_void_p
_sz = _c.c_size_t
_i = _c.c_int
_PP = _c.POINTER(SgbmParams)
SIGNATURES = [
    ("sdr_sgbm_params_default", None, [_PP]),
    ("sdr_right_matcher_params", None, [_PP, _PP]),
    ("sdr_sgbm_create", _i, [_PP, _i, _c.POINTER(_vp)]),
    ("sdr_sgbm_destroy", _i, [_vp]),
    ("sdr_sgbm_set_params", _i, [_vp, _PP]),
    ("sdr_sgbm_get_params", _i, [_vp, _PP]),
    ("sdr_sgbm_set_cost", _i, [_vp, _i]),
    ("sdr_sgbm_get_cost", _i, [_vp]),
    ("sdr_sgbm_set_stream", _i, [_vp, _vp]),
    ("sdr_sgbm_set_stream_ex", _i, [_vp, _vp, _i]),
    ("sdr_sgbm_reset_stream", _i, [_vp]),
    ("sdr_sgbm_get_stream", _vp, [_vp]),
    ("sdr_sgbm_compute", _i, [_vp, _vp, _vp, _i, _i, _i, _sz, _vp, _sz]),
    ("sdr_sgbm_compute_device", _i, [_vp, _vp, _vp, _i, _i, _sz, _sz, _i, _vp, _sz, _sz]),
    ("sdr_sgbm_compute_device_cn", _i, [_vp, _vp, _vp, _i, _i, _i, _sz, _sz, _i, _vp, _sz, _sz]),
    ("sdr_host_alloc", _i, [_sz, _c.POINTER(_c.c_void_p)]),
    ("sdr_host_free", _i, [_vp]),
    ("sdr_sgbm_compute_reproject", _i,
     [_vp, _vp, _vp, _i, _i, _sz, _vp, _sz, _c.POINTER(_c.c_double), _i, _vp, _sz]),
    ("sdr_sgbm_compute_reproject_device", _i,
     [_vp, _vp, _vp, _i, _i, _sz, _sz, _i, _vp, _c.POINTER(_c.c_double), _i, _vp]),
    ("sdr_reproject", _i, [_vp, _i, _i, _sz, _c.POINTER(_c.c_double), _i, _vp, _sz]),
    ("sdr_reproject_device", _i, [_vp, _i, _i, _sz, _c.POINTER(_c.c_double), _i, _vp, _sz, _i, _vp]),
    ("sdr_disp16_reproject_device", _i,
     [_vp, _i, _i, _sz, _c.POINTER(_c.c_double), _i, _vp, _sz, _i, _vp]),
    ("sdr_disp16_to_float_device", _i, [_vp, _vp, _sz, _vp]),
    ("sdr_filter_speckles_device", _i, [_vp, _i, _i, _i, _i, _i, _i, _vp]),
    ("sdr_bgr2gray_device", _i, [_vp, _i, _i, _sz, _vp, _sz, _i, _vp]),
    ("sdr_resize_area_half_device", _i, [_vp, _i, _i, _sz, _vp, _sz, _i, _vp]),
    ("sdr_stereo_class_compute", _i,
     [_vp, _vp, _vp, _vp, _vp, _i, _i, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    ("sdr_wls_params_for_sgbm", None, [_PP, _c.POINTER(WlsParams)]),
    ("sdr_wls_create", _i, [_c.POINTER(WlsParams), _i, _c.POINTER(_vp)]),
    ("sdr_wls_destroy", _i, [_vp]),
    ("sdr_wls_set_params", _i, [_vp, _c.POINTER(WlsParams)]),
    ("sdr_wls_get_params", _i, [_vp, _c.POINTER(WlsParams)]),
    ("sdr_wls_set_stream", _i, [_vp, _vp]),
    ("sdr_wls_get_stream", _vp, [_vp]),
    ("sdr_wls_reset_stream", _i, [_vp]),
    ("sdr_rectifier_reset_stream", _i, [_vp]),
    ("sdr_wls_get_roi", _i, [_vp, _i, _i, _c.POINTER(_c.c_int)]),
    ("sdr_wls_filter_device", _i, [_vp, _vp, _vp, _vp, _i, _i, _sz, _sz, _i, _vp, _vp]),
    ("sdr_wls_filter", _i, [_vp, _vp, _vp, _vp, _i, _i, _sz, _vp, _vp]),
    ("sdr_init_undistort_rectify_map", _i,
     [_c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _i, _c.POINTER(_c.c_double),
      _c.POINTER(_c.c_double), _i, _i, _i, _i, _vp, _vp]),
    ("sdr_remap_bilinear_device", _i, [_vp, _i, _i, _sz, _sz, _i, _vp, _vp, _i, _i, _vp, _sz, _sz, _i, _vp]),
    ("sdr_rectifier_create", _i,
     [_c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _i, _c.POINTER(_c.c_double),
      _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _i,
      _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _i, _i, _i, _i, _c.POINTER(_vp)]),
    ("sdr_rectifier_destroy", _i, [_vp]),
    ("sdr_rectifier_set_stream", _i, [_vp, _vp]),
    ("sdr_rectifier_get_maps", _i, [_vp, _i, _vp, _vp]),
    ("sdr_rectify_device", _i, [_vp, _vp, _vp, _sz, _sz, _i, _i, _vp, _vp, _sz, _sz]),
    ("sdr_rectify_sbs_device", _i, [_vp, _vp, _sz, _sz, _i, _vp, _vp, _vp, _vp]),
    ("sdr_stereo_class_compute_device", _i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    ("sdr_stereo_class_depth_device", _i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp,
                                           _c.POINTER(_c.c_double), _vp]),
    ("sdr_xyz_to_cloud_device", _i, [_vp, _vp, _sz, _sz, _i, _i, _i, _vp, _vp]),
    ("sdr_voxel_grid_device", _i, [_vp, _i, _c.c_float, _c.c_float, _c.c_float, _vp,
                                   _c.POINTER(_i), _c.POINTER(_i), _vp]),
    ("sdr_pcd_header", _i, [_i, _i, _c.c_char_p, _sz]),
    ("sdr_write_pcd_binary", _i, [_c.c_char_p, _vp, _i, _i]),
    ("sdr_fgs_filter_device", _i, [_vp, _sz, _i, _i, _c.c_double, _c.c_double, _c.c_double, _i,
                                   _vp, _i, _i, _vp]),
    ("sdr_fgs_rcp_selftest", _i, [_i, _c.POINTER(_c.c_uint)]),
    ("sdr_fgs_plan_query", _i, [_i, _i, _i, _i, _i, _i, _i, _c.POINTER(FgsPlan)]),
    ("sdr_colormap_lut", _i, [_i, _vp]),
    ("sdr_display_create", _i, [_i, _c.POINTER(_vp)]),
    ("sdr_display_destroy", _i, [_vp]),
    ("sdr_display_set_stream", _i, [_vp, _vp]),
    ("sdr_display_reset_stream", _i, [_vp]),
    ("sdr_display_reset", _i, [_vp]),
    ("sdr_show_disparity_map_device", _i, [_vp, _vp, _i, _i, _sz, _sz, _i, _i, _vp]),
    ("sdr_show_depth_map_device", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _c.POINTER(_c.c_double)]),
    ("sdr_depth_coverage_device", _i, [_vp, _vp, _i, _i, _i, _i, _c.POINTER(_c.c_double)]),
    ("sdr_disparity_overlay_device", _i, [_vp, _vp, _vp, _sz, _sz, _i, _i, _i, _vp, _vp, _vp]),
    ("sdr_show_disparity_map", _i, [_vp, _vp, _i, _i, _sz, _i, _vp, _sz]),
    ("sdr_show_depth_map", _i, [_vp, _vp, _i, _i, _i, _c.POINTER(_c.c_double), _vp, _c.POINTER(_c.c_double)]),
    ("sdr_disparity_overlay", _i, [_vp, _vp, _vp, _sz, _i, _i, _vp, _vp]),
    ("sdr_depth_coverage", _i, [_vp, _vp, _i, _i, _i, _c.POINTER(_c.c_double)]),
    ("sdr_sgbm_scratch_bytes", _sz, [_PP, _i, _i, _i]),
    ("sdr_sgbm_scratch_bytes_cn", _sz, [_PP, _i, _i, _i, _i]),
    ("sdr_sgbm_scratch_bytes_ex", _sz, [_PP, _i, _i, _i, _i, _i]),
    ("sdr_sgbm_enable_timing", _i, [_vp, _i]),
    ("sdr_sgbm_last_timing", _i, [_vp, _c.POINTER(_c.c_float), _c.POINTER(_c.c_float),
                                  _c.POINTER(_c.c_float)]),
    ("sdr_selftest_wave_ops", _i, [_c.POINTER(_c.c_int)]),
    ("sdr_sgbm_debug_stage", _i, [_vp, _i, _vp, _sz]),
    ("sdr_sgbm_kernel_time", _i, [_vp, _i, _i, _c.POINTER(_c.c_float), _c.POINTER(_c.c_int)]),
    ("sdr_sgbm_last_status", _i, [_vp]),
    ("sdr_stream_probe", _i, [_i, _sz, _i, _c.POINTER(_c.c_double)]),
    ("sdr_stream_probe_ex", _i, [_i, _sz, _i, _c.POINTER(_c.c_double)]),
    ("sdr_sgbm_debug_knob", _i, [_vp, _i, _i]),
    ("sdr_sgbm_plan_query", _i, [_PP, _i, _i, _i, _i, _i, _i, _c.POINTER(SgbmLaunches)]),
    ("sdr_sgbm_last_plan", _i, [_vp, _c.POINTER(SgbmLaunches)]),
    ("sdr_sgbm_records_query", _i, [_PP, _i, _i, _i, _i, _i, _i, _c.POINTER(SgbmRecords)]),
    ("sdr_sgbm_last_records", _i, [_vp, _c.POINTER(SgbmRecords)]),
    ("sdr_ruler_params_default", None, [_c.POINTER(RulerParams)]),
    ("sdr_measure_disp_device", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _c.POINTER(_c.c_double),
                                     _c.POINTER(RulerParams), _vp, _i, _vp, _vp, _vp]),
    ("sdr_measure_xyz_device", _i, [_vp, _sz, _sz, _i, _i, _i, _vp, _i, _vp, _vp]),
    ("sdr_measure_disp", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _c.POINTER(_c.c_double),
                              _c.POINTER(RulerParams), _vp, _i, _vp, _vp]),
    ("sdr_measure_xyz", _i, [_vp, _sz, _sz, _i, _i, _i, _vp, _i, _vp]),
    ("sdr_measurements_csv", _i, [_vp, _vp, _vp, _i, _i, _vp, _sz]),
    ("sdr_plane_params_default", None, [_c.POINTER(PlaneParams)]),
    ("sdr_fit_planes_device", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _c.POINTER(_c.c_double),
                                   _c.POINTER(PlaneParams), _vp, _i, _vp, _vp]),
    ("sdr_plane_distance_device", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _c.POINTER(_c.c_double),
                                       _c.POINTER(RulerParams), _vp, _i, _vp, _i, _vp, _vp]),
    ("sdr_fit_planes", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _c.POINTER(_c.c_double),
                            _c.POINTER(PlaneParams), _vp, _i, _vp]),
    ("sdr_plane_distance", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _c.POINTER(_c.c_double),
                                _c.POINTER(RulerParams), _vp, _i, _vp, _i, _vp]),
    ("sdr_plane_search_params_default", None, [_c.POINTER(PlaneSearchParams)]),
    ("sdr_find_planes_device", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _c.POINTER(_c.c_double),
                                    _c.POINTER(PlaneSearchParams), _vp, _vp, _vp, _vp, _vp, _vp]),
    ("sdr_find_planes", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _c.POINTER(_c.c_double),
                             _c.POINTER(PlaneSearchParams), _vp, _vp, _vp, _vp, _vp]),
    ("sdr_relief_params_default", None, [_c.POINTER(ReliefParams)]),
    ("sdr_plane_relief_device", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _vp, _c.POINTER(_c.c_double),
                                     _c.POINTER(ReliefParams), _vp, _i, _vp, _i, _vp, _vp]),
    ("sdr_plane_relief", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _vp, _c.POINTER(_c.c_double),
                              _c.POINTER(ReliefParams), _vp, _i, _vp, _i, _vp]),
    ("sdr_footprint_params_default", None, [_c.POINTER(FootprintParams)]),
    ("sdr_footprint_direction", _i, [_i, _c.POINTER(_c.c_int32), _c.POINTER(_c.c_int32)]),
    ("sdr_plane_footprint_device", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _vp, _c.POINTER(_c.c_double),
                                        _c.POINTER(FootprintParams), _vp, _i, _vp, _i, _vp, _vp]),
    ("sdr_plane_footprint", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _vp, _c.POINTER(_c.c_double),
                                 _c.POINTER(FootprintParams), _vp, _i, _vp, _i, _vp]),
    ("sdr_object_params_default", None, [_c.POINTER(ObjectParams)]),
    ("sdr_find_objects_device", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _vp, _c.POINTER(_c.c_double),
                                     _c.POINTER(ObjectParams), _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    ("sdr_find_objects", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _vp, _c.POINTER(_c.c_double),
                              _c.POINTER(ObjectParams), _vp, _i, _vp, _vp, _vp, _vp]),
    ("sdr_clearance_params_default", None, [_c.POINTER(ClearanceParams)]),
    ("sdr_clearance_device", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _vp, _c.POINTER(_c.c_double),
                                  _c.POINTER(ClearanceParams), _vp, _i, _vp, _i, _vp, _vp]),
    ("sdr_clearance", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _vp, _c.POINTER(_c.c_double),
                           _c.POINTER(ClearanceParams), _vp, _i, _vp, _i, _vp]),
    ("sdr_clearance_debug_knob", _i, [_i, _i]),
    ("sdr_fuse_params_default", None, [_c.POINTER(FuseParams)]),
    ("sdr_fuse_disp_device", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _c.POINTER(FuseParams), _vp, _vp, _vp, _vp,
                                  _vp]),
    ("sdr_fuse_disp", _i, [_vp, _i, _sz, _sz, _i, _i, _i, _vp, _c.POINTER(FuseParams), _vp, _vp, _vp, _vp]),
    ("sdr_build_id", _c.c_char_p, []),
    ("sdr_last_error", _c.c_char_p, []),
    ("sdr_abi_version", _i, []),
]


def lib():
    """Loads lib/libsdr.so (raises if the HIP extension has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_path):
            raise RuntimeError(
                f"HIP engine library missing: {_path}. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950).")
        L = ctypes.CDLL(_path)
        for name, res, args in SIGNATURES:
            # an earlier build loaded for an A/B (use_library) may lack an entry this header added
            # since; lib/libsdr.so itself must export every one
            if _path != LIB_PATH and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int):
    if rc != SDR_OK:
        raise SDRError(rc, lib().sdr_last_error().decode(errors="replace"))
    return rc
