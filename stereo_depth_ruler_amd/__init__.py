"""stereo_depth_ruler_amd -- MI355X-native drop-in for the stereo hot path of
Amar-Aliaga/Stereo_Depth_Ruler: cv::StereoSGBM::compute + cv::reprojectImageTo3D as hand-written
HIP/CDNA4 kernels behind a C ABI (include/sdr/sdr.h), with an OpenCV-shaped Python surface.
"""
from ._lib import SDRError, SgbmParams, WlsParams, LIB_PATH  # noqa: F401
from .sgbm import (  # noqa: F401
    COST_BT, COST_CENSUS, MODE_HH, MODE_HH4, MODE_SGBM, MODE_SGBM_3WAY, StereoSGBM, createRightMatcher,
    cvt_bgr2gray, disparity_to_float, filterSpeckles, host_empty, reprojectImageTo3D, resize_area_half,
)
from . import cloud  # noqa: F401
from . import display  # noqa: F401
from .display import COLORMAP_JET, COLORMAP_TURBO, Display, colormap_lut  # noqa: F401
from .ximgproc import (  # noqa: F401
    DisparityWLSFilter, createDisparityWLSFilter, fastGlobalSmootherFilter,
)
from .ruler import (  # noqa: F401
    MEASUREMENT_DTYPE, PDIST_NO_PLANE, PDIST_OUT_OF_RANGE, PDIST_VALID, PLANE_DEGENERATE,
    PLANE_DISTANCE_DTYPE, PLANE_DTYPE, PLANE_NONFINITE, PLANE_OK, PLANE_OUT_OF_RANGE,
    PLANE_SEARCH_ROUND_DTYPE, SEARCH_FEW_INLIERS, SEARCH_LOW_SCORE, SEARCH_NO_HYPOTHESIS, SEARCH_NOT_RUN,
    SEARCH_RAN, SEARCH_REFIT_DEGENERATE, MeasurementLog, Ruler, plane_angle_deg,
    RELIEF_DTYPE, RELIEF_EMPTY, RELIEF_NO_PLANE, RELIEF_OUT_OF_RANGE, RELIEF_VALID, as_relief_queries,
    FOOTPRINT_CLIPPED, FOOTPRINT_DTYPE, FOOTPRINT_EMPTY, FOOTPRINT_NO_PLANE, FOOTPRINT_OUT_OF_RANGE, FOOTPRINT_VALID,
    footprint_length_width,
    OBJECT_CUT, OBJECT_DTYPE, OBJECT_SCAN_DTYPE, OBJECT_VALID, OBJECTS_EMPTY, OBJECTS_NO_PLANE, OBJECTS_OUT_OF_RANGE,
    OBJECTS_TRUNCATED, OBJECTS_VALID,
    CLEARANCE_DTYPE, CLEARANCE_EMPTY, CLEARANCE_NO_PLANE, CLEARANCE_OUT_OF_RANGE, CLEARANCE_VALID,
    as_clearance_queries,
    FUSE_MEAN, FUSE_MEDIAN, FUSION_DTYPE, FuseParams,
)
from .stereo_disparity import StereoDisparity  # noqa: F401

__all__ = [
    "SDRError", "SgbmParams", "StereoSGBM", "createRightMatcher", "reprojectImageTo3D",
    "disparity_to_float", "filterSpeckles", "cvt_bgr2gray", "resize_area_half",
    "MODE_SGBM", "MODE_HH", "MODE_SGBM_3WAY", "MODE_HH4", "WlsParams", "DisparityWLSFilter",
    "createDisparityWLSFilter", "fastGlobalSmootherFilter", "StereoDisparity", "Display",
    "colormap_lut", "COLORMAP_JET", "COLORMAP_TURBO", "host_empty", "COST_BT", "COST_CENSUS",
    "Ruler", "MeasurementLog", "MEASUREMENT_DTYPE", "PLANE_DTYPE", "PLANE_DISTANCE_DTYPE",
    "PLANE_OK", "PLANE_DEGENERATE", "PLANE_NONFINITE", "PLANE_OUT_OF_RANGE", "PDIST_VALID",
    "PDIST_OUT_OF_RANGE", "PDIST_NO_PLANE", "plane_angle_deg", "PLANE_SEARCH_ROUND_DTYPE", "SEARCH_RAN",
    "SEARCH_NO_HYPOTHESIS", "SEARCH_LOW_SCORE", "SEARCH_REFIT_DEGENERATE", "SEARCH_FEW_INLIERS", "SEARCH_NOT_RUN",
    "RELIEF_DTYPE", "RELIEF_VALID", "RELIEF_OUT_OF_RANGE", "RELIEF_NO_PLANE", "RELIEF_EMPTY", "as_relief_queries",
    "FOOTPRINT_DTYPE", "FOOTPRINT_VALID", "FOOTPRINT_OUT_OF_RANGE", "FOOTPRINT_NO_PLANE", "FOOTPRINT_EMPTY",
    "FOOTPRINT_CLIPPED", "footprint_length_width",
    "OBJECT_DTYPE", "OBJECT_SCAN_DTYPE", "OBJECT_VALID", "OBJECT_CUT", "OBJECTS_VALID", "OBJECTS_OUT_OF_RANGE",
    "OBJECTS_NO_PLANE", "OBJECTS_EMPTY", "OBJECTS_TRUNCATED",
    "CLEARANCE_DTYPE", "CLEARANCE_VALID", "CLEARANCE_OUT_OF_RANGE", "CLEARANCE_NO_PLANE", "CLEARANCE_EMPTY",
    "as_clearance_queries",
    "FUSE_MEAN", "FUSE_MEDIAN", "FUSION_DTYPE", "FuseParams",
]
