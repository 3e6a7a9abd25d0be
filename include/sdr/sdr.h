/*
 * sdr.h -- C ABI of the MI355X-native stereo disparity engine (stereo_depth_ruler_amd).
 *
 * Drop-in boundary for the reference's hot path: every entry point takes plain pointers and
 * sizes (no OpenCV, no torch types) and replaces one OpenCV call the reference makes:
 *
 *   sdr_sgbm_create / sdr_sgbm_set_params
 *       <- cv::StereoSGBM::create(0, 80, 5, 600, 2400, 1, 63, 12, 200, 2, MODE_SGBM_3WAY)
 *          stereo_vision/src/stereo_disparity.cpp:5-9, point_cloud/src/pcd_write.cpp:102-108
 *   sdr_sgbm_compute / sdr_sgbm_compute_device
 *       <- matcher->compute(L, R, disp)  stereo_vision/src/stereo_disparity.cpp:27-28,
 *          sgbm->compute(left_gray, right_gray, disp)  point_cloud/src/pcd_write.cpp:111
 *   sdr_reproject / sdr_reproject_device / sdr_disp16_reproject_device
 *       <- cv::reprojectImageTo3D(disp, xyz, Q, handleMissing)  stereo_disparity.cpp:78,
 *          pcd_write.cpp:116 (with disp.convertTo(CV_32F, 1/16) at pcd_write.cpp:112)
 *   sdr_bgr2gray_device / sdr_resize_area_half_device
 *       <- cv::cvtColor(BGR2GRAY) / cv::resize(0.5, INTER_AREA)  stereo_disparity.cpp:19-24
 *   sdr_right_matcher_params
 *       <- cv::ximgproc::createRightMatcher(matcher)  stereo_disparity.cpp:10
 *
 * Error behaviour mirrors the CV_Assert()s of StereoSGBMImpl::compute: a negative status is
 * returned instead of throwing; sdr_last_error() returns the thread's last message.
 * Threading: one handle = one HIP stream + scratch; a handle must not be used by two threads at
 * once (as with cv::StereoSGBM, whose impl owns a scratch buffer); handles are independent.
 */
#ifndef SDR_SDR_H
#define SDR_SDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDR_ABI_VERSION 4

/* cv::StereoSGBM::MODE_* */
enum { SDR_MODE_SGBM = 0, SDR_MODE_HH = 1, SDR_MODE_SGBM_3WAY = 2, SDR_MODE_HH4 = 3 };

/* uniqueness test form: AUTO = 3WAY uses OpenCV's SIMD threshold form
 * cost <= (100*minS)/(100-u), SGBM/HH the scalar form cost*(100-u) < minS*100 */
enum { SDR_UNIQ_AUTO = 0, SDR_UNIQ_SCALAR = 1, SDR_UNIQ_SIMD = 2 };

/* status codes */
enum {
    SDR_OK = 0,
    SDR_ERR_ARG = -1,         /* null pointer, non-positive size, bad stride */
    SDR_ERR_NUMDISP = -2,     /* numDisparities <= 0 or not a multiple of 16 (OpenCV assert) */
    SDR_ERR_MODE = -3,        /* unknown mode */
    SDR_ERR_SIZE = -4,        /* image too narrow for the disparity range / block size */
    SDR_ERR_TYPE = -5,        /* channels other than 1 or 3 (CV_8UC1 / CV_8UC3) */
    SDR_ERR_DEVICE = -6,      /* HIP runtime error */
    SDR_ERR_NOMEM = -7,
    SDR_ERR_LIMIT = -8        /* numDisparities > 512, or outside the int16 cost domain */
};

/* Field order and meaning of cv::StereoSGBM::create(...) + two knobs OpenCV fixes internally. */
typedef struct sdr_sgbm_params {
    int minDisparity;
    int numDisparities;
    int blockSize;
    int P1;
    int P2;
    int disp12MaxDiff;
    int preFilterCap;
    int uniquenessRatio;
    int speckleWindowSize;
    int speckleRange;
    int mode;
    int nstripes;   /* MODE_SGBM_3WAY stripes; 0 -> 4 (OpenCV 4.x fixed value) */
    int uniq_rule;  /* SDR_UNIQ_* */
} sdr_sgbm_params;

typedef struct sdr_sgbm sdr_sgbm;
typedef struct sdr_wls sdr_wls; /* ximgproc::DisparityWLSFilter (below) */

/* StereoSGBM::create defaults: (0, 16, 3, 0, 0, 0, 0, 0, 0, 0, MODE_SGBM) */
void sdr_sgbm_params_default(sdr_sgbm_params* p);
/* createRightMatcher: minD' = -(minD+numD)+1, uniqueness 0, disp12MaxDiff 1e6, speckle off */
void sdr_right_matcher_params(const sdr_sgbm_params* left, sdr_sgbm_params* right);

int sdr_sgbm_create(const sdr_sgbm_params* p, int device, sdr_sgbm** out);
int sdr_sgbm_destroy(sdr_sgbm* h);
int sdr_sgbm_set_params(sdr_sgbm* h, const sdr_sgbm_params* p);
int sdr_sgbm_get_params(const sdr_sgbm* h, sdr_sgbm_params* p);

/* The matching cost of a handle (not part of sdr_sgbm_params, whose layout is fixed): a new handle
 * uses SDR_COST_BT, OpenCV's Birchfield-Tomasi cost on the Sobel-prefiltered and raw images.
 *
 * SDR_COST_CENSUS_9X7 is this project's own definition (OpenCV has no census cost):
 *   - Descriptor T(y, x) of an 8-bit single-channel H x W image I, a 62-bit value in a uint64:
 *     bit k (k = 0 the LSB) is 1 iff I(clamp(y+dy, 0, H-1), clamp(x+dx, 0, W-1)) < I(y, x)
 *     (strict <, replicated border), k counting the offsets (dy, dx) in row-major order over
 *     dy = -3..3, dx = -4..4 with the centre (0, 0) skipped; bits 62 and 63 are 0.  The transform
 *     reads raw intensities: no Sobel prefilter, preFilterCap is ignored.
 *   - Pixel cost pc(y, x, d) = popcount(T_left(y, x) XOR T_right(y, x - d)), in [0, 62], for the
 *     same matched columns and disparities as the BT cost.
 *   - Cost volume: C = P2 + the blockSize x blockSize box sum of pc with the BT path's border
 *     rules (blockSize defaulting stays OpenCV's); everything after C is unchanged.
 *   - Cost domain: 2*P2 + 62*blockSize^2 <= 32767, else SDR_ERR_LIMIT (the BT bound, which depends
 *     on preFilterCap, does not apply).  A census block cost is at most 62*blockSize^2, so P1 / P2
 *     scaled for BT are large for it.
 *   - Limits, each refused loudly: 3-channel input (SDR_ERR_TYPE), effective blockSize > 11 and
 *     numDisparities > 256 (SDR_ERR_LIMIT).
 * Any strictly increasing intensity change of one image leaves the census disparity unchanged.
 * The paired class-path launch needs equal cost types; matchers that differ run unpaired. */
enum { SDR_COST_BT = 0, SDR_COST_CENSUS_9X7 = 1 };
int sdr_sgbm_set_cost(sdr_sgbm* h, int cost); /* SDR_ERR_ARG on a null handle or an unknown value */
int sdr_sgbm_get_cost(const sdr_sgbm* h);     /* SDR_COST_*, or a negative status on a null handle */
/* HIP stream (hipStream_t) the handle launches on (NULL = the HIP null stream, e.g. torch's
 * default stream); a new handle uses a stream of its own, restored by sdr_sgbm_reset_stream.
 * Changing the stream orders the handle's earlier work before the new stream's.
 * sdr_sgbm_set_stream binds a TRANSIENT stream: the caller may destroy it as soon as the calls
 * made on it have returned (and its work is done, as hipStreamDestroy requires); the handle
 * never touches it afterwards -- at the end of every call on it the handle records an event
 * there and relays it through its own stream, which later switches, sdr_sgbm_last_status and
 * sdr_sgbm_destroy use instead.  The next call must follow a set_stream / reset_stream naming a
 * live stream.
 * sdr_sgbm_set_stream_ex(.., SDR_STREAM_PERSISTENT) binds a stream that outlives the handle's use
 * of it (a pooled stream such as torch's, or one the caller keeps until it has moved the handle
 * off it): no event is recorded per call, only at the next switch (an event record is a queue
 * barrier: ~6 us of idle queue per class-path frame when recorded after every call).  The
 * Python layer passes the flag for torch's pooled and default streams, not for external ones. */
enum { SDR_STREAM_PERSISTENT = 1 };
int sdr_sgbm_set_stream(sdr_sgbm* h, void* stream);
int sdr_sgbm_set_stream_ex(sdr_sgbm* h, void* stream, int flags);
int sdr_sgbm_reset_stream(sdr_sgbm* h);
void* sdr_sgbm_get_stream(const sdr_sgbm* h);

/* Host-pointer compute (H2D, compute, D2H, synchronous): left/right 8-bit with `channels` (1 or 3)
 * interleaved channels, `stride` bytes per row; disp int16 (1/16 px), `disp_stride` ELEMENTS per row.  Replaces StereoSGBM::compute on
 * host cv::Mat (stereo_disparity.cpp:27-34, pcd_write.cpp:111).  The copies go through the
 * handle's persistent page-locked staging in ~1 MB row chunks that overlap the CPU copy with the
 * DMA; no allocation per call once the handle has seen the frame size. */
int sdr_sgbm_compute(sdr_sgbm* h, const uint8_t* left, const uint8_t* right, int width, int height,
                     int channels, size_t stride, int16_t* disp, size_t disp_stride);

/* Host-pointer form of the fused hot path of pcd_write.cpp:111-116 (synchronous): compute ->
 * convertTo(CV_32F, 1/16) -> reprojectImageTo3D(Q, handle_missing) with the disparity kept on
 * the device; xyz float32x3 rows of `xyz_stride` ELEMENTS (>= 3*width).  disp (optional, may be
 * NULL) receives the int16 disparity as sdr_sgbm_compute would, its copy-out overlapping the
 * reprojection. */
int sdr_sgbm_compute_reproject(sdr_sgbm* h, const uint8_t* left, const uint8_t* right, int width,
                               int height, size_t stride, int16_t* disp, size_t disp_stride,
                               const double Q[16], int handle_missing, float* xyz,
                               size_t xyz_stride);

/* Device-pointer batch compute, asynchronous on the handle's stream: nframes frames spaced
 * frame_stride bytes (inputs) / disp_frame_stride elements (output) apart.  Once a call of the
 * same shape has sized the scratch, the enqueue allocates nothing and may be captured into a
 * hipGraph on the handle's stream (hipStreamBeginCapture, global mode) and replayed; a captured
 * batched MODE_HH call takes the per-direction chains instead of the row sweeps. */
int sdr_sgbm_compute_device(sdr_sgbm* h, const uint8_t* d_left, const uint8_t* d_right,
                            int width, int height, size_t stride, size_t frame_stride,
                            int nframes, int16_t* d_disp, size_t disp_stride,
                            size_t disp_frame_stride);

/* sdr_sgbm_compute_device for 8-bit images with `channels` (1 or 3) interleaved channels (stride
 * and frame_stride in bytes): StereoSGBM::compute on CV_8UC3 input, whose calcPixelCostBT sums each
 * channel's Sobel and raw costs (stereosgbm.cpp, cn == 3 branch). */
int sdr_sgbm_compute_device_cn(sdr_sgbm* h, const uint8_t* d_left, const uint8_t* d_right,
                               int width, int height, int channels, size_t stride,
                               size_t frame_stride, int nframes, int16_t* d_disp,
                               size_t disp_stride, size_t disp_frame_stride);

/* Fused hot path of point_cloud/src/pcd_write.cpp:111-116 on device: compute + convertTo(1/16)
 * + reprojectImageTo3D(Q, handle_missing) -> xyz float32x3 [nframes][height][width][3]. */
int sdr_sgbm_compute_reproject_device(sdr_sgbm* h, const uint8_t* d_left, const uint8_t* d_right,
                                      int width, int height, size_t stride, size_t frame_stride,
                                      int nframes, int16_t* d_disp, const double Q[16],
                                      int handle_missing, float* d_xyz);

/* reprojectImageTo3D on a CV_32F disparity (host pointers, synchronous; per-thread persistent
 * device buffers and page-locked staging, no allocation per call). */
int sdr_reproject(const float* disp, int width, int height, size_t disp_stride, const double Q[16],
                  int handle_missing, float* xyz, size_t xyz_stride);
/* Device versions (asynchronous on `stream`, a hipStream_t; NULL = default stream). */
int sdr_reproject_device(const float* d_disp, int width, int height, size_t disp_stride,
                         const double Q[16], int handle_missing, float* d_xyz, size_t xyz_stride,
                         int nframes, void* stream);
int sdr_disp16_reproject_device(const int16_t* d_disp, int width, int height, size_t disp_stride,
                                const double Q[16], int handle_missing, float* d_xyz,
                                size_t xyz_stride, int nframes, void* stream);
/* cv::filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on dense int16 frames [nframes][H][W],
 * in place, asynchronous on `stream`.  This is the post-filter StereoSGBM::compute applies with
 * newVal = (minDisparity-1)*16, maxDiff = 16*speckleRange; scratch is
 * stream-ordered, from a device memory pool the library keeps for the process (freed blocks stay
 * mapped for the next call). */
int sdr_filter_speckles_device(int16_t* d_img, int width, int height, int nframes, int newVal,
                               int maxSpeckleSize, int maxDiff, void* stream);
/* disp.convertTo(f, CV_32F, 1/16) on device. */
int sdr_disp16_to_float_device(const int16_t* d_disp, float* d_out, size_t n, void* stream);

/* Class-path pre-steps on device (stereo_disparity.cpp:19-24). */
int sdr_bgr2gray_device(const uint8_t* d_bgr, int width, int height, size_t bgr_stride,
                        uint8_t* d_gray, size_t gray_stride, int nframes, void* stream);
int sdr_resize_area_half_device(const uint8_t* d_src, int width, int height, size_t stride,
                                uint8_t* d_dst, size_t dst_stride, int nframes, void* stream);

/* StereoDisparity::computeDisparity class path (stereo_disparity.cpp:17-39) on host BGR frames:
 * cvtColor(BGR2GRAY) -> resize(0.5, INTER_AREA) -> left->compute(L, R) -> right->compute(R, L)
 * -> wls->filter(dl, left_small, filtered, dr) -> convertTo(CV_32F, 1/16), all on the left
 * matcher's device.  out: float (height/2)x(width/2).  right and wls may be NULL (no WLS: out is
 * the left matcher's disparity).  disp_left/disp_right/filtered (int16) and conf (float, the
 * getConfidenceMap() of stereo_disparity.cpp:36) are optional host outputs of (h/2)x(w/2). */
int sdr_stereo_class_compute(sdr_sgbm* left, sdr_sgbm* right, sdr_wls* wls,
                             const uint8_t* bgr_left, const uint8_t* bgr_right, int width,
                             int height, size_t bgr_stride, float* out, size_t out_stride,
                             int16_t* disp_left, int16_t* disp_right, int16_t* filtered,
                             float* conf);

/* ---- ximgproc DisparityWLSFilter / FastGlobalSmootherFilter (class path, stereo_disparity.cpp:11-13,31,36) ----
 * Field meaning follows opencv_contrib 4.6 ximgproc (disparity_filters.cpp, fgs_filter.cpp):
 * the valid ROI of a W x H left map is (left_offset, top_offset, W-left-right, H-top-bottom). */
typedef struct sdr_wls_params {
    double lambda;                  /* setLambda (default 8000; the reference sets 8000) */
    double sigma_color;             /* setSigmaColor (default 1.5; the reference sets 1.1) */
    int lrc_thresh;                 /* setLRCthresh (24) */
    int depth_discontinuity_radius; /* setDepthDiscontinuityRadius (SGBM: ceil(0.5*blockSize)) */
    float roll_off;                 /* depth_discontinuity_roll_off_factor (0.001) */
    double lambda_attenuation;      /* FGS lambda attenuation per iteration (0.25) */
    int num_iter;                   /* FGS iterations (3) */
    int left_offset, right_offset, top_offset, bottom_offset;
    int min_disp;                   /* outside-ROI value is 16*(min_disp-1) */
    int fgs_solver;                 /* SDR_FGS_THOMAS (default) or SDR_FGS_PCR (below) */
} sdr_wls_params;

/* Solver of the FGS line systems (I + lambda*L) u = f.  ximgproc runs the sequential Thomas
 * elimination; SDR_FGS_THOMAS (the default since round 5) reproduces it operation for operation
 * (bit-exact with oracle/wls_oracle.c fgs_line), one lane per image line, the later passes'
 * elimination coefficients computed alongside the first.  SDR_FGS_PCR solves the same systems by
 * parallel cyclic reduction, a workgroup per line, with the diagonal carried as the row sum: it is
 * ~200x closer to the exact solution than the sequential sweep in float32, and on the reference's
 * own frames within 1 int16 level of it, but where the confidence map is sparse the sequential
 * sweep's own float error reaches hundreds of levels (profiles/r5_pcr_vs_thomas.json), so PCR is
 * not a drop-in there; lines of at most 4096 samples. */
enum { SDR_FGS_PCR = 0, SDR_FGS_THOMAS = 1 };

/* cv::ximgproc::createDisparityWLSFilter(matcher_left) (stereo_disparity.cpp:11): fills the
 * filter parameters for an SGBM left matcher AND mutates the matcher's parameters the way
 * ximgproc does (disp12MaxDiff = 1000000, speckleWindowSize = 0, uniquenessRatio = 0). */
void sdr_wls_params_for_sgbm(sdr_sgbm_params* left_matcher, sdr_wls_params* out);
int sdr_wls_create(const sdr_wls_params* p, int device, sdr_wls** out);
int sdr_wls_destroy(sdr_wls* h);
int sdr_wls_set_params(sdr_wls* h, const sdr_wls_params* p);
int sdr_wls_get_params(const sdr_wls* h, sdr_wls_params* p);
/* HIP stream the filter launches on (NULL = the HIP null stream); reset = its own stream */
int sdr_wls_set_stream(sdr_wls* h, void* stream);
int sdr_wls_reset_stream(sdr_wls* h);
void* sdr_wls_get_stream(const sdr_wls* h);
/* DisparityWLSFilter::getROI for a W x H map: roi = {x, y, w, h}. */
int sdr_wls_get_roi(const sdr_wls* h, int width, int height, int roi[4]);
/* DisparityWLSFilter::filter(disp_left, left_view, filtered, disp_right) on device, async on the
 * handle's stream: dense int16 maps [nframes][H][W], 8-bit gray guide (guide_stride bytes per
 * row, guide_frame_stride bytes per frame) -> filtered int16 [nframes][H][W].  d_conf
 * (nullable) receives getConfidenceMap() as float [nframes][H][W]. */
int sdr_wls_filter_device(sdr_wls* h, const int16_t* d_disp_left, const int16_t* d_disp_right,
                          const uint8_t* d_guide, int width, int height, size_t guide_stride,
                          size_t guide_frame_stride, int nframes, int16_t* d_out, float* d_conf);
/* Host-pointer version (synchronous). */
int sdr_wls_filter(sdr_wls* h, const int16_t* disp_left, const int16_t* disp_right,
                   const uint8_t* guide, int width, int height, size_t guide_stride,
                   int16_t* out, float* conf);
/* cv::ximgproc::fastGlobalSmootherFilter(guide, src, dst, lambda, sigma, attenuation, iters) on
 * nimg float images [nimg][h][w] sharing one 8-bit guide, in place, async on `stream`; solver
 * SDR_FGS_PCR or SDR_FGS_THOMAS.  SDR_FGS_THOMAS needs every pass's lambda * attenuation^k in
 * [0, 2^100] and allocates (stream-ordered per call, from the library's device memory pool)
 * 4 * (6 + 10 * num_iter) bytes a sample of
 * w x h rounded up to 4 each way: the coefficients of its 2 * num_iter passes (20 B a sample each)
 * and the pass layouts. */
int sdr_fgs_filter_device(const uint8_t* d_guide, size_t guide_stride, int width, int height,
                          double lambda, double sigma_color, double lambda_attenuation,
                          int num_iter, float* d_img, int nimg, int solver, void* stream);
/* Self-test of the reciprocal the SDR_FGS_THOMAS coefficient jobs use (v_rcp_f32 + one Newton
 * step, sdr_fgs_seq.hip fgs_rcp) against the IEEE quotient 1.0f / d, on the current device, for all
 * 2^23 mantissas of d in [2^e, 2^(e+1)), 0 <= e <= 126: *mismatches = how many differ (0 expected
 * for e <= 125, where 1/d is normal: the jobs' bit-exactness rests on it; SDR_FGS_THOMAS refuses
 * lambda > 2^100 so that its pivots stay below 2^126). Synchronous. */
int sdr_fgs_rcp_selftest(int e, unsigned int* mismatches);

/* Which kernel a filter's FGS launches take (host-only when cus != 0): the launchers' own
 * dispatch code, environment knobs (SDR_FGS_LR, SDR_FGS_LRJOB, SDR_FGS_LR_MAXL) included, so a
 * test can assert the instantiation a shape reaches.  `lines` is the lines a workgroup: the
 * template argument L of k_fgs_lr, a job's L in k_fgs_lrjob, LPB of k_fgs_th, and for k_fgs_pcr the
 * short lines sharing a workgroup. */
enum {
    SDR_FGS_KERNEL_NONE = 0,  /* no such launch (SDR_FGS_PCR has no coefficient jobs) */
    SDR_FGS_KERNEL_LR = 1,    /* k_fgs_lr<lines> */
    SDR_FGS_KERNEL_LRJOB = 2, /* k_fgs_lrjob, this job on `lines` lines a workgroup */
    SDR_FGS_KERNEL_TH = 3,    /* k_fgs_th<two right-hand sides, lines> */
    SDR_FGS_KERNEL_PCR = 4    /* k_fgs_pcr */
};
typedef struct sdr_fgs_launch {
    int32_t kernel; /* SDR_FGS_KERNEL_* */
    int32_t lines;
} sdr_fgs_launch;
typedef struct sdr_fgs_plan {
    sdr_fgs_launch row_pass, col_pass; /* the passes along the rows (lines of `width` samples) and
                                          along the columns */
    sdr_fgs_launch row_job, col_job;   /* their coefficient jobs, in the filter's first job launch
                                          (the jobs of its first 8 passes) */
    int32_t cus;                       /* the compute units the plan holds for (SDR_FGS_THOMAS) */
    int32_t reserved;
} sdr_fgs_plan;
/* The plan of one filter call on width x height lines (the WLS filter: its ROI), nframes frames
 * a launch (sdr_fgs_filter_device: 1), nimg = 1 or 2 right-hand sides solved together (the WLS
 * filter: 2; sdr_fgs_filter_device solves a stack in pairs and a left-over image alone), num_iter
 * iterations (the job launch holds min(2 * num_iter, 8) jobs, which k_fgs_th's choice depends on).
 * cus = 0 asks the current device for its compute units; any other value keeps the call off the
 * GPU.  SDR_ERR_SIZE where SDR_FGS_PCR would refuse the size. */
int sdr_fgs_plan_query(int width, int height, int nframes, int nimg, int num_iter, int solver,
                       int cus, sdr_fgs_plan* out);

/* ---- ingest in front of the path: StereoRectifier + SBS split ----
 * cv::initUndistortRectifyMap(K, dist, R, P, size, CV_16SC2, map1, map2)   stereo_rectifier.cpp:7-11
 * computed on the device (f64, OpenCV's scalar loop): map1 int16 [H][W][2], map2 uint16 [H][W]
 * (5-bit fractions, (v&31)*32 + (u&31)); host outputs.  dist has 0/4/5/8/12/14 coefficients
 * (14: tauX = tauY = 0 only, the tilted-sensor model is refused with SDR_ERR_ARG); P is row-major
 * 3 x p_cols (p_cols 3 or 4, only the first 3 columns are used). */
int sdr_init_undistort_rectify_map(const double K[9], const double* dist, int ndist,
                                   const double R[9], const double* P, int p_cols, int width,
                                   int height, int device, int16_t* map1, uint16_t* map2);
/* cv::remap(src, dst, map1, map2, INTER_LINEAR) with BORDER_CONSTANT 0 on 8-bit images with 1 or
 * 3 channels, nframes frames (src/dst frame strides in bytes), async on `stream`. */
int sdr_remap_bilinear_device(const uint8_t* d_src, int src_width, int src_height,
                              size_t src_stride, size_t src_frame_stride, int channels,
                              const int16_t* d_map1, const uint16_t* d_map2, int width, int height,
                              uint8_t* d_dst, size_t dst_stride, size_t dst_frame_stride,
                              int nframes, void* stream);

typedef struct sdr_rectifier sdr_rectifier;
/* StereoRectifier(config) (stereo_rectifier.cpp:6-11): both eyes' maps built on `device`. */
int sdr_rectifier_create(const double K_left[9], const double* dist_left, int ndist_left,
                         const double R1[9], const double* P1, const double K_right[9],
                         const double* dist_right, int ndist_right, const double R2[9],
                         const double* P2, int p_cols, int width, int height, int device,
                         sdr_rectifier** out);
int sdr_rectifier_destroy(sdr_rectifier* h);
int sdr_rectifier_set_stream(sdr_rectifier* h, void* stream); /* NULL = the HIP null stream */
int sdr_rectifier_reset_stream(sdr_rectifier* h);                /* back to its own stream */
/* host copies of eye `which` (0 left, 1 right) maps */
int sdr_rectifier_get_maps(const sdr_rectifier* h, int which, int16_t* map1, uint16_t* map2);
/* StereoRectifier::rectify (stereo_rectifier.cpp:17-41) on device; either eye may be NULL. */
int sdr_rectify_device(sdr_rectifier* h, const uint8_t* d_left, const uint8_t* d_right,
                       size_t stride, size_t frame_stride, int channels, int nframes,
                       uint8_t* d_left_out, uint8_t* d_right_out, size_t out_stride,
                       size_t out_frame_stride);
/* Side-by-side BGR frames [nframes] of (2*width) x height (stereo_displayer.cpp:155-159): split +
 * rectify both eyes in one pass.  Outputs (each nullable, dense): rectified BGR [F][H][W][3] per
 * eye, and/or the class path's input BGR2GRAY + INTER_AREA 0.5x of the rectified eye
 * [F][H/2][W/2] (stereo_disparity.cpp:19-24), with OpenCV's intermediate u8 roundings. */
int sdr_rectify_sbs_device(sdr_rectifier* h, const uint8_t* d_sbs, size_t sbs_stride,
                           size_t sbs_frame_stride, int nframes, uint8_t* d_bgr_left,
                           uint8_t* d_bgr_right, uint8_t* d_small_left, uint8_t* d_small_right);

/* Class path from the half-size gray pair already on the device (after sdr_rectify_sbs_device),
 * async on the left matcher's stream: left/right matchers (+ WLS when wls != NULL) for nframes
 * dense [F][h][w] frames.  Outputs (device, dense): d_out float disparity in px (the value
 * computeDisparity returns), d_filtered int16 (nullable), d_conf float (nullable).  The right
 * matcher runs on a side stream owned by the left handle, forked from and joined back to the left
 * handle's stream with events (the call stays stream-ordered for the caller). */
int sdr_stereo_class_compute_device(sdr_sgbm* left, sdr_sgbm* right, sdr_wls* wls,
                                    const uint8_t* d_small_left, const uint8_t* d_small_right,
                                    int width, int height, int nframes, float* d_out,
                                    int16_t* d_filtered, float* d_conf);
/* The reference's per-frame pair computeDisparity -> computeDepth (stereo_displayer.cpp:161-162,
 * stereo_disparity.cpp:17-39,76-80) in one call: sdr_stereo_class_compute_device plus
 * reprojectImageTo3D(d_out, Q, handleMissing = false) -> d_xyz float32x3 [F][h][w][3], fused into
 * the WLS filter's last kernel when wls != NULL. */
int sdr_stereo_class_depth_device(sdr_sgbm* left, sdr_sgbm* right, sdr_wls* wls,
                                  const uint8_t* d_small_left, const uint8_t* d_small_right,
                                  int width, int height, int nframes, float* d_out,
                                  int16_t* d_filtered, float* d_conf, const double Q[16],
                                  float* d_xyz);

/* ---- point-cloud emit after the path, point_cloud/src/pcd_write.cpp ----
 * Points are pcl::PointXYZRGB as savePCDFileBinary lays them out: 16-byte records
 * {float x, y, z; uint32 rgba}. */
/* convertCVMatToPCL(xyz, left) (pcd_write.cpp:17-51): xyz float [F][H][W][3], bgr u8 3-channel
 * rows of bgr_stride bytes (0 = 3 * width), frames bgr_frame_stride bytes apart (0 = bgr_stride *
 * height, with the row length in force), or NULL -> organised cloud [F][H*W]; non-finite points
 * get NaN x/y/z and no colour.  Async on `stream`.  SDR_ERR_ARG (nothing is enqueued): d_xyz or
 * d_points NULL, width, height or nframes <= 0, a non-zero bgr_stride < 3 * width with d_bgr given. */
int sdr_xyz_to_cloud_device(const float* d_xyz, const uint8_t* d_bgr, size_t bgr_stride,
                            size_t bgr_frame_stride, int width, int height, int nframes,
                            void* d_points, void* stream);
/* pcl::VoxelGrid<PointXYZRGB> with leaf (lx, ly, lz) (pcd_write.cpp:122-130) on n device points
 * -> d_out (capacity n) and *out_count.  PCL's int32-overflow case (leaf too small for the extent,
 * the reference's 5 mm leaf on millimetre clouds) copies the input through and sets *passthrough.
 * Synchronous on `stream` (the count is a host value).  n == 0, or no finite point: *out_count = 0.
 * `passthrough` may be NULL.  SDR_ERR_ARG (nothing written, the count included): d_points, d_out
 * or out_count NULL, n < 0, a leaf that is not > 0 on any axis (0, negative, NaN).  Scratch: ~44 B a point plus the sort's
 * histograms, from a grow-only device arena a call leases and returns idle (one arena per call in
 * flight at once, kept for the process). */
int sdr_voxel_grid_device(const void* d_points, int n, float lx, float ly, float lz, void* d_out,
                          int* out_count, int* passthrough, void* stream);
/* pcl::io::savePCDFileBinary (pcd_write.cpp:141): header + width*height records (host memory).
 * sdr_pcd_header returns the header length (writing it to buf when buf != NULL). */
int sdr_pcd_header(int width, int height, char* buf, size_t cap);
int sdr_write_pcd_binary(const char* path, const void* points, int width, int height);

/* ---- display outputs: StereoDisparity::show_disparityMap / show_depthMap,
 * the live loop's JET overlay and StereoDisplayer::depth_coverage ----
 * Colour tables are 256 BGR triples (cv::applyColorMap's LUT); NULL = the built-in table of the
 * colormap the reference uses (TURBO for the depth map, JET for the overlay), generated from the
 * published colormap definitions by sdr_colormap_lut.  A display handle owns the EMA history
 * (prev_vis / prev_depth_vis of stereo_disparity.hpp:11) and a default range state. */
enum { SDR_COLORMAP_JET = 2, SDR_COLORMAP_TURBO = 20 }; /* cv::COLORMAP_* */
typedef struct sdr_display sdr_display;
int sdr_colormap_lut(int colormap, uint8_t* lut_bgr /* 768 bytes */);
int sdr_display_create(int device, sdr_display** out);
int sdr_display_destroy(sdr_display* h);
int sdr_display_set_stream(sdr_display* h, void* stream); /* NULL = the HIP null stream */
int sdr_display_reset_stream(sdr_display* h);              /* back to its own stream */
/* forget the EMA history and reset the handle's range state to {1000, 2000} */
int sdr_display_reset(sdr_display* h);
/* show_disparityMap (stereo_disparity.cpp:42-73) on nframes float disparities (px; `stride` and
 * `frame_stride` in ELEMENTS, both used as given: there is no 0 = dense shorthand, and
 * frame_stride is not read when nframes == 1) -> d_vis u8 [F][H][W] dense, frames in order through
 * the EMA.  SDR_ERR_ARG: a NULL argument, width, height or nframes <= 0, stride < width. */
int sdr_show_disparity_map_device(sdr_display* h, const float* d_disp, int width, int height,
                                  size_t stride, size_t frame_stride, int nframes,
                                  int num_disparities, uint8_t* d_vis);
/* show_depthMap (stereo_disparity.cpp:83-124) on computeDepth outputs (channels 3: Z is channel 2;
 * channels 1: Z itself), dense [F][H][W][channels] -> d_bgr u8 [F][H][W][3].  d_zrange: device
 * {zmin_smooth, zmax_smooth} (the reference's function-static doubles, shared by every caller
 * that passes the same pointer), NULL = the handle's own.  coverage_pct (host [F], nullable):
 * depth_coverage of each frame (stereo_displayer.cpp:105-118, columns >= 80); synchronises.
 * Valid Z for the range: 0 < Z < 10000 (10000 itself is not), a denormal included; a frame with
 * fewer than two distinct valid Z takes 1000 / 2000.  SDR_ERR_ARG: h, d_xyz or d_bgr NULL, a size
 * <= 0; SDR_ERR_TYPE: channels other than 1 or 3. */
int sdr_show_depth_map_device(sdr_display* h, const float* d_xyz, int width, int height,
                              int channels, int nframes, double* d_zrange, const uint8_t* lut_bgr,
                              uint8_t* d_bgr, double* coverage_pct);
/* StereoDisplayer::depth_coverage of xyz [F][H][W][3]: percent of Z in [0, 12000] among columns
 * >= col0 (80 in the reference), over all H*W pixels (host pct[F]; synchronous); -0.0 and 12000
 * count, NaN does not; col0 >= width gives 0.  SDR_ERR_ARG: a NULL argument, a size <= 0. */
int sdr_depth_coverage_device(sdr_display* h, const float* d_xyz, int width, int height,
                              int nframes, int col0, double* pct);
/* stereo_displayer.cpp:167-173: applyColorMap(vis, JET) -> d_heat (nullable) and
 * addWeighted(resize(left_rect, 0.5, INTER_AREA), 0.7, heat, 0.3, 0) -> d_overlay (nullable), from
 * the FULL-resolution rectified left BGR view (2*width x 2*height, left_stride bytes per row, as
 * given; left_frame_stride bytes per frame, 0 = left_stride * 2 * height); vis/heat/overlay are
 * dense [F][H][W](x3).  d_left_bgr is read only for d_overlay and may be NULL for a heat map alone.
 * SDR_ERR_ARG: h or d_vis NULL, neither output, d_overlay without d_left_bgr, a size <= 0,
 * left_stride < 3 * (2 * width) with d_left_bgr given. */
int sdr_disparity_overlay_device(sdr_display* h, const uint8_t* d_vis, const uint8_t* d_left_bgr,
                                 size_t left_stride, size_t left_frame_stride, int width,
                                 int height, int nframes, const uint8_t* lut_bgr, uint8_t* d_heat,
                                 uint8_t* d_overlay);
/* Host-pointer versions (synchronous; `stride` in elements, out_stride in bytes, both >= width,
 * left_stride >= 3 * (2 * width); one frame, other arrays dense).  zrange: host {zmin_smooth,
 * zmax_smooth} in/out, NULL = the handle's own state.  sdr_disparity_overlay needs left_bgr for
 * either output.  The refusals are those of the device versions. */
int sdr_show_disparity_map(sdr_display* h, const float* disp, int width, int height, size_t stride,
                           int num_disparities, uint8_t* out, size_t out_stride);
int sdr_show_depth_map(sdr_display* h, const float* xyz, int width, int height, int channels,
                       double* zrange, uint8_t* out_bgr, double* coverage_pct);
int sdr_disparity_overlay(sdr_display* h, const uint8_t* vis, const uint8_t* left_bgr,
                          size_t left_stride, int width, int height, uint8_t* heat,
                          uint8_t* overlay);
/* StereoDisplayer::depth_coverage of a host xyz map [H][W][3] (synchronous); read-only like the
 * reference's: the handle's EMA history and range state are untouched. */
int sdr_depth_coverage(sdr_display* h, const float* xyz, int width, int height, int col0, double* pct);

/* ---- the ruler: StereoDisplayer::onMouseMeasure (stereo_displayer.cpp:24-63) and save_csvFile
 * (:74-102) ----
 * A measurement is the 3-D distance between two pixels of a frame.  sdr_measure_xyz* is the
 * reference's own: it reads the computeDepth map at the two pixels and takes cv::norm of the Vec3f
 * difference.  sdr_measure_disp* measures from the disparity map instead and is robust to holes:
 *   - Sample at (x, y): the window [y-r, y+r] x [x-r, x+r] clipped to the image, in row-major
 *     order.  A value d is valid iff it is finite, d > min_disp (strict) and, with a confidence
 *     map, conf >= conf_min (a NaN confidence is invalid).  With n valid values, n < min_count
 *     makes the sample invalid (disparity and XYZ NaN); otherwise d_med is the LOWER median,
 *     element (n-1)/2 of the valid values in ascending order (a value of the window, never an
 *     average), XYZ = reprojectImageTo3D's pixel formula at (x, y, d_med) with handleMissing off,
 *     and the sample is valid iff X, Y and Z are finite (an endpoint that fails only this test
 *     keeps its d_med and XYZ in the record, with its valid flag off).  radius 0 with min_count 1 gives the pixel
 *     of reprojectImageTo3D bit for bit.  int16 disparities are read as (float)v * 0.0625f.
 *   - Segment walk: n = max(|x1-x0|, |y1-y0|) + 1 samples, sample i at x0 + rdiv(i*(x1-x0), n-1),
 *     y likewise, rdiv(a, b) = floor((2a + b) / (2b)); samples 0 and n-1 are the endpoints P0, P1.
 *     Ties round up, towards +x / +y, not away from P0: the walk from P1 to P0 visits the same
 *     pixels in reverse (rdiv(a - m*d, m) = rdiv(a, m) - d), so swapping the endpoints only swaps
 *     p0 / p1 in the record, but the walk of a mirrored segment is not the mirror image.
 *   - distance: the Vec3f difference per component in float, squares summed in double in x, y, z
 *     order, double sqrt (cv::norm); NaN unless both endpoints are valid.
 *   - profile = 1: every sample of the walk is evaluated: path_samples = n, path_valid the valid
 *     ones, max_gap the longest run of invalid samples, z_min / z_max over valid samples (NaN with
 *     none), max_dz the largest |Z_i - Z_prev| (float) over consecutive valid samples, invalid
 *     ones skipped (NaN with fewer than two).  d_profile (nullable) is float [K][profile_cap][4]:
 *     rows i < min(n, profile_cap) receive {X, Y, Z, d_med} (four NaNs for an invalid sample),
 *     other rows stay untouched.  A buffer with profile_cap == 0 has no rows and counts as no
 *     buffer (SDR_MEAS_PROFILE_TRUNCATED is not set).  profile = 0: the three counts are 0 and the
 *     three floats NaN.
 *   - A segment whose frame is outside [0, F) or with an endpoint outside the image: flag
 *     SDR_MEAS_OUT_OF_RANGE, both points invalid, every float field NaN, nothing read.
 *   - Every NaN the ruler computes (XYZ, distance) is written as the canonical quiet NaN
 *     (0x7fc00000, 0x7ff8000000000000): the sign and payload of a computed NaN differ between
 *     machines.  d_med is a value of the window and finite.
 *   - XYZ-map mode: p0 / p1 are the map's values as read (their bits, NaNs included), d0 = d1 = NaN, n0 = n1 = 1, distance
 *     as above without a validity gate (inf or NaN where the reference prints that); flag bits 0
 *     and 1 say whether each point is finite; no window, no profile. */
typedef struct sdr_segment {
    int32_t frame, x0, y0, x1, y1;
} sdr_segment;

typedef struct sdr_ruler_params {
    int32_t radius;      /* window radius r, 0..4 */
    int32_t min_count;   /* >= 1 */
    float min_disp;      /* valid iff d > min_disp */
    float conf_min;      /* valid iff conf >= conf_min (with a confidence map) */
    int32_t profile;     /* 0 / 1 */
    int32_t profile_cap; /* rows per segment of d_profile */
} sdr_ruler_params;

enum {
    SDR_MEAS_P0_VALID = 1, SDR_MEAS_P1_VALID = 2, SDR_MEAS_OUT_OF_RANGE = 4,
    SDR_MEAS_PROFILE_TRUNCATED = 8 /* n > profile_cap with a profile buffer */
};

typedef struct sdr_measurement { /* 80 bytes */
    float p0[3], p1[3];  /* XYZ of the endpoints */
    float d0, d1;        /* their median disparities (px) */
    double distance;
    int32_t n0, n1;      /* valid values in each endpoint's window */
    int32_t path_samples, path_valid, max_gap;
    float z_min, z_max, max_dz;
    uint32_t flags;      /* SDR_MEAS_* */
    int32_t reserved;    /* 0 */
} sdr_measurement;

enum { SDR_DISP_F32 = 0, SDR_DISP_S16 = 1 };

/* {0, 1, -1.0f, 0.0f, 0, 0}: the reference's single-pixel lookup on a minDisparity-0 matcher */
void sdr_ruler_params_default(sdr_ruler_params* p);
/* K segments on device maps, asynchronous on `stream`: d_disp [F][H][W] of disp_type (float px or
 * int16 1/16 px), rows `stride` and frames `frame_stride` ELEMENTS apart; d_conf (nullable) dense
 * float [F][H][W]; d_segs K sdr_segment; d_out K sdr_measurement; d_profile nullable.  K == 0 is
 * SDR_OK with no launch.  Arguments are checked on the host before any device call. */
int sdr_measure_disp_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride,
                            int width, int height, int nframes, const float* d_conf,
                            const double Q[16], const sdr_ruler_params* params,
                            const sdr_segment* d_segs, int K, sdr_measurement* d_out,
                            float* d_profile, void* stream);
/* d_xyz [F][H][W][3] float, rows xyz_stride and frames xyz_frame_stride ELEMENTS apart. */
int sdr_measure_xyz_device(const float* d_xyz, size_t xyz_stride, size_t xyz_frame_stride, int width,
                           int height, int nframes, const sdr_segment* d_segs, int K,
                           sdr_measurement* d_out, void* stream);
/* Host-pointer versions (synchronous; per-thread persistent device buffers as sdr_reproject).  The
 * host checks the arguments, not the segments' coordinates: a segment outside the maps is refused
 * per segment by the kernel (SDR_MEAS_OUT_OF_RANGE), exactly as in the device versions. */
int sdr_measure_disp(const void* disp, int disp_type, size_t stride, size_t frame_stride, int width,
                     int height, int nframes, const float* conf, const double Q[16],
                     const sdr_ruler_params* params, const sdr_segment* segs, int K,
                     sdr_measurement* out, float* profile);
int sdr_measure_xyz(const float* xyz, size_t xyz_stride, size_t xyz_frame_stride, int width,
                    int height, int nframes, const sdr_segment* segs, int K, sdr_measurement* out);
/* save_csvFile (stereo_displayer.cpp:74-102), byte for byte, of n records: with_header the line
 * "Image, First_point,   Second_point, Distance\n", then per record
 * "%d, [%d, %d],    [%d, %d], %.5f cm   \n" of image_index[i], the endpoints and distance / 10.
 * segs[i] holds record i's endpoints (its frame is ignored).  Returns the byte length (without a
 * terminator), writing the text and a terminator when buf != NULL (cap too small: SDR_ERR_ARG).
 * Pure host code. */
int sdr_measurements_csv(const int* image_index, const sdr_segment* segs,
                         const sdr_measurement* records, int n, int with_header, char* buf,
                         size_t cap);

/* ---- the ruler against a surface: robust plane fit and point-to-plane distance ----
 * sdr_fit_planes* fits a plane d = a*u + b*v + c to the disparities of a rectangle (a plane in
 * (x, y, d) is a plane in XYZ under any Q) and reports it in pixels and as a 3-D plane;
 * sdr_plane_distance* measures sampled points against fitted planes.  Every output is defined to
 * the bit: the fit rests on exact integer moments, so it has no floating-point reduction.
 *   - Region: an sdr_segment read as a rectangle of frame `frame` with corners (x0, y0), (x1, y1) in
 *     any order; xs = min, xe = max of the x, ys / ye of the y, inclusive; u = x - xs, v = y - ys;
 *     area = (xe-xs+1) * (ye-ys+1).  The record's x0 / y0 are xs / ys.  A frame outside [0, F) or a
 *     corner outside the image: SDR_PLANE_OUT_OF_RANGE, nothing read, every float field the
 *     canonical NaN, every count (area, n_valid, n_inliers, fits) 0.  xe == xs or ye == ys makes
 *     the fit degenerate (SDR_PLANE_DEGENERATE; n_valid is still counted).
 *   - Valid pixel: the ruler's rule (finite, d > min_disp, and with a confidence map
 *     conf >= conf_min; int16 read as (float)v * 0.0625f), and for float maps fabsf(d) < 2048.  The
 *     fit works on the 1/16 px grid: q = v for int16, q = (int)rint((double)d * 16.0)
 *     (round-half-even) for float.
 *   - Moments of a pixel set: nine exact int64 sums n, Su, Sv, Sq, Suu, Suv, Svv, Suq, Svq.  The
 *     host refuses width or height > 8192 and width * height > 2^24, so no sum can overflow.
 *   - Solve, in double, no contraction, every operation rounded, in this order: N = (double)n,
 *     su, sv, sq the sums converted; cuu = N*Suu - su*su; cuv = N*Suv - su*sv; cvv = N*Svv - sv*sv;
 *     cuq = N*Suq - su*sq; cvq = N*Svq - sv*sq; det = cuu*cvv - cuv*cuv;
 *     a = (cuq*cvv - cvq*cuv) / det; b = (cvq*cuu - cuq*cuv) / det; c = ((sq - a*su) - b*sv) / N.
 *     The fit is degenerate iff n < min_inliers, or !(det > 0), or a, b or c is not finite.
 *   - Residual of a pixel, in 1/16 px: r = (double)q - ((a*u + b*v) + c); T = (double)inlier_px * 16.
 *   - Schedule: fit 0 uses every valid pixel; refit k = 1..iterations uses the valid pixels with
 *     |r| <= T * 2^(iterations-k) against the previous plane (the last refit uses T itself).  A
 *     degenerate fit stops the chain: SDR_PLANE_DEGENERATE, `fits` the number of fits completed,
 *     coef, normal, offset, centroid, rms_px and max_abs_px NaN, n_inliers 0.
 *   - Statistics against the last plane: n_inliers = the valid pixels with |r| <= T;
 *     See = sum of e*e over them as int64, e = llrint(r * 16); rms_px = sqrt((double)See /
 *     (double)n_inliers) / 256 and max_abs_px = (float)(max |r| / 16) over them (both NaN with no
 *     inlier).
 *   - coef = {a/16, b/16, c/16}: px per px and px, relative to (xs, ys) (an exact scaling).
 *   - 3-D plane: the anchors (xs, ys), (xe, ys), (xs, ye) with the plane's disparity
 *     ((a*u + b*v) + c) * 0.0625 are reprojected in double: the four row sums of
 *     reprojectImageTo3D in its order (from 0: + Q[i][0]*x, + Q[i][1]*y, + Q[i][2]*d, + Q[i][3]*1),
 *     X = h0/h3, Y = h1/h3, Z = h2/h3 (no float rounding).  e1 = P1 - P0, e2 = P2 - P0;
 *     m = e1 x e2 with mx = e1y*e2z - e1z*e2y, my = e1z*e2x - e1x*e2z, mz = e1x*e2y - e1y*e2x;
 *     len = sqrt((mx*mx + my*my) + mz*mz); normal = m / len; offset = -((nx*P0x + ny*P0y) + nz*P0z);
 *     offset < 0 negates normal and offset (the camera origin is on the non-negative side).
 *     centroid: the same reprojection at the real-valued pixel (xs + su/N, ys + sv/N) of the last
 *     fit's set with the plane's disparity ((a*(su/N) + b*(sv/N)) + c) * 0.0625.  A non-finite
 *     value among them: SDR_PLANE_NONFINITE, normal, offset and centroid NaN, the rest stays.
 *     SDR_PLANE_OK is set iff none of DEGENERATE, NONFINITE and OUT_OF_RANGE is.
 *   - Point query {frame, x, y, plane}: (x, y) is sampled exactly as an endpoint of
 *     sdr_measure_disp (radius, min_count, lower median, reprojection); p, d and n are the
 *     sample's.  distance = ((nx*X + ny*Y) + nz*Z) + offset in double from the float XYZ, positive
 *     towards the camera, with SDR_PDIST_VALID iff the sample is valid and the plane is OK; NaN
 *     otherwise.  SDR_PDIST_OUT_OF_RANGE: frame or pixel outside, nothing read of the maps, p and
 *     d NaN, n 0.  SDR_PDIST_NO_PLANE: `plane` outside [0, P) or a plane without SDR_PLANE_OK.
 *   - Every NaN computed is written as the canonical quiet NaN, as in the ruler. */
typedef struct sdr_plane_params { /* 32 bytes */
    int32_t iterations;  /* refits after the first fit, 0..8 */
    int32_t min_inliers; /* >= 3 */
    float inlier_px;     /* the final band in px: finite, 0 < inlier_px <= 64 */
    float min_disp;      /* valid iff d > min_disp */
    float conf_min;      /* valid iff conf >= conf_min (with a confidence map) */
    int32_t reserved[3]; /* 0 */
} sdr_plane_params;

enum {
    SDR_PLANE_OK = 1, SDR_PLANE_DEGENERATE = 2, SDR_PLANE_NONFINITE = 4, SDR_PLANE_OUT_OF_RANGE = 8
};

typedef struct sdr_plane { /* 128 bytes */
    double coef[3];      /* a, b (px / px) and c (px): d = a*(x-x0) + b*(y-y0) + c */
    double normal[3];    /* unit normal of the 3-D plane */
    double offset;       /* normal . X + offset = 0 on the plane; offset >= 0 */
    double centroid[3];  /* the plane's point under the centroid of the last fit's pixels */
    double rms_px;       /* of the inliers' residuals */
    float max_abs_px;    /* largest inlier residual */
    int32_t x0, y0;      /* xs, ys: the origin of coef */
    int32_t frame, area, n_valid, n_inliers, fits;
    uint32_t flags;      /* SDR_PLANE_* */
    int32_t reserved;    /* 0 */
} sdr_plane;

typedef struct sdr_plane_query { /* 16 bytes */
    int32_t frame, x, y, plane;
} sdr_plane_query;

enum { SDR_PDIST_VALID = 1, SDR_PDIST_OUT_OF_RANGE = 2, SDR_PDIST_NO_PLANE = 4 };

/* The record shares its name with the host entry point below, as struct stat does with stat():
 * it has no typedef and is written `struct sdr_plane_distance`. */
struct sdr_plane_distance { /* 32 bytes */
    float p[3];          /* XYZ of the sampled point */
    float d;             /* its median disparity (px) */
    double distance;     /* signed distance to the plane, positive towards the camera */
    int32_t n;           /* valid values in the window */
    uint32_t flags;      /* SDR_PDIST_* */
};

/* {3, 16, 1.0f, -1.0f, 0.0f, {0, 0, 0}} */
void sdr_plane_params_default(sdr_plane_params* p);
/* K regions on device maps (arguments as sdr_measure_disp_device), asynchronous on `stream`:
 * iterations + 2 sweeps over the regions' pixels and one launch that writes d_planes (K sdr_plane);
 * the moment accumulators are stream-ordered scratch.  K == 0 is SDR_OK with no launch.  Every
 * argument is checked on the host before any device call; here a bad disp_type is SDR_ERR_ARG
 * too. */
int sdr_fit_planes_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride,
                          int width, int height, int nframes, const float* d_conf,
                          const double Q[16], const sdr_plane_params* params,
                          const sdr_segment* d_regions, int K, sdr_plane* d_planes, void* stream);
/* K queries against the P planes of d_planes (e.g. the records sdr_fit_planes_device wrote
 * earlier on the same stream); params: radius, min_count, min_disp and conf_min of the sample. */
int sdr_plane_distance_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride,
                              int width, int height, int nframes, const float* d_conf,
                              const double Q[16], const sdr_ruler_params* params,
                              const sdr_plane* d_planes, int P, const sdr_plane_query* d_queries,
                              int K, struct sdr_plane_distance* d_out, void* stream);
/* Host-pointer versions (synchronous; per-thread persistent device buffers as sdr_measure_disp). */
int sdr_fit_planes(const void* disp, int disp_type, size_t stride, size_t frame_stride, int width,
                   int height, int nframes, const float* conf, const double Q[16],
                   const sdr_plane_params* params, const sdr_segment* regions, int K,
                   sdr_plane* planes);
int sdr_plane_distance(const void* disp, int disp_type, size_t stride, size_t frame_stride, int width,
                       int height, int nframes, const float* conf, const double Q[16],
                       const sdr_ruler_params* params, const sdr_plane* planes, int P,
                       const sdr_plane_query* queries, int K, struct sdr_plane_distance* out);

/* ---- the dominant planes of a region: a seeded search without a prior ----
 * sdr_find_planes* finds up to max_planes planes in one rectangle, the largest first, and says
 * which pixel lies on which.  Fit 0 of sdr_fit_planes is a least-squares fit of every valid pixel,
 * which lies on no surface when the rectangle holds several; here each round draws M three-point
 * hypotheses, scores them on the pixels no earlier round has claimed, refits the winner with the
 * plane fit's schedule and claims its inliers.  Hypothesis generation, scoring and selection are
 * exact integer arithmetic; the refit is the plane fit's (exact moments, the same solve): every
 * output is defined to the bit, for any grid shape and any order the workgroups finish in.
 *   - Region, valid pixel, q, u, v, xs, xe, ys, ye, rw = xe-xs+1, rh = ye-ys+1, area = rw*rh, the
 *     moments, the solve, the residual r and T = (double)fit.inlier_px * 16: the plane fit's,
 *     above.  Tq = (int64)floor(T) (at most 1024).  A pixel is FREE in round r iff it is valid and
 *     no round before r has claimed it.
 *   - Round r = 0 .. max_planes-1, while the search has not stopped:
 *     1. Draws.  mix(x) on uint32: x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b;
 *        x ^= x>>16.  R(r,h,j,t) = mix(mix(mix(seed ^ (0x9E3779B9u*(r+1))) ^ h) ^ (16*j + t)).
 *        Hypothesis h in [0, M) draws the points j = 0, 1, 2; point j tries t = 0..15 the pixel of
 *        index p = ((uint64)R * area) >> 32 of the region's row-major order (v = p / rw,
 *        u = p % rw) and takes the first try that is free.  No free pixel in 16 tries makes the
 *        hypothesis VOID.  (Two points may be the same pixel: C == 0 below.)
 *     2. The plane through P_j = (u_j, v_j, q_j), with (du1, dv1, dq1) = P1 - P0 and
 *        (du2, dv2, dq2) = P2 - P0:  A = dv1*dq2 - dq1*dv2;  B = dq1*du2 - du1*dq2;
 *        C = du1*dv2 - dv1*du2;  D = A*u0 + B*v0 + C*q0 (int64).  C == 0 makes the hypothesis
 *        void.  The guards keep |du|, |dv| <= 8191 and |dq| <= 65536 (|q| <= 32768), so
 *        |A|, |B| <= 2 * 8191 * 65536 < 2^31 and, as du*dv < area <= 2^24, |C| < 2^25 < 2^28: they
 *        are int32.  A*u, B*v < 2^44, C*q < 2^43, |D| < 2^45, Tq*|C| < 2^38: every product and sum
 *        below stays below 2^46 in int64.
 *     3. Score of a hypothesis that is not void: the number of free pixels with
 *        |A*u + B*v + C*q - D| <= Tq * |C|, in int64, no floating point.  (Its own three points
 *        count: a score is at least 3.)
 *     4. Pick.  The winner is the highest score among the hypotheses that are not void, ties to the
 *        lowest h.  All void: the search stops with SDR_SEARCH_NO_HYPOTHESIS.  The winner's score
 *        < fit.min_inliers: it stops with SDR_SEARCH_LOW_SCORE.
 *     5. Seed plane in 1/16 px, each one rounded double division of exactly converted integers:
 *        a = -(double)A / (double)C;  b = -(double)B / (double)C;  c = (double)D / (double)C.
 *     6. Refits k = 1..fit.iterations, the plane fit's schedule with the seed plane in the place of
 *        fit 0: the set of refit k is the free pixels with |r| <= T * 2^(iterations-k) against the
 *        previous plane; its nine moments, the same solve (degenerate also with fewer than
 *        min_inliers pixels).  A degenerate solve stops the search: SDR_SEARCH_REFIT_DEGENERATE.
 *     7. The inliers are the free pixels with |r| <= T against the last refit's plane.  Fewer than
 *        fit.min_inliers: the search stops with SDR_SEARCH_FEW_INLIERS and claims nothing.
 *        Otherwise they are claimed (label r) and record r is what sdr_fit_planes writes for the
 *        region, with: the plane the last refit's; n_valid the free pixels at the start of the
 *        round; n_inliers, rms_px, max_abs_px over the claimed pixels; fits = iterations + 1; the
 *        centroid from the last refit's moments; area, x0, y0, frame the region's; flags
 *        SDR_PLANE_OK or SDR_PLANE_NONFINITE (a non-finite 3-D plane still claims its pixels and
 *        the search goes on).  rounds[r] = {winner h, its score, the number of void hypotheses, 0}.
 *   - After a stop in round r: *count = r (max_planes when no round stopped); the records r.. are
 *     the plane fit's DEGENERATE record (floats the canonical NaN, n_valid, n_inliers, fits 0; area,
 *     x0, y0, frame the region's); rounds[r] = {h, score, voids, stop code} with what the round had
 *     found: {-1, 0, M, NO_HYPOTHESIS}, else the winner and its score; rounds after r are
 *     {-1, 0, 0, SDR_SEARCH_NOT_RUN}.
 *   - A region out of range (the plane fit's rule): *count = 0, every record the plane fit's
 *     OUT_OF_RANGE record, every round {-1, 0, 0, SDR_SEARCH_NOT_RUN}, every label 255.
 *   - Labels: uint8 [height][width] of the region's frame, 255 everywhere but on claimed pixels,
 *     which hold their round: the count of label r is planes[r].n_inliers.
 *   - A region one pixel wide or high has C == 0 in every hypothesis: count 0, NO_HYPOTHESIS. */
typedef struct sdr_plane_search_params { /* 64 bytes */
    sdr_plane_params fit; /* as in sdr_fit_planes, but iterations in 1..8 */
    int32_t max_planes;   /* rounds, 1..8 */
    int32_t hypotheses;   /* M, 1..4096 */
    uint32_t seed;
    int32_t reserved[5];  /* 0 */
} sdr_plane_search_params;

enum { /* sdr_plane_search_round.stop */
    SDR_SEARCH_RAN = 0, SDR_SEARCH_NO_HYPOTHESIS = 1, SDR_SEARCH_LOW_SCORE = 2,
    SDR_SEARCH_REFIT_DEGENERATE = 3, SDR_SEARCH_FEW_INLIERS = 4, SDR_SEARCH_NOT_RUN = 5
};

typedef struct sdr_plane_search_round { /* 16 bytes */
    int32_t hypothesis;  /* the winner, -1 without one */
    int32_t score;       /* its score */
    int32_t voids;       /* void hypotheses of the round */
    uint32_t stop;       /* SDR_SEARCH_* */
} sdr_plane_search_round;

/* {{3, 64, 1.0f, -1.0f, 0.0f, {0, 0, 0}}, 4, 256, 0, {0, 0, 0, 0, 0}} */
void sdr_plane_search_params_default(sdr_plane_search_params* p);
/* One region (d_region: one sdr_segment on the device) of device maps (arguments as
 * sdr_fit_planes_device), asynchronous on `stream` with no host synchronisation between rounds: a
 * fixed sequence of launches for max_planes rounds, which a stopped search leaves at once.  Writes
 * every one of the max_planes records of d_planes, *d_count, and when they are not NULL the
 * max_planes records of d_rounds and the width * height labels of d_labels; hypotheses, scores,
 * moments, the search's state and, without d_labels, the claim map are stream-ordered scratch.
 * Every argument is checked on the host before any device call. */
int sdr_find_planes_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride,
                           int width, int height, int nframes, const float* d_conf,
                           const double Q[16], const sdr_plane_search_params* params,
                           const sdr_segment* d_region, sdr_plane* d_planes, int32_t* d_count,
                           sdr_plane_search_round* d_rounds, uint8_t* d_labels, void* stream);
/* Host-pointer version (synchronous; per-thread persistent device buffers as sdr_fit_planes). */
int sdr_find_planes(const void* disp, int disp_type, size_t stride, size_t frame_stride, int width,
                    int height, int nframes, const float* conf, const double Q[16],
                    const sdr_plane_search_params* params, const sdr_segment* region,
                    sdr_plane* planes, int32_t* count, sdr_plane_search_round* rounds,
                    uint8_t* labels);

/* ---- the relief of a region: a surface's height statistics above a fitted plane ----
 * sdr_plane_relief* measures every pixel of a rectangle against a plane record (of sdr_fit_planes*
 * or sdr_find_planes*), optionally only the pixels that carry one label of sdr_find_planes*'
 * label map, and reports counts, extremes, means and order statistics of the heights.  Every output
 * is a count, an exact integer sum, an extreme or an element of the set: none depends on the grid
 * shape or on the order the workgroups finish in, and every one is defined to the bit.
 *   - Query {frame, x0, y0, x1, y1, plane, label, 0}.  Region: the plane fit's rule (corners in
 *     any order, xs / xe / ys / ye, area).  A frame outside [0, F) or a corner outside the image,
 *     a label outside -1..255, or a label >= 0 without a label map: SDR_RELIEF_OUT_OF_RANGE,
 *     nothing read, every count (area too) 0, both sums 0, every float and double the canonical NaN.
 *     Otherwise `plane` outside [0, P) or a record without SDR_PLANE_OK: SDR_RELIEF_NO_PLANE, the
 *     maps are not read, area is the region's, the other counts and the sums 0, the floats NaN.
 *   - Pixel (x, y) of the rectangle, in this order:
 *     1. masked in iff label < 0 or labels[frame][y][x] == label (n_masked counts these);
 *     2. valid by the ruler's rule for a radius-0, min_count-1 sample: d finite, d > min_disp, and
 *        with a confidence map conf >= conf_min; int16 read as (float)v * 0.0625f (n_valid counts
 *        the masked-in pixels that are valid);
 *     3. XYZ in float by reprojectImageTo3D's pixel formula at (x, y, d), handleMissing off (the
 *        ruler's sample);
 *     4. h = ((nx*X + ny*Y) + nz*Z) + offset in double from the float XYZ, no contraction
 *        (sdr_plane_distance's expression); hf = (float)h + 0.0f (a negative zero becomes +0);
 *     5. member iff X, Y and Z are finite and fabsf(hf) < 1048576.0f (n counts the members;
 *        n_rejected = n_valid - n).
 *   - Over the members: n_above counts hf > band, n_below hf < -band (float comparisons); h_min and
 *     h_max are the extreme hf; e = llrint((double)hf * 256.0) (the product is exact, |e| < 2^28:
 *     2^24 pixels cannot overflow int64); sum256 the sum of e, sum256_above the same over hf > band;
 *     mean = ((double)sum256 / (double)n) / 256.0, mean_above likewise over n_above (NaN with none).
 *   - Quantile j < nq: k = ((int64)(n - 1) * permille[j]) / 1000 and q[j] is element k (0-based) of
 *     the members' hf in ascending order: 500 is the lower median, element (n-1)/2, 0 is h_min,
 *     1000 is h_max.  q[j] for j >= nq is the canonical NaN.
 *   - n == 0: SDR_RELIEF_EMPTY, the counts as found, the sums 0, every float and double NaN.
 *     Otherwise SDR_RELIEF_VALID.  Every NaN written is the canonical quiet NaN.
 *   - frame, plane and label of a record are its query's in every case. */
typedef struct sdr_relief_query { /* 32 bytes */
    int32_t frame, x0, y0, x1, y1; /* the rectangle, the plane fit's region rule */
    int32_t plane;                 /* index into the P plane records */
    int32_t label;                 /* -1: no mask; 0..255: only pixels whose label equals it */
    int32_t reserved;              /* 0 */
} sdr_relief_query;

typedef struct sdr_relief_params { /* 64 bytes */
    float min_disp, conf_min;      /* the ruler's validity rule */
    float band;                    /* finite, >= 0, in Q's units (mm) */
    int32_t nq;                    /* quantiles asked for, 0..8 */
    int32_t permille[8];           /* each 0..1000; any order, repeats allowed; entries >= nq ignored */
    int32_t reserved[4];           /* 0 */
} sdr_relief_params;

enum { SDR_RELIEF_VALID = 1, SDR_RELIEF_OUT_OF_RANGE = 2, SDR_RELIEF_NO_PLANE = 4, SDR_RELIEF_EMPTY = 8 };

typedef struct sdr_relief { /* 128 bytes */
    float q[8];                    /* the quantiles; entries >= nq the canonical NaN */
    float h_min, h_max;
    double mean, mean_above;
    int64_t sum256, sum256_above;  /* the exact sums the means come from */
    int32_t area, n_masked, n_valid, n, n_above, n_below, n_rejected;
    int32_t frame, plane, label;   /* the query's */
    uint32_t flags;                /* SDR_RELIEF_* */
    int32_t reserved[3];           /* 0 */
} sdr_relief;

/* {-1.0f, 0.0f, 0.0f, 3, {50, 500, 950, 0, 0, 0, 0, 0}, {0, 0, 0, 0}} */
void sdr_relief_params_default(sdr_relief_params* p);
/* K queries on device maps against the P records of d_planes (arguments as
 * sdr_plane_distance_device), asynchronous on `stream`: a fixed sequence of launches with no host
 * synchronisation, a radix selection over the members' ordered keys in three passes of 11, 11 and
 * 10 bits; the histograms and accumulators are stream-ordered scratch.  d_labels (nullable) is a
 * dense uint8 [F][H][W]; with F = 1 it is exactly what sdr_find_planes_device writes.  d_out: K
 * sdr_relief.  K == 0 is SDR_OK with no launch.  The host refuses, before any device call and with
 * SDR_ERR_ARG: what sdr_fit_planes_device refuses of the maps (nulls, sizes, strides, disp_type,
 * width or height > 8192, width * height > 2^24), K < 0, P < 0 or P > 0 without d_planes, nq
 * outside 0..8, one of the first nq permille outside 0..1000, a band that is not finite or
 * negative, a non-zero reserved field of the parameters.  The queries are device memory: what is
 * wrong with one is refused per record (above). */
int sdr_plane_relief_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride,
                            int width, int height, int nframes, const float* d_conf,
                            const uint8_t* d_labels, const double Q[16],
                            const sdr_relief_params* params, const sdr_plane* d_planes, int P,
                            const sdr_relief_query* d_queries, int K, sdr_relief* d_out,
                            void* stream);
/* Host-pointer version (synchronous; per-thread persistent device buffers as sdr_fit_planes). */
int sdr_plane_relief(const void* disp, int disp_type, size_t stride, size_t frame_stride, int width,
                     int height, int nframes, const float* conf, const uint8_t* labels,
                     const double Q[16], const sdr_relief_params* params, const sdr_plane* planes,
                     int P, const sdr_relief_query* queries, int K, sdr_relief* out);

/* ---- the footprint of a region: a surface's oriented length and width on a plane ----
 * sdr_plane_footprint* takes the pixels of a rectangle (optionally only those carrying one label,
 * optionally only those in a band of heights), bins them on a grid of square cells IN a plane
 * record's plane, drops the cells that stray pixels occupy alone, and reports the minimum-area
 * bounding rectangle of the kept cells over 90 whole-degree orientations: two sides, the angle and
 * four 3-D corners.  Every step is a count, an integer extreme or a correctly rounded double
 * operation (no contraction): no output depends on the grid shape or on the order the workgroups
 * finish in, and every one is defined to the bit.
 *   - Query: an sdr_relief_query under the relief's rules.  SDR_FOOTPRINT_OUT_OF_RANGE (a frame or
 *     corner outside, a label outside -1..255, a label >= 0 without a label map): nothing read,
 *     every count (area too) 0.  Otherwise SDR_FOOTPRINT_NO_PLANE (`plane` outside [0, P), a record
 *     without SDR_PLANE_OK, or a basis below that is not finite): the maps are not read, area is
 *     the region's, the other counts 0.
 *   - Basis, once a query, in double: n = the record's normal; the camera X axis if
 *     fabs(nx) <= fabs(ny), else the Y axis, minus its component along n:
 *     X axis: (a, b, c) = (1 - nx*nx, -(nx*ny), -(nx*nz)); Y axis: (-(nx*ny), 1 - ny*ny, -(ny*nz));
 *     len = sqrt((a*a + b*b) + c*c); e_s = (a/len, b/len, c/len); e_t = n x e_s by the plane fit's
 *     expressions: tx = ny*esz - nz*esy, ty = nz*esx - nx*esz, tz = nx*esy - ny*esx.
 *   - Member: a pixel that passes the relief's steps 1 to 5 (mask, validity, float XYZ, h, hf,
 *     X / Y / Z finite and fabsf(hf) < 1048576.0f; n_masked and n_valid count as there), then
 *     h_lo <= hf && hf <= h_hi (float comparisons), then with
 *     s = (esx*X + esy*Y) + esz*Z, t likewise with e_t (double, from the float XYZ),
 *     qs = s / (double)cell, qt = t / (double)cell: fabs(qs) < 2^30 and fabs(qt) < 2^30.
 *     si = (int64)floor(qs), ti = (int64)floor(qt).  n counts the members.
 *   - Grid: i0 = min si, j0 = min ti over the members; a member's cell is (si - i0, ti - j0), inside
 *     iff both indices are < grid.  n_outside counts the members outside; n_outside > 0 sets
 *     SDR_FOOTPRINT_CLIPPED beside the record's other flag.  count[i][j] = the inside members of
 *     the cell.  span_s = max si - i0 + 1, span_t = max ti - j0 + 1 (int64, saturated to int32).
 *   - Kept cells: count[i][j] >= 1 and the sum of count over the cell's 3 x 3 neighbourhood (cells
 *     outside the grid count 0) >= support.  n_cells_raw = the cells with count >= 1, n_cells = the
 *     kept ones.  n_cells == 0 (n == 0 too): SDR_FOOTPRINT_EMPTY, the counts, i0, j0 and the spans
 *     as found (0 with no member).  Otherwise SDR_FOOTPRINT_VALID.
 *   - Directions: the table c_k = lrint(16384 * cos(k deg)), s_k = lrint(16384 * sin(k deg)),
 *     k = 0..89, a literal in the source (sdr_footprint_direction returns it).  c_k*c_k + s_k*s_k
 *     is 2^28 only to about 6e-5 of it: a direction's length is 1 to about 3e-5, and so is a side.
 *   - Extents of direction k over the kept cells (i, j), int32 (grid <= 1024: |p|, |r| < 2^25):
 *     p = c_k*i + s_k*j, r = -s_k*i + c_k*j; the unit cell square projects to [p, p + c_k + s_k] and
 *     [r - s_k, r + c_k]: U0 = min p, U1 = max p + c_k + s_k, V0 = min r - s_k, V1 = max r + c_k;
 *     A_k = (int64)(U1 - U0) * (int64)(V1 - V0).  The answer is the k of the smallest A_k, ties to
 *     the lowest k; angle_deg = k: side[0] runs along e_s turned by k degrees towards e_t.
 *   - side[0] = ((double)(U1 - U0) / 16384.0) * (double)cell, side[1] likewise from V;
 *     fill = (double)n_cells / (((double)(U1 - U0) / 16384.0) * ((double)(V1 - V0) / 16384.0)).
 *   - Corners, in the order (U0, V0), (U1, V0), (U1, V1), (U0, V1): a = U / 16384.0,
 *     b = V / 16384.0, ch = c_k / 16384.0, sh = s_k / 16384.0; gi = ch*a - sh*b; gj = sh*a + ch*b;
 *     S = ((double)i0 + gi) * (double)cell; T = ((double)j0 + gj) * (double)cell; each component
 *     corner[x] = (S*es[x] + T*et[x]) - offset*n[x]: the point of the plane at (S, T).
 *   - A record that is not VALID: every double the canonical NaN, angle_deg -1.  frame, plane and
 *     label are the query's in every case.  Occupied area and volume are deliberately not reported:
 *     holes and the aliasing of pixel spacing against the cell put them 10 to 35 % off; n_cells and
 *     fill are quality indicators only. */
typedef struct sdr_footprint_params { /* 64 bytes */
    float min_disp, conf_min;      /* the ruler's validity rule */
    float cell;                    /* cell side in Q's units (mm): finite, 0.0625 .. 65536 */
    float h_lo, h_hi;              /* members have h_lo <= hf <= h_hi; not NaN, h_lo <= h_hi */
    int32_t grid;                  /* cells a side, 16..1024 */
    int32_t support;               /* members a kept cell's 3 x 3 neighbourhood holds, 1..255 */
    int32_t reserved[9];           /* 0 */
} sdr_footprint_params;

enum {
    SDR_FOOTPRINT_VALID = 1, SDR_FOOTPRINT_OUT_OF_RANGE = 2, SDR_FOOTPRINT_NO_PLANE = 4,
    SDR_FOOTPRINT_EMPTY = 8, SDR_FOOTPRINT_CLIPPED = 16
};

typedef struct sdr_footprint { /* 256 bytes */
    double side[2];                /* along the direction angle_deg and across it, Q's units */
    double fill;                   /* kept cells / the rectangle's area in cells */
    double corner[4][3];           /* the rectangle's corners in 3-D, on the plane */
    double basis_s[3], basis_t[3]; /* e_s, e_t */
    int64_t i0, j0;                /* the grid's origin in cells */
    int32_t angle_deg;             /* k, 0..89; -1 without a rectangle */
    int32_t span_s, span_t;        /* the members' extent in cells, before the grid clips it */
    int32_t area, n_masked, n_valid, n, n_outside, n_cells_raw, n_cells;
    int32_t frame, plane, label;   /* the query's */
    uint32_t flags;                /* SDR_FOOTPRINT_* */
    int32_t reserved[4];           /* 0 */
} sdr_footprint;

/* {-1.0f, 0.0f, 4.0f, -1048576.0f, 1048576.0f, 512, 4, {0, ...}} */
void sdr_footprint_params_default(sdr_footprint_params* p);
/* The direction table: *c = c_k, *s = s_k and SDR_OK for k in 0..89, else SDR_ERR_ARG (also for a
 * null pointer).  Pure host code. */
int sdr_footprint_direction(int k, int32_t* c, int32_t* s);
/* K queries on device maps against the P records of d_planes (arguments as
 * sdr_plane_relief_device), asynchronous on `stream`: a fixed sequence of launches a batch of
 * queries with no host synchronisation (setup, a sweep for the counts and the origin, a sweep that
 * bins, a pass over the cells, the record).  The grids and accumulators are stream-ordered scratch;
 * the queries run in batches so that the grids take at most 64 MiB.  K == 0 is SDR_OK with no
 * launch.  The host refuses, before any device call and with SDR_ERR_ARG: what
 * sdr_plane_relief_device refuses of the maps, K < 0, P < 0 or P > 0 without d_planes, a cell that
 * is not finite or outside [0.0625, 65536], grid outside 16..1024, support outside 1..255, h_lo or
 * h_hi NaN or h_lo > h_hi, a non-zero reserved field of the parameters. */
int sdr_plane_footprint_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride,
                               int width, int height, int nframes, const float* d_conf,
                               const uint8_t* d_labels, const double Q[16],
                               const sdr_footprint_params* params, const sdr_plane* d_planes, int P,
                               const sdr_relief_query* d_queries, int K, sdr_footprint* d_out,
                               void* stream);
/* Host-pointer version (synchronous; per-thread persistent device buffers as sdr_fit_planes). */
int sdr_plane_footprint(const void* disp, int disp_type, size_t stride, size_t frame_stride, int width,
                        int height, int nframes, const float* conf, const uint8_t* labels,
                        const double Q[16], const sdr_footprint_params* params,
                        const sdr_plane* planes, int P, const sdr_relief_query* queries, int K,
                        sdr_footprint* out);

/* ---- the objects of a region: connected sets of pixels in a band of heights above a plane ----
 * sdr_find_objects* labels the connected sets of a rectangle's pixels that stand in a band of
 * heights above a plane record and whose disparities change by at most max_diff from pixel to
 * pixel, and reports the largest of them, largest first, as records and as a label map in the form
 * sdr_plane_relief* and sdr_plane_footprint* take: a floor from sdr_find_planes*, one label a thing
 * standing on it from here, each thing's height, length and width from those two.  Every output is
 * a count, an integer sum, an extreme or a set membership: none depends on the grid shape or on the
 * order the workgroups finish in, and every one is defined to the bit.
 *   - Query: one sdr_relief_query under the relief's rules (rectangle xs, xe, ys, ye, rw, rh, area;
 *     the label mask against the INPUT label map).  SDR_OBJECTS_OUT_OF_RANGE (a frame or corner
 *     outside, a label outside -1..255, a label >= 0 without an input label map): nothing read,
 *     every count (area too) 0.  Otherwise SDR_OBJECTS_NO_PLANE (`plane` outside [0, P) or a record
 *     without SDR_PLANE_OK): the maps are not read, area is the region's, the other counts 0.
 *     label = 255 with sdr_find_planes*' map selects the pixels no plane claimed.
 *   - Member: a pixel that passes the relief's steps 1 to 5 (n_masked and n_valid count as there),
 *     then h_lo <= hf && hf <= h_hi (float comparisons, the footprint's band).  n counts the members.
 *   - Adjacent: with connectivity 4 two pixels of the rectangle that share an edge, with 8 two that
 *     share an edge or a corner.  Joined: two adjacent members p, q with fabsf(d_p - d_q) <= max_diff,
 *     d the float disparity as step 2 reads it (int16: (float)v * 0.0625f): one float subtraction,
 *     one comparison.
 *   - Component: a class of the transitive closure of "joined"; its root is the smallest index
 *     v * rw + u (u = x - xs, v = y - ys) of its pixels.  n_components counts the components.
 *   - Kept: the components of at least min_pixels pixels, n_kept of them, ordered by size
 *     descending, ties to the lower root.  count = min(n_kept, max_objects); n_kept > max_objects
 *     sets SDR_OBJECTS_TRUNCATED beside the other flag; n_kept == 0 gives SDR_OBJECTS_EMPTY (the
 *     counts as found), else SDR_OBJECTS_VALID.  largest_dropped is the size of the largest
 *     component that is not kept (smaller than min_pixels), 0 with none.
 *   - Object k < count: n and root; x0, y0, x1, y1 the bounding box in image coordinates, inclusive;
 *     sum_x, sum_y the sums of the image x and y; sum256 the sum of the relief's
 *     e = llrint((double)hf * 256.0); h_min, h_max the extreme hf; flags SDR_OBJECT_VALID, and
 *     SDR_OBJECT_CUT iff the box touches the rectangle's border (x0 == xs || x1 == xe || y0 == ys ||
 *     y1 == ye).  Records k >= count (all max_objects are written): n 0, root and the box -1, the
 *     sums 0, the floats the canonical NaN, flags 0.
 *   - Scan record: flags, the counts, and the query's frame, plane and label in every case.
 *   - Labels: uint8 [height][width] of the query's frame, 255 everywhere but on the pixels of object
 *     k < count, which hold k: the count of label k is objects[k].n.  A refused query writes 255
 *     everywhere. */
typedef struct sdr_object_params { /* 64 bytes */
    float min_disp, conf_min;      /* the ruler's validity rule */
    float h_lo, h_hi;              /* members have h_lo <= hf <= h_hi; not NaN, h_lo <= h_hi */
    float max_diff;                /* joined: |d_p - d_q| <= max_diff (px); finite, >= 0 */
    int32_t connectivity;          /* 4 or 8 */
    int32_t min_pixels;            /* a kept component's least size, 1..2^24 */
    int32_t max_objects;           /* records (and labels) written, 1..64 */
    int32_t reserved[8];           /* 0 */
} sdr_object_params;

enum {
    SDR_OBJECTS_VALID = 1, SDR_OBJECTS_OUT_OF_RANGE = 2, SDR_OBJECTS_NO_PLANE = 4,
    SDR_OBJECTS_EMPTY = 8, SDR_OBJECTS_TRUNCATED = 16
};
enum { SDR_OBJECT_VALID = 1, SDR_OBJECT_CUT = 2 };

typedef struct sdr_object { /* 64 bytes */
    int32_t n;                     /* pixels */
    int32_t root;                  /* the smallest v * rw + u of its pixels; -1: no object */
    int32_t x0, y0, x1, y1;        /* the bounding box, image coordinates, inclusive */
    int64_t sum_x, sum_y;          /* sums of the image x and y: the centroid is sum / n */
    int64_t sum256;                /* the sum of llrint(hf * 256): the mean height is sum256 / n / 256 */
    float h_min, h_max;
    uint32_t flags;                /* SDR_OBJECT_* */
    int32_t reserved;              /* 0 */
} sdr_object;

typedef struct sdr_object_scan { /* 64 bytes */
    uint32_t flags;                /* SDR_OBJECTS_* */
    int32_t area, n_masked, n_valid, n;
    int32_t n_components, n_kept, count, largest_dropped;
    int32_t frame, plane, label;   /* the query's */
    int32_t reserved[4];           /* 0 */
} sdr_object_scan;

/* {-1.0f, 0.0f, 10.0f, 1048576.0f, 1.0f, 8, 64, 16, {0, ...}} */
void sdr_object_params_default(sdr_object_params* p);
/* One query (d_query: one sdr_relief_query on the device) on device maps against the P records of
 * d_planes (arguments as sdr_plane_relief_device; d_labels_in, nullable, is its dense uint8
 * [F][H][W] label map), asynchronous on `stream`: a fixed sequence of launches with no host
 * synchronisation and no workgroup that waits on another (32 x 32 tiles labelled in LDS, tile
 * borders merged by a lock-free min-root union-find, sizes, a ranking of the kept roots, one sweep
 * for the records and the labels).  Writes the max_objects records of d_objects, *d_scan and, when
 * it is not NULL, the width * height labels of d_labels_out, which must not be d_labels_in.  The
 * query is device memory, so the stream-ordered scratch is sized for the frame: 8 bytes a pixel of
 * width * height (a parent and a size), 8 * max_objects + 16 bytes for every 2048 pixels (candidate
 * keys, counts), 16 bytes a 32 x 32 tile (counts) and 3616 bytes of state: 1.87 MB for 640 x 360
 * at max_objects 16.  The host refuses, before any device call and with SDR_ERR_ARG: what
 * sdr_plane_relief_device refuses of the maps and planes, a null d_query, d_objects or d_scan,
 * d_labels_out == d_labels_in (not NULL), h_lo or h_hi NaN or h_lo > h_hi, a max_diff that is not
 * finite or negative, a connectivity other than 4 or 8, min_pixels outside 1..2^24, max_objects
 * outside 1..64, a non-zero reserved field of the parameters. */
int sdr_find_objects_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride,
                            int width, int height, int nframes, const float* d_conf,
                            const uint8_t* d_labels_in, const double Q[16],
                            const sdr_object_params* params, const sdr_plane* d_planes, int P,
                            const sdr_relief_query* d_query, sdr_object* d_objects,
                            sdr_object_scan* d_scan, uint8_t* d_labels_out, void* stream);
/* Host-pointer version (synchronous; per-thread persistent device buffers as sdr_fit_planes);
 * labels_out (nullable): width * height bytes. */
int sdr_find_objects(const void* disp, int disp_type, size_t stride, size_t frame_stride, int width,
                     int height, int nframes, const float* conf, const uint8_t* labels_in,
                     const double Q[16], const sdr_object_params* params, const sdr_plane* planes,
                     int P, const sdr_relief_query* query, sdr_object* objects,
                     sdr_object_scan* scan, uint8_t* labels_out);

/* ---- the clearance of two labelled things: the smallest 3-D distance between two pixel sets ----
 * sdr_clearance* takes the pixels of a rectangle that carry one label of a label map (set A) and
 * those that carry another (set B), gives every pixel the ruler's sample taken over its own set, and
 * reports the closest pair of points, one of each set: the distance, where it is attained, and its
 * split along and across a plane record's normal (the floor the two things stand on).  The result is
 * a minimum with an index tie-break over all pairs: it depends neither on the order the pairs are
 * visited in nor on the order the workgroups finish in, and every output is defined to the bit.
 *   - Query {frame, x0, y0, x1, y1, plane, label_a, label_b}.  Region: the plane fit's rule
 *     (xs, xe, ys, ye, rw, rh, area; u = x - xs, v = y - ys).  A dense uint8 label map is required.
 *     A frame outside [0, F) or a corner outside the image, a label outside 0..255, or
 *     label_a == label_b: SDR_CLEARANCE_OUT_OF_RANGE, nothing read, every count (area too) 0, every
 *     float and double the canonical NaN, the pixel coordinates -1.  Otherwise `plane` outside
 *     [0, P) or a record without SDR_PLANE_OK: SDR_CLEARANCE_NO_PLANE, the maps are not read, area
 *     is the region's, the other counts 0, the floats NaN, the pixel coordinates -1.
 *   - Member of set S (S = A with label_a, S = B with label_b): a pixel of the rectangle that passes
 *     the relief's steps 1 to 5 with S's label (mask, validity, float XYZ, h, hf, X / Y / Z finite
 *     and fabsf(hf) < 1048576.0f), then h_lo <= hf && hf <= h_hi (float comparisons, the
 *     footprint's band).  n_a and n_b count the members.
 *   - Point of a member at (x, y): the window [y - radius, y + radius] x [x - radius, x + radius]
 *     clipped to the RECTANGLE (not the image); the disparities (as step 2 reads them) of the
 *     window's pixels that are members of the same set, in the window's row-major order; fewer than
 *     min_count of them: no point.  Otherwise d_med is their lower median, element (n - 1) / 2 in
 *     ascending order (equal values in window order: the ruler's selection), XYZ the float
 *     reprojection of (x, y, d_med) (step 3's formula), and the member has a point iff X, Y and Z
 *     are finite.  m_a and m_b count the points.  With radius 0 and min_count 1 a member's point
 *     is its own.
 *   - Pair (p a point of A, q a point of B): v = q - p per component in float;
 *     s = (v0*v0 + v1*v1) + v2*v2 in double from the float v, no contraction (sdr_measure_disp's
 *     distance expression; never NaN, as the points are finite; it may be +inf).
 *   - Result: the pair of the smallest s, ties to the smaller index v * rw + u of p, then of q.
 *     distance = sqrt(s); along = (nx*v0 + ny*v1) + nz*v2 in double with the record's normal
 *     (positive: B's point is farther from the plane on the camera's side); across =
 *     sqrt(max(s - along*along, 0.0)) with max(t, 0.0) = t > 0.0 ? t : 0.0 (0.0 for a NaN t, which
 *     an infinite s can give).  xa, ya, xb, yb are the two pixels in image coordinates, p_a, p_b
 *     the two points, d_a, d_b their d_med.
 *   - m_a == 0 or m_b == 0: SDR_CLEARANCE_EMPTY, the counts as found, the floats NaN, the pixel
 *     coordinates -1.  Otherwise SDR_CLEARANCE_VALID.  Every NaN written is the canonical quiet NaN.
 *   - frame, plane, label_a and label_b of a record are its query's in every case. */
typedef struct sdr_clearance_query { /* 32 bytes */
    int32_t frame, x0, y0, x1, y1; /* the rectangle, the plane fit's region rule */
    int32_t plane;                 /* index into the P plane records */
    int32_t label_a, label_b;      /* 0..255 each, different */
} sdr_clearance_query;

typedef struct sdr_clearance_params { /* 64 bytes */
    float min_disp, conf_min;      /* the ruler's validity rule */
    float h_lo, h_hi;              /* members have h_lo <= hf <= h_hi; not NaN, h_lo <= h_hi */
    int32_t radius;                /* the same-set sample's window radius, 0..4 */
    int32_t min_count;             /* same-set pixels a window must hold, >= 1 */
    int32_t reserved[10];          /* 0 */
} sdr_clearance_params;

enum {
    SDR_CLEARANCE_VALID = 1, SDR_CLEARANCE_OUT_OF_RANGE = 2, SDR_CLEARANCE_NO_PLANE = 4,
    SDR_CLEARANCE_EMPTY = 8
};

/* the most queries a call takes (they run one behind another on the stream) */
enum { SDR_CLEARANCE_MAX_QUERIES = 64 };

/* The record shares its name with the host entry point below, as sdr_plane_distance does: it has no
 * typedef and is written `struct sdr_clearance`. */
struct sdr_clearance { /* 128 bytes */
    double distance;               /* sqrt(s) of the closest pair, Q's units */
    double along, across;          /* its parts along the plane's normal (signed) and in the plane */
    float p_a[3], p_b[3];          /* the two points */
    float d_a, d_b;                /* their median disparities (px) */
    int32_t xa, ya, xb, yb;        /* their pixels, image coordinates; -1 without a pair */
    int32_t area, n_a, n_b, m_a, m_b;
    int32_t frame, plane, label_a, label_b; /* the query's */
    uint32_t flags;                /* SDR_CLEARANCE_* */
    int32_t reserved[4];           /* 0 */
};

/* {-1.0f, 0.0f, -1048576.0f, 1048576.0f, 0, 1, {0, ...}} */
void sdr_clearance_params_default(sdr_clearance_params* p);
/* K queries on device maps against the P records of d_planes (the maps, planes and labels arguments
 * are sdr_plane_relief_device's; d_labels must not be NULL), asynchronous on `stream`: a fixed
 * sequence of launches a query, one query behind another, with no host synchronisation and no
 * workgroup that waits on another (a sweep that marks the members, a sweep that samples them and
 * appends the points to one list a set, the bounds of every 256 points, all pairs of the two lists
 * block against block, the record).  A pair of blocks is skipped only where a lower bound of its s
 * from the blocks' bounds is strictly greater than an s already found, so the record is the brute
 * force's.  d_out: K struct sdr_clearance.  K == 0 is SDR_OK with no launch.  The queries are device
 * memory, so the stream-ordered scratch is sized for the frame and serves every query in turn:
 * 21 bytes a pixel of width * height (a mark, a median and a 16-byte point), 304 bytes for every
 * 256 pixels (two blocks' bounds and sixteen candidates) and at most 2 KB of state and alignment:
 * 5.1 MB for 640 x 360, whatever K and whatever the rectangles; 372 MB for the largest map the host
 * admits (2^24 pixels), which a caller with such maps has to have free.
 * The host refuses, before any device call and with SDR_ERR_ARG: what sdr_plane_relief_device
 * refuses of the maps and planes, a null d_labels, K < 0 or K > SDR_CLEARANCE_MAX_QUERIES, h_lo
 * or h_hi NaN or h_lo > h_hi, a radius outside 0..4, min_count < 1, a non-zero reserved field of
 * the parameters. */
int sdr_clearance_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride,
                         int width, int height, int nframes, const float* d_conf,
                         const uint8_t* d_labels, const double Q[16],
                         const sdr_clearance_params* params, const sdr_plane* d_planes, int P,
                         const sdr_clearance_query* d_queries, int K, struct sdr_clearance* d_out,
                         void* stream);
/* Measurement hook, process-wide and safe to call from any thread (an atomic the entries read once
 * a call).  SDR_DEBUG_CLEARANCE_PRUNE: 0 makes every block pair run, any other value (the default)
 * lets the calls that start afterwards skip block pairs as above; the records do not change, only
 * the time does (scripts/clearance_bench.py).  An unknown knob is SDR_ERR_ARG. */
enum { SDR_DEBUG_CLEARANCE_PRUNE = 1 };
int sdr_clearance_debug_knob(int knob, int value);
/* Host-pointer version (synchronous; per-thread persistent device buffers as sdr_fit_planes). */
int sdr_clearance(const void* disp, int disp_type, size_t stride, size_t frame_stride, int width,
                  int height, int nframes, const float* conf, const uint8_t* labels,
                  const double Q[16], const sdr_clearance_params* params, const sdr_plane* planes,
                  int P, const sdr_clearance_query* queries, int K, struct sdr_clearance* out);

/* ---- the ruler over time: one disparity map from a still scene's last frames ----
 * The reference measures on a frozen frame (the `f` key, stereo_displayer.cpp:191-196): camera and
 * scene are still, and the frames before the freeze saw the same surfaces.  sdr_fuse_disp* makes one
 * map of a stack of F frames, pixel by pixel: the valid values of a pixel vote, the ones within
 * `tol` of their median are averaged, and a pixel whose frames are too few or disagree is a hole.
 * The result is float [H][W] in px and goes into every sdr_measure_disp / sdr_fit_planes / ... call
 * as a one-frame SDR_DISP_F32 map WITHOUT a confidence map (the gate was applied frame by frame).
 * Every output is defined to the bit.  For pixel (x, y), v_k its value in frame k, k = 0..F-1
 * (int16 disparities are read as (float)v * 0.0625f):
 *   1. v_k is VALID by the ruler's rule: finite, v_k > min_disp (strict) and, with a confidence
 *      map, conf_k >= conf_min (a NaN confidence is invalid).  n is the number of valid values.
 *   2. n == 0: the pixel is EMPTY.
 *   3. m is the LOWER median: element (n-1)/2 of the valid values in ascending order by < on floats,
 *      equal values in frame order (-0.0 and +0.0 are equal: the earlier frame's bits win).  m is a
 *      value of the stack, never an average.
 *   4. v_k AGREES iff it is valid and fabsf(v_k - m) <= tol (one float subtraction, no contraction).
 *      n_in counts the agreeing values; m agrees, so n_in >= 1.
 *   5. n_in < min_count: the pixel is SPARSE if n < min_count, otherwise UNSTABLE (the frames
 *      disagree: something moved, or the matcher flickers between two surfaces).
 *   6. Otherwise the pixel is FUSED.  SDR_FUSE_MEDIAN writes m.  SDR_FUSE_MEAN writes
 *      (float)(s / (double)n_in), s the double sum of (double)v_k over the agreeing k in ascending k
 *      from +0.0 (exact for int16 input; for float input the order defines it), the division the
 *      correctly rounded IEEE one.
 *   - d_out (required, float [H][W], dense, not overlapping an input): the fused value, or `fill`
 *     on an EMPTY, SPARSE or UNSTABLE pixel.
 *   - d_support (nullable, uint8 [H][W]): n_in on a FUSED pixel, 0 elsewhere.
 *   - d_spread (nullable, float [H][W]): on a FUSED pixel hi - lo (one float subtraction), lo the
 *     smallest and hi the largest agreeing value by <, of equal ones the earliest frame's; on any
 *     other pixel the canonical quiet NaN (0x7fc00000).
 *   - d_rec (nullable): one sdr_fusion, every field an exact count, complete when the stream
 *     reaches the end of the call.
 * F == 1 is allowed (the validity gate, with min_count's rule). */
enum { SDR_FUSE_MEAN = 0, SDR_FUSE_MEDIAN = 1 };
enum { SDR_FUSE_MAX_FRAMES = 32 };

typedef struct sdr_fuse_params { /* 32 bytes */
    float min_disp, conf_min;      /* the ruler's validity rule */
    float tol;                     /* px: a value agrees with the pixel's median iff |v - m| <= tol */
    float fill;                    /* written where the stack has no consensus; not a valid value */
    int32_t min_count;             /* agreeing values a pixel needs, 1..32 */
    int32_t mode;                  /* SDR_FUSE_MEAN / SDR_FUSE_MEDIAN */
    int32_t reserved[2];           /* 0 */
} sdr_fuse_params;

typedef struct sdr_fusion { /* 64 bytes */
    int32_t frames, width, height, mode;             /* the call's */
    int32_t n_fused, n_empty, n_sparse, n_unstable;  /* sum = width * height */
    int32_t n_filled;    /* FUSED pixels whose LAST frame (F-1) was invalid: holes the stack filled */
    int32_t n_replaced;  /* FUSED pixels whose last frame was valid but does not agree: outliers removed */
    int64_t sum_support; /* sum of n_in over FUSED pixels */
    int64_t n_disagree;  /* valid values, over FUSED pixels, that do not agree */
    int64_t reserved;    /* 0 */
} sdr_fusion;

/* {-1.0f, 0.0f, 1.0f, -1.0f, 2, SDR_FUSE_MEAN, {0, 0}}: fill = min_disp */
void sdr_fuse_params_default(sdr_fuse_params* p);
/* One stack on device maps, asynchronous on `stream` (the maps arguments are
 * sdr_measure_disp_device's): one launch, no host
 * synchronisation; with d_rec a second short launch adds up the workgroups' partial records, which
 * live in the stream-ordered scratch of the other device calls (4 KB).  A thread reads its pixels
 * (two float, four int16; two int16 with more than 16 frames) with one 8-byte (4-byte) access where
 * d_disp, stride and frame_stride keep that alignment, one by one otherwise; the results do not
 * depend on it.
 * The host refuses, before any device call: with SDR_ERR_ARG a null d_disp, d_out or params; width,
 * height or nframes < 1; stride < width; frame_stride < stride * height when nframes > 1; an unknown
 * disp_type or mode; tol not finite or < 0; min_count outside 1..32; a non-zero reserved field; a
 * `fill` that is itself valid (finite and > min_disp: the result must never make a hole look
 * measured).  With SDR_ERR_LIMIT: nframes > SDR_FUSE_MAX_FRAMES, width * height > INT32_MAX. */
int sdr_fuse_disp_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride,
                         int width, int height, int nframes, const float* d_conf,
                         const sdr_fuse_params* params, float* d_out, uint8_t* d_support,
                         float* d_spread, sdr_fusion* d_rec, void* stream);
/* Host-pointer version (synchronous; per-thread persistent device buffers as sdr_measure_disp). */
int sdr_fuse_disp(const void* disp, int disp_type, size_t stride, size_t frame_stride, int width,
                  int height, int nframes, const float* conf, const sdr_fuse_params* params,
                  float* out, uint8_t* support, float* spread, sdr_fusion* rec);

/* Bytes of device scratch the handle holds for the given frame shape (for capacity planning);
 * 0 when compute would refuse the shape or parameters.  sdr_sgbm_scratch_bytes is the CV_8UC1
 * figure, sdr_sgbm_scratch_bytes_cn takes the channel count (1 or 3: colour input holds three
 * operand sets per image). */
size_t sdr_sgbm_scratch_bytes(const sdr_sgbm_params* p, int width, int height, int nframes);
size_t sdr_sgbm_scratch_bytes_cn(const sdr_sgbm_params* p, int width, int height, int channels,
                                 int nframes);
/* sdr_sgbm_scratch_bytes_cn for a handle of cost type `cost` (SDR_COST_*; host-only): 0, with
 * sdr_last_error() saying why, when compute would refuse.  The census descriptors live in the BT
 * operand planes' buffers, so the figure does not depend on the cost type. */
size_t sdr_sgbm_scratch_bytes_ex(const sdr_sgbm_params* p, int cost, int width, int height,
                                 int channels, int nframes);

/* Timing with HIP events on the handle's stream.  level 1: per-stage timing of the last compute
 * (sdr_sgbm_last_timing: cost volume / path aggregation / LR+median+speckle, ms).  level 2 also
 * brackets every kernel launch; sdr_sgbm_kernel_time sums the launches of one SDR_KERNEL_* kind
 * (kind < 0: all) since the last reset. */
enum {
    SDR_KERNEL_PREFILTER = 0, SDR_KERNEL_COST = 1, SDR_KERNEL_PATHS = 2,
    SDR_KERNEL_WTA_LR = 3,   /* k_south_wta: top-to-bottom path fused with WTA/uniqueness/disp2 */
    SDR_KERNEL_MEDIAN = 4, SDR_KERNEL_SPECKLE = 5, SDR_KERNEL_REPROJECT = 6,
    SDR_KERNEL_LR_CHECK = 7, /* the LR-checked map materialised (debug stage 2 only since round 3) */
    SDR_KERNEL_SWEEP = 8,    /* k_sweep: batched MODE_HH's up pass (N, NE, NW) */
    /* the class path's WLS filter (sdr_stereo_class_*), recorded on the left matcher's handle */
    SDR_KERNEL_WLS_PREP = 9, /* k_wls_prep (or k_wls_disc + k_wls_conf past 4096 ROI columns) */
    SDR_KERNEL_FGS = 10,     /* one FGS pass: k_fgs_pcr, or k_fgs_th (SDR_FGS_THOMAS) */
    SDR_KERNEL_WLS_FINAL = 11, /* k_wls_final (+ /16 + computeDepth epilogue) */
    SDR_KERNEL_SWEEP_DOWN = 12, /* batched MODE_HH's down pass (SE, SW): timed apart from the up pass */
    SDR_KERNEL_FGS_COEF = 13 /* SDR_FGS_THOMAS: the coefficient jobs of a filter's passes (one launch) */
};
int sdr_sgbm_enable_timing(sdr_sgbm* h, int level);
int sdr_sgbm_last_timing(const sdr_sgbm* h, float* cost_ms, float* paths_ms, float* post_ms);
int sdr_sgbm_kernel_time(sdr_sgbm* h, int kind, int reset, float* total_ms, int* count);

/* Status of the handle's device batches since the last report (synchronises the handle's
 * stream).  A batched MODE_HH call (>= 8 frames, sdr_sgbm_compute_device*) runs row sweeps whose
 * workgroups wait on their neighbours; they assume every workgroup of the sweep is resident, i.e.
 * that this process has the device to itself (sweeps of one process are ordered among themselves).
 * If a wait still gives up (another process's persistent kernel holding CUs for about a second),
 * that batch's output frames are written as INVALID ((minDisparity-1)*16, the reprojection's
 * frame minima too) and SDR_ERR_DEVICE is returned once for the timeouts seen since the last
 * report -- by this call, or by the next compute call if it sees them first -- then SDR_OK again
 * (the device keeps a count, so copies of it still in flight cannot report a timeout twice).  The
 * host-pointer entry points compute one frame and never take the sweeps. */
int sdr_sgbm_last_status(sdr_sgbm* h);
/* Test hooks.  SDR_DEBUG_SWEEP_SPIN: polls a sweep's neighbour wait makes before it gives up
 * (<= 0: the default, about a second); a small value forces the failure path above.
 * SDR_DEBUG_PLAN_CUS: the compute-unit count this handle's calls give the two chain-count
 * thresholds of the path launches (two chains a wave in k_paths_tc above 4 x CUs chains, two
 * columns a workgroup in k_south_wta above 8 x CUs, and through them the 12-bit record format);
 * <= 0: the device's own count.  1 sends a frame of a few hundred chains to the two-column kernels
 * and a large value keeps it off them, on any GPU.  Both forms compute the same maps, so the knob
 * changes which kernel runs and nothing else.  It never reaches the sweeps' tiling, the cost
 * kernels' row bands or anything else that sizes a resident grid: a sweep sized for compute units
 * that are not there would wait on a workgroup that never runs.
 * SDR_DEBUG_COST_ROWS: the rows of a row band of the one-pass cost kernels (k_cost, the census cost
 * kernel); <= 0: the launcher's own rule, the tallest band that fills the device's resident-block
 * slots in one pass and at least 4 rows -- which gives every small frame 4-row bands, whose row loop
 * never completes an unrolled trip.  Any height >= 1 computes the same volume (a cost block waits on
 * no other block), so the knob moves the band borders and nothing else; sdr_sgbm_last_plan reports
 * the height and the band count a launch took.  The two-pass generic cost ignores it. */
enum { SDR_DEBUG_SWEEP_SPIN = 1, SDR_DEBUG_PLAN_CUS = 2, SDR_DEBUG_COST_ROWS = 3 };
int sdr_sgbm_debug_knob(sdr_sgbm* h, int knob, int value);

/* Which kernels a matcher call launches: the record the launchers themselves switch on, so a test
 * can assert the instantiation a shape reaches.  Template arguments as in csrc/sdr_paths.hip:
 * dpl = disparities a lane of a chain wave (2, 4, 8: D <= 128, 256, 512), pad = D below its class's
 * 64 * dpl, r12 = 12-bit records, np = the directions the fused pass reads (P - 1), tc = two
 * columns a workgroup. */
enum {
    SDR_SGBM_COST_NONE = 0,
    SDR_SGBM_COST_ONE_PASS = 1, /* k_cost<nr, k, cn>: nr = blockSize rows, k = disparity pairs a lane */
    SDR_SGBM_COST_CENSUS = 2,   /* the census cost kernel (nr and k as above, cn = 1) */
    SDR_SGBM_COST_GENERIC = 3   /* the two-pass cost (blockSize > 11 or D > 256); nr = k = 0 */
};
enum {
    SDR_SGBM_PATHS_NONE = 0,
    SDR_SGBM_PATHS_CHAIN = 1, /* k_paths<dpl, pad, r12> */
    SDR_SGBM_PATHS_TC = 2     /* k_paths_tc<pad> (dpl 4: two chains a wave) */
};
enum {
    SDR_SGBM_SOUTH_NONE = 0,
    SDR_SGBM_SOUTH_WTA = 1,  /* k_south_wta<dpl, pad, np, tc, r12> */
    SDR_SGBM_SOUTH_SWEEP = 2 /* batched MODE_HH: k_sweep16<dw, pad, up> twice (up, then down + WTA) */
};
enum {
    SDR_SGBM_POST_NONE = 0,
    SDR_SGBM_POST_SPECKLE = 1,     /* LR check and median inside the speckle filter's labelling */
    SDR_SGBM_POST_MEDIAN_LR = 2,   /* k_median3_lr */
    SDR_SGBM_POST_MEDIAN_COLS = 3  /* k_median3_cols (the LR check cannot fire) */
};
typedef struct sdr_sgbm_launches {
    int32_t cost_kernel, cost_nr, cost_k, cost_cn;
    int32_t paths_kernel, paths_dpl, paths_pad, paths_r12;
    int32_t south_kernel, south_dpl, south_pad, south_np, south_tc, south_r12;
    int32_t sweep_dw, sweep_pad;             /* a sweep: disparity words a lane (4, 8), D < 32 * dw */
    int32_t sweep_nslots[2], sweep_ntiles[2]; /* [0] the down pass, [1] the up pass */
    int32_t post;
    int32_t paths_chains, south_chains; /* chains of the two launches, all frames (a sweep: 0 south) */
    int32_t cus;                        /* the compute units the two thresholds were taken at */
    /* the last one-pass cost launch: rows of a main row band and the number of main bands (3WAY's
     * stripe-start bands come on top).  0 for the generic cost, and from sdr_sgbm_plan_query: the
     * launcher's rule needs the device's occupancy query */
    int32_t cost_rows, cost_bands;
} sdr_sgbm_launches;
/* The launches of one call of nframes frames of width x height x channels under p and the cost
 * type.  cus = 0 asks the current device for its compute units; any other value keeps the call off
 * the GPU.  Off the GPU a batch that could sweep (MODE_HH, >= 8 frames, D <= 256) is reported as
 * SDR_SGBM_SOUTH_SWEEP with zero nslots and ntiles -- the tiling needs the device's occupancy
 * query -- and on it a batch whose tiles do not fit the resident grid reports the chains it takes
 * instead.  SDR_PATH_REC=16 in the environment is honoured as a new handle would.  A call the
 * engine would refuse returns that status; a frame that matches no column reports no launch. */
int sdr_sgbm_plan_query(const sdr_sgbm_params* p, int cost, int width, int height, int nframes,
                        int channels, int cus, sdr_sgbm_launches* out);
/* What the handle's last call launched (of a paired class call: the left handle's, both matchers'
 * frames in one batch); SDR_ERR_ARG before the first call that ran the stages. */
int sdr_sgbm_last_plan(const sdr_sgbm* h, sdr_sgbm_launches* out);

/* How a call lays the path-cost records out in device memory (sdr_sgbm_debug_stage(4) hands them
 * out by row whatever the order was).  A pixel's R records are `pix` contiguous int16 elements; the
 * records of pixel (x, y) of frame f start at element f * frame + x * xs + y * ys.
 *  - by row, [F][H][W1]: xs = pix, ys = W1 * pix.
 *  - by column, [F][W1][H]: xs = H * pix, ys = pix.  The default (SDR_PATH_ORDER=row in the
 *    environment when the handle is created keeps every call by row; col or anything else is the
 *    default), but only where the fused pass is the one-column k_south_wta fed by k_paths with one chain a wave (south_tc = 0,
 *    paths_kernel = SDR_SGBM_PATHS_CHAIN), in either record format; MODE_SGBM_3WAY, the sweeps and
 *    the two-column / two-chain kernels keep the records by row, as does a frame so tall that a
 *    diagonal chain's 32 steps of column stride would span 2^31 bytes.  The maps a call computes do
 *    not depend on the order.
 * reach: elements from a frame's first record to the end of the farthest one the fused pass loads
 * (its last partial block of 12 rows reads whole; 0 for a sweep).  reach - frame <= slack, the
 * elements the buffer keeps in front of the first frame's records and behind the last frame's span. */
enum { SDR_SGBM_RECORDS_BY_ROW = 0, SDR_SGBM_RECORDS_BY_COLUMN = 1 };
typedef struct sdr_sgbm_records {
    int32_t order;          /* SDR_SGBM_RECORDS_BY_* */
    int32_t r12;            /* 12-bit records */
    int32_t nrec, pix;      /* R; int16 elements of a pixel's R records */
    int64_t xs, ys;         /* int16 elements a step along x, along y */
    int64_t frame;          /* int16 elements between frames (R*H*W1*D in either format) */
    int64_t slack, reach;
} sdr_sgbm_records;
/* sdr_sgbm_plan_query's arguments and rules (SDR_PATH_ORDER and SDR_PATH_REC of the environment
 * are honoured as a new handle would); a frame that matches no column reports all zeros. */
int sdr_sgbm_records_query(const sdr_sgbm_params* p, int cost, int width, int height, int nframes,
                           int channels, int cus, sdr_sgbm_records* out);
/* The records of the handle's last call that ran the stages. */
int sdr_sgbm_last_records(const sdr_sgbm* h, sdr_sgbm_records* out);

/* Device self-test of the cross-lane primitives the kernels rely on (DPP wave shifts,
 * permlane swaps); fills 4 failure counters, all zero on a healthy gfx950. */
int sdr_selftest_wave_ops(int* failures4);

/* The device's streaming rate: `iters` back-to-back copies of a `bytes` buffer, the fastest of
 * several access shapes (16-byte loads, 4 or 8 in flight per thread, plain or non-temporal
 * stores, 2-16 workgroups a CU), read + write bytes per second in GB/s.  bench.py records it
 * beside the dominant kernel's rate (box-to-box spread).  _ex fills gbs3 = {copy, read-only,
 * write-only}. */
int sdr_stream_probe(int device, size_t bytes, int iters, double* gbs);
int sdr_stream_probe_ex(int device, size_t bytes, int iters, double* gbs3);

/* Diagnostics: synchronously copy an internal buffer of the last compute to host memory.
 * stage 0 = cost volume C [F][H][W1][D] s16, 1 = WTA disparity before the LR check [F][H][W] s16,
 * 2 = after the LR check (computed from stages 1 and 5 on request: the pipeline's median computes
 * it per tile and never writes it), 3 = final (median + speckle), 4 = the raw bytes of the path-cost
 * records (every direction but top-to-bottom, whose L is consumed on chip by the fused WTA pass;
 * the formats below), 5 = the right view's WTA keys [F][H][W] u32: (minS << 16 | 0xffff - x) of the
 * winning left pixel x (matched column) per right-view column, 0xffffffff where none (not built
 * when the LR check cannot fire), 6 = MODE_SGBM_3WAY's stripe-start cost rows [F][stripes][rows][W1][D]
 * s16 (rows = the largest stripe's count); stage 1 holds values only in the matched columns,
 * 7 = the census descriptors [F][2][H][W] u64 (index 0: the frame's left-role image, 1: its
 * right-role image; an error when the last compute used SDR_COST_BT),
 * 8 = the prefilter's left operands [F][H][W][3*cn] u32, per channel c the words 3c..3c+2 of 16-bit
 * halves {sobel | sobel_lo << 16} {sobel_hi | raw << 16} {raw_lo | raw_hi << 16} (lo / hi: the
 * Birchfield-Tomasi envelope of the value and its two half-sample neighbours), 9 = the right
 * operands [F][3*cn][H][W] u64, per channel c the planes 3c..3c+2 of words q(x) | q(max(x-1, 0)) << 16
 * with q = {sobel | sobel_lo << 32} {sobel_hi | raw << 32} {raw_lo | raw_hi << 32} (stages 8 and 9:
 * an error when the last compute used the census cost; a frame of a paired batch's second half
 * holds its roles swapped).
 *
 * Stage 4, the path-cost records, pixel-interleaved in the summation order E, W, [N,] SE, SW[, NE,
 * NW] (R = P-1 directions; frames R*H*W1*D*2 bytes apart in either format; always in the row order
 * below -- a call that kept them by column, sdr_sgbm_last_records, has them turned on the host):
 *  - int16: [F][H][W1][R][D] s16, the path costs L themselves.
 *  - 12-bit (the default where it applies: P2 <= 4095, numDisparities = 128, MODE_SGBM, MODE_HH4 or
 *    unbatched MODE_HH, and launches that run one chain a wave; SDR_PATH_REC=16 in the environment
 *    when the handle is created forces int16): [F][H][W1][R][D/8] groups of 12 bytes, e = C - L
 *    (0 <= e <= P2) of 8 consecutive disparities d0..d0+7.  As three little-endian u32 w0, w1, w2:
 *    e[d0+2j] = w_j & 0xfff and e[d0+2j+1] = (w_j >> 16) & 0xfff for j = 0..2; e[d0+6] =
 *    (w0 >> 12 & 0xf) | (w1 >> 12 & 0xf) << 4 | (w2 >> 12 & 0xf) << 8, and e[d0+7] the same from
 *    bits 28..31.  A pixel's R records take R*D*3/2 bytes; the rest of a frame's span is unused.
 *  - a batch that swept (MODE_HH, >= 8 frames; sdr_sgbm_last_plan says SDR_SGBM_SOUTH_SWEEP):
 *    [F][H][W1][3][D] s16, frames 3*H*W1*D*2 bytes apart: record 0 = L of E, record 1 = L of W,
 *    record 2 = the up record, min(32767, L_N + L_NE + L_NW) -- the saturating sum of the three
 *    bottom-to-top directions' path costs, written by the up sweep.  The down sweep adds S, SE and
 *    SW on chip; path costs are non-negative, so the grouped saturating sum equals the sum of all
 *    eight in the order above. */
int sdr_sgbm_debug_stage(const sdr_sgbm* h, int stage, void* host_dst, size_t bytes);

/* Page-locked host memory (the role of cv::cuda::HostMem): host buffers from sdr_host_alloc that
 * are passed to the host-pointer entry points are copied to and from by DMA directly, without
 * the staging copy pageable memory needs. */
int sdr_host_alloc(size_t bytes, void** out);
int sdr_host_free(void* p);

const char* sdr_last_error(void);
int sdr_abi_version(void);
/* Hash of the sources the library was built from (stereo_depth_ruler_amd/build.py source_hash):
 * the build and the smoke test compare it with the tree's sources. */
const char* sdr_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
