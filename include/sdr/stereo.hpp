// stereo.hpp -- header-only C++ facade over the C ABI (sdr.h) with the reference's C++ surface:
//
//   sdr::StereoSGBM::create(...) / compute(L, R, disp)      <- cv::StereoSGBM
//       reference stereo_vision/src/stereo_disparity.cpp:5-9,27-28, point_cloud/src/pcd_write.cpp:102-111
//   sdr::reprojectImageTo3D(disp, xyz, Q, handleMissing)    <- cv::reprojectImageTo3D
//       stereo_disparity.cpp:78, pcd_write.cpp:116
//   sdr::ximgproc::createRightMatcher(left)                 <- cv::ximgproc::createRightMatcher
//   sdr::ximgproc::createDisparityWLSFilter(left)           <- cv::ximgproc::createDisparityWLSFilter
//       stereo_disparity.cpp:10-13,31,36
//   sdr::StereoDisparity                                     <- class StereoDisparity
//       stereo_vision/include/stereo_disparity.hpp:8-24
//   sdr::Display                                             <- show_disparityMap / show_depthMap,
//       the displayer's JET overlay and depth_coverage (stereo_displayer.cpp:105-118,164-173)
//   sdr::Ruler / sdr::MeasurementLog                         <- onMouseMeasure / save_csvFile
//       stereo_displayer.cpp:24-63,74-102
//
// sdr::Mat is a minimal owning image (rows, cols, OpenCV type code, row step) so that callers
// can switch from cv::Mat without OpenCV present; when OpenCV is available, wrap cv::Mat data
// pointers with sdr::Mat::view(...) at zero cost.  Errors throw sdr::Exception (cf. cv::Exception).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "sdr.h"

namespace sdr {

enum { CV_8UC1 = 0, CV_16SC1 = 3, CV_32FC1 = 5, CV_64FC1 = 6, CV_8UC3 = 16, CV_32FC3 = 21 };

inline size_t elem_size(int type) {
    switch (type) {
    case CV_8UC1: return 1;
    case CV_16SC1: return 2;
    case CV_32FC1: return 4;
    case CV_64FC1: return 8;
    case CV_8UC3: return 3;
    case CV_32FC3: return 12;
    default: throw std::invalid_argument("sdr::Mat: unsupported type");
    }
}

class Exception : public std::runtime_error {
public:
    Exception(int code, const std::string& msg) : std::runtime_error(msg), code(code) {}
    int code;
};

inline void check(int rc) {
    if (rc != SDR_OK) throw Exception(rc, sdr_last_error());
}

namespace detail {
// Page-locked blocks are expensive to allocate (the driver pins every page), and the reference's
// calls return fresh Mats per frame (StereoDisparity::computeDisparity, computeDepth): released
// blocks are kept here and handed to the next allocation of a similar size (best fit within 2x),
// up to kPinPoolBytes, so a per-frame Mat costs no pinning after the first frames.  The pool is
// never destroyed (Mats may outlive static destruction); the process exit releases its blocks.
struct PinPool {
    static constexpr size_t kPinPoolBytes = (size_t)512 << 20;
    std::mutex mu;
    std::multimap<size_t, void*> free_;
    size_t held = 0;
    void* get(size_t n, size_t* got) {
        {
            std::lock_guard<std::mutex> lk(mu);
            auto it = free_.lower_bound(n);
            if (it != free_.end() && it->first <= 2 * n) {
                void* p = it->second;
                *got = it->first;
                held -= it->first;
                free_.erase(it);
                return p;
            }
        }
        void* p = nullptr;
        if (sdr_host_alloc(n, &p) != SDR_OK) return nullptr;
        *got = n;
        return p;
    }
    void put(void* p, size_t n) {
        std::lock_guard<std::mutex> lk(mu);
        free_.emplace(n, p);
        held += n;
        while (held > kPinPoolBytes && !free_.empty()) {  // evict the largest blocks first
            auto it = std::prev(free_.end());
            held -= it->first;
            sdr_host_free(it->second);
            free_.erase(it);
        }
    }
};
inline PinPool& pin_pool() {
    static PinPool* pool = new PinPool();
    return *pool;
}
// a page-locked block of at least n bytes (nullptr if page-locked memory is unavailable)
inline std::shared_ptr<void> pinned_block(size_t n) {
    size_t got = 0;
    void* p = pin_pool().get(n, &got);
    if (!p) return nullptr;
    return std::shared_ptr<void>(p, [got](void* q) { pin_pool().put(q, got); });
}
}  // namespace detail

class Mat {
public:
    int rows = 0, cols = 0, type = CV_8UC1;
    size_t step = 0;  // bytes per row
    uint8_t* data = nullptr;

    Mat() = default;
    Mat(int r, int c, int t) { create(r, c, t); }
    static Mat view(int r, int c, int t, void* p, size_t step_bytes = 0) {
        Mat m;
        m.rows = r; m.cols = c; m.type = t;
        m.step = step_bytes ? step_bytes : (size_t)c * elem_size(t);
        m.data = (uint8_t*)p;
        return m;
    }
    // like cv::Mat::create: reallocates only when the shape or type changes.  The storage is
    // page-locked (sdr_host_alloc), so the engine's host-pointer calls DMA straight to and from
    // every Mat the facade allocates -- compute()'s disparity, reprojectImageTo3D's xyz,
    // computeDisparity's output -- with no staging copy; where page-locked memory is unavailable
    // (no HIP device) it falls back to ordinary memory, which the engine stages.
    void create(int r, int c, int t) {
        if (data && r == rows && c == cols && t == type) return;
        alloc(r, c, t, true);
    }
    // explicit page-locked storage (cv::cuda::HostMem(PAGE_LOCKED).createMatHeader()); throws if
    // it cannot be had
    static Mat page_locked(int r, int c, int t) {
        Mat m;
        m.rows = r; m.cols = c; m.type = t;
        m.step = (size_t)c * elem_size(t);
        auto b = detail::pinned_block(std::max<size_t>((size_t)r * m.step, 1));
        if (!b) throw Exception(SDR_ERR_NOMEM, std::string("page-locked allocation failed: ") + sdr_last_error());
        m.store_ = b;
        m.data = (uint8_t*)b.get();
        return m;
    }
    // ordinary (pageable) storage
    static Mat pageable(int r, int c, int t) {
        Mat m;
        m.alloc(r, c, t, false);
        return m;
    }
    bool empty() const { return !data || rows == 0 || cols == 0; }
    template <typename T> T* ptr(int y) { return (T*)(data + (size_t)y * step); }
    template <typename T> const T* ptr(int y) const { return (const T*)(data + (size_t)y * step); }
    template <typename T> T& at(int y, int x) { return ptr<T>(y)[x]; }
    Mat clone() const {
        Mat m(rows, cols, type);
        for (int y = 0; y < rows; y++) std::memcpy(m.ptr<uint8_t>(y), ptr<uint8_t>(y), (size_t)cols * elem_size(type));
        return m;
    }

private:
    void alloc(int r, int c, int t, bool pinned) {
        rows = r; cols = c; type = t;
        step = (size_t)c * elem_size(t);
        const size_t bytes = std::max<size_t>((size_t)r * step, 1);
        if (pinned) {
            if (auto b = detail::pinned_block(bytes)) {
                store_ = b;
                data = (uint8_t*)b.get();
                return;
            }
        }
        auto v = std::make_shared<std::vector<uint8_t>>(bytes);
        data = v->data();
        store_ = v;
    }
    std::shared_ptr<void> store_;
};

template <class T> using Ptr = std::shared_ptr<T>;

// Q (4x4, CV_64F or CV_32F) as 16 doubles
inline void q_of(const Mat& Q, double q[16]) {
    if (Q.rows != 4 || Q.cols != 4) throw Exception(SDR_ERR_ARG, "Q must be 4x4");
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            q[i * 4 + j] = Q.type == CV_64FC1 ? Q.ptr<double>(i)[j] : (double)Q.ptr<float>(i)[j];
}

class StereoSGBM {
public:
    enum { MODE_SGBM = SDR_MODE_SGBM, MODE_HH = SDR_MODE_HH, MODE_SGBM_3WAY = SDR_MODE_SGBM_3WAY,
           MODE_HH4 = SDR_MODE_HH4 };
    // the matching cost (sdr.h): OpenCV's Birchfield-Tomasi cost, or the 9x7 census Hamming cost
    enum { COST_BT = SDR_COST_BT, COST_CENSUS = SDR_COST_CENSUS_9X7 };

    static Ptr<StereoSGBM> create(int minDisparity = 0, int numDisparities = 16, int blockSize = 3,
                                  int P1 = 0, int P2 = 0, int disp12MaxDiff = 0, int preFilterCap = 0,
                                  int uniquenessRatio = 0, int speckleWindowSize = 0,
                                  int speckleRange = 0, int mode = MODE_SGBM, int device = 0) {
        sdr_sgbm_params p;
        sdr_sgbm_params_default(&p);
        p.minDisparity = minDisparity; p.numDisparities = numDisparities; p.blockSize = blockSize;
        p.P1 = P1; p.P2 = P2; p.disp12MaxDiff = disp12MaxDiff; p.preFilterCap = preFilterCap;
        p.uniquenessRatio = uniquenessRatio; p.speckleWindowSize = speckleWindowSize;
        p.speckleRange = speckleRange; p.mode = mode;
        return Ptr<StereoSGBM>(new StereoSGBM(p, device));
    }
    static Ptr<StereoSGBM> create(const sdr_sgbm_params& p, int device = 0) {
        return Ptr<StereoSGBM>(new StereoSGBM(p, device));
    }
    ~StereoSGBM() { sdr_sgbm_destroy(h_); }
    StereoSGBM(const StereoSGBM&) = delete;
    StereoSGBM& operator=(const StereoSGBM&) = delete;

    // StereoMatcher::compute: CV_8UC1 or CV_8UC3 pair -> CV_16SC1 disparity (1/16 px); disp is
    // (re)allocated
    void compute(const Mat& left, const Mat& right, Mat& disparity) {
        if (left.rows != right.rows || left.cols != right.cols || left.type != right.type)
            throw Exception(SDR_ERR_ARG, "left and right images must have the same size and type");
        if ((left.type != CV_8UC1 && left.type != CV_8UC3) || left.step != right.step)
            throw Exception(SDR_ERR_TYPE, "8-bit 1- or 3-channel images with equal steps are required");
        disparity.create(left.rows, left.cols, CV_16SC1);
        check(sdr_sgbm_compute(h_, left.data, right.data, left.cols, left.rows,
                               left.type == CV_8UC3 ? 3 : 1, left.step, (int16_t*)disparity.data,
                               disparity.step / 2));
    }

    // compute -> convertTo(CV_32F, 1/16) -> reprojectImageTo3D(Q, handleMissingValues) in one call
    // (pcd_write.cpp:111-116), the float disparity kept on the device; xyz CV_32FC3
    void computeReproject(const Mat& left, const Mat& right, const Mat& Q, bool handleMissingValues,
                          Mat& disparity, Mat& xyz) {
        if (left.rows != right.rows || left.cols != right.cols || left.type != right.type)
            throw Exception(SDR_ERR_ARG, "left and right images must have the same size and type");
        if (left.type != CV_8UC1 || left.step != right.step)
            throw Exception(SDR_ERR_TYPE, "8-bit single-channel images with equal steps are required");
        double q[16];
        q_of(Q, q);
        disparity.create(left.rows, left.cols, CV_16SC1);
        xyz.create(left.rows, left.cols, CV_32FC3);
        check(sdr_sgbm_compute_reproject(h_, left.data, right.data, left.cols, left.rows, left.step,
                                         (int16_t*)disparity.data, disparity.step / 2, q,
                                         handleMissingValues ? 1 : 0, (float*)xyz.data, xyz.step / 4));
    }

    int getMinDisparity() const { return p_.minDisparity; }
    void setMinDisparity(int v) { p_.minDisparity = v; push(); }
    int getNumDisparities() const { return p_.numDisparities; }
    void setNumDisparities(int v) { p_.numDisparities = v; push(); }
    int getBlockSize() const { return p_.blockSize; }
    void setBlockSize(int v) { p_.blockSize = v; push(); }
    int getP1() const { return p_.P1; }
    void setP1(int v) { p_.P1 = v; push(); }
    int getP2() const { return p_.P2; }
    void setP2(int v) { p_.P2 = v; push(); }
    int getDisp12MaxDiff() const { return p_.disp12MaxDiff; }
    void setDisp12MaxDiff(int v) { p_.disp12MaxDiff = v; push(); }
    int getPreFilterCap() const { return p_.preFilterCap; }
    void setPreFilterCap(int v) { p_.preFilterCap = v; push(); }
    int getUniquenessRatio() const { return p_.uniquenessRatio; }
    void setUniquenessRatio(int v) { p_.uniquenessRatio = v; push(); }
    int getSpeckleWindowSize() const { return p_.speckleWindowSize; }
    void setSpeckleWindowSize(int v) { p_.speckleWindowSize = v; push(); }
    int getSpeckleRange() const { return p_.speckleRange; }
    void setSpeckleRange(int v) { p_.speckleRange = v; push(); }
    int getMode() const { return p_.mode; }
    void setMode(int v) { p_.mode = v; push(); }
    int getCostType() const {
        const int c = sdr_sgbm_get_cost(h_);
        if (c < 0) check(c);
        return c;
    }
    void setCostType(int v) { check(sdr_sgbm_set_cost(h_, v)); }

    const sdr_sgbm_params& params() const { return p_; }
    sdr_sgbm* handle() const { return h_; }
    int device() const { return dev_; }

private:
    StereoSGBM(const sdr_sgbm_params& p, int device) : p_(p), dev_(device) {
        check(sdr_sgbm_create(&p_, device, &h_));
    }
    void push() { check(sdr_sgbm_set_params(h_, &p_)); }
    sdr_sgbm_params p_;
    sdr_sgbm* h_ = nullptr;
    int dev_ = 0;
};

// cv::reprojectImageTo3D(disparity CV_32F or CV_16S, _3dImage CV_32FC3, Q 4x4, handleMissing)
// convertTo: disp.convertTo(f, CV_32F, 1/16) as the reference does before reprojecting
inline void convertTo32F(const Mat& disp16, Mat& f, double scale) {
    if (disp16.type != CV_16SC1) throw Exception(SDR_ERR_TYPE, "convertTo32F expects CV_16S");
    f.create(disp16.rows, disp16.cols, CV_32FC1);
    const float a = (float)scale;
    for (int y = 0; y < disp16.rows; y++) {  // a plain loop per row: the compiler vectorises it
        const int16_t* __restrict__ s = disp16.ptr<int16_t>(y);
        float* __restrict__ d = f.ptr<float>(y);
        for (int x = 0; x < disp16.cols; x++) d[x] = (float)s[x] * a;
    }
}

inline void reprojectImageTo3D(const Mat& disparity, Mat& xyz, const Mat& Q,
                               bool handleMissingValues = false) {
    double q[16];
    q_of(Q, q);
    Mat f = disparity;
    if (disparity.type == CV_16SC1) {  // OpenCV reads CV_16S values as-is (no 1/16 scaling)
        f = Mat::pageable(disparity.rows, disparity.cols, CV_32FC1);
        for (int y = 0; y < disparity.rows; y++)
            for (int x = 0; x < disparity.cols; x++) f.ptr<float>(y)[x] = (float)disparity.ptr<int16_t>(y)[x];
    } else if (disparity.type != CV_32FC1) {
        throw Exception(SDR_ERR_TYPE, "disparity must be CV_32F or CV_16S");
    }
    xyz.create(disparity.rows, disparity.cols, CV_32FC3);
    check(sdr_reproject(f.ptr<float>(0), f.cols, f.rows, f.step / 4, q, handleMissingValues ? 1 : 0,
                        xyz.ptr<float>(0), xyz.step / 4));
}

namespace ximgproc {
// cv::ximgproc::createRightMatcher(matcher_left)
inline Ptr<StereoSGBM> createRightMatcher(const Ptr<StereoSGBM>& left) {
    sdr_sgbm_params r;
    sdr_right_matcher_params(&left->params(), &r);
    Ptr<StereoSGBM> right = StereoSGBM::create(r, left->device());
    right->setCostType(left->getCostType());
    return right;
}

// cv::ximgproc::DisparityWLSFilter (stereo_disparity.cpp:11-13,31,36)
class DisparityWLSFilter {
public:
    DisparityWLSFilter(const sdr_wls_params& p, int device) : p_(p) { check(sdr_wls_create(&p_, device, &h_)); }
    ~DisparityWLSFilter() { sdr_wls_destroy(h_); }
    DisparityWLSFilter(const DisparityWLSFilter&) = delete;
    DisparityWLSFilter& operator=(const DisparityWLSFilter&) = delete;

    double getLambda() const { return p_.lambda; }
    void setLambda(double v) { p_.lambda = v; push(); }
    double getSigmaColor() const { return p_.sigma_color; }
    void setSigmaColor(double v) { p_.sigma_color = v; push(); }
    int getLRCthresh() const { return p_.lrc_thresh; }
    void setLRCthresh(int v) { p_.lrc_thresh = v; push(); }
    int getDepthDiscontinuityRadius() const { return p_.depth_discontinuity_radius; }
    void setDepthDiscontinuityRadius(int v) { p_.depth_discontinuity_radius = v; push(); }
    // engine extension: FGS line solver, SDR_FGS_THOMAS (default) or SDR_FGS_PCR (sdr.h)
    int getFgsSolver() const { return p_.fgs_solver; }
    void setFgsSolver(int v) { p_.fgs_solver = v; push(); }

    // filter(disparity_map_left CV_16S, left_view CV_8UC1, filtered CV_16S, disparity_map_right CV_16S)
    void filter(const Mat& dl, const Mat& left_view, Mat& filtered, const Mat& dr) {
        if (dl.type != CV_16SC1 || dr.type != CV_16SC1 || dl.rows != dr.rows || dl.cols != dr.cols)
            throw Exception(SDR_ERR_TYPE, "disparity maps must be CV_16S of equal size");
        if (left_view.type != CV_8UC1 || left_view.rows != dl.rows || left_view.cols != dl.cols)
            throw Exception(SDR_ERR_TYPE, "left_view must be CV_8UC1 of the disparity map's size");
        if (dl.step != (size_t)dl.cols * 2 || dr.step != (size_t)dr.cols * 2)
            throw Exception(SDR_ERR_ARG, "disparity maps must be continuous");
        filtered.create(dl.rows, dl.cols, CV_16SC1);
        conf_.create(dl.rows, dl.cols, CV_32FC1);
        check(sdr_wls_filter(h_, dl.ptr<int16_t>(0), dr.ptr<int16_t>(0), left_view.data, dl.cols,
                             dl.rows, left_view.step, filtered.ptr<int16_t>(0), conf_.ptr<float>(0)));
    }
    Mat getConfidenceMap() const { return conf_; }
    sdr_wls* handle() const { return h_; }

private:
    void push() { check(sdr_wls_set_params(h_, &p_)); }
    sdr_wls_params p_;
    sdr_wls* h_ = nullptr;
    Mat conf_;
};

// cv::ximgproc::createDisparityWLSFilter(matcher_left): also switches the left matcher to
// disp12MaxDiff = 1e6, speckleWindowSize = 0, uniquenessRatio = 0, as ximgproc does
inline Ptr<DisparityWLSFilter> createDisparityWLSFilter(const Ptr<StereoSGBM>& left) {
    sdr_sgbm_params m = left->params();
    sdr_wls_params p;
    sdr_wls_params_for_sgbm(&m, &p);
    left->setDisp12MaxDiff(m.disp12MaxDiff);
    left->setSpeckleWindowSize(m.speckleWindowSize);
    left->setUniquenessRatio(m.uniquenessRatio);
    return Ptr<DisparityWLSFilter>(new DisparityWLSFilter(p, left->device()));
}
}  // namespace ximgproc

// Display outputs on the engine: the EMA history of one StereoDisparity
// (prev_vis / prev_depth_vis, stereo_disparity.hpp:11), show_disparityMap / show_depthMap, the live
// loop's JET overlay and StereoDisplayer::depth_coverage (stereo_displayer.cpp:105-118,167-173).
class Display {
public:
    explicit Display(int device = 0) { check(sdr_display_create(device, &h_)); }
    ~Display() { sdr_display_destroy(h_); }
    Display(const Display&) = delete;
    Display& operator=(const Display&) = delete;

    // CV_32F disparity (px) -> CV_8UC1
    Mat show_disparityMap(const Mat& disparity, int numDisparities) {
        if (disparity.type != CV_32FC1) throw Exception(SDR_ERR_TYPE, "show_disparityMap expects CV_32F");
        Mat out(disparity.rows, disparity.cols, CV_8UC1);
        check(sdr_show_disparity_map(h_, disparity.ptr<float>(0), disparity.cols, disparity.rows,
                                     disparity.step / 4, numDisparities, out.data, out.step));
        return out;
    }
    // CV_32FC3 depth (Z = channel 2) or CV_32F Z -> CV_8UC3 (TURBO); zrange = {zmin, zmax} state
    Mat show_depthMap(const Mat& depth, double* zrange, double* coverage_pct = nullptr) {
        if (depth.type != CV_32FC3 && depth.type != CV_32FC1)
            throw Exception(SDR_ERR_TYPE, "show_depthMap expects CV_32FC3 or CV_32F");
        const int ch = depth.type == CV_32FC3 ? 3 : 1;
        if (depth.step != (size_t)depth.cols * 4 * ch) throw Exception(SDR_ERR_ARG, "depth must be continuous");
        Mat out(depth.rows, depth.cols, CV_8UC3);
        check(sdr_show_depth_map(h_, depth.ptr<float>(0), depth.cols, depth.rows, ch, zrange, out.data,
                                 coverage_pct));
        return out;
    }
    // applyColorMap(vis, JET) + addWeighted(resize(left_rect, 0.5, INTER_AREA), 0.7, heat, 0.3, 0)
    Mat overlay(const Mat& vis, const Mat& left_rect) {
        if (vis.type != CV_8UC1 || left_rect.type != CV_8UC3 || left_rect.rows != 2 * vis.rows ||
            left_rect.cols != 2 * vis.cols || vis.step != (size_t)vis.cols)
            throw Exception(SDR_ERR_TYPE, "overlay expects CV_8UC1 vis and a CV_8UC3 left view of twice its size");
        Mat out(vis.rows, vis.cols, CV_8UC3);
        check(sdr_disparity_overlay(h_, vis.data, left_rect.data, left_rect.step, vis.cols, vis.rows,
                                    nullptr, out.data));
        return out;
    }
    // StereoDisplayer::depth_coverage(depth_map): percent of Z in [0, 12000] in columns >= 80;
    // read-only (this Display's show_depthMap history is untouched)
    double depth_coverage(const Mat& depth) {
        if (depth.type != CV_32FC3 || depth.step != (size_t)depth.cols * 12)
            throw Exception(SDR_ERR_TYPE, "depth_coverage expects a continuous CV_32FC3 map");
        double pct = 0;
        check(sdr_depth_coverage(h_, depth.ptr<float>(0), depth.cols, depth.rows, 80, &pct));
        return pct;
    }
    sdr_display* handle() const { return h_; }

private:
    sdr_display* h_ = nullptr;
};

// The ruler: StereoDisplayer::onMouseMeasure (stereo_displayer.cpp:24-63) and save_csvFile (:74-102).
using Measurement = sdr_measurement;
using Plane = sdr_plane;
using PlaneDistance = struct sdr_plane_distance;  // the C record shares its name with a function
using Relief = sdr_relief;
using Footprint = sdr_footprint;
using Object = sdr_object;
using ObjectScan = sdr_object_scan;
using Clearance = struct sdr_clearance;  // the C record shares its name with a function
struct Point {
    int x = 0, y = 0;
};

class Ruler {
public:
    explicit Ruler(const Mat& Q_matrix, int radius = 0, int min_count = 1, float min_disp = -1.0f,
                   float conf_min = 0.0f, bool profile = false) {
        q_of(Q_matrix, q_);
        sdr_ruler_params_default(&p_);
        p_.radius = radius;
        p_.min_count = min_count;
        p_.min_disp = min_disp;
        p_.conf_min = conf_min;
        p_.profile = profile ? 1 : 0;
    }
    const sdr_ruler_params& params() const { return p_; }

    // K segments on one disparity map (CV_32F in px, or CV_16S in 1/16 px) with an optional
    // continuous CV_32F confidence map; profile (optional, with profile = true): rows of
    // {X, Y, Z, d_med}, `cap` a segment, NaN where nothing is written
    std::vector<Measurement> measure(const Mat& disparity, const std::vector<sdr_segment>& segs,
                                     const Mat* conf = nullptr, std::vector<float>* profile = nullptr,
                                     int cap = 0) const {
        check_maps(disparity, conf, "measure");
        std::vector<Measurement> out(segs.size());
        sdr_ruler_params p = p_;
        float* prof = nullptr;
        if (profile && p.profile) {
            p.profile_cap = cap;
            profile->assign(segs.size() * (size_t)cap * 4, std::numeric_limits<float>::quiet_NaN());
            prof = profile->empty() ? nullptr : profile->data();
        }
        on_maps(sdr_measure_disp, disparity, conf, q_, &p, segs.empty() ? nullptr : segs.data(), (int)segs.size(),
                out.empty() ? nullptr : out.data(), prof);
        return out;
    }
    Measurement measure(const Mat& disparity, Point a, Point b, const Mat* conf = nullptr) const {
        return measure(disparity, {sdr_segment{0, a.x, a.y, b.x, b.y}}, conf)[0];
    }
    // the reference's own measurement on a computeDepth map (CV_32FC3)
    std::vector<Measurement> measure_xyz(const Mat& depth, const std::vector<sdr_segment>& segs) const {
        if (depth.type != CV_32FC3) throw Exception(SDR_ERR_TYPE, "measure_xyz expects a CV_32FC3 map");
        std::vector<Measurement> out(segs.size());
        check(sdr_measure_xyz(depth.ptr<float>(0), depth.step / 4, depth.step / 4 * depth.rows, depth.cols,
                              depth.rows, 1, segs.empty() ? nullptr : segs.data(), (int)segs.size(),
                              out.empty() ? nullptr : out.data()));
        return out;
    }
    Measurement measure_xyz(const Mat& depth, Point a, Point b) const {
        return measure_xyz(depth, {sdr_segment{0, a.x, a.y, b.x, b.y}})[0];
    }

    // Against a surface (sdr.h, "the ruler against a surface"): robust plane fits of rectangles
    // {frame, x0, y0, x1, y1} (corners in any order) of one disparity map, with the ruler's
    // min_disp and conf_min
    std::vector<Plane> fit_plane(const Mat& disparity, const std::vector<sdr_segment>& regions,
                                 const Mat* conf = nullptr, int iterations = 3, float inlier_px = 1.0f,
                                 int min_inliers = 16) const {
        check_maps(disparity, conf, "fit_plane");
        sdr_plane_params pp;
        sdr_plane_params_default(&pp);
        pp.iterations = iterations;
        pp.inlier_px = inlier_px;
        pp.min_inliers = min_inliers;
        pp.min_disp = p_.min_disp;
        pp.conf_min = p_.conf_min;
        std::vector<Plane> out(regions.size());
        on_maps(sdr_fit_planes, disparity, conf, q_, &pp, regions.empty() ? nullptr : regions.data(),
                (int)regions.size(), out.empty() ? nullptr : out.data());
        return out;
    }
    Plane fit_plane(const Mat& disparity, Point a, Point b, const Mat* conf = nullptr, int iterations = 3,
                    float inlier_px = 1.0f, int min_inliers = 16) const {
        return fit_plane(disparity, {sdr_segment{0, a.x, a.y, b.x, b.y}}, conf, iterations, inlier_px,
                         min_inliers)[0];
    }
    // The dominant planes of a rectangle without a prior (sdr.h, "the dominant planes of a region"):
    // a seeded search, the largest plane first.  planes: the planes found (rounds that stopped are
    // left out); rounds: one record a round of max_planes; labels (with_labels): CV_8UC1 of the
    // map's size, the index of the plane a pixel lies on, 255 on none
    struct PlaneSearch {
        std::vector<Plane> planes;
        std::vector<sdr_plane_search_round> rounds;
        Mat labels;
    };
    PlaneSearch find_planes(const Mat& disparity, Point a, Point b, const Mat* conf = nullptr, int max_planes = 4,
                            int hypotheses = 256, uint32_t seed = 0, int iterations = 3, float inlier_px = 1.0f,
                            int min_inliers = 64, bool with_labels = false) const {
        check_maps(disparity, conf, "find_planes");
        sdr_plane_search_params sp;
        sdr_plane_search_params_default(&sp);
        sp.fit.iterations = iterations;
        sp.fit.inlier_px = inlier_px;
        sp.fit.min_inliers = min_inliers;
        sp.fit.min_disp = p_.min_disp;
        sp.fit.conf_min = p_.conf_min;
        sp.max_planes = max_planes;
        sp.hypotheses = hypotheses;
        sp.seed = seed;
        const size_t n = max_planes > 0 ? (size_t)max_planes : 0;
        PlaneSearch out;
        out.planes.resize(n);
        out.rounds.resize(n);
        if (with_labels) out.labels = Mat::pageable(disparity.rows, disparity.cols, CV_8UC1);
        const sdr_segment reg{0, a.x, a.y, b.x, b.y};
        int32_t count = 0;
        on_maps(sdr_find_planes, disparity, conf, q_, &sp, &reg, n ? out.planes.data() : nullptr, &count,
                n ? out.rounds.data() : nullptr, with_labels ? out.labels.data : nullptr);
        out.planes.resize((size_t)count);
        return out;
    }
    // signed distances of points {frame, x, y, plane}, sampled with the ruler's radius and
    // min_count, to `planes`; positive towards the camera
    std::vector<PlaneDistance> plane_distance(const Mat& disparity, const std::vector<Plane>& planes,
                                              const std::vector<sdr_plane_query>& points,
                                              const Mat* conf = nullptr) const {
        check_maps(disparity, conf, "plane_distance");
        sdr_ruler_params p = p_;
        p.profile = 0;
        p.profile_cap = 0;
        std::vector<PlaneDistance> out(points.size());
        on_maps(sdr_plane_distance, disparity, conf, q_, &p, planes.empty() ? nullptr : planes.data(),
                (int)planes.size(), points.empty() ? nullptr : points.data(), (int)points.size(),
                out.empty() ? nullptr : out.data());
        return out;
    }
    PlaneDistance plane_distance(const Mat& disparity, const Plane& plane, Point at,
                                 const Mat* conf = nullptr) const {
        return plane_distance(disparity, std::vector<Plane>{plane}, {sdr_plane_query{0, at.x, at.y, 0}}, conf)[0];
    }
    // The relief of rectangles {frame, x0, y0, x1, y1, plane, label, 0} above `planes` (sdr.h, "the
    // relief of a region"): counts, extremes, exact means and the quantiles (permille, at most 8) of
    // the pixels' heights; labels (optional): a continuous CV_8UC1 map of the disparity's size as
    // find_planes returns it, for queries with label >= 0; band: n_above / n_below count beyond it
    std::vector<Relief> relief(const Mat& disparity, const std::vector<Plane>& planes,
                               const std::vector<sdr_relief_query>& regions, const Mat* labels = nullptr,
                               const Mat* conf = nullptr, const std::vector<int>& quantiles = {50, 500, 950},
                               float band = 0.0f) const {
        check_maps(disparity, conf, "relief");
        check_labels(disparity, labels);
        if (quantiles.size() > 8) throw Exception(SDR_ERR_ARG, "relief takes at most 8 quantiles");
        sdr_relief_params rp;
        sdr_relief_params_default(&rp);
        rp.min_disp = p_.min_disp;
        rp.conf_min = p_.conf_min;
        rp.band = band;
        rp.nq = (int)quantiles.size();
        for (size_t j = 0; j < 8; j++) rp.permille[j] = j < quantiles.size() ? quantiles[j] : 0;
        std::vector<Relief> out(regions.size());
        on_maps(sdr_plane_relief, disparity, conf, labels ? labels->data : nullptr, q_, &rp,
                planes.empty() ? nullptr : planes.data(), (int)planes.size(),
                regions.empty() ? nullptr : regions.data(), (int)regions.size(), out.empty() ? nullptr : out.data());
        return out;
    }
    Relief relief(const Mat& disparity, const Plane& plane, Point a, Point b, const Mat* labels = nullptr,
                  int label = -1, const Mat* conf = nullptr) const {
        return relief(disparity, std::vector<Plane>{plane}, {sdr_relief_query{0, a.x, a.y, b.x, b.y, 0, label, 0}},
                      labels, conf)[0];
    }
    // The footprint of rectangles {frame, x0, y0, x1, y1, plane, label, 0} in the planes of `planes`
    // (sdr.h, "the footprint of a region"): the minimum-area bounding rectangle, over 90 whole-degree
    // directions, of the plane's cells of `cell` (Q's units) that the pixels occupy with `support`
    // members in their 3 x 3 neighbourhood, on a grid of `grid` cells a side; h_lo / h_hi: only the
    // pixels whose height above the plane lies between them; labels and conf as in relief
    std::vector<Footprint> footprint(const Mat& disparity, const std::vector<Plane>& planes,
                                     const std::vector<sdr_relief_query>& regions, const Mat* labels = nullptr,
                                     const Mat* conf = nullptr, float cell = 4.0f, int grid = 512, int support = 4,
                                     float h_lo = -1048576.0f, float h_hi = 1048576.0f) const {
        check_maps(disparity, conf, "footprint");
        check_labels(disparity, labels);
        sdr_footprint_params fp;
        sdr_footprint_params_default(&fp);
        fp.min_disp = p_.min_disp;
        fp.conf_min = p_.conf_min;
        fp.cell = cell;
        fp.grid = grid;
        fp.support = support;
        fp.h_lo = h_lo;
        fp.h_hi = h_hi;
        std::vector<Footprint> out(regions.size());
        on_maps(sdr_plane_footprint, disparity, conf, labels ? labels->data : nullptr, q_, &fp,
                planes.empty() ? nullptr : planes.data(), (int)planes.size(),
                regions.empty() ? nullptr : regions.data(), (int)regions.size(), out.empty() ? nullptr : out.data());
        return out;
    }
    Footprint footprint(const Mat& disparity, const Plane& plane, Point a, Point b, const Mat* labels = nullptr,
                        int label = -1, const Mat* conf = nullptr) const {
        return footprint(disparity, std::vector<Plane>{plane},
                         {sdr_relief_query{0, a.x, a.y, b.x, b.y, 0, label, 0}}, labels, conf)[0];
    }
    // The objects of the rectangle a..b standing on `plane` (sdr.h, "the objects of a region"): the
    // connected sets of pixels whose height above the plane lies in h_lo..h_hi and whose disparities
    // step by at most max_diff between neighbours (connectivity 4 or 8), those of at least min_pixels
    // pixels, the largest first, at most max_objects.  objects: the objects found; scan: the counts and
    // flags; labels (with_labels): CV_8UC1 of the map's size, k on object k's pixels and 255 elsewhere,
    // which relief and footprint take with label k.  labels_in / label: the mask of relief
    struct Objects {
        std::vector<Object> objects;
        ObjectScan scan;
        Mat labels;
    };
    Objects find_objects(const Mat& disparity, const std::vector<Plane>& planes, const sdr_relief_query& region,
                         const Mat* labels_in = nullptr, const Mat* conf = nullptr, float h_lo = 10.0f,
                         float h_hi = 1048576.0f, float max_diff = 1.0f, int connectivity = 8, int min_pixels = 64,
                         int max_objects = 16, bool with_labels = true) const {
        check_maps(disparity, conf, "find_objects");
        check_labels(disparity, labels_in);
        sdr_object_params op;
        sdr_object_params_default(&op);
        op.min_disp = p_.min_disp;
        op.conf_min = p_.conf_min;
        op.h_lo = h_lo;
        op.h_hi = h_hi;
        op.max_diff = max_diff;
        op.connectivity = connectivity;
        op.min_pixels = min_pixels;
        op.max_objects = max_objects;
        Objects out;
        out.objects.resize(max_objects > 0 && max_objects <= 64 ? (size_t)max_objects : 1);
        std::memset(&out.scan, 0, sizeof out.scan);
        if (with_labels) out.labels = Mat::pageable(disparity.rows, disparity.cols, CV_8UC1);
        on_maps(sdr_find_objects, disparity, conf, labels_in ? labels_in->data : nullptr, q_, &op,
                planes.empty() ? nullptr : planes.data(), (int)planes.size(), &region, out.objects.data(), &out.scan,
                with_labels ? out.labels.data : nullptr);
        out.objects.resize((size_t)out.scan.count);
        return out;
    }
    Objects find_objects(const Mat& disparity, const Plane& plane, Point a, Point b, const Mat* labels_in = nullptr,
                         int label = -1, const Mat* conf = nullptr) const {
        return find_objects(disparity, std::vector<Plane>{plane}, sdr_relief_query{0, a.x, a.y, b.x, b.y, 0, label, 0},
                            labels_in, conf);
    }
    // The clearance of pairs of labelled things {frame, x0, y0, x1, y1, plane, label_a, label_b}
    // (sdr.h, "the clearance of two labelled things"): the smallest 3-D distance between a point of
    // label_a and a point of label_b of `labels` (the map find_objects or find_planes returned), each
    // pixel's point the ruler's sample (radius, min_count) over the pixels of its own label, with the
    // two pixels and points and the distance's parts along and across the plane's normal; h_lo / h_hi:
    // only the pixels whose height above the plane lies between them
    std::vector<Clearance> clearance(const Mat& disparity, const std::vector<Plane>& planes,
                                     const std::vector<sdr_clearance_query>& pairs, const Mat& labels,
                                     const Mat* conf = nullptr, float h_lo = -1048576.0f,
                                     float h_hi = 1048576.0f) const {
        check_maps(disparity, conf, "clearance");
        check_labels(disparity, &labels);
        sdr_clearance_params cp;
        sdr_clearance_params_default(&cp);
        cp.min_disp = p_.min_disp;
        cp.conf_min = p_.conf_min;
        cp.h_lo = h_lo;
        cp.h_hi = h_hi;
        cp.radius = p_.radius;
        cp.min_count = p_.min_count;
        std::vector<Clearance> out(pairs.size());
        on_maps(sdr_clearance, disparity, conf, labels.data, q_, &cp, planes.empty() ? nullptr : planes.data(),
                (int)planes.size(), pairs.empty() ? nullptr : pairs.data(), (int)pairs.size(),
                out.empty() ? nullptr : out.data());
        return out;
    }
    Clearance clearance(const Mat& disparity, const Plane& plane, Point a, Point b, const Mat& labels, int label_a,
                        int label_b, const Mat* conf = nullptr) const {
        return clearance(disparity, std::vector<Plane>{plane},
                         {sdr_clearance_query{0, a.x, a.y, b.x, b.y, 0, label_a, label_b}}, labels, conf)[0];
    }
    // One map of a still scene's last frames (sdr.h, "the ruler over time"; the frames before the `f`
    // freeze of stereo_displayer.cpp:191-196): `frames` 1..32 disparity maps of one size and type,
    // oldest first, `confs` none or as many continuous CV_32F confidence maps.  map is CV_32F in px
    // and goes into every call above WITHOUT a confidence map (the gate was applied frame by frame);
    // fill: the value of a pixel without a consensus, null for the ruler's min_disp.
    struct Fused {
        Mat map;            // CV_32F: the fused value, `fill` without a consensus
        sdr_fusion record;  // the pixels of each class, the holes filled, the outliers replaced
        Mat support;        // CV_8U: the agreeing values of a fused pixel (with_maps only)
        Mat spread;         // CV_32F: their range, NaN where the pixel is not fused (with_maps only)
    };
    Fused fuse(const std::vector<Mat>& frames, const std::vector<Mat>& confs = {}, float tol = 1.0f, int min_count = 2,
               int mode = SDR_FUSE_MEAN, const float* fill = nullptr, bool with_maps = false) const {
        if (frames.empty()) throw Exception(SDR_ERR_ARG, "fuse needs at least one frame");
        if (!confs.empty() && confs.size() != frames.size())
            throw Exception(SDR_ERR_ARG, "fuse takes no confidence maps or one a frame");
        const Mat& f0 = frames[0];
        const size_t es = elem_size(f0.type), row = (size_t)f0.cols * es, frame = row * f0.rows;
        // the entry takes one stack: the frames' rows behind one another
        std::vector<uint8_t> stack(frames.size() * frame);
        std::vector<float> cstack(confs.size() * (size_t)f0.cols * f0.rows);
        for (size_t k = 0; k < frames.size(); k++) {
            const Mat& f = frames[k];
            check_maps(f, confs.empty() ? nullptr : &confs[k], "fuse");
            if (f.type != f0.type || f.rows != f0.rows || f.cols != f0.cols)
                throw Exception(SDR_ERR_ARG, "fuse takes frames of one size and type");
            for (int y = 0; y < f.rows; y++) std::memcpy(stack.data() + k * frame + y * row, f.ptr<uint8_t>(y), row);
            if (!confs.empty()) std::memcpy(cstack.data() + k * (frame / es), confs[k].data, frame / es * 4);
        }
        sdr_fuse_params fp;
        sdr_fuse_params_default(&fp);
        fp.min_disp = p_.min_disp;
        fp.conf_min = p_.conf_min;
        fp.tol = tol;
        fp.fill = fill ? *fill : p_.min_disp;
        fp.min_count = min_count;
        fp.mode = mode;
        Fused out;
        out.map = Mat(f0.rows, f0.cols, CV_32FC1);
        if (with_maps) {
            out.support = Mat::pageable(f0.rows, f0.cols, CV_8UC1);
            out.spread = Mat::pageable(f0.rows, f0.cols, CV_32FC1);
        }
        check(sdr_fuse_disp(stack.data(), f0.type == CV_32FC1 ? SDR_DISP_F32 : SDR_DISP_S16, (size_t)f0.cols,
                            (size_t)f0.cols * f0.rows, f0.cols, f0.rows, (int)frames.size(),
                            confs.empty() ? nullptr : cstack.data(), &fp, out.map.ptr<float>(0),
                            with_maps ? out.support.data : nullptr, with_maps ? out.spread.ptr<float>(0) : nullptr,
                            &out.record));
        return out;
    }

private:
    static void check_labels(const Mat& disparity, const Mat* labels) {
        if (labels && (labels->type != CV_8UC1 || labels->rows != disparity.rows || labels->cols != disparity.cols ||
                       labels->step != (size_t)labels->cols))
            throw Exception(SDR_ERR_TYPE, "labels must be a continuous CV_8U map of the disparity's size");
    }
    static void check_maps(const Mat& disparity, const Mat* conf, const char* what) {
        if (disparity.type != CV_32FC1 && disparity.type != CV_16SC1)
            throw Exception(SDR_ERR_TYPE, std::string(what) + " expects a CV_32F or CV_16S disparity");
        if (conf && (conf->type != CV_32FC1 || conf->rows != disparity.rows || conf->cols != disparity.cols ||
                     conf->step != (size_t)conf->cols * 4))
            throw Exception(SDR_ERR_TYPE, "conf must be a continuous CV_32F map of the disparity's size");
    }
    // entry(the maps' run of a one-frame call: data, type, strides, size, conf; then rest...), checked
    template <typename Entry, typename... Rest>
    static void on_maps(Entry entry, const Mat& disparity, const Mat* conf, Rest... rest) {
        const size_t es = elem_size(disparity.type);
        check(entry(disparity.data, disparity.type == CV_32FC1 ? SDR_DISP_F32 : SDR_DISP_S16, disparity.step / es,
                    disparity.step / es * disparity.rows, disparity.cols, disparity.rows, 1,
                    conf ? conf->ptr<float>(0) : nullptr, rest...));
    }
    double q_[16];
    sdr_ruler_params p_;
};

// measurement_record + save_csvFile: the reference's file, byte for byte
class MeasurementLog {
public:
    void add(int image_index, const Measurement& rec, Point a, Point b) {
        idx_.push_back(image_index);
        segs_.push_back(sdr_segment{0, a.x, a.y, b.x, b.y});
        recs_.push_back(rec);
    }
    size_t size() const { return recs_.size(); }
    std::string to_csv(bool header = true) const {
        const int n = (int)recs_.size();
        const int len = sdr_measurements_csv(idx_.data(), segs_.data(), recs_.data(), n, header, nullptr, 0);
        if (len < 0) check(len);
        std::string s((size_t)len + 1, '\0');
        const int rc = sdr_measurements_csv(idx_.data(), segs_.data(), recs_.data(), n, header, &s[0], s.size());
        if (rc < 0) check(rc);
        s.resize((size_t)len);
        return s;
    }
    // appends (std::ios::app), the header included, as the reference does at every save
    void save_csv(const std::string& path, bool header = true) const {
        const std::string s = to_csv(header);
        FILE* f = std::fopen(path.c_str(), "ab");
        if (!f) throw Exception(SDR_ERR_ARG, "cannot open " + path);
        const bool ok = std::fwrite(s.data(), 1, s.size(), f) == s.size();
        if (std::fclose(f) != 0 || !ok) throw Exception(SDR_ERR_DEVICE, "write failed: " + path);
    }

private:
    std::vector<int> idx_;
    std::vector<sdr_segment> segs_;
    std::vector<Measurement> recs_;
};

// class StereoDisparity (reference stereo_vision/include/stereo_disparity.hpp:8-24)
class StereoDisparity {
public:
    explicit StereoDisparity(const Mat& Q_matrix, int device = 0, int cost = StereoSGBM::COST_BT)
        : Q(Q_matrix.clone()) {
        // stereo_disparity.cpp:5-9: StereoSGBM::create(0, 80, 5, 8*5*5*3, 32*5*5*3, 1, 63, 12, 200, 2, 3WAY)
        matcher = StereoSGBM::create(0, 80, 5, 8 * 5 * 5 * 3, 32 * 5 * 5 * 3, 1, 63, 12, 200, 2,
                                     StereoSGBM::MODE_SGBM_3WAY, device);
        matcher->setCostType(cost);
        right_matcher = ximgproc::createRightMatcher(matcher);          // :10 (copies the cost type)
        wls_filter = ximgproc::createDisparityWLSFilter(matcher);       // :11
        wls_filter->setLambda(8000.0);                                   // :12
        wls_filter->setSigmaColor(1.1);                                  // :13
    }
    // BGR 8UC3 rectified pair (full res) -> CV_32F disparity in px at half resolution
    Mat computeDisparity(const Mat& left, const Mat& right) {
        if (left.type != CV_8UC3 || right.type != CV_8UC3 || left.rows != right.rows ||
            left.cols != right.cols || left.step != right.step)
            throw Exception(SDR_ERR_TYPE, "computeDisparity expects two equal-size BGR images");
        Mat out(left.rows / 2, left.cols / 2, CV_32FC1);
        conf_map.create(left.rows / 2, left.cols / 2, CV_32FC1);
        check(sdr_stereo_class_compute(matcher->handle(), right_matcher->handle(),
                                       wls_filter->handle(), left.data, right.data, left.cols,
                                       left.rows, left.step, out.ptr<float>(0), out.step / 4,
                                       nullptr, nullptr, nullptr, conf_map.ptr<float>(0)));
        return out;
    }
    Mat computeDepth(const Mat& disparity) {  // stereo_disparity.cpp:76-80 (handleMissing=false)
        Mat depth;
        reprojectImageTo3D(disparity, depth, Q);
        return depth;
    }
    // a Ruler with this object's Q that treats the matcher's invalid value (minDisparity - 1) as a hole
    Ruler ruler(int radius = 0, int min_count = 1, float conf_min = 0.0f, bool profile = false) const {
        return Ruler(Q, radius, min_count, (float)(matcher->getMinDisparity() - 1), conf_min, profile);
    }
    // onMouseMeasure (stereo_displayer.cpp:24-63) between two pixels of computeDisparity's map
    Measurement measure(const Mat& disparity, Point a, Point b, int radius = 0, int min_count = 1) const {
        return ruler(radius, min_count).measure(disparity, a, b);
    }
    const Ptr<StereoSGBM> get_matcher() const { return matcher; }
    const Mat& getConfidenceMap() const { return conf_map; }  // wls_filter->getConfidenceMap() (:36)

    // stereo_disparity.cpp:42-73: gamma map with the EMA against this object's previous frame
    Mat show_disparityMap(const Mat& disparity) {
        return display().show_disparityMap(disparity, matcher->getNumDisparities());
    }
    // stereo_disparity.cpp:83-124: the range state is function-static in the reference, i.e. one
    // pair of doubles for every StereoDisparity of the process; so it is here
    Mat show_depthMap(const Mat& depth) {
        static double zrange[2] = {1000.0, 2000.0};
        return display().show_depthMap(depth, zrange);
    }

private:
    Display& display() {
        if (!display_) display_ = std::make_shared<Display>(matcher->device());
        return *display_;
    }
    Ptr<StereoSGBM> matcher, right_matcher;
    Ptr<ximgproc::DisparityWLSFilter> wls_filter;
    Mat Q, conf_map;
    Ptr<Display> display_;
};

}  // namespace sdr
