// sdr_entries.hip -- the C entries that take no matcher handle: the error text, parameter
// defaults, reprojection, the post filters and conversions on a caller's stream, the probes and
// the self-test (their kernels: sdr_post.hip).  sdr_reproject, the one host-pointer entry here,
// keeps its stream, buffers and staging a thread (sdr_host.hpp ThreadState).
#include "sdr_host.hpp"
#include "sdr_staging.hpp"

#include <cstring>
#include <string>

namespace {
thread_local std::string g_last_error;

// what sdr_reproject keeps a thread (sdr_host.hpp ThreadState): device buffers and staging
struct ReprojectRes {
    sdr::Buf dd, dx, mins;
    sdr::HostXfer hx;
    void release() {
        sdr::free_bufs({&dd, &dx, &mins});
        hx.release();
    }
};
}  // namespace

int sdr::set_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

using sdr::Buf;
using sdr::check_dims;
using sdr::ensure;
using sdr::set_error;
using sdr::stage_bytes;

extern "C" {

const char* sdr_last_error(void) { return g_last_error.c_str(); }
int sdr_abi_version(void) { return SDR_ABI_VERSION; }

void sdr_sgbm_params_default(sdr_sgbm_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->numDisparities = 16;
    p->blockSize = 3;
    p->mode = SDR_MODE_SGBM;
    p->nstripes = 4;
}

void sdr_right_matcher_params(const sdr_sgbm_params* l, sdr_sgbm_params* r) {
    if (!l || !r) return;
    // ximgproc createRightMatcher: StereoSGBM::create(-(min+num)+1, num, wsize) + setters
    sdr_sgbm_params_default(r);
    r->minDisparity = -(l->minDisparity + l->numDisparities) + 1;
    r->numDisparities = l->numDisparities;
    r->blockSize = l->blockSize;
    r->uniquenessRatio = 0;
    r->P1 = l->P1;
    r->P2 = l->P2;
    r->mode = l->mode;
    r->preFilterCap = l->preFilterCap;
    r->disp12MaxDiff = 1000000;
    r->speckleWindowSize = 0;
    r->speckleRange = l->speckleRange;
    r->nstripes = l->nstripes;
    r->uniq_rule = l->uniq_rule;
}

int sdr_reproject_device(const float* d_disp, int W, int H, size_t disp_stride, const double Q[16],
                         int handle_missing, float* d_xyz, size_t xyz_stride, int F,
                         void* stream) {
    if (!d_disp || !Q || !d_xyz) return set_error(SDR_ERR_ARG, "null argument");
    int rc = check_dims(W, H, disp_stride, F);
    if (rc) return rc;
    if (xyz_stride < (size_t)W * 3) return set_error(SDR_ERR_ARG, "xyz_stride < 3*width");
    // the frames' minima, when missing values are handled
    sdr::ScratchLayout lay;
    const auto s_mins = lay.take<int>((size_t)F);
    sdr::Scratch sc((hipStream_t)stream);
    if (handle_missing && (rc = sc.open(lay))) return rc;
    sdr::launch_reproject_f32(d_disp, W, H, disp_stride, disp_stride * H, Q, handle_missing,
                              handle_missing ? sc.at(s_mins) : nullptr, d_xyz, xyz_stride, xyz_stride * H, F, sc.st);
    return sc.finish();
}

int sdr_filter_speckles_device(int16_t* d_img, int W, int H, int F, int newVal, int maxSpeckleSize,
                               int maxDiff, void* stream) {
    if (!d_img) return set_error(SDR_ERR_ARG, "null argument");
    int rc = check_dims(W, H, (size_t)W, F);
    if (rc) return rc;
    if ((size_t)W * H > (size_t)INT32_MAX) return set_error(SDR_ERR_SIZE, "frame too large");
    if (maxSpeckleSize <= 0) return SDR_OK;  // OpenCV: nothing to do
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)F * W * H;
    sdr::ScratchLayout lay;
    const auto s_labels = lay.take<int>(n), s_sizes = lay.take<int>(n);
    sdr::Scratch sc(st);
    if ((rc = sc.open(lay))) return rc;
    sdr::launch_speckle(d_img, d_img, W, H, F, newVal, maxSpeckleSize, maxDiff, sc.at(s_labels), sc.at(s_sizes),
                        nullptr, st);
    return sc.finish();
}

int sdr_disp16_reproject_device(const int16_t* d_disp, int W, int H, size_t disp_stride,
                                const double Q[16], int handle_missing, float* d_xyz,
                                size_t xyz_stride, int F, void* stream) {
    if (!d_disp || !Q || !d_xyz) return set_error(SDR_ERR_ARG, "null argument");
    int rc = check_dims(W, H, disp_stride, F);
    if (rc) return rc;
    if (xyz_stride < (size_t)W * 3) return set_error(SDR_ERR_ARG, "xyz_stride < 3*width");
    if (handle_missing && disp_stride != (size_t)W)
        return set_error(SDR_ERR_ARG, "handle_missing needs a dense disparity (disp_stride == width)");
    hipStream_t st = (hipStream_t)stream;
    // the frames' partial minima, when missing values are handled
    sdr::ScratchLayout lay;
    const auto s_mins = lay.take<int>((size_t)F * sdr::kMinSlots);
    sdr::Scratch sc(st);
    int* mins = nullptr;
    if (handle_missing) {
        if ((rc = sc.open(lay))) return rc;
        mins = sc.at(s_mins);
        sdr::launch_min_s16(d_disp, (size_t)W * H, disp_stride * H, F, mins, st);
    }
    sdr::launch_reproject_s16(d_disp, W, H, disp_stride, disp_stride * H, Q, handle_missing, mins,
                              d_xyz, xyz_stride, xyz_stride * H, F, st);
    return sc.finish();
}

int sdr_reproject(const float* disp, int W, int H, size_t disp_stride, const double Q[16],
                  int handle_missing, float* xyz, size_t xyz_stride) {
    if (!disp || !Q || !xyz) return set_error(SDR_ERR_ARG, "null argument");
    int rc = check_dims(W, H, disp_stride, 1);
    if (rc) return rc;
    if (xyz_stride < (size_t)W * 3) return set_error(SDR_ERR_ARG, "xyz_stride < 3*width");
    static thread_local sdr::ThreadState<ReprojectRes> S;
    if ((rc = S.acquire())) return rc;
    const size_t px = (size_t)W * H;
    if ((rc = ensure(S.dd, px * 4)) || (rc = ensure(S.dx, px * 12)) || (rc = ensure(S.mins, 4))) return rc;
    if ((rc = S.hx.begin(stage_bytes(px * 4) + stage_bytes(px * 12)))) return rc;
    float* dd = (float*)S.dd.p;
    float* dx = (float*)S.dx.p;
    if ((rc = S.hx.upload(dd, (size_t)W * 4, disp, disp_stride * 4, (size_t)W * 4, H, S.st))) return rc;
    sdr::launch_reproject_f32(dd, W, H, W, px, Q, handle_missing, handle_missing ? (int*)S.mins.p : nullptr, dx,
                              (size_t)W * 3, px * 3, 1, S.st);
    SDR_HIP(hipGetLastError());
    if ((rc = S.hx.download(xyz, xyz_stride * 4, dx, (size_t)W * 12, (size_t)W * 12, H, S.st))) return rc;
    return S.hx.drain();
}

int sdr_disp16_to_float_device(const int16_t* d_disp, float* d_out, size_t n, void* stream) {
    if (!d_disp || !d_out) return set_error(SDR_ERR_ARG, "null argument");
    sdr::launch_disp16_to_f32(d_disp, d_out, n, (hipStream_t)stream);
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

int sdr_bgr2gray_device(const uint8_t* d_bgr, int W, int H, size_t bgr_stride, uint8_t* d_gray,
                        size_t gray_stride, int F, void* stream) {
    if (!d_bgr || !d_gray) return set_error(SDR_ERR_ARG, "null argument");
    int rc = check_dims(W, H, gray_stride, F);
    if (rc) return rc;
    if (bgr_stride < (size_t)W * 3) return set_error(SDR_ERR_ARG, "bgr_stride < 3*width");
    sdr::launch_bgr2gray(d_bgr, W, H, bgr_stride, d_gray, gray_stride, F, (hipStream_t)stream);
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

int sdr_resize_area_half_device(const uint8_t* d_src, int W, int H, size_t stride, uint8_t* d_dst,
                                size_t dst_stride, int F, void* stream) {
    if (!d_src || !d_dst) return set_error(SDR_ERR_ARG, "null argument");
    int rc = check_dims(W, H, stride, F);
    if (rc) return rc;
    if ((W & 1) || (H & 1)) return set_error(SDR_ERR_SIZE, "INTER_AREA 0.5x needs even width and height");
    if (dst_stride < (size_t)W / 2) return set_error(SDR_ERR_ARG, "dst_stride < width/2");
    sdr::launch_area_half(d_src, W, H, stride, d_dst, dst_stride, F, (hipStream_t)stream);
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

int sdr_stream_probe(int device, size_t bytes, int iters, double* gbs) {
    if (!gbs || bytes < 16 || iters < 1) return set_error(SDR_ERR_ARG, "bad argument");
    int ndev = 0;
    SDR_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return set_error(SDR_ERR_DEVICE, "invalid device index");
    SDR_HIP(hipSetDevice(device));
    return sdr::stream_probe(bytes, iters, gbs) ? set_error(SDR_ERR_NOMEM, "stream probe failed") : SDR_OK;
}

int sdr_stream_probe_ex(int device, size_t bytes, int iters, double* gbs3) {
    if (!gbs3 || bytes < 16 || iters < 1) return set_error(SDR_ERR_ARG, "bad argument");
    int ndev = 0;
    SDR_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return set_error(SDR_ERR_DEVICE, "invalid device index");
    SDR_HIP(hipSetDevice(device));
    return sdr::stream_probe_ex(bytes, iters, gbs3) ? set_error(SDR_ERR_NOMEM, "stream probe failed") : SDR_OK;
}

int sdr_selftest_wave_ops(int* failures4) {
    if (!failures4) return set_error(SDR_ERR_ARG, "null argument");
    return sdr::selftest_wave_ops(failures4) ? set_error(SDR_ERR_DEVICE, "selftest launch failed") : SDR_OK;
}

}  // extern "C"
