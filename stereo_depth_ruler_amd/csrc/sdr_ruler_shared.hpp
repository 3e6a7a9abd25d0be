// sdr_ruler_shared.hpp -- what the ruler's units (sdr_ruler.hip, sdr_relief.hip, sdr_footprint.hip) share: the device
// helpers of the region rule, the disparity loads and the canonical NaN, and the host side of the
// host-pointer calls (the argument guards of the maps, the per-thread persistent buffers).
#pragma once
#include <string>

#include "sdr_device.hpp"
#include "sdr_internal.hpp"

namespace sdr {

__device__ __forceinline__ float ruler_nan() { return __builtin_nanf(""); }
// every NaN the ruler computes is written as the canonical quiet NaN (sdr.h): the sign and payload
// of a computed NaN differ between machines
// (tested on the bits: a compiler may fold `v != v ? NaN : v` to v, a NaN's bits being unspecified)
__device__ __forceinline__ float canon(float v) {
    const uint32_t b = __float_as_uint(v);
    return __uint_as_float((b & 0x7fffffffu) > 0x7f800000u ? 0x7fc00000u : b);
}
__device__ __forceinline__ double canon(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return __longlong_as_double((long long)((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull ? 0x7ff8000000000000ull : b));
}
__device__ __forceinline__ bool finite3(const float* p) {
    return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

__device__ __forceinline__ float load_disp(const float* p) { return *p; }
__device__ __forceinline__ float load_disp(const int16_t* p) { return (float)*p * 0.0625f; }

__device__ __forceinline__ bool segment_in_range(const sdr_segment& s, int W, int H, int F) {
    return s.frame >= 0 && s.frame < F && s.x0 >= 0 && s.x0 < W && s.x1 >= 0 && s.x1 < W &&
           s.y0 >= 0 && s.y0 < H && s.y1 >= 0 && s.y1 < H;
}

struct PlaneRect {
    int xs, ys, rw, rh;
};
__device__ __forceinline__ PlaneRect plane_rect(const sdr_segment& s) {
    PlaneRect r;
    r.xs = min(s.x0, s.x1);
    r.ys = min(s.y0, s.y1);
    r.rw = max(s.x0, s.x1) - r.xs + 1;
    r.rh = max(s.y0, s.y1) - r.ys + 1;
    return r;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- host side ----
namespace ruler_host {

#define RULER_HIP(call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return sdr::set_error(SDR_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline int rfail(int code, const char* msg) { return sdr::set_error(code, msg); }

// argument guards shared by the plane fit, the point query and the relief (host only):
// check_disp_args' rules for the maps, with a bad disp_type an argument error too, and the sizes the
// moments allow
inline int check_plane_maps(const void* disp, int disp_type, size_t stride, size_t fstride, int W, int H, int F,
                            const double* Q, const void* params, const void* items, int K, const void* out) {
    if (!disp || !Q || !params) return rfail(SDR_ERR_ARG, "null argument");
    if (K < 0) return rfail(SDR_ERR_ARG, "negative count");
    if (K > 0 && (!items || !out)) return rfail(SDR_ERR_ARG, "null argument");
    if (W <= 0 || H <= 0 || F <= 0) return rfail(SDR_ERR_ARG, "bad size");
    if (W > 8192 || H > 8192 || (size_t)W * (size_t)H > ((size_t)1 << 24))
        return rfail(SDR_ERR_ARG, "the plane fit takes maps of at most 8192 x 8192 and 2^24 pixels");
    if (stride < (size_t)W || fstride < stride * (size_t)(H - 1) + (size_t)W)
        return rfail(SDR_ERR_ARG, "bad stride");
    if (disp_type != SDR_DISP_F32 && disp_type != SDR_DISP_S16)
        return rfail(SDR_ERR_ARG, "disp_type must be SDR_DISP_F32 or SDR_DISP_S16");
    return SDR_OK;
}

// per-thread persistent device buffers and stream of the host-pointer calls (per current device)
struct HostState {
    int device = -1;
    hipStream_t st = nullptr;
    sdr::Buf map, conf, segs, out, prof, planes;
    void release() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (st) (void)hipStreamSynchronize(st);
        for (sdr::Buf* b : {&map, &conf, &segs, &out, &prof, &planes}) {
            if (b->p) (void)hipFree(b->p);
            *b = sdr::Buf();
        }
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
        device = -1;
    }
    ~HostState() { release(); }
};

// one state a thread, whichever unit asks (an inline function's local is one object)
inline int host_state(HostState** out) {
    static thread_local HostState S;
    int dev = 0;
    RULER_HIP(hipGetDevice(&dev));
    if (S.device != dev) {
        S.release();
        RULER_HIP(hipSetDevice(dev));
        RULER_HIP(hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking));
        S.device = dev;
    }
    *out = &S;
    return SDR_OK;
}

// rows of `row_bytes` of F frames of H rows into a dense device buffer
inline int upload_rows(void* dst, const void* src, size_t row_bytes, size_t src_row, size_t src_frame, int H,
                       int F, hipStream_t st) {
    for (int f = 0; f < F; f++)
        RULER_HIP(hipMemcpy2DAsync((char*)dst + (size_t)f * row_bytes * H, row_bytes,
                                   (const char*)src + (size_t)f * src_frame, src_row, row_bytes, H,
                                   hipMemcpyHostToDevice, st));
    return SDR_OK;
}

// the host-pointer calls' maps into the thread's persistent buffers (dense rows)
inline int upload_maps(HostState* S, const void* disp, int disp_type, size_t stride, size_t fstride, int W, int H,
                       int F, const float* conf) {
    const size_t es = disp_type == SDR_DISP_F32 ? 4 : 2, px = (size_t)W * H;
    int rc;
    if ((rc = sdr::ensure(S->map, (size_t)F * px * es)) || (rc = sdr::ensure(S->conf, conf ? (size_t)F * px * 4 : 0)))
        return rc;
    if ((rc = upload_rows(S->map.p, disp, (size_t)W * es, stride * es, fstride * es, H, F, S->st))) return rc;
    if (conf) RULER_HIP(hipMemcpyAsync(S->conf.p, conf, (size_t)F * px * 4, hipMemcpyHostToDevice, S->st));
    return SDR_OK;
}

}  // namespace ruler_host
}  // namespace sdr
