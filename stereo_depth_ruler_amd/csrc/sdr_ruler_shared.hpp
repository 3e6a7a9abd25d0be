// sdr_ruler_shared.hpp -- what the ruler's units (sdr_ruler.hip, sdr_plane.hip, sdr_relief.hip,
// sdr_footprint.hip, sdr_objects.hip, sdr_clearance.hip) share: on the device the disparity loads, the canonical NaN, the
// ordered key of a float, the wave reductions, a rectangle's range test, the maps of a call as its
// kernels take them (RegionMaps, one argument by value: the frame offsets and a rectangle's origin
// are its members and written nowhere else; RegionDims for a kernel that reads no map) and the
// ruler's sample; on the host (ruler_host) the argument
// guards, the Q and disparity-type plumbing of a launch, the per-thread persistent buffers (held in
// sdr_host.hpp's ThreadState) and the staged host-pointer call over them (HostCall).  The region
// rule and the prologue of the kernels that apply it are in sdr_region.hpp.
#pragma once
#include <string>
#include <type_traits>

#include "sdr_device.hpp"
#include "sdr_host.hpp"

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

// float -> key with the floats' order (no NaN among the members); and back
__device__ __forceinline__ unsigned ordered_key(float hf) {
    const unsigned b = __float_as_uint(hf);
    return b ^ ((b & 0x80000000u) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ordered_unkey(unsigned k) {
    return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu));
}

// The size of a call's maps and whether it has label maps: what a kernel takes that reads no map.
struct RegionDims {
    int W, H, F, has_labels;
    __device__ __forceinline__ bool holds(const sdr_segment& s) const { return segment_in_range(s, W, H, F); }
};

// One frame's maps: the disparity with its row stride, the dense confidence and label maps or null.
template <typename T>
struct FrameMaps {
    const T* fd;
    const float* fc;
    const uint8_t* fl;
    size_t stride;
    int W, H;
};

// A rectangle of a frame: the maps at its origin (L: const uint8_t, or uint8_t for the sweep that
// writes labels), so that pixel (u, v) of the rectangle is fd[v * stride + u], fc[v * W + u],
// fl[v * W + u].
template <typename T, typename L = const uint8_t>
struct RegionView {
    PlaneRect R;
    const T* fd;
    const float* fc;
    L* fl;
    size_t stride;
    int W;
};

// The maps of a ruler call, as every kernel that reads one takes them (by value): F frames of
// H x W, the disparity with its strides in elements, the dense confidence and label maps or null.
// Its members are the only place where a frame index or a rectangle's origin becomes an address.
template <typename T>
struct RegionMaps {
    using elem = T;
    const T* disp;
    const float* conf;
    const uint8_t* labels;
    size_t stride, fstride;
    int W, H, F;

    __host__ __device__ RegionDims dims() const { return RegionDims{W, H, F, labels != nullptr}; }
    __device__ __forceinline__ bool holds(const sdr_segment& s) const { return segment_in_range(s, W, H, F); }
    __device__ __forceinline__ bool holds(int frame, int x, int y) const {
        return frame >= 0 && frame < F && x >= 0 && x < W && y >= 0 && y < H;
    }
    __device__ __forceinline__ const T* frame_disp(int f) const { return disp + (size_t)f * fstride; }
    __device__ __forceinline__ const float* frame_conf(int f) const {
        return conf ? conf + (size_t)f * H * W : nullptr;
    }
    __device__ __forceinline__ const uint8_t* frame_labels(int f) const {
        return labels ? labels + (size_t)f * H * W : nullptr;
    }
    __device__ __forceinline__ FrameMaps<T> frame(int f) const {
        return FrameMaps<T>{frame_disp(f), frame_conf(f), frame_labels(f), stride, W, H};
    }
    // the rectangle sg (in range) of frame sg.frame with the label map `fl` of that frame (or null)
    template <typename L>
    __device__ __forceinline__ RegionView<T, L> view(const sdr_segment& sg, L* fl) const {
        RegionView<T, L> v;
        v.R = plane_rect(sg);
        const size_t org = (size_t)v.R.ys * W + (size_t)v.R.xs;
        const float* fc = frame_conf(sg.frame);
        v.fd = frame_disp(sg.frame) + (size_t)v.R.ys * stride + (size_t)v.R.xs;
        v.fc = fc ? fc + org : nullptr;
        v.fl = fl ? fl + org : nullptr;
        v.stride = stride;
        v.W = W;
        return v;
    }
};

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <typename V>
__device__ __forceinline__ V wave_min(V v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
template <typename V>
__device__ __forceinline__ V wave_max(V v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

struct RulerSample {
    float xyz[3];
    float d;
    int n;
    bool valid;
};

// The selection of one sample by one wave (every lane returns the same values): a window's <= 81
// values two a lane (value j = lane + 64 * k of the window's cnt), `ok` which of them count; the
// number that count, and with at least max(min_count, 1) of them *dmed their lower median, by
// counting, for each lane's values, the values that sort before them (ties by window index).
__device__ __forceinline__ int ruler_select(const float (&v)[2], const bool (&ok)[2], int cnt, int min_count,
                                            int lane, float* dmed) {
    const unsigned long long m0 = __ballot(ok[0]), m1 = __ballot(ok[1]);
    const int n = __popcll(m0) + __popcll(m1);
    if (n < min_count || n == 0) return n;
    int rank[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        unsigned long long m = k ? m1 : m0;
        while (m) {
            const int c = __builtin_ctzll(m);
            m &= m - 1;
            const float vc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[k]), c));
            const int jc = c + 64 * k;
            rank[0] += (vc < v[0] || (vc == v[0] && jc < lane)) ? 1 : 0;
            if (cnt > 64) rank[1] += (vc < v[1] || (vc == v[1] && jc < lane + 64)) ? 1 : 0;  // radius 4 only
        }
    }
    const int want = (n - 1) >> 1;
    const unsigned long long h0 = __ballot(ok[0] && rank[0] == want);
    const unsigned long long h1 = __ballot(ok[1] && rank[1] == want);
    // exactly one valid value has rank `want`
    *dmed = h0 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[0]), __builtin_ctzll(h0)))
               : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[1]), __builtin_ctzll(h1 | (1ull << 63))));
    return n;
}

// One sample by one wave (every lane returns the same values): the window's valid values, their
// selection (above), then the reprojection.
template <typename T>
__device__ __forceinline__ RulerSample ruler_sample(const FrameMaps<T>& fm, const Q16& Q, const sdr_ruler_params& P,
                                                    int x, int y, int lane) {
    const T* __restrict__ disp = fm.fd;
    const float* __restrict__ conf = fm.fc;
    const size_t stride = fm.stride;
    const int W = fm.W, H = fm.H;
    const int r = P.radius;
    const int xs = max(x - r, 0), xe = min(x + r, W - 1);
    const int ys = max(y - r, 0), ye = min(y + r, H - 1);
    const int ww = xe - xs + 1, cnt = ww * (ye - ys + 1);
    float v[2];
    bool ok[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int j = lane + 64 * k;
        v[k] = 0.f;
        ok[k] = false;
        if (j < cnt) {
            const int wy = j / ww, wx = j - wy * ww;
            const size_t py = (size_t)(ys + wy), px = (size_t)(xs + wx);
            // both loads issue before either is used (a NaN confidence fails the comparison)
            const float d = load_disp(disp + py * stride + px);
            const float c = conf ? conf[py * (size_t)W + px] : 0.f;
            v[k] = d;
            ok[k] = isfinite(d) && d > P.min_disp && (!conf || c >= P.conf_min);
        }
    }
    RulerSample s;
    s.d = s.xyz[0] = s.xyz[1] = s.xyz[2] = ruler_nan();
    s.valid = false;
    float dmed = 0.f;
    s.n = ruler_select(v, ok, cnt, P.min_count, lane, &dmed);
    if (s.n < P.min_count || s.n == 0) return s;
    s.d = dmed;
    reproject_px(Q, x, y, (double)dmed, 0.0, 0, s.xyz);
    s.valid = finite3(s.xyz);
    return s;
}

// ---- host side ----
namespace ruler_host {

inline int rfail(int code, const char* msg) { return sdr::set_error(code, msg); }

inline sdr::Q16 make_q16(const double* Q) {
    sdr::Q16 q;
    for (int i = 0; i < 16; i++) q.q[i] = Q[i];
    return q;
}

// f(the call's maps as RegionMaps<float> or RegionMaps<int16_t>): the launches of a checked
// disp_type; the arguments are an entry's run (labels: null for an entry that takes none)
template <typename Fn>
inline void with_maps(const void* disp, int disp_type, size_t stride, size_t fstride, int W, int H, int F,
                      const float* conf, const uint8_t* labels, Fn&& f) {
    if (disp_type == SDR_DISP_F32)
        f(sdr::RegionMaps<float>{(const float*)disp, conf, labels, stride, fstride, W, H, F});
    else
        f(sdr::RegionMaps<int16_t>{(const int16_t*)disp, conf, labels, stride, fstride, W, H, F});
}
// the maps' element type from with_maps' argument
template <typename M>
using disp_elem_t = typename std::remove_cv_t<std::remove_reference_t<M>>::elem;

inline int check_planes_arg(const void* planes, int P) {
    if (P < 0 || (P > 0 && !planes)) return rfail(SDR_ERR_ARG, "bad plane count or null planes");
    return SDR_OK;
}

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

// the device buffers of the host-pointer calls, kept by the thread (sdr_host.hpp ThreadState): the
// maps, the confidence, the query rows (segments, regions, points), the outputs of one call, the
// profile, the plane records and the label maps that go in
struct HostBufs {
    sdr::Buf map, conf, rows, out, prof, planes, labels;
    void release() { sdr::free_bufs({&map, &conf, &rows, &out, &prof, &planes, &labels}); }
};
using HostState = sdr::ThreadState<HostBufs>;

// one state a thread, whichever unit asks (an inline function's local is one object)
inline int host_state(HostState** out) {
    static thread_local HostState S;
    *out = &S;
    return S.acquire();
}

// One host-pointer call over the thread's state, from its guards on: the inputs are staged into the
// thread's buffers on the thread's stream, the outputs get places in S->out (sdr_layout.hpp's rule)
// and the host pointers they go back to, the entry runs its device form on stream() and returns
// finish().  The first failure sticks in `rc`: every later operation does nothing and hands out
// null, and ready() and finish() return it.
struct HostCall {
    struct Maps {
        const void* disp;
        const float* conf;
        size_t stride, fstride;  // of the dense device map, in elements
    };
    struct Back {
        void* host;
        const sdr::Buf* buf;
        size_t off, bytes;
    };
    HostState* S = nullptr;
    int rc;
    sdr::ScratchLayout outs;
    Back back[4];  // the most outputs a call has (the plane search)
    int nback = 0;

    HostCall() : rc(host_state(&S)) {}
    void* stream() const { return S->st; }

    int hip(hipError_t e, const char* what) {
        if (e != hipSuccess && !rc) rc = sdr::set_error(SDR_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
        return rc;
    }
    // `bytes` of room in a buffer of the thread; null on a failure
    void* room(sdr::Buf& b, size_t bytes) {
        if (!rc) rc = sdr::ensure(b, bytes);
        return rc ? nullptr : b.p;
    }
    void copy_back(void* host, const sdr::Buf& b, size_t off, size_t bytes) {
        if (rc || !host || !bytes) return;
        if (nback == (int)(sizeof back / sizeof back[0])) {
            rc = rfail(SDR_ERR_ARG, "too many outputs of a host call");
            return;
        }
        back[nback++] = Back{host, &b, off, bytes};
    }

    // F frames of H rows of `row_bytes` (rows src_row, frames src_frame bytes apart) as dense rows
    void* rows(sdr::Buf& b, const void* src, size_t row_bytes, size_t src_row, size_t src_frame, int H, int F) {
        char* dst = (char*)room(b, (size_t)F * H * row_bytes);
        for (int f = 0; f < F && !rc; f++)
            hip(hipMemcpy2DAsync(dst + (size_t)f * row_bytes * H, row_bytes, (const char*)src + (size_t)f * src_frame,
                                 src_row, row_bytes, H, hipMemcpyHostToDevice, S->st),
                "hipMemcpy2DAsync (map rows)");
        return rc ? nullptr : dst;
    }
    // the disparity maps and the optional dense confidence maps
    Maps maps(const void* disp, int disp_type, size_t stride, size_t fstride, int W, int H, int F, const float* conf) {
        const size_t es = disp_type == SDR_DISP_F32 ? 4 : 2;
        Maps m{};
        m.disp = rows(S->map, disp, (size_t)W * es, stride * es, fstride * es, H, F);
        m.conf = input(S->conf, conf, conf ? (size_t)F * W * H : 0);
        m.stride = (size_t)W;
        m.fstride = (size_t)W * H;
        return m;
    }
    // an input array in a buffer of the thread; null for an absent or empty one
    template <typename T>
    T* input(sdr::Buf& b, const T* host, size_t count) {
        if (!host || !count) return nullptr;
        T* d = (T*)room(b, count * sizeof(T));
        if (!rc) hip(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, S->st), "hipMemcpyAsync (input)");
        return rc ? nullptr : d;
    }
    // an array that goes in and comes back (the profile: the rows the kernel leaves untouched keep
    // the caller's values)
    template <typename T>
    T* inout(sdr::Buf& b, T* host, size_t count) {
        T* d = input(b, host, count);
        if (d) copy_back(host, b, 0, count * sizeof(T));
        return d;
    }
    // room for `count` records in S->out, which finish() copies to `host` (null: to nowhere)
    template <typename T>
    sdr::Slice<T> output(T* host, size_t count) {
        const sdr::Slice<T> s = outs.take<T>(count);
        copy_back(host, S->out, s.off, s.bytes());
        return s;
    }
    // after the last output(): S->out holds them all
    int ready() {
        room(S->out, outs.total);
        return rc;
    }
    template <typename T>
    T* at(const sdr::Slice<T>& s) const {
        return (T*)((char*)S->out.p + s.off);
    }
    // after the device form: the registered copies back, then one wait for the stream
    int finish() {
        for (int i = 0; i < nback && !rc; i++)
            hip(hipMemcpyAsync(back[i].host, (const char*)back[i].buf->p + back[i].off, back[i].bytes,
                               hipMemcpyDeviceToHost, S->st),
                "hipMemcpyAsync (output)");
        if (!rc) hip(hipStreamSynchronize(S->st), "hipStreamSynchronize");
        return rc;
    }
};

// The host-pointer form of an entry that measures regions against plane records (the relief, the
// footprint, the clearance): `check` is the entry's parameter guard, `entry` its device form.
template <typename Params, typename Query, typename Rec, typename Check, typename Entry>
inline int region_host_call(Check check, Entry entry, const void* disp, int disp_type, size_t stride,
                            size_t frame_stride, int W, int H, int F, const float* conf, const uint8_t* labels,
                            const double* Q, const Params* params, const sdr_plane* planes, int P,
                            const Query* queries, int K, Rec* out) {
    int rc = check_plane_maps(disp, disp_type, stride, frame_stride, W, H, F, Q, params, queries, K, out);
    if (rc || (rc = check(params, planes, P))) return rc;
    if (K == 0) return SDR_OK;
    HostCall c;
    const HostCall::Maps m = c.maps(disp, disp_type, stride, frame_stride, W, H, F, conf);
    const sdr_plane* d_planes = c.input(c.S->planes, planes, (size_t)P);
    const Query* d_queries = c.input(c.S->rows, queries, (size_t)K);
    const uint8_t* d_labels = c.input(c.S->labels, labels, (size_t)F * W * H);
    const auto s_out = c.output(out, (size_t)K);
    if ((rc = c.ready())) return rc;
    rc = entry(m.disp, disp_type, m.stride, m.fstride, W, H, F, m.conf, d_labels, Q, params, d_planes, P, d_queries,
               K, c.at(s_out), c.stream());
    return rc ? rc : c.finish();
}

}  // namespace ruler_host
}  // namespace sdr
