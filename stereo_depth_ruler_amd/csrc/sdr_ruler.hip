// sdr_ruler.hip -- the ruler: StereoDisplayer::onMouseMeasure (stereo_displayer.cpp:24-63) on the
// device, from the XYZ map as the reference does (k_ruler_xyz) or from the disparity map with a
// windowed lower median and a depth profile along the segment (k_ruler), and save_csvFile
// (:74-102) as text.  The definition is in include/sdr/sdr.h.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "sdr_device.hpp"
#include "sdr_internal.hpp"
#include "sdr_ruler_shared.hpp"

namespace sdr {

static_assert(sizeof(sdr_measurement) == 80, "sdr_measurement is 80 bytes");
static_assert(sizeof(sdr_ruler_params) == 24, "sdr_ruler_params is 24 bytes");
static_assert(sizeof(sdr_segment) == 20, "sdr_segment is 20 bytes");

// the profile's block: 8 waves a segment take its samples round-robin, a chunk of 512 samples at a
// time (the samples are independent, and a sample is a chain of dependent operations on its wave)
constexpr int kRulerThreads = 512;
constexpr int kRulerWaves = kRulerThreads / 64;
constexpr int kRulerEndThreads = 128;  // without the profile: one wave an endpoint

// cv::norm(Vec3f a - Vec3f b): the difference in float, the squares summed in double in order
__device__ __forceinline__ double ruler_distance(const float* a, const float* b) {
#pragma clang fp contract(off)
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float df = a[i] - b[i];
        const double v = (double)df;
        s += v * v;
    }
    return sqrt(s);
}

// x0 + rdiv(i * dx, m), rdiv(a, b) = floor((2a + b) / (2b)), for 0 <= i <= m, |dx| <= m, m >= 1:
// the numerator is shifted by 2m * m so that the division is unsigned
__device__ __forceinline__ int walk_coord(int c0, int dx, int i, int m) {
    if (m <= 32767) {  // 4 m^2 + m < 2^32: one 32-bit division
        const unsigned num = (unsigned)(2 * i * dx + m) + 2u * (unsigned)m * (unsigned)m;
        return c0 + (int)(num / (2u * (unsigned)m)) - m;
    }
    // unsigned throughout: i * dx fits 63 bits, and the sum, 4 m^2 + m at most, fits 64
    const unsigned long long um = (unsigned long long)m;
    const unsigned long long num = 2ull * (unsigned long long)((long long)i * dx) + um + 2ull * um * um;
    return c0 + (int)(num / (2ull * um)) - m;
}

__device__ __forceinline__ void write_measurement(sdr_measurement* o, const float* p0, const float* p1,
                                                  float d0, float d1, double dist, int n0, int n1,
                                                  int samples, int nvalid, int gap, float zmin,
                                                  float zmax, float dz, uint32_t flags) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        o->p0[i] = p0[i];
        o->p1[i] = p1[i];
    }
    o->d0 = d0;
    o->d1 = d1;
    o->distance = dist;
    o->n0 = n0;
    o->n1 = n1;
    o->path_samples = samples;
    o->path_valid = nvalid;
    o->max_gap = gap;
    o->z_min = zmin;
    o->z_max = zmax;
    o->max_dz = dz;
    o->flags = flags;
    o->reserved = 0;
}

__device__ __forceinline__ void write_out_of_range(sdr_measurement* o) {
    const float q = ruler_nan();
    const float p[3] = {q, q, q};
    write_measurement(o, p, p, q, q, __builtin_nan(""), 0, 0, 0, 0, 0, q, q, q, SDR_MEAS_OUT_OF_RANGE);
}

// inclusive maximum scan over the wave's lanes
__device__ __forceinline__ int wave_scan_max(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v = max(v, t);
    }
    return v;
}

struct RulerShared {
    float z[kRulerThreads];    // Z of the chunk's samples
    int ok[kRulerThreads];     // their validity
    int wmax[kRulerWaves];     // last valid local index of each wave's lanes (-1: none)
    float ep[2][4];            // the endpoints' {X, Y, Z, d}
    int epn[2], epok[2];
    int carry_idx;             // last valid sample before the chunk (-1: none) and its Z
    float carry_z;
    int red_i[kRulerWaves][2];
    float red_f[kRulerWaves][3];
};

template <typename T>
__global__ __launch_bounds__(kRulerThreads) void k_ruler(RegionMaps<T> maps, Q16 Q, sdr_ruler_params P,
                                                         const sdr_segment* __restrict__ segs,
                                                         sdr_measurement* __restrict__ out,
                                                         float* __restrict__ profile) {
    __shared__ RulerShared sh;
    const int k = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const sdr_segment sg = segs[k];
    if (!maps.holds(sg)) {  // block-uniform
        if (tid == 0) write_out_of_range(out + k);
        return;
    }
    const FrameMaps<T> fm = maps.frame(sg.frame);
    const int dx = sg.x1 - sg.x0, dy = sg.y1 - sg.y0;
    const int m = max(abs(dx), abs(dy)), n = m + 1;
    float* prow = (P.profile && profile) ? profile + (size_t)k * P.profile_cap * 4 : nullptr;

    // sample i by the calling wave: the endpoint slots, and with the profile its chunk slot and row
    auto process = [&](int i, int slot) {
        const int x = m ? walk_coord(sg.x0, dx, i, m) : sg.x0;
        const int y = m ? walk_coord(sg.y0, dy, i, m) : sg.y0;
        const RulerSample s = ruler_sample(fm, Q, P, x, y, lane);
        if (lane == 0) {
            if (i == 0 || i == m) {
                const int e0 = i == 0 ? 0 : 1, e1 = i == m ? 1 : 0;  // n == 1: both
                for (int e = e0; e <= e1; e++) {
                    sh.ep[e][0] = s.xyz[0];
                    sh.ep[e][1] = s.xyz[1];
                    sh.ep[e][2] = s.xyz[2];
                    sh.ep[e][3] = s.d;
                    sh.epn[e] = s.n;
                    sh.epok[e] = s.valid;
                }
            }
            if (slot >= 0) {
                sh.z[slot] = s.xyz[2];
                sh.ok[slot] = s.valid;
            }
            if (prow && i < P.profile_cap) {
                const float q = ruler_nan();
                float* o = prow + (size_t)i * 4;
                o[0] = s.valid ? s.xyz[0] : q;
                o[1] = s.valid ? s.xyz[1] : q;
                o[2] = s.valid ? s.xyz[2] : q;
                o[3] = s.valid ? s.d : q;
            }
        }
    };

    int nvalid = 0, gap = 0;
    float zmin = INFINITY, zmax = -INFINITY, dz = -1.f;
    if (!P.profile) {
        if (wave == 0) process(0, -1);
        if (wave == 1 && m > 0) process(m, -1);
        __syncthreads();
    } else {
        if (tid == 0) {
            sh.carry_idx = -1;
            sh.carry_z = 0.f;
        }
        for (int base = 0; base < n; base += kRulerThreads) {
            const int here = min(n - base, kRulerThreads);
            for (int t = wave; t < here; t += kRulerWaves) process(base + t, t);
            __syncthreads();
            // the previous valid sample of each sample of the chunk: a maximum scan of the valid
            // local indices, exclusive of the sample itself
            const bool mine = tid < here && sh.ok[tid];
            const int incl = wave_scan_max(mine ? tid : -1, lane);
            if (lane == 63) sh.wmax[wave] = incl;
            __syncthreads();
            int prev = __shfl_up(incl, 1, 64);
            if (lane == 0) prev = -1;
            for (int w = 0; w < wave; w++) prev = max(prev, sh.wmax[w]);
            const int cidx = sh.carry_idx;
            const float cz = sh.carry_z;
            if (mine) {
                const float z = sh.z[tid];
                const int pidx = prev >= 0 ? base + prev : cidx;
                const float pz = prev >= 0 ? sh.z[prev] : cz;
                nvalid++;
                zmin = fminf(zmin, z);
                zmax = fmaxf(zmax, z);
                gap = max(gap, base + tid - pidx - 1);
                if (pidx >= 0) dz = fmaxf(dz, fabsf(z - pz));
            }
            __syncthreads();
            if (tid == 0) {
                int last = -1;
                for (int w = 0; w < kRulerWaves; w++) last = max(last, sh.wmax[w]);
                if (last >= 0) {
                    sh.carry_idx = base + last;
                    sh.carry_z = sh.z[last];
                }
            }
            __syncthreads();
        }
        // minima, maxima and counts only: the result does not depend on the order of the waves
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            nvalid += __shfl_xor(nvalid, o, 64);
            gap = max(gap, __shfl_xor(gap, o, 64));
            zmin = fminf(zmin, __shfl_xor(zmin, o, 64));
            zmax = fmaxf(zmax, __shfl_xor(zmax, o, 64));
            dz = fmaxf(dz, __shfl_xor(dz, o, 64));
        }
        if (lane == 0) {
            sh.red_i[wave][0] = nvalid;
            sh.red_i[wave][1] = gap;
            sh.red_f[wave][0] = zmin;
            sh.red_f[wave][1] = zmax;
            sh.red_f[wave][2] = dz;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const float q = ruler_nan();
    int samples = 0;
    float zmn = q, zmx = q, mdz = q;
    nvalid = 0;
    gap = 0;
    if (P.profile) {
        zmin = INFINITY, zmax = -INFINITY, dz = -1.f;
        for (int w = 0; w < kRulerWaves; w++) {
            nvalid += sh.red_i[w][0];
            gap = max(gap, sh.red_i[w][1]);
            zmin = fminf(zmin, sh.red_f[w][0]);
            zmax = fmaxf(zmax, sh.red_f[w][1]);
            dz = fmaxf(dz, sh.red_f[w][2]);
        }
        samples = n;
        gap = max(gap, n - 1 - sh.carry_idx);  // the invalid run at the end (all of it: n)
        if (nvalid >= 1) {
            zmn = zmin;
            zmx = zmax;
        }
        if (nvalid >= 2) mdz = dz;
    }
    const bool v0 = sh.epok[0], v1 = sh.epok[1];
    uint32_t flags = (v0 ? SDR_MEAS_P0_VALID : 0) | (v1 ? SDR_MEAS_P1_VALID : 0);
    if (prow && n > P.profile_cap) flags |= SDR_MEAS_PROFILE_TRUNCATED;
    const double dist = (v0 && v1) ? canon(ruler_distance(sh.ep[0], sh.ep[1])) : __builtin_nan("");
    const float e0[3] = {canon(sh.ep[0][0]), canon(sh.ep[0][1]), canon(sh.ep[0][2])};
    const float e1[3] = {canon(sh.ep[1][0]), canon(sh.ep[1][1]), canon(sh.ep[1][2])};
    write_measurement(out + k, e0, e1, sh.ep[0][3], sh.ep[1][3], dist, sh.epn[0], sh.epn[1],
                      samples, nvalid, gap, zmn, zmx, mdz, flags);
}

// The reference's measurement: the XYZ map's values at the two pixels, one lane a segment.
__global__ __launch_bounds__(256) void k_ruler_xyz(const float* __restrict__ xyz, size_t stride,
                                                   size_t fstride, int W, int H, int F,
                                                   const sdr_segment* __restrict__ segs, int K,
                                                   sdr_measurement* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const sdr_segment sg = segs[k];
    if (!segment_in_range(sg, W, H, F)) {
        write_out_of_range(out + k);
        return;
    }
    const float* f = xyz + (size_t)sg.frame * fstride;
    const float* a = f + (size_t)sg.y0 * stride + 3 * (size_t)sg.x0;
    const float* b = f + (size_t)sg.y1 * stride + 3 * (size_t)sg.x1;
    const float p0[3] = {a[0], a[1], a[2]}, p1[3] = {b[0], b[1], b[2]};
    const float q = ruler_nan();
    const uint32_t flags = (finite3(p0) ? SDR_MEAS_P0_VALID : 0) | (finite3(p1) ? SDR_MEAS_P1_VALID : 0);
    write_measurement(out + k, p0, p1, q, q, canon(ruler_distance(p0, p1)), 1, 1, 0, 0, 0, q, q, q, flags);
}

}  // namespace sdr

namespace {

using namespace sdr::ruler_host;

// argument guards of the disparity mode (host only)
int check_disp_args(const void* disp, int disp_type, size_t stride, size_t fstride, int W, int H, int F,
                    const double* Q, const sdr_ruler_params* p, const void* segs, int K, const void* out,
                    const void* profile) {
    if (!disp || !Q || !p) return rfail(SDR_ERR_ARG, "null argument");
    if (K < 0) return rfail(SDR_ERR_ARG, "negative segment count");
    if (K > 0 && (!segs || !out)) return rfail(SDR_ERR_ARG, "null argument");
    if (W <= 0 || H <= 0 || F <= 0) return rfail(SDR_ERR_ARG, "bad size");
    if (stride < (size_t)W || fstride < stride * (size_t)(H - 1) + (size_t)W)
        return rfail(SDR_ERR_ARG, "bad stride");
    if (p->radius < 0 || p->radius > 4) return rfail(SDR_ERR_ARG, "radius must be in 0..4");
    if (p->min_count < 1) return rfail(SDR_ERR_ARG, "min_count must be >= 1");
    if (p->profile != 0 && p->profile != 1) return rfail(SDR_ERR_ARG, "profile must be 0 or 1");
    if (profile && p->profile_cap < 0) return rfail(SDR_ERR_ARG, "negative profile_cap");
    if (disp_type != SDR_DISP_F32 && disp_type != SDR_DISP_S16)
        return rfail(SDR_ERR_TYPE, "disp_type must be SDR_DISP_F32 or SDR_DISP_S16");
    return SDR_OK;
}

int check_xyz_args(const void* xyz, size_t stride, size_t fstride, int W, int H, int F, const void* segs,
                   int K, const void* out) {
    if (!xyz) return rfail(SDR_ERR_ARG, "null argument");
    if (K < 0) return rfail(SDR_ERR_ARG, "negative segment count");
    if (K > 0 && (!segs || !out)) return rfail(SDR_ERR_ARG, "null argument");
    if (W <= 0 || H <= 0 || F <= 0) return rfail(SDR_ERR_ARG, "bad size");
    if (stride < (size_t)W * 3 || fstride < stride * (size_t)(H - 1) + (size_t)W * 3)
        return rfail(SDR_ERR_ARG, "bad stride");
    return SDR_OK;
}

}  // namespace

extern "C" {

void sdr_ruler_params_default(sdr_ruler_params* p) {
    if (!p) return;
    p->radius = 0;
    p->min_count = 1;
    p->min_disp = -1.0f;
    p->conf_min = 0.0f;
    p->profile = 0;
    p->profile_cap = 0;
}

int sdr_measure_disp_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride,
                            int W, int H, int F, const float* d_conf, const double Q[16],
                            const sdr_ruler_params* params, const sdr_segment* d_segs, int K,
                            sdr_measurement* d_out, float* d_profile, void* stream) {
    const int rc = check_disp_args(d_disp, disp_type, stride, frame_stride, W, H, F, Q, params, d_segs, K,
                                   d_out, d_profile);
    if (rc) return rc;
    if (K == 0) return SDR_OK;
    if (params->profile_cap == 0) d_profile = nullptr;  // no rows: not a profile buffer (sdr.h)
    const sdr::Q16 q = make_q16(Q);
    const dim3 grid((unsigned)K), block(params->profile ? sdr::kRulerThreads : sdr::kRulerEndThreads);
    with_maps(d_disp, disp_type, stride, frame_stride, W, H, F, d_conf, nullptr, [&](auto maps) {
        hipLaunchKernelGGL(sdr::k_ruler<disp_elem_t<decltype(maps)>>, grid, block, 0, (hipStream_t)stream, maps, q,
                           *params, d_segs, d_out, d_profile);
    });
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

int sdr_measure_xyz_device(const float* d_xyz, size_t xyz_stride, size_t xyz_frame_stride, int W, int H,
                           int F, const sdr_segment* d_segs, int K, sdr_measurement* d_out,
                           void* stream) {
    const int rc = check_xyz_args(d_xyz, xyz_stride, xyz_frame_stride, W, H, F, d_segs, K, d_out);
    if (rc) return rc;
    if (K == 0) return SDR_OK;
    hipLaunchKernelGGL(sdr::k_ruler_xyz, dim3((unsigned)((K + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, d_xyz, xyz_stride, xyz_frame_stride, W, H, F, d_segs, K, d_out);
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

int sdr_measure_disp(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H,
                     int F, const float* conf, const double Q[16], const sdr_ruler_params* params,
                     const sdr_segment* segs, int K, sdr_measurement* out, float* profile) {
    int rc = check_disp_args(disp, disp_type, stride, frame_stride, W, H, F, Q, params, segs, K, out, profile);
    if (rc) return rc;
    if (K == 0) return SDR_OK;
    HostCall c;
    const HostCall::Maps m = c.maps(disp, disp_type, stride, frame_stride, W, H, F, conf);
    const sdr_segment* d_segs = c.input(c.S->rows, segs, (size_t)K);
    // the profile rows, 4 floats each, when the call writes any
    const bool prof = params->profile && params->profile_cap > 0;
    float* d_profile = c.inout(c.S->prof, prof ? profile : nullptr, (size_t)K * params->profile_cap * 4);
    const auto s_out = c.output(out, (size_t)K);
    if ((rc = c.ready())) return rc;
    rc = sdr_measure_disp_device(m.disp, disp_type, m.stride, m.fstride, W, H, F, m.conf, Q, params, d_segs, K,
                                 c.at(s_out), d_profile, c.stream());
    return rc ? rc : c.finish();
}

int sdr_measure_xyz(const float* xyz, size_t xyz_stride, size_t xyz_frame_stride, int W, int H, int F,
                    const sdr_segment* segs, int K, sdr_measurement* out) {
    int rc = check_xyz_args(xyz, xyz_stride, xyz_frame_stride, W, H, F, segs, K, out);
    if (rc) return rc;
    if (K == 0) return SDR_OK;
    HostCall c;
    const float* d_xyz = (const float*)c.rows(c.S->map, xyz, (size_t)W * 12, xyz_stride * 4, xyz_frame_stride * 4, H, F);
    const sdr_segment* d_segs = c.input(c.S->rows, segs, (size_t)K);
    const auto s_out = c.output(out, (size_t)K);
    if ((rc = c.ready())) return rc;
    rc = sdr_measure_xyz_device(d_xyz, (size_t)W * 3, (size_t)W * H * 3, W, H, F, d_segs, K, c.at(s_out), c.stream());
    return rc ? rc : c.finish();
}

int sdr_measurements_csv(const int* image_index, const sdr_segment* segs, const sdr_measurement* records,
                         int n, int with_header, char* buf, size_t cap) {
    if (n < 0 || (n > 0 && (!image_index || !segs || !records))) return rfail(SDR_ERR_ARG, "bad arguments");
    // operator<<: std::right and setw(4) land on "  Second_point, " and "Distance\n" (longer than 4:
    // no padding), and in a row on cv::Point's "[" (three spaces) and on "\n" (three spaces)
    std::string s;
    if (with_header) s += "Image, First_point,   Second_point, Distance\n";
    char line[160];
    for (int i = 0; i < n; i++) {
        snprintf(line, sizeof line, "%d, [%d, %d],    [%d, %d], %.5f cm   \n", image_index[i], segs[i].x0,
                 segs[i].y0, segs[i].x1, segs[i].y1, records[i].distance / 10);
        s += line;
    }
    if (s.size() > (size_t)INT32_MAX) return rfail(SDR_ERR_SIZE, "text longer than INT_MAX");
    if (buf) {
        if (cap < s.size() + 1) return rfail(SDR_ERR_ARG, "buffer too small");
        memcpy(buf, s.c_str(), s.size() + 1);
    }
    return (int)s.size();
}

}  // extern "C"
