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

struct RulerSample {
    float xyz[3];
    float d;
    int n;
    bool valid;
};

// One sample by one wave (every lane returns the same values): the window's <= 81 values two a
// lane, the valid mask as two ballots, the lower median by counting, for each lane's values, the
// valid values that sort before them (ties by window index), then the reprojection.
template <typename T>
__device__ __forceinline__ RulerSample ruler_sample(const T* __restrict__ disp, size_t stride,
                                                    const float* __restrict__ conf, int W, int H,
                                                    const Q16& Q, const sdr_ruler_params& P, int x,
                                                    int y, int lane) {
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
    const unsigned long long m0 = __ballot(ok[0]), m1 = __ballot(ok[1]);
    RulerSample s;
    s.n = __popcll(m0) + __popcll(m1);
    s.d = s.xyz[0] = s.xyz[1] = s.xyz[2] = ruler_nan();
    s.valid = false;
    if (s.n < P.min_count || s.n == 0) return s;
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
    const int want = (s.n - 1) >> 1;
    const unsigned long long h0 = __ballot(ok[0] && rank[0] == want);
    const unsigned long long h1 = __ballot(ok[1] && rank[1] == want);
    // exactly one valid value has rank `want`
    const float dmed = h0 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[0]), __builtin_ctzll(h0)))
                          : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[1]), __builtin_ctzll(h1 | (1ull << 63))));
    s.d = dmed;
    reproject_px(Q, x, y, (double)dmed, 0.0, 0, s.xyz);
    s.valid = finite3(s.xyz);
    return s;
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
__global__ __launch_bounds__(kRulerThreads) void k_ruler(const T* __restrict__ disp, size_t stride,
                                                         size_t fstride, int W, int H, int F,
                                                         const float* __restrict__ conf, Q16 Q,
                                                         sdr_ruler_params P,
                                                         const sdr_segment* __restrict__ segs,
                                                         sdr_measurement* __restrict__ out,
                                                         float* __restrict__ profile) {
    __shared__ RulerShared sh;
    const int k = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const sdr_segment sg = segs[k];
    if (!segment_in_range(sg, W, H, F)) {  // block-uniform
        if (tid == 0) write_out_of_range(out + k);
        return;
    }
    const T* fd = disp + (size_t)sg.frame * fstride;
    const float* fc = conf ? conf + (size_t)sg.frame * W * H : nullptr;
    const int dx = sg.x1 - sg.x0, dy = sg.y1 - sg.y0;
    const int m = max(abs(dx), abs(dy)), n = m + 1;
    float* prow = (P.profile && profile) ? profile + (size_t)k * P.profile_cap * 4 : nullptr;

    // sample i by the calling wave: the endpoint slots, and with the profile its chunk slot and row
    auto process = [&](int i, int slot) {
        const int x = m ? walk_coord(sg.x0, dx, i, m) : sg.x0;
        const int y = m ? walk_coord(sg.y0, dy, i, m) : sg.y0;
        const RulerSample s = ruler_sample(fd, stride, fc, W, H, Q, P, x, y, lane);
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

// ---- the plane fit (the definition: sdr.h, "the ruler against a surface") ----
static_assert(sizeof(sdr_plane_params) == 32, "sdr_plane_params is 32 bytes");
static_assert(sizeof(sdr_plane) == 128, "sdr_plane is 128 bytes");
static_assert(sizeof(sdr_plane_query) == 16, "sdr_plane_query is 16 bytes");
static_assert(sizeof(struct sdr_plane_distance) == 32, "sdr_plane_distance is 32 bytes");

// A region is cut into slices of kPlaneSlice pixels of its row-major order, a workgroup a slice.
// The sums are integers, so neither the slice size nor the order the workgroups finish in shows
// in the result.
constexpr int kPlaneThreads = 256;
constexpr int kPlaneWaves = kPlaneThreads / 64;
constexpr int kPlanePix = 8;  // pixels a thread
constexpr int kPlaneSlice = kPlaneThreads * kPlanePix;
// accumulators of a region: [iterations + 2 sweeps][kPlaneSlots] int64.  Sweeps 0..iterations hold
// the nine moments of their fit's pixel set {n, Su, Sv, Sq, Suu, Suv, Svv, Suq, Svq}, the last
// sweep {n_inliers, See, the bits of max |r|}
constexpr int kPlaneSlots = 16;
constexpr int kPlaneMoments = 9;

struct PlaneFit {
    double a, b, c;  // in 1/16 px
    bool ok;
};

// The solve of sdr.h from a set's moments.  Every workgroup of a sweep and the record writer
// repeat it from the same integers: the same bits everywhere.
__device__ __forceinline__ PlaneFit plane_solve(const long long* __restrict__ m, int min_inliers) {
#pragma clang fp contract(off)
    const long long n = m[0];
    const double N = (double)n, su = (double)m[1], sv = (double)m[2], sq = (double)m[3];
    const double cuu = N * (double)m[4] - su * su;
    const double cuv = N * (double)m[5] - su * sv;
    const double cvv = N * (double)m[6] - sv * sv;
    const double cuq = N * (double)m[7] - su * sq;
    const double cvq = N * (double)m[8] - sv * sq;
    const double det = cuu * cvv - cuv * cuv;
    PlaneFit f;
    f.a = (cuq * cvv - cvq * cuv) / det;
    f.b = (cvq * cuu - cuq * cuv) / det;
    f.c = ((sq - f.a * su) - f.b * sv) / N;
    f.ok = n >= (long long)min_inliers && det > 0.0 && isfinite(f.a) && isfinite(f.b) && isfinite(f.c);
    return f;
}

__device__ __forceinline__ double plane_at(const PlaneFit& f, double u, double v) {
#pragma clang fp contract(off)
    return (f.a * u + f.b * v) + f.c;
}

// the valid pixel's value on the 1/16 px grid
__device__ __forceinline__ bool plane_q(const float* p, float min_disp, int* q) {
    const float d = *p;
    *q = (int)rint((double)d * 16.0);
    return isfinite(d) && d > min_disp && fabsf(d) < 2048.f;
}
__device__ __forceinline__ bool plane_q(const int16_t* p, float min_disp, int* q) {
    const int v = *p;
    *q = v;
    return (float)v * 0.0625f > min_disp;
}

// The plane search's state (sdr_find_planes*), written by its one-workgroup kernels and read by the
// kernels behind them on the stream.
struct SearchState {
    int stopped;      // a round has stopped the search (or the region is out of range)
    int winner;       // the round's winning hypothesis
    int score, voids;
    double a, b, c;   // its seed plane, in 1/16 px
};
constexpr uint8_t kFreeLabel = 255;

// One sweep over the regions' pixels: grid (slices of a W x H frame, regions).  Sweep 0 sums the
// moments of the valid pixels, sweep s = 1..iterations those of the pixels within the scheduled
// band of fit s - 1, sweep iterations + 1 the statistics against the last fit.  A region that is
// out of range, a slice past its area and a chain that a degenerate fit has stopped leave at once
// (block-uniform); no workgroup waits on another.
//
// kSearch (sdr_find_planes*): one region, `acc` its round's accumulators, the sweeps 1..iterations + 1
// only; a pixel counts only while it is free (its label 255), sweep 1's previous plane is the
// round's seed plane, and a stopped search leaves at once.  The sums and the residual are the
// same code either way.
template <typename T, bool kSearch>
__global__ __launch_bounds__(kPlaneThreads) void k_plane_sweep(const T* __restrict__ disp, size_t stride,
                                                               size_t fstride, int W, int H, int F,
                                                               const float* __restrict__ conf,
                                                               sdr_plane_params P,
                                                               const sdr_segment* __restrict__ regs,
                                                               long long* __restrict__ acc, int sweep,
                                                               const uint8_t* __restrict__ labels,
                                                               const SearchState* __restrict__ state) {
#pragma clang fp contract(off)
    __shared__ long long red[kPlaneWaves][kPlaneMoments];
    const int k = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (kSearch && state->stopped) return;  // block-uniform
    const sdr_segment sg = regs[k];
    if (!segment_in_range(sg, W, H, F)) return;
    const PlaneRect R = plane_rect(sg);
    const unsigned area = (unsigned)R.rw * (unsigned)R.rh;  // <= W * H <= 2^24
    const unsigned base = blockIdx.x * (unsigned)kPlaneSlice;
    if (base >= area) return;
    long long* A = acc + (size_t)k * (size_t)(P.iterations + 2) * kPlaneSlots;
    const bool last = sweep == P.iterations + 1;
    PlaneFit fit = {0.0, 0.0, 0.0, true};
    double band = 0.0;
    if (sweep > 0) {
        if (kSearch && sweep == 1)
            fit = PlaneFit{state->a, state->b, state->c, true};
        else
            fit = plane_solve(A + (size_t)(sweep - 1) * kPlaneSlots, P.min_inliers);
        if (!fit.ok) return;  // the chain has stopped: the later sweeps' accumulators stay 0
        band = (double)P.inlier_px * 16.0 * (double)(1 << (last ? 0 : P.iterations - sweep));
    }
    const T* fd = disp + (size_t)sg.frame * fstride + (size_t)R.ys * stride + (size_t)R.xs;
    const float* fc = conf ? conf + ((size_t)sg.frame * H + (size_t)R.ys) * W + (size_t)R.xs : nullptr;
    const uint8_t* fl = kSearch ? labels + (size_t)R.ys * W + (size_t)R.xs : nullptr;

    long long m[kPlaneMoments];
#pragma unroll
    for (int i = 0; i < kPlaneMoments; i++) m[i] = 0;
    double rmax = 0.0;
#pragma unroll
    for (int j = 0; j < kPlanePix; j++) {
        const unsigned p = base + (unsigned)(j * kPlaneThreads + tid);
        if (p >= area) continue;
        const unsigned v = p / (unsigned)R.rw, u = p - v * (unsigned)R.rw;
        int q;
        bool ok = plane_q(fd + (size_t)v * stride + u, P.min_disp, &q);
        if (fc) ok = ok && fc[(size_t)v * W + u] >= P.conf_min;
        if (kSearch) ok = ok && fl[(size_t)v * W + u] == kFreeLabel;
        double r = 0.0;
        if (sweep > 0) {
            r = (double)q - plane_at(fit, (double)u, (double)v);
            ok = ok && fabs(r) <= band;
        }
        if (!ok) continue;
        if (last) {
            const long long e = llrint(r * 16.0);
            m[0] += 1;
            m[1] += e * e;
            rmax = fmax(rmax, fabs(r));
        } else {
            const long long lu = u, lv = v, lq = q;
            m[0] += 1;
            m[1] += lu;
            m[2] += lv;
            m[3] += lq;
            m[4] += lu * lu;
            m[5] += lu * lv;
            m[6] += lv * lv;
            m[7] += lu * lq;
            m[8] += lv * lq;
        }
    }
    // wave butterflies, then the waves' sums through LDS; a maximum of non-negative doubles is
    // the maximum of their bits
    const int nsum = last ? 2 : kPlaneMoments;
#pragma unroll
    for (int i = 0; i < kPlaneMoments; i++) {
        if (i < nsum) {  // block-uniform
            const long long s = wave_sum(m[i]);
            if (lane == 0) red[wave][i] = s;
        }
    }
    if (last) {
        long long b = __double_as_longlong(rmax);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) b = max(b, __shfl_xor(b, o, 64));
        if (lane == 0) red[wave][2] = b;
    }
    __syncthreads();
    long long* dst = A + (size_t)sweep * kPlaneSlots;
    if (tid < nsum) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < kPlaneWaves; w++) s += red[w][tid];
        if (s) atomicAdd((unsigned long long*)dst + tid, (unsigned long long)s);
    } else if (last && tid == 2) {
        long long b = 0;
#pragma unroll
        for (int w = 0; w < kPlaneWaves; w++) b = max(b, red[w][2]);
        if (b) atomicMax((unsigned long long*)dst + 2, (unsigned long long)b);
    }
}

// reprojectImageTo3D's row sums at a real-valued pixel, the point kept in double
__device__ __forceinline__ void plane_reproject(const Q16& Q, double x, double y, double d, double* o) {
#pragma clang fp contract(off)
    double h[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double s = 0.0;
        s += Q.q[i * 4 + 0] * x;
        s += Q.q[i * 4 + 1] * y;
        s += Q.q[i * 4 + 2] * d;
        s += Q.q[i * 4 + 3] * 1.0;
        h[i] = s;
    }
    o[0] = h[0] / h[3];
    o[1] = h[1] / h[3];
    o[2] = h[2] / h[3];
}

// The statistics, coefficients and 3-D plane of a record from the last fit, its moment set M and
// the statistics sweep's sums L = {n_inliers, See, the bits of max |r|}; o.flags becomes
// SDR_PLANE_OK or SDR_PLANE_NONFINITE.
__device__ __forceinline__ void plane_record(sdr_plane& o, const PlaneRect& R, const PlaneFit& fit,
                                             const long long* __restrict__ M,
                                             const long long* __restrict__ L, const Q16& Q) {
#pragma clang fp contract(off)
    o.n_inliers = (int)L[0];
    if (L[0] > 0) {
        o.rms_px = canon(sqrt((double)L[1] / (double)L[0]) / 256.0);
        o.max_abs_px = (float)(__longlong_as_double(L[2]) / 16.0);
    }
    o.coef[0] = fit.a * 0.0625;
    o.coef[1] = fit.b * 0.0625;
    o.coef[2] = fit.c * 0.0625;
    const double ue = (double)(R.rw - 1), ve = (double)(R.rh - 1);
    const double xs = (double)R.xs, ys = (double)R.ys;
    double p0[3], p1[3], p2[3], ce[3];
    plane_reproject(Q, xs, ys, plane_at(fit, 0.0, 0.0) * 0.0625, p0);
    plane_reproject(Q, (double)(R.xs + R.rw - 1), ys, plane_at(fit, ue, 0.0) * 0.0625, p1);
    plane_reproject(Q, xs, (double)(R.ys + R.rh - 1), plane_at(fit, 0.0, ve) * 0.0625, p2);
    const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    const double mx = e1y * e2z - e1z * e2y;
    const double my = e1z * e2x - e1x * e2z;
    const double mz = e1x * e2y - e1y * e2x;
    const double len = sqrt((mx * mx + my * my) + mz * mz);
    double nx = mx / len, ny = my / len, nz = mz / len;
    double off = -((nx * p0[0] + ny * p0[1]) + nz * p0[2]);
    if (off < 0.0) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
        off = -off;
    }
    const double N = (double)M[0];
    const double cu = (double)M[1] / N, cv = (double)M[2] / N;
    plane_reproject(Q, xs + cu, ys + cv, plane_at(fit, cu, cv) * 0.0625, ce);
    if (isfinite(nx) && isfinite(ny) && isfinite(nz) && isfinite(off) && isfinite(ce[0]) && isfinite(ce[1]) &&
        isfinite(ce[2])) {
        o.normal[0] = nx;
        o.normal[1] = ny;
        o.normal[2] = nz;
        o.offset = off;
        for (int i = 0; i < 3; i++) o.centroid[i] = ce[i];
        o.flags = SDR_PLANE_OK;
    } else {
        o.flags = SDR_PLANE_NONFINITE;
    }
}

// The records, one lane a region, from the accumulators the sweeps have left.
__global__ __launch_bounds__(64) void k_plane_finish(const sdr_segment* __restrict__ regs, int K, int W,
                                                     int H, int F, Q16 Q, sdr_plane_params P,
                                                     const long long* __restrict__ acc,
                                                     sdr_plane* __restrict__ out) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    const sdr_segment sg = regs[k];
    const double qn = __builtin_nan("");
    sdr_plane o;
    for (int i = 0; i < 3; i++) o.coef[i] = o.normal[i] = o.centroid[i] = qn;
    o.offset = o.rms_px = qn;
    o.max_abs_px = ruler_nan();
    o.x0 = min(sg.x0, sg.x1);
    o.y0 = min(sg.y0, sg.y1);
    o.frame = sg.frame;
    o.area = o.n_valid = o.n_inliers = o.fits = 0;
    o.flags = SDR_PLANE_OUT_OF_RANGE;
    o.reserved = 0;
    if (!segment_in_range(sg, W, H, F)) {
        out[k] = o;
        return;
    }
    const PlaneRect R = plane_rect(sg);
    const long long* A = acc + (size_t)k * (size_t)(P.iterations + 2) * kPlaneSlots;
    o.area = R.rw * R.rh;
    o.n_valid = (int)A[0];
    PlaneFit fit = {0.0, 0.0, 0.0, false};
    const long long* M = A;
    for (int s = 0; s <= P.iterations; s++) {
        M = A + (size_t)s * kPlaneSlots;
        fit = plane_solve(M, P.min_inliers);
        if (!fit.ok) break;
        o.fits++;
    }
    if (!fit.ok) {
        o.flags = SDR_PLANE_DEGENERATE;
        out[k] = o;
        return;
    }
    plane_record(o, R, fit, M, A + (size_t)(P.iterations + 1) * kPlaneSlots, Q);
    out[k] = o;
}

// ---- the plane search (the definition: sdr.h, "the dominant planes of a region") ----
static_assert(sizeof(sdr_plane_search_params) == 64, "sdr_plane_search_params is 64 bytes");
static_assert(sizeof(sdr_plane_search_round) == 16, "sdr_plane_search_round is 16 bytes");
static_assert(sizeof(SearchState) == 40, "SearchState is 40 bytes");

// A hypothesis: the plane A*u + B*v + C*q = D through its three points; C == 0: void.
struct SearchHyp {
    int A, B, C, pad;
    long long D;
    long long pad2;
};
static_assert(sizeof(SearchHyp) == 32, "SearchHyp is 32 bytes");

constexpr int kSearchTries = 16;
constexpr int kSearchChunk = 64;  // hypotheses a workgroup of the score kernel (grid y)

__device__ __forceinline__ uint32_t search_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// the record of a round that did not run, or of a region out of range (flags)
__device__ __forceinline__ void search_empty_record(sdr_plane* o, const sdr_segment& sg, int area, uint32_t flags) {
    const double qn = __builtin_nan("");
    for (int i = 0; i < 3; i++) o->coef[i] = o->normal[i] = o->centroid[i] = qn;
    o->offset = o->rms_px = qn;
    o->max_abs_px = ruler_nan();
    o->x0 = min(sg.x0, sg.x1);
    o->y0 = min(sg.y0, sg.y1);
    o->frame = sg.frame;
    o->area = area;
    o->n_valid = o->n_inliers = o->fits = 0;
    o->flags = flags;
    o->reserved = 0;
}

__device__ __forceinline__ void search_round(sdr_plane_search_round* rounds, int r, int h, int score, int voids,
                                             uint32_t stop) {
    if (!rounds) return;
    rounds[r].hypothesis = h;
    rounds[r].score = score;
    rounds[r].voids = voids;
    rounds[r].stop = stop;
}

// One thread stops the search in round r: the count, the records r.., the rounds r..
__device__ __forceinline__ void search_stop(SearchState* st, const sdr_segment& sg, int area, int r, int max_planes,
                                            int h, int score, int voids, uint32_t code, uint32_t rec_flags,
                                            sdr_plane* planes, int32_t* count, sdr_plane_search_round* rounds) {
    st->stopped = 1;
    *count = r;
    for (int i = r; i < max_planes; i++) {
        search_empty_record(planes + i, sg, area, rec_flags);
        if (i == r && code != SDR_SEARCH_NOT_RUN)
            search_round(rounds, i, h, score, voids, code);
        else
            search_round(rounds, i, -1, 0, 0, SDR_SEARCH_NOT_RUN);
    }
}

// Before round 0: a region out of range stops the search with its records.
__global__ __launch_bounds__(64) void k_search_init(const sdr_segment* __restrict__ reg, int W, int H, int F,
                                                    int max_planes, SearchState* __restrict__ st,
                                                    sdr_plane* __restrict__ planes, int32_t* __restrict__ count,
                                                    sdr_plane_search_round* __restrict__ rounds) {
    if (threadIdx.x != 0) return;
    const sdr_segment sg = reg[0];
    *count = 0;
    if (!segment_in_range(sg, W, H, F))
        search_stop(st, sg, 0, 0, max_planes, -1, 0, 0, SDR_SEARCH_NOT_RUN, SDR_PLANE_OUT_OF_RANGE, planes, count,
                    rounds);
}

// The draws of round r, a thread a hypothesis.
template <typename T>
__global__ __launch_bounds__(64) void k_search_draw(const T* __restrict__ disp, size_t stride, size_t fstride, int W,
                                                    int H, int F, const float* __restrict__ conf,
                                                    sdr_plane_params P, const sdr_segment* __restrict__ reg,
                                                    const uint8_t* __restrict__ labels, int r, int M, uint32_t seed,
                                                    const SearchState* __restrict__ st,
                                                    SearchHyp* __restrict__ hyp) {
    if (st->stopped) return;
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= M) return;
    const sdr_segment sg = reg[0];
    const PlaneRect R = plane_rect(sg);  // in range: k_search_init
    const unsigned area = (unsigned)R.rw * (unsigned)R.rh;
    const T* fd = disp + (size_t)sg.frame * fstride + (size_t)R.ys * stride + (size_t)R.xs;
    const float* fc = conf ? conf + ((size_t)sg.frame * H + (size_t)R.ys) * W + (size_t)R.xs : nullptr;
    const uint8_t* fl = labels + (size_t)R.ys * W + (size_t)R.xs;
    const uint32_t key = search_mix(search_mix(seed ^ (0x9E3779B9u * (uint32_t)(r + 1))) ^ (uint32_t)h);
    int pu[3], pv[3], pq[3];
    bool found = true;
    for (int j = 0; j < 3; j++) {
        bool got = false;
        for (int t = 0; t < kSearchTries && !got; t++) {
            const uint32_t x = search_mix(key ^ (uint32_t)(16 * j + t));
            const unsigned p = (unsigned)(((unsigned long long)x * area) >> 32);  // < area
            const unsigned v = p / (unsigned)R.rw, u = p - v * (unsigned)R.rw;
            int q;
            bool ok = plane_q(fd + (size_t)v * stride + u, P.min_disp, &q);
            if (fc) ok = ok && fc[(size_t)v * W + u] >= P.conf_min;
            ok = ok && fl[(size_t)v * W + u] == kFreeLabel;
            if (ok) {
                pu[j] = (int)u;
                pv[j] = (int)v;
                pq[j] = q;
                got = true;
            }
        }
        found = found && got;
        if (!got) pu[j] = pv[j] = pq[j] = 0;
    }
    SearchHyp o = {0, 0, 0, 0, 0, 0};
    if (found) {
        const long long du1 = pu[1] - pu[0], dv1 = pv[1] - pv[0], dq1 = pq[1] - pq[0];
        const long long du2 = pu[2] - pu[0], dv2 = pv[2] - pv[0], dq2 = pq[2] - pq[0];
        const long long A = dv1 * dq2 - dq1 * dv2, B = dq1 * du2 - du1 * dq2, C = du1 * dv2 - dv1 * du2;
        if (C != 0) {  // |A|, |B| < 2^31, |C| < 2^25 (sdr.h)
            o.A = (int)A;
            o.B = (int)B;
            o.C = (int)C;
            o.D = A * pu[0] + B * pv[0] + C * pq[0];
        }
    }
    hyp[h] = o;
}

// The scores of round r: grid (slices of a W x H frame, chunks of kSearchChunk hypotheses).  A
// workgroup keeps its slice's pixels in registers and walks its chunk's hypotheses (their index is
// wave-uniform: scalar loads).  A wave counts a hypothesis' pixels by
// ballots, the waves' counts meet in LDS, and one integer atomic a (workgroup, hypothesis with a
// count) goes to the score array: neither the slices' order nor the grid shows in the result.  It
// also counts the round's free pixels (the record's n_valid) into acc[0].
template <typename T>
__global__ __launch_bounds__(kPlaneThreads) void k_search_score(const T* __restrict__ disp, size_t stride,
                                                                size_t fstride, int W, int H, int F,
                                                                const float* __restrict__ conf,
                                                                sdr_plane_params P,
                                                                const sdr_segment* __restrict__ reg,
                                                                const uint8_t* __restrict__ labels, int M,
                                                                const SearchState* __restrict__ st,
                                                                const SearchHyp* __restrict__ hyp,
                                                                unsigned* __restrict__ scores,
                                                                long long* __restrict__ acc) {
    __shared__ unsigned cnt[kPlaneWaves][kSearchChunk];
    if (st->stopped) return;  // block-uniform
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const sdr_segment sg = reg[0];
    const PlaneRect R = plane_rect(sg);
    const unsigned area = (unsigned)R.rw * (unsigned)R.rh;
    const unsigned base = blockIdx.x * (unsigned)kPlaneSlice;
    if (base >= area) return;
    const T* fd = disp + (size_t)sg.frame * fstride + (size_t)R.ys * stride + (size_t)R.xs;
    const float* fc = conf ? conf + ((size_t)sg.frame * H + (size_t)R.ys) * W + (size_t)R.xs : nullptr;
    const uint8_t* fl = labels + (size_t)R.ys * W + (size_t)R.xs;
    const long long Tq = (long long)floor((double)P.inlier_px * 16.0);

    int pu[kPlanePix], pv[kPlanePix], pq[kPlanePix];
    bool pf[kPlanePix];
    int nfree = 0;
#pragma unroll
    for (int j = 0; j < kPlanePix; j++) {
        const unsigned p = base + (unsigned)(j * kPlaneThreads + tid);
        pu[j] = pv[j] = pq[j] = 0;
        pf[j] = false;
        if (p < area) {
            const unsigned v = p / (unsigned)R.rw, u = p - v * (unsigned)R.rw;
            int q;
            bool ok = plane_q(fd + (size_t)v * stride + u, P.min_disp, &q);
            if (fc) ok = ok && fc[(size_t)v * W + u] >= P.conf_min;
            ok = ok && fl[(size_t)v * W + u] == kFreeLabel;
            pu[j] = (int)u;
            pv[j] = (int)v;
            pq[j] = ok ? q : 0;
            pf[j] = ok;
        }
        nfree += __popcll(__ballot(pf[j]));  // the wave's count, in every lane
    }
    const int c0 = (int)blockIdx.y * kSearchChunk;  // < M: the grid
    if (c0 == 0 && lane == 0 && nfree) atomicAdd((unsigned long long*)acc, (unsigned long long)nfree);
    {
        const int nh = min(M - c0, kSearchChunk);
        for (int i = 0; i < nh; i++) {  // at most kSearchChunk
            const SearchHyp hp = hyp[c0 + i];  // wave-uniform
            unsigned c = 0;
            if (hp.C != 0) {
                const long long thr = Tq * (long long)abs(hp.C);
#pragma unroll
                for (int j = 0; j < kPlanePix; j++) {
                    const long long e = ((long long)hp.A * pu[j] + (long long)hp.B * pv[j] +
                                         (long long)hp.C * pq[j]) - hp.D;
                    const bool in = pf[j] && (e < 0 ? -e : e) <= thr;
                    c += (unsigned)__popcll(__ballot(in));
                }
            }
            if (lane == 0) cnt[wave][i] = c;
        }
        __syncthreads();
        if (tid < nh) {
            unsigned s = 0;
#pragma unroll
            for (int w = 0; w < kPlaneWaves; w++) s += cnt[w][tid];
            if (s) atomicAdd(scores + c0 + tid, s);
        }
    }
}

// The pick of round r by one workgroup: the highest score among the hypotheses that are not void,
// ties to the lowest index (the maximum of (score << 32) | ~h), the stop decision, the seed plane.
__global__ __launch_bounds__(kPlaneThreads) void k_search_pick(const sdr_segment* __restrict__ reg, int r,
                                                               int max_planes, int M, int min_inliers,
                                                               const SearchHyp* __restrict__ hyp,
                                                               const unsigned* __restrict__ scores,
                                                               SearchState* __restrict__ st,
                                                               sdr_plane* __restrict__ planes,
                                                               int32_t* __restrict__ count,
                                                               sdr_plane_search_round* __restrict__ rounds) {
#pragma clang fp contract(off)
    __shared__ unsigned long long best[kPlaneWaves];
    __shared__ int nvoid[kPlaneWaves];
    if (st->stopped) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long key = 0;
    int voids = 0;
    for (int h = tid; h < M; h += kPlaneThreads) {  // at most 16 passes
        if (hyp[h].C == 0) {
            voids++;
        } else {
            const unsigned long long k = ((unsigned long long)scores[h] << 32) | (unsigned long long)(0xffffffffu - (unsigned)h);
            key = max(key, k);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        key = max(key, (unsigned long long)__shfl_xor((long long)key, o, 64));
        voids += __shfl_xor(voids, o, 64);
    }
    if (lane == 0) {
        best[wave] = key;
        nvoid[wave] = voids;
    }
    __syncthreads();
    if (tid != 0) return;
    key = 0;
    voids = 0;
    for (int w = 0; w < kPlaneWaves; w++) {
        key = max(key, best[w]);
        voids += nvoid[w];
    }
    const sdr_segment sg = reg[0];
    const PlaneRect R = plane_rect(sg);
    const int area = R.rw * R.rh;
    if (voids == M) {
        search_stop(st, sg, area, r, max_planes, -1, 0, voids, SDR_SEARCH_NO_HYPOTHESIS, SDR_PLANE_DEGENERATE, planes,
                    count, rounds);
        return;
    }
    const int h = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    const int score = (int)(key >> 32);
    if (score < min_inliers) {
        search_stop(st, sg, area, r, max_planes, h, score, voids, SDR_SEARCH_LOW_SCORE, SDR_PLANE_DEGENERATE, planes,
                    count, rounds);
        return;
    }
    const SearchHyp hp = hyp[h];
    st->winner = h;
    st->score = score;
    st->voids = voids;
    st->a = -(double)hp.A / (double)hp.C;
    st->b = -(double)hp.B / (double)hp.C;
    st->c = (double)hp.D / (double)hp.C;
}

// The record of round r from its accumulators, or the stop the refits or the statistics call for.
__global__ __launch_bounds__(64) void k_search_finish(const sdr_segment* __restrict__ reg, int r, int max_planes,
                                                      Q16 Q, sdr_plane_params P, const long long* __restrict__ A,
                                                      SearchState* __restrict__ st, sdr_plane* __restrict__ planes,
                                                      int32_t* __restrict__ count,
                                                      sdr_plane_search_round* __restrict__ rounds) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || st->stopped) return;
    const sdr_segment sg = reg[0];
    const PlaneRect R = plane_rect(sg);
    const int area = R.rw * R.rh;
    const int h = st->winner, score = st->score, voids = st->voids;
    PlaneFit fit = {0.0, 0.0, 0.0, false};
    const long long* M = A;
    for (int s = 1; s <= P.iterations; s++) {
        M = A + (size_t)s * kPlaneSlots;
        fit = plane_solve(M, P.min_inliers);
        if (!fit.ok) break;
    }
    const long long* L = A + (size_t)(P.iterations + 1) * kPlaneSlots;
    if (!fit.ok || L[0] < (long long)P.min_inliers) {
        search_stop(st, sg, area, r, max_planes, h, score, voids,
                    fit.ok ? SDR_SEARCH_FEW_INLIERS : SDR_SEARCH_REFIT_DEGENERATE, SDR_PLANE_DEGENERATE, planes,
                    count, rounds);
        return;
    }
    sdr_plane o;
    search_empty_record(&o, sg, area, 0);
    o.n_valid = (int)A[0];
    o.fits = P.iterations + 1;
    plane_record(o, R, fit, M, L, Q);
    planes[r] = o;
    *count = r + 1;
    search_round(rounds, r, h, score, voids, SDR_SEARCH_RAN);
}

// The claim of round r: the statistics sweep's inliers (the same residual against the same plane)
// get the round's label.  A pass of its own behind k_search_finish: a round that stops claims
// nothing, and no sweep can see a partly claimed map.
template <typename T>
__global__ __launch_bounds__(kPlaneThreads) void k_search_claim(const T* __restrict__ disp, size_t stride,
                                                                size_t fstride, int W, int H, int F,
                                                                const float* __restrict__ conf,
                                                                sdr_plane_params P,
                                                                const sdr_segment* __restrict__ reg,
                                                                uint8_t* __restrict__ labels, int r,
                                                                const SearchState* __restrict__ st,
                                                                const long long* __restrict__ A) {
#pragma clang fp contract(off)
    if (st->stopped) return;  // block-uniform
    const int tid = threadIdx.x;
    const sdr_segment sg = reg[0];
    const PlaneRect R = plane_rect(sg);
    const unsigned area = (unsigned)R.rw * (unsigned)R.rh;
    const unsigned base = blockIdx.x * (unsigned)kPlaneSlice;
    if (base >= area) return;
    const PlaneFit fit = plane_solve(A + (size_t)P.iterations * kPlaneSlots, P.min_inliers);  // ok: not stopped
    const double band = (double)P.inlier_px * 16.0;
    const T* fd = disp + (size_t)sg.frame * fstride + (size_t)R.ys * stride + (size_t)R.xs;
    const float* fc = conf ? conf + ((size_t)sg.frame * H + (size_t)R.ys) * W + (size_t)R.xs : nullptr;
    uint8_t* fl = labels + (size_t)R.ys * W + (size_t)R.xs;
#pragma unroll
    for (int j = 0; j < kPlanePix; j++) {
        const unsigned p = base + (unsigned)(j * kPlaneThreads + tid);
        if (p >= area) continue;
        const unsigned v = p / (unsigned)R.rw, u = p - v * (unsigned)R.rw;
        int q;
        bool ok = plane_q(fd + (size_t)v * stride + u, P.min_disp, &q);
        if (fc) ok = ok && fc[(size_t)v * W + u] >= P.conf_min;
        ok = ok && fl[(size_t)v * W + u] == kFreeLabel;
        const double res = (double)q - plane_at(fit, (double)u, (double)v);
        if (ok && fabs(res) <= band) fl[(size_t)v * W + u] = (uint8_t)r;
    }
}

// Point queries, one wave a query: the ruler's sample and its distance to a fitted plane.
template <typename T>
__global__ __launch_bounds__(kPlaneThreads) void k_plane_distance(const T* __restrict__ disp, size_t stride,
                                                                  size_t fstride, int W, int H, int F,
                                                                  const float* __restrict__ conf, Q16 Q,
                                                                  sdr_ruler_params P,
                                                                  const sdr_plane* __restrict__ planes, int NP,
                                                                  const sdr_plane_query* __restrict__ qs, int K,
                                                                  struct sdr_plane_distance* __restrict__ out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * kPlaneWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (k >= K) return;  // wave-uniform
    const sdr_plane_query q = qs[k];
    const bool inside = q.frame >= 0 && q.frame < F && q.x >= 0 && q.x < W && q.y >= 0 && q.y < H;
    uint32_t flags = inside ? 0 : SDR_PDIST_OUT_OF_RANGE;
    double n[3] = {0.0, 0.0, 0.0}, off = 0.0;
    bool plane_ok = q.plane >= 0 && q.plane < NP;
    if (plane_ok) {
        const sdr_plane* pl = planes + q.plane;
        plane_ok = (pl->flags & SDR_PLANE_OK) != 0;
        n[0] = pl->normal[0];
        n[1] = pl->normal[1];
        n[2] = pl->normal[2];
        off = pl->offset;
    }
    if (!plane_ok) flags |= SDR_PDIST_NO_PLANE;
    RulerSample s;
    s.d = s.xyz[0] = s.xyz[1] = s.xyz[2] = ruler_nan();
    s.n = 0;
    s.valid = false;
    if (inside)
        s = ruler_sample(disp + (size_t)q.frame * fstride, stride,
                         conf ? conf + (size_t)q.frame * W * H : nullptr, W, H, Q, P, q.x, q.y, lane);
    if (lane != 0) return;
    double dist = __builtin_nan("");
    if (s.valid && plane_ok) {
        dist = canon(((n[0] * (double)s.xyz[0] + n[1] * (double)s.xyz[1]) + n[2] * (double)s.xyz[2]) + off);
        flags |= SDR_PDIST_VALID;
    }
    struct sdr_plane_distance* o = out + k;
    o->p[0] = canon(s.xyz[0]);
    o->p[1] = canon(s.xyz[1]);
    o->p[2] = canon(s.xyz[2]);
    o->d = s.d;
    o->distance = dist;
    o->n = s.n;
    o->flags = flags;
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

int check_plane_params(const sdr_plane_params* p) {
    if (p->iterations < 0 || p->iterations > 8) return rfail(SDR_ERR_ARG, "iterations must be in 0..8");
    if (p->min_inliers < 3) return rfail(SDR_ERR_ARG, "min_inliers must be >= 3");
    if (!(p->inlier_px > 0.0f && p->inlier_px <= 64.0f)) return rfail(SDR_ERR_ARG, "inlier_px must be in (0, 64]");
    return SDR_OK;
}

int check_search_params(const sdr_plane_search_params* p) {
    const int rc = check_plane_params(&p->fit);
    if (rc) return rc;
    if (p->fit.iterations < 1) return rfail(SDR_ERR_ARG, "the plane search takes iterations in 1..8");
    if (p->max_planes < 1 || p->max_planes > 8) return rfail(SDR_ERR_ARG, "max_planes must be in 1..8");
    if (p->hypotheses < 1 || p->hypotheses > 4096) return rfail(SDR_ERR_ARG, "hypotheses must be in 1..4096");
    return SDR_OK;
}

int check_query_params(const sdr_ruler_params* p, const void* planes, int P) {
    if (p->radius < 0 || p->radius > 4) return rfail(SDR_ERR_ARG, "radius must be in 0..4");
    if (p->min_count < 1) return rfail(SDR_ERR_ARG, "min_count must be >= 1");
    if (P < 0 || (P > 0 && !planes)) return rfail(SDR_ERR_ARG, "bad plane count or null planes");
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
    sdr::Q16 q;
    for (int i = 0; i < 16; i++) q.q[i] = Q[i];
    const dim3 grid((unsigned)K), block(params->profile ? sdr::kRulerThreads : sdr::kRulerEndThreads);
    if (disp_type == SDR_DISP_F32)
        hipLaunchKernelGGL(sdr::k_ruler<float>, grid, block, 0, (hipStream_t)stream, (const float*)d_disp,
                           stride, frame_stride, W, H, F, d_conf, q, *params, d_segs, d_out, d_profile);
    else
        hipLaunchKernelGGL(sdr::k_ruler<int16_t>, grid, block, 0, (hipStream_t)stream,
                           (const int16_t*)d_disp, stride, frame_stride, W, H, F, d_conf, q, *params,
                           d_segs, d_out, d_profile);
    RULER_HIP(hipGetLastError());
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
    RULER_HIP(hipGetLastError());
    return SDR_OK;
}

int sdr_measure_disp(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H,
                     int F, const float* conf, const double Q[16], const sdr_ruler_params* params,
                     const sdr_segment* segs, int K, sdr_measurement* out, float* profile) {
    int rc = check_disp_args(disp, disp_type, stride, frame_stride, W, H, F, Q, params, segs, K, out, profile);
    if (rc) return rc;
    if (K == 0) return SDR_OK;
    HostState* S = nullptr;
    if ((rc = host_state(&S))) return rc;
    const size_t px = (size_t)W * H;
    const bool prof = profile && params->profile && params->profile_cap > 0;
    const size_t prof_bytes = prof ? (size_t)K * params->profile_cap * 16 : 0;
    if ((rc = sdr::ensure(S->segs, (size_t)K * sizeof(sdr_segment))) ||
        (rc = sdr::ensure(S->out, (size_t)K * sizeof(sdr_measurement))) || (rc = sdr::ensure(S->prof, prof_bytes)) ||
        (rc = upload_maps(S, disp, disp_type, stride, frame_stride, W, H, F, conf)))
        return rc;
    RULER_HIP(hipMemcpyAsync(S->segs.p, segs, (size_t)K * sizeof(sdr_segment), hipMemcpyHostToDevice, S->st));
    // rows the kernel leaves untouched keep the caller's values
    if (prof) RULER_HIP(hipMemcpyAsync(S->prof.p, profile, prof_bytes, hipMemcpyHostToDevice, S->st));
    rc = sdr_measure_disp_device(S->map.p, disp_type, (size_t)W, px, W, H, F, conf ? (const float*)S->conf.p : nullptr,
                                 Q, params, (const sdr_segment*)S->segs.p, K, (sdr_measurement*)S->out.p,
                                 prof ? (float*)S->prof.p : nullptr, S->st);
    if (rc) return rc;
    RULER_HIP(hipMemcpyAsync(out, S->out.p, (size_t)K * sizeof(sdr_measurement), hipMemcpyDeviceToHost, S->st));
    if (prof) RULER_HIP(hipMemcpyAsync(profile, S->prof.p, prof_bytes, hipMemcpyDeviceToHost, S->st));
    RULER_HIP(hipStreamSynchronize(S->st));
    return SDR_OK;
}

int sdr_measure_xyz(const float* xyz, size_t xyz_stride, size_t xyz_frame_stride, int W, int H, int F,
                    const sdr_segment* segs, int K, sdr_measurement* out) {
    int rc = check_xyz_args(xyz, xyz_stride, xyz_frame_stride, W, H, F, segs, K, out);
    if (rc) return rc;
    if (K == 0) return SDR_OK;
    HostState* S = nullptr;
    if ((rc = host_state(&S))) return rc;
    const size_t px = (size_t)W * H;
    if ((rc = sdr::ensure(S->map, (size_t)F * px * 12)) || (rc = sdr::ensure(S->segs, (size_t)K * sizeof(sdr_segment))) ||
        (rc = sdr::ensure(S->out, (size_t)K * sizeof(sdr_measurement))))
        return rc;
    if ((rc = upload_rows(S->map.p, xyz, (size_t)W * 12, xyz_stride * 4, xyz_frame_stride * 4, H, F, S->st))) return rc;
    RULER_HIP(hipMemcpyAsync(S->segs.p, segs, (size_t)K * sizeof(sdr_segment), hipMemcpyHostToDevice, S->st));
    rc = sdr_measure_xyz_device((const float*)S->map.p, (size_t)W * 3, px * 3, W, H, F, (const sdr_segment*)S->segs.p,
                                K, (sdr_measurement*)S->out.p, S->st);
    if (rc) return rc;
    RULER_HIP(hipMemcpyAsync(out, S->out.p, (size_t)K * sizeof(sdr_measurement), hipMemcpyDeviceToHost, S->st));
    RULER_HIP(hipStreamSynchronize(S->st));
    return SDR_OK;
}

void sdr_plane_params_default(sdr_plane_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->iterations = 3;
    p->min_inliers = 16;
    p->inlier_px = 1.0f;
    p->min_disp = -1.0f;
    p->conf_min = 0.0f;
}

int sdr_fit_planes_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride, int W,
                          int H, int F, const float* d_conf, const double Q[16],
                          const sdr_plane_params* params, const sdr_segment* d_regions, int K,
                          sdr_plane* d_planes, void* stream) {
    int rc = check_plane_maps(d_disp, disp_type, stride, frame_stride, W, H, F, Q, params, d_regions, K, d_planes);
    if (rc || (rc = check_plane_params(params))) return rc;
    if (K == 0) return SDR_OK;
    hipStream_t st = (hipStream_t)stream;
    sdr::Q16 q;
    for (int i = 0; i < 16; i++) q.q[i] = Q[i];
    const int sweeps = params->iterations + 2;
    const size_t per = (size_t)sweeps * sdr::kPlaneSlots, bytes = (size_t)K * per * sizeof(long long);
    long long* acc = nullptr;
    RULER_HIP(sdr::scratch_alloc((void**)&acc, bytes, st));
    RULER_HIP(hipMemsetAsync(acc, 0, bytes, st));
    const unsigned slices = (unsigned)(((size_t)W * H + sdr::kPlaneSlice - 1) / sdr::kPlaneSlice);
    for (int s = 0; s < sweeps; s++)
        for (int k0 = 0; k0 < K; k0 += 65535) {  // the grid's y extent
            const dim3 grid(slices, (unsigned)std::min(K - k0, 65535)), block(sdr::kPlaneThreads);
            if (disp_type == SDR_DISP_F32)
                hipLaunchKernelGGL((sdr::k_plane_sweep<float, false>), grid, block, 0, st, (const float*)d_disp, stride,
                                   frame_stride, W, H, F, d_conf, *params, d_regions + k0, acc + k0 * per, s,
                                   (const uint8_t*)nullptr, (const sdr::SearchState*)nullptr);
            else
                hipLaunchKernelGGL((sdr::k_plane_sweep<int16_t, false>), grid, block, 0, st, (const int16_t*)d_disp,
                                   stride, frame_stride, W, H, F, d_conf, *params, d_regions + k0,
                                   acc + k0 * per, s, (const uint8_t*)nullptr, (const sdr::SearchState*)nullptr);
        }
    hipLaunchKernelGGL(sdr::k_plane_finish, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, st, d_regions, K, W, H,
                       F, q, *params, (const long long*)acc, d_planes);
    const hipError_t le = hipGetLastError();
    RULER_HIP(sdr::scratch_free(acc, st));
    RULER_HIP(le);
    return SDR_OK;
}

void sdr_plane_search_params_default(sdr_plane_search_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    sdr_plane_params_default(&p->fit);
    p->fit.min_inliers = 64;
    p->max_planes = 4;
    p->hypotheses = 256;
    p->seed = 0;
}

int sdr_find_planes_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride, int W, int H,
                           int F, const float* d_conf, const double Q[16], const sdr_plane_search_params* params,
                           const sdr_segment* d_region, sdr_plane* d_planes, int32_t* d_count,
                           sdr_plane_search_round* d_rounds, uint8_t* d_labels, void* stream) {
    int rc = check_plane_maps(d_disp, disp_type, stride, frame_stride, W, H, F, Q, params, d_region, 1, d_planes);
    if (rc) return rc;
    if (!d_count) return rfail(SDR_ERR_ARG, "null argument");
    if ((rc = check_search_params(params))) return rc;
    hipStream_t st = (hipStream_t)stream;
    sdr::Q16 q;
    for (int i = 0; i < 16; i++) q.q[i] = Q[i];
    const sdr_plane_params P = params->fit;
    const int NP = params->max_planes, M = params->hypotheses;
    const size_t px = (size_t)W * H;
    // scratch: {state, the rounds' accumulators, the rounds' scores} zeroed, the hypotheses of one
    // round (every round writes all M before it reads them), the claim map when the caller has none
    const size_t per = (size_t)(P.iterations + 2) * sdr::kPlaneSlots;
    const size_t o_acc = 64, o_sc = o_acc + (size_t)NP * per * sizeof(long long);
    const size_t o_hyp = (o_sc + (size_t)NP * M * sizeof(unsigned) + 63) & ~(size_t)63;
    const size_t o_lab = o_hyp + (size_t)M * sizeof(sdr::SearchHyp);
    char* sc = nullptr;
    RULER_HIP(sdr::scratch_alloc((void**)&sc, o_lab + (d_labels ? 0 : px), st));
    sdr::SearchState* state = (sdr::SearchState*)sc;
    long long* acc = (long long*)(sc + o_acc);
    unsigned* scores = (unsigned*)(sc + o_sc);
    sdr::SearchHyp* hyp = (sdr::SearchHyp*)(sc + o_hyp);
    uint8_t* labels = d_labels ? d_labels : (uint8_t*)(sc + o_lab);
    hipError_t e = hipMemsetAsync(sc, 0, o_hyp, st);
    if (e == hipSuccess) e = hipMemsetAsync(labels, 0xff, px, st);
    if (e != hipSuccess) {
        (void)sdr::scratch_free(sc, st);
        RULER_HIP(e);
    }
    const unsigned slices = (unsigned)((px + sdr::kPlaneSlice - 1) / sdr::kPlaneSlice);
    const dim3 sgrid(slices), sblock(sdr::kPlaneThreads), dgrid((unsigned)((M + 63) / 64)), one(1), wave(64);
    const dim3 cgrid(slices, (unsigned)((M + sdr::kSearchChunk - 1) / sdr::kSearchChunk));
    hipLaunchKernelGGL(sdr::k_search_init, one, wave, 0, st, d_region, W, H, F, NP, state, d_planes, d_count,
                       d_rounds);
    auto round = [&](auto* disp, int r) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(disp)>>;
        long long* A = acc + (size_t)r * per;
        unsigned* S = scores + (size_t)r * M;
        hipLaunchKernelGGL(sdr::k_search_draw<T>, dgrid, wave, 0, st, disp, stride, frame_stride, W, H, F, d_conf, P,
                           d_region, (const uint8_t*)labels, r, M, params->seed, (const sdr::SearchState*)state, hyp);
        hipLaunchKernelGGL(sdr::k_search_score<T>, cgrid, sblock, 0, st, disp, stride, frame_stride, W, H, F, d_conf,
                           P, d_region, (const uint8_t*)labels, M, (const sdr::SearchState*)state,
                           (const sdr::SearchHyp*)hyp, S, A);
        hipLaunchKernelGGL(sdr::k_search_pick, one, sblock, 0, st, d_region, r, NP, M, P.min_inliers,
                           (const sdr::SearchHyp*)hyp, (const unsigned*)S, state, d_planes, d_count, d_rounds);
        for (int s = 1; s <= P.iterations + 1; s++)
            hipLaunchKernelGGL((sdr::k_plane_sweep<T, true>), sgrid, sblock, 0, st, disp, stride, frame_stride, W, H,
                               F, d_conf, P, d_region, A, s, (const uint8_t*)labels, (const sdr::SearchState*)state);
        hipLaunchKernelGGL(sdr::k_search_finish, one, wave, 0, st, d_region, r, NP, q, P, (const long long*)A, state,
                           d_planes, d_count, d_rounds);
        hipLaunchKernelGGL(sdr::k_search_claim<T>, sgrid, sblock, 0, st, disp, stride, frame_stride, W, H, F, d_conf,
                           P, d_region, labels, r, (const sdr::SearchState*)state, (const long long*)A);
    };
    for (int r = 0; r < NP; r++) {
        if (disp_type == SDR_DISP_F32)
            round((const float*)d_disp, r);
        else
            round((const int16_t*)d_disp, r);
    }
    const hipError_t le = hipGetLastError();
    RULER_HIP(sdr::scratch_free(sc, st));
    RULER_HIP(le);
    return SDR_OK;
}

int sdr_find_planes(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H, int F,
                    const float* conf, const double Q[16], const sdr_plane_search_params* params,
                    const sdr_segment* region, sdr_plane* planes, int32_t* count, sdr_plane_search_round* rounds,
                    uint8_t* labels) {
    int rc = check_plane_maps(disp, disp_type, stride, frame_stride, W, H, F, Q, params, region, 1, planes);
    if (rc) return rc;
    if (!count) return rfail(SDR_ERR_ARG, "null argument");
    if ((rc = check_search_params(params))) return rc;
    HostState* S = nullptr;
    if ((rc = host_state(&S))) return rc;
    const int NP = params->max_planes;
    const size_t px = (size_t)W * H, rbytes = (size_t)NP * sizeof(sdr_plane_search_round);
    // out: {count, padding to 16 bytes, the rounds}; prof: the labels
    if ((rc = upload_maps(S, disp, disp_type, stride, frame_stride, W, H, F, conf)) ||
        (rc = sdr::ensure(S->segs, sizeof(sdr_segment))) || (rc = sdr::ensure(S->planes, (size_t)NP * sizeof(sdr_plane))) ||
        (rc = sdr::ensure(S->out, 16 + rbytes)) || (rc = sdr::ensure(S->prof, labels ? px : 0)))
        return rc;
    RULER_HIP(hipMemcpyAsync(S->segs.p, region, sizeof(sdr_segment), hipMemcpyHostToDevice, S->st));
    rc = sdr_find_planes_device(S->map.p, disp_type, (size_t)W, px, W, H, F, conf ? (const float*)S->conf.p : nullptr, Q,
                                params, (const sdr_segment*)S->segs.p, (sdr_plane*)S->planes.p, (int32_t*)S->out.p,
                                (sdr_plane_search_round*)((char*)S->out.p + 16), labels ? (uint8_t*)S->prof.p : nullptr,
                                S->st);
    if (rc) return rc;
    RULER_HIP(hipMemcpyAsync(planes, S->planes.p, (size_t)NP * sizeof(sdr_plane), hipMemcpyDeviceToHost, S->st));
    RULER_HIP(hipMemcpyAsync(count, S->out.p, sizeof(int32_t), hipMemcpyDeviceToHost, S->st));
    if (rounds) RULER_HIP(hipMemcpyAsync(rounds, (char*)S->out.p + 16, rbytes, hipMemcpyDeviceToHost, S->st));
    if (labels) RULER_HIP(hipMemcpyAsync(labels, S->prof.p, px, hipMemcpyDeviceToHost, S->st));
    RULER_HIP(hipStreamSynchronize(S->st));
    return SDR_OK;
}

int sdr_plane_distance_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride, int W,
                              int H, int F, const float* d_conf, const double Q[16],
                              const sdr_ruler_params* params, const sdr_plane* d_planes, int P,
                              const sdr_plane_query* d_queries, int K,
                              struct sdr_plane_distance* d_out,
                              void* stream) {
    int rc = check_plane_maps(d_disp, disp_type, stride, frame_stride, W, H, F, Q, params, d_queries, K, d_out);
    if (rc || (rc = check_query_params(params, d_planes, P))) return rc;
    if (K == 0) return SDR_OK;
    sdr::Q16 q;
    for (int i = 0; i < 16; i++) q.q[i] = Q[i];
    const dim3 grid((unsigned)((K + sdr::kPlaneWaves - 1) / sdr::kPlaneWaves)), block(sdr::kPlaneThreads);
    if (disp_type == SDR_DISP_F32)
        hipLaunchKernelGGL(sdr::k_plane_distance<float>, grid, block, 0, (hipStream_t)stream,
                           (const float*)d_disp, stride, frame_stride, W, H, F, d_conf, q, *params, d_planes, P,
                           d_queries, K, d_out);
    else
        hipLaunchKernelGGL(sdr::k_plane_distance<int16_t>, grid, block, 0, (hipStream_t)stream,
                           (const int16_t*)d_disp, stride, frame_stride, W, H, F, d_conf, q, *params, d_planes,
                           P, d_queries, K, d_out);
    RULER_HIP(hipGetLastError());
    return SDR_OK;
}

int sdr_fit_planes(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H, int F,
                   const float* conf, const double Q[16], const sdr_plane_params* params,
                   const sdr_segment* regions, int K, sdr_plane* planes) {
    int rc = check_plane_maps(disp, disp_type, stride, frame_stride, W, H, F, Q, params, regions, K, planes);
    if (rc || (rc = check_plane_params(params))) return rc;
    if (K == 0) return SDR_OK;
    HostState* S = nullptr;
    if ((rc = host_state(&S))) return rc;
    if ((rc = upload_maps(S, disp, disp_type, stride, frame_stride, W, H, F, conf)) ||
        (rc = sdr::ensure(S->segs, (size_t)K * sizeof(sdr_segment))) ||
        (rc = sdr::ensure(S->planes, (size_t)K * sizeof(sdr_plane))))
        return rc;
    RULER_HIP(hipMemcpyAsync(S->segs.p, regions, (size_t)K * sizeof(sdr_segment), hipMemcpyHostToDevice, S->st));
    rc = sdr_fit_planes_device(S->map.p, disp_type, (size_t)W, (size_t)W * H, W, H, F,
                               conf ? (const float*)S->conf.p : nullptr, Q, params, (const sdr_segment*)S->segs.p,
                               K, (sdr_plane*)S->planes.p, S->st);
    if (rc) return rc;
    RULER_HIP(hipMemcpyAsync(planes, S->planes.p, (size_t)K * sizeof(sdr_plane), hipMemcpyDeviceToHost, S->st));
    RULER_HIP(hipStreamSynchronize(S->st));
    return SDR_OK;
}

int sdr_plane_distance(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H,
                       int F, const float* conf, const double Q[16], const sdr_ruler_params* params,
                       const sdr_plane* planes, int P, const sdr_plane_query* queries, int K,
                       struct sdr_plane_distance* out) {
    int rc = check_plane_maps(disp, disp_type, stride, frame_stride, W, H, F, Q, params, queries, K, out);
    if (rc || (rc = check_query_params(params, planes, P))) return rc;
    if (K == 0) return SDR_OK;
    HostState* S = nullptr;
    if ((rc = host_state(&S))) return rc;
    if ((rc = upload_maps(S, disp, disp_type, stride, frame_stride, W, H, F, conf)) ||
        (rc = sdr::ensure(S->segs, (size_t)K * sizeof(sdr_plane_query))) ||
        (rc = sdr::ensure(S->planes, (size_t)P * sizeof(sdr_plane))) ||
        (rc = sdr::ensure(S->out, (size_t)K * sizeof(struct sdr_plane_distance))))
        return rc;
    RULER_HIP(hipMemcpyAsync(S->segs.p, queries, (size_t)K * sizeof(sdr_plane_query), hipMemcpyHostToDevice, S->st));
    if (P) RULER_HIP(hipMemcpyAsync(S->planes.p, planes, (size_t)P * sizeof(sdr_plane), hipMemcpyHostToDevice, S->st));
    rc = sdr_plane_distance_device(S->map.p, disp_type, (size_t)W, (size_t)W * H, W, H, F,
                                   conf ? (const float*)S->conf.p : nullptr, Q, params,
                                   P ? (const sdr_plane*)S->planes.p : nullptr, P,
                                   (const sdr_plane_query*)S->segs.p, K, (struct sdr_plane_distance*)S->out.p, S->st);
    if (rc) return rc;
    RULER_HIP(hipMemcpyAsync(out, S->out.p, (size_t)K * sizeof(struct sdr_plane_distance), hipMemcpyDeviceToHost, S->st));
    RULER_HIP(hipStreamSynchronize(S->st));
    return SDR_OK;
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
