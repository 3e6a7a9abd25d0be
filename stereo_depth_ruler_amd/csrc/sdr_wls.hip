// sdr_wls.hip -- the class path's post-filter on the GPU:
//   cv::ximgproc::createDisparityWLSFilter(matcher)    stereo_vision/src/stereo_disparity.cpp:11-13
//   wls_filter->filter(disp_left, left_small, filtered, disp_right)               :31
//   wls_filter->getConfidenceMap()                                                :36
// restating opencv_contrib 4.6 ximgproc disparity_filters.cpp + fgs_filter.cpp as the oracle
// does (oracle/wls_oracle.c, the checker; parity against OpenCV itself is unpinned there).
//
// Kernels (all float work with contraction off and IEEE division, so every rounding matches the
// oracle's operation order bit for bit; the FGS weight table is computed once on the host with
// the same expf the oracle uses):
//   k_wls_disc     depth-discontinuity map of the RIGHT view over its ROI: 1 - roll_off * var
//                  of a (2r+1)^2 box, BORDER_REFLECT_101 inside the ROI, sums in int64/double
//   k_wls_conf     left discontinuity (inline) + discontinuity-aware LR check -> confidence
//                  x255 (full map for getConfidenceMap) and the two FGS inputs conf*d, conf,
//                  compacted to the ROI
//   k_wls_prep     the whole front end of one ROI row in one workgroup (ROIs up to 4096 columns,
//                  radius <= 9): both discontinuity maps, the LR check, the confidence, the FGS
//                  inputs in the solver's layout and the row's FGS weights
//   k_fgs_weights  the FGS weights of a guide from the table, in the solver's layouts (where
//                  k_wls_prep has not written them)
//   k_fgs_pack     row-major images -> the sequential solver's first-pass layout (transposed, both
//                  right-hand sides interleaved), where k_wls_prep has not written it
//   k_transpose2   LDS-tiled transpose of two arrays (64x64 tiles); no launch uses it at present
//   k_wls_final    FGS(conf*d) / FGS(conf) -> saturate_cast<short>, 16*(min_disp-1) outside ROI
// The FGS line solves are in sdr_fgs_seq.hip (SDR_FGS_THOMAS, the default) and sdr_fgs_pcr.hip
// (SDR_FGS_PCR); launch_fgs here orchestrates them, and the filter's handle and C ABI follow it.
#include "sdr_fgs.hpp"
#include "sdr_host.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace sdr {

constexpr int kFgsLevels = 65026;  // 255^2 + 1 squared differences of two 8-bit gray levels

__device__ __forceinline__ int reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// 1 - roll_off * (boxmean(d^2) - boxmean(d)^2), clamped at 0, at ROI pixel (i, j) of map d
// (ComputeDepthDisc: convertTo(CV_32F), multiply, boxFilter(CV_32F) x2 with double row sums)
__device__ __forceinline__ float disc_at(const int16_t* __restrict__ d, int W, int rx, int ry,
                                         int rw, int rh, int i, int j, int radius, double scale,
                                         float roll_off) {
    long long s = 0, s2 = 0;
    for (int a = -radius; a <= radius; a++) {
        const int ii = reflect101(i + a, rh);
        const int16_t* row = d + (size_t)(ry + ii) * W + rx;
        for (int b = -radius; b <= radius; b++) {
            const long long v = row[reflect101(j + b, rw)];
            s += v;
            s2 += v * v;
        }
    }
    const float mean = (float)((double)s * scale);
    const float msq = (float)((double)s2 * scale);
    const float var = msq - mean * mean;
    const float c = 1.0f - roll_off * var;
    return c > 0.0f ? c : 0.0f;
}

__global__ __launch_bounds__(256) void k_wls_disc(const int16_t* __restrict__ dr, WlsGeom g,
                                                  float* __restrict__ rdisc) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (j >= g.rw || i >= g.rh) return;
    const size_t fo = (size_t)blockIdx.z * g.W * g.H;
    rdisc[fo + (size_t)(g.ry + i) * g.W + g.rrx + j] =
        disc_at(dr + fo, g.W, g.rrx, g.ry, g.rw, g.rh, i, j, g.radius, g.scale, g.roll_off);
}

// ComputeDiscontinuityAwareLRC + confidence_map = 255 * map; A = conf * d, B = conf (ROI-compact)
__global__ __launch_bounds__(256) void k_wls_conf(const int16_t* __restrict__ dl,
                                                  const int16_t* __restrict__ dr,
                                                  const float* __restrict__ rdisc, WlsGeom g,
                                                  float* __restrict__ conf_full,
                                                  float* __restrict__ A, float* __restrict__ B) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    const size_t fo = (size_t)blockIdx.z * g.W * g.H;
    const size_t o = fo + (size_t)y * g.W + x;
    const int j = x - g.rx, i = y - g.ry;
    const bool in_roi = j >= 0 && j < g.rw && i >= 0 && i < g.rh;
    float c = 1.0f;
    int v = 0;
    if (in_roi) {
        c = disc_at(dl + fo, g.W, g.rx, g.ry, g.rw, g.rh, i, j, g.radius, g.scale, g.roll_off);
        v = dl[o];
        const int ridx = x - (v >> 4);
        if (ridx >= g.rrx && ridx < g.rrx + g.rw) {
            const size_t ro = fo + (size_t)y * g.W + ridx;
            if (abs(v + (int)dr[ro]) < g.lrc_thresh) {
                const float rc = rdisc[ro];
                c = c < rc ? c : rc;
            } else {
                c = 0.0f;
            }
        }
    }
    const float conf = 255.0f * c;
    if (conf_full) conf_full[o] = conf;
    if (in_roi) {
        const size_t co = (size_t)blockIdx.z * g.rw * g.rh + (size_t)i * g.rw + j;
        A[co] = conf * (float)v;
        B[co] = conf;
    }
}

// R0 (and R1) row-major [h][w] -> the first row pass's input: transposed [w][hp] (hp = h rounded
// up to 4, frames fgs_pad4(w) * hp apart), the two images interleaved (float2) when R1 is given;
// 64x64 LDS tiles
__global__ __launch_bounds__(256) void k_fgs_pack(const float* __restrict__ r0, const float* __restrict__ r1,
                                                  float* __restrict__ dst, int h, int w) {
    __shared__ float tile[2][64][65];
    const int c0 = blockIdx.x * 64, rw0 = blockIdx.y * 64;
    const size_t fo = (size_t)blockIdx.z * h * w;
    const int hp = fgs_pad4(h);
    const size_t fd = (size_t)blockIdx.z * fgs_pad4(w) * hp;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int rr = rw0 + r, cc = c0 + tx;
        if (rr < h && cc < w) {
            tile[0][r][tx] = r0[fo + (size_t)rr * w + cc];
            if (r1) tile[1][r][tx] = r1[fo + (size_t)rr * w + cc];
        }
    }
    __syncthreads();
    for (int c = ty; c < 64; c += 4) {
        const int cc = c0 + c, rr = rw0 + tx;
        if (rr < h && cc < w) {
            const size_t o = fd + (size_t)cc * hp + rr;
            if (r1) ((float2*)dst)[o] = make_float2(tile[0][tx][c], tile[1][tx][c]);
            else dst[o] = tile[0][tx][c];
        }
    }
}

// FGS weights of one guide (per frame): Ch (weight between (i, j) and (i, j+1): column-major at
// j*h + i for the sequential sweep, row-major at i*w + j for k_fgs_pcr) and Cv (row-major:
// (i, j)-(i+1, j) at i*w + j)
__global__ __launch_bounds__(256) void k_fgs_weights(const uint8_t* __restrict__ guide, size_t gstride,
                                                     size_t gfstride, const float* __restrict__ lut,
                                                     int w, int h, int ch_rowmajor, float* __restrict__ ChT,
                                                     float* __restrict__ Cv) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (j >= w || i >= h) return;
    const uint8_t* g = guide + (size_t)blockIdx.z * gfstride + (size_t)i * gstride + j;
    // the sequential solver's layouts: Ch at j*hp + i, Cv at i*wp + j (fgs_pad4)
    const int wp = ch_rowmajor ? w : fgs_pad4(w), hp = ch_rowmajor ? h : fgs_pad4(h);
    const size_t fo = (size_t)blockIdx.z * wp * hp;
    const int v = g[0];
    float ch = 0.0f, cv = 0.0f;
    if (j + 1 < w) {
        const int d = v - g[1];
        ch = lut[d * d];
    }
    if (i + 1 < h) {
        const int d = v - g[gstride];
        cv = lut[d * d];
    }
    ChT[fo + (ch_rowmajor ? (size_t)i * w + j : (size_t)j * hp + i)] = ch;
    Cv[fo + (size_t)i * wp + j] = cv;
}

// dst[f][c][r] = src[f][r][c] for two arrays (rows x cols per frame), 64x64 LDS tiles
__global__ __launch_bounds__(256) void k_transpose2(const float* __restrict__ s0,
                                                    const float* __restrict__ s1, float* __restrict__ d0,
                                                    float* __restrict__ d1, int rows, int cols) {
    __shared__ float tile[2][64][65];
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const size_t fo = (size_t)blockIdx.z * rows * cols;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int rr = r0 + r, cc = c0 + tx;
        if (rr < rows && cc < cols) {
            tile[0][r][tx] = s0[fo + (size_t)rr * cols + cc];
            if (s1) tile[1][r][tx] = s1[fo + (size_t)rr * cols + cc];
        }
    }
    __syncthreads();
    for (int c = ty; c < 64; c += 4) {
        const int cc = c0 + c, rr = r0 + tx;
        if (rr < rows && cc < cols) {
            d0[fo + (size_t)cc * rows + rr] = tile[0][tx][c];
            if (s1) d1[fo + (size_t)cc * rows + rr] = tile[1][tx][c];
        }
    }
}

// The whole filter front end of one ROI row in one workgroup (grid: rows x frames), replacing
// k_wls_disc + k_wls_conf + k_fgs_weights:
//   1. vertical (2r+1)-row sums of d and d^2 of both maps over the row's window (BORDER_REFLECT_101
//      inside the ROI), one column per thread, into LDS (int32 / int64: exact integers)
//   2. horizontal sums of those -> the depth-discontinuity value of every ROI column of both maps
//      (the same integers as disc_at's 2-D loop, so the same floats) into LDS
//   3. the discontinuity-aware LR check of the row (its partner column x - (d >> 4) is in the same
//      row, so the row's right map is all it needs): full-size confidence x255, A = conf * d,
//      B = conf (ROI-compact)
//   4. the row's FGS weights from the guide (Ch row-major for k_fgs_pcr or column-major for the
//      sequential sweep, Cv row-major), computed in step 1's column loop
// Rows outside the ROI only get the confidence map's 255.  Dynamic LDS: 32 B per ROI column
// (int64 + int32 column sums and a float discontinuity value, per map).
template <int RMAX>
__global__ __launch_bounds__(256) void k_wls_prep(const int16_t* __restrict__ dl, const int16_t* __restrict__ dr,
                                                  WlsGeom g, const uint8_t* __restrict__ guide,
                                                  size_t gstride, size_t gfstride,
                                                  const float* __restrict__ lut, int ch_rowmajor,
                                                  float* __restrict__ conf_full, float* __restrict__ A,
                                                  float* __restrict__ B, float* __restrict__ ChW,
                                                  float* __restrict__ Cv, int border, WlsOut wo) {
    extern __shared__ int64_t wls_smem[];
    const int y = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, T = blockDim.x;
    const size_t fo = (size_t)f * g.W * g.H;
    const int i = y - g.ry;
    // border: this row's outputs outside the ROI (16 * (min_disp - 1)) are final now (the last FGS
    // pass writes the ROI's)
    if (border)
        for (int x = tid; x < g.W; x += T)
            if (i < 0 || i >= g.rh || x < g.rx || x >= g.rx + g.rw) wls_emit(wo, g, f, x, y, (int16_t)g.fill);
    if (i < 0 || i >= g.rh) {
        if (conf_full)
            for (int x = tid; x < g.W; x += T) conf_full[fo + (size_t)y * g.W + x] = 255.0f;
        return;
    }
    const int rw = g.rw, r = g.radius;
    int64_t* V2 = wls_smem;                // [2][rw] column sums of d^2 (left, right)
    int* V = (int*)(V2 + 2 * rw);          // [2][rw] column sums of d
    float* disc = (float*)(V + 2 * rw);    // [2][rw] discontinuity values
    const int16_t* L = dl + fo;
    const int16_t* R = dr + fo;
    // the window's rows (wave-uniform: one image row per workgroup), then all 2(2r+1) loads of a
    // column at once: RMAX taps unrolled, those past the radius loading a duplicate row and masked
    // (a runtime-length tap loop issued its loads one iteration at a time)
    size_t rowo[2 * RMAX + 1];
#pragma unroll
    for (int t = 0; t <= 2 * RMAX; t++)
        rowo[t] = (size_t)(g.ry + reflect101(i + min(max(t - RMAX, -r), r), g.rh)) * g.W;
    // the row's FGS weights from the guide (k_fgs_weights' formulas; the sequential solver's
    // layouts: Ch at j*hp + i, Cv at i*wp + j, fgs_pad4), computed in the first phase's column loop
    // so that their loads share its round trips
    const uint8_t* gr = guide + (size_t)f * gfstride + (size_t)(g.ry + i) * gstride + g.rx;
    const int wp = ch_rowmajor ? rw : fgs_pad4(rw), hp = ch_rowmajor ? g.rh : fgs_pad4(g.rh);
    const size_t wfo = (size_t)f * wp * hp;
    const int gs = i + 1 < g.rh ? (int)gstride : 0;
    for (int j = tid; j < rw; j += T) {
        int vl[2 * RMAX + 1], vr[2 * RMAX + 1];
        const int gv = gr[j], gh = gr[min(j + 1, rw - 1)], gd = gr[gs + j];
#pragma unroll
        for (int t = 0; t <= 2 * RMAX; t++) {
            vl[t] = L[rowo[t] + g.rx + j];
            vr[t] = R[rowo[t] + g.rrx + j];
        }
        {
            // (unconditional lookups from clamped neighbours, then the edges' zeros)
            const int dh = gv - gh, dv = gv - gd;
            const float ch = lut[dh * dh], cv = lut[dv * dv];
            ChW[wfo + (ch_rowmajor ? (size_t)i * rw + j : (size_t)j * hp + i)] = j + 1 < rw ? ch : 0.0f;
            Cv[wfo + (size_t)i * wp + j] = gs ? cv : 0.0f;
        }
        int s0 = 0, s1 = 0;
        int64_t q0 = 0, q1 = 0;
#pragma unroll
        for (int t = 0; t <= 2 * RMAX; t++) {
            const int a = t - RMAX;
            const int ml = a >= -r && a <= r ? vl[t] : 0, mr = a >= -r && a <= r ? vr[t] : 0;
            s0 += ml;
            q0 += (int64_t)ml * ml;
            s1 += mr;
            q1 += (int64_t)mr * mr;
        }
        V[j] = s0;
        V[rw + j] = s1;
        V2[j] = q0;
        V2[rw + j] = q1;
    }
    __syncthreads();
    // BORDER_REFLECT_101 of a column index one reflection deep (rw > RMAX; narrower ROIs loop)
    const bool shallow = rw > RMAX;
    auto refl = [&](int p) { return shallow ? (p < 0 ? -p : p >= rw ? 2 * rw - 2 - p : p) : reflect101(p, rw); };
    for (int j = tid; j < rw; j += T) {
#pragma unroll
        for (int m = 0; m < 2; m++) {
            long long s = 0, s2 = 0;
#pragma unroll
            for (int t = 0; t <= 2 * RMAX; t++) {
                const int b = t - RMAX;
                if (b < -r || b > r) continue;  // uniform
                const int jj = refl(j + b);
                s += V[m * rw + jj];
                s2 += V2[m * rw + jj];
            }
            const float mean = (float)((double)s * g.scale);
            const float msq = (float)((double)s2 * g.scale);
            const float var = msq - mean * mean;
            const float c = 1.0f - g.roll_off * var;
            disc[m * rw + j] = c > 0.0f ? c : 0.0f;
        }
    }
    __syncthreads();
    const size_t cf = (size_t)f * rw * g.rh + (size_t)i * rw;
    for (int x = tid; x < g.W; x += T) {
        const size_t o = (size_t)y * g.W + x;
        const int j = x - g.rx;
        const bool in_roi = j >= 0 && j < rw;
        float c = 1.0f;
        int v = 0;
        if (in_roi) {
            c = disc[j];
            v = L[o];
            const int ridx = x - (v >> 4);
            if (ridx >= g.rrx && ridx < g.rrx + rw) {
                if (abs(v + (int)R[(size_t)y * g.W + ridx]) < g.lrc_thresh) {
                    const float rc = disc[rw + ridx - g.rrx];
                    c = c < rc ? c : rc;
                } else {
                    c = 0.0f;
                }
            }
        }
        const float conf = 255.0f * c;
        if (conf_full) conf_full[fo + o] = conf;
        if (in_roi) {
            if (ch_rowmajor) {
                A[cf + j] = conf * (float)v;
                B[cf + j] = conf;
            } else {
                // the sequential solver's first pass reads them transposed ([column][row]), the two
                // right-hand sides interleaved (A is its pass buffer, B unused)
                ((float2*)A)[(size_t)f * fgs_pad4(rw) * fgs_pad4(g.rh) + (size_t)j * fgs_pad4(g.rh) + i] =
                    make_float2(conf * (float)v, conf);
            }
        }
    }

}

// saturate_cast<short>(float): round half to even, saturate; 0 where FGS(conf) == 0 (cv::divide
// of floats returns 0 for a zero divisor)
// Optional epilogue of the class path (stereo_disparity.cpp:34, :76-80), fused: fout = out / 16
// (convertTo(CV_32F, 1/16)) and xyz = reprojectImageTo3D(fout, Q) (computeDepth,
// handleMissing = false).
__global__ __launch_bounds__(256) void k_wls_final(const float* __restrict__ A,
                                                   const float* __restrict__ B, WlsGeom g, WlsOut wo) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    const int j = x - g.rx, i = y - g.ry;
    int16_t r = (int16_t)g.fill;
    if (j >= 0 && j < g.rw && i >= 0 && i < g.rh) {
        const size_t co = (size_t)blockIdx.z * g.rw * g.rh + (size_t)i * g.rw + j;
        r = wls_value(A[co], B[co]);
    }
    wls_emit(wo, g, blockIdx.z, x, y, r);
}

// FastGlobalSmootherFilter::filter on R0 (and R1 when non-null: a second right-hand side of the
// same systems), row-major w x h per frame, F frames with per-frame guides, in place.
//   SDR_FGS_THOMAS: weights (ChT column-major = the row pass's k-major, Cv row-major = the column
//                   pass's), the right-hand sides transposed into s.A (in_transposed: the caller
//                   already wrote them there), one launch of coefficient jobs (every pass's
//                   (a, den, 1/den, t)), then the passes alternating between the two layouts (row
//                   pass: s.A -> s.B, column pass: s.B -> s.A; the last column pass into R0 / R1):
//                   2 * iters + 1 launches, each on the kernel fgs_plan names (sdr_fgs_seq.hip)
//   SDR_FGS_PCR:    weights (Ch, Cv row-major), then per iteration k_fgs_pcr over the rows and
//                   over the columns of the images themselves (2 launches per iteration)
static int launch_fgs(const uint8_t* guide, size_t gstride, size_t gfstride, const float* lut,
                      float* R0, float* R1, int w, int h, int F, double lambda, double att,
                      int iters, int solver, const FgsScratch& s, hipStream_t st,
                      bool weights_ready = false, sdr_sgbm* timer = nullptr,
                      const WlsGeom* fin_g = nullptr, const WlsOut* fin_o = nullptr,
                      bool in_transposed = false) {
    const size_t fs = (size_t)w * h;
    const bool pcr = solver == SDR_FGS_PCR;
    if (!weights_ready)
        hipLaunchKernelGGL(k_fgs_weights, dim3((w + 63) / 64, (h + 3) / 4, F), dim3(256), 0, st, guide,
                           gstride, gfstride, lut, w, h, pcr ? 1 : 0, s.ChT, s.Cv);
    float lam = (float)lambda;
    const float fa = (float)att;
    if (!pcr) {
        if (iters <= 0) return 0;
        const bool two = R1 != nullptr;
        if (!in_transposed)
            hipLaunchKernelGGL(k_fgs_pack, dim3((w + 63) / 64, (h + 63) / 64, F), dim3(256), 0, st, R0, R1, s.A, h, w);
        const int npass = 2 * iters;
        // pass p: iteration p / 2, rows (even p: lines = rows, k = column) or columns (odd p);
        // k-major arrays with sample rows of fgs_pad4(lines)
        const int wp = fgs_pad4(w), hp = fgs_pad4(h);
        const size_t fsp = (size_t)wp * hp;
        std::vector<float> lams(iters);
        for (int it = 0; it < iters; it++, lam = lam * fa) lams[it] = lam;  // lambda *= attenuation
        auto pass_args = [&](int p) {
            FgsThArgs a{};
            const bool rows = (p & 1) == 0;
            fgs_pass_shape(p, w, h, &a.nl, &a.n);
            a.st = rows ? hp : wp;
            a.onp = rows ? wp : hp;
            a.fs = fsp;
            a.ost = (size_t)w;
            a.ofs = fs;
            // rows: transposed (s.A) -> row-major (s.B); columns: row-major (s.B) -> transposed (s.A),
            // the last pass split back into R0 / R1
            a.U = rows ? s.A : s.B;
            const bool last = p == npass - 1;
            a.O = last ? nullptr : rows ? s.B : s.A;
            a.O0 = last ? R0 : nullptr;
            a.O1 = last ? R1 : nullptr;
            // the pass's coefficient block: float4 (a, den, 1/den, t), then t alone
            float* cb = s.coef + (size_t)p * 5 * F * fsp;
            a.coef = (const float4*)cb;
            a.tt = cb + 4 * F * fsp;
            return a;
        };
        // the coefficient jobs of every pass (kFgsMaxJobs a launch), then the passes, each on the
        // kernel the plan names
        const FgsPlan plan = fgs_plan(w, h, F, two, iters, device_cus());
        for (int p0 = 0; p0 < npass; p0 += kFgsMaxJobs) {
            FgsThArgs c{};
            c.fs = fsp;
            for (int p = p0; p < npass && c.njobs < kFgsMaxJobs; p++) {
                const FgsThArgs q = pass_args(p);
                const bool rows = (p & 1) == 0;
                FgsCoefJob& j = c.job[c.njobs++];
                j.Cw = rows ? s.ChT : s.Cv;
                j.coef = (float4*)q.coef;
                j.tt = (float*)q.tt;
                j.lam = lams[p / 2];
                j.nl = q.nl;
                j.n = q.n;
                j.st = q.st;
            }
            KScope kt(timer, SDR_KERNEL_FGS_COEF);
            launch_fgs_jobs(c, &plan.job[p0], two, F, st);
        }
        for (int p = 0; p < npass; p++) {
            KScope kt(timer, SDR_KERNEL_FGS);
            launch_fgs_pass(pass_args(p), plan.pass[p], two, F, st);
        }
        return 0;
    }
    for (int it = 0; it < iters; it++) {
        for (int rows = 1; rows >= 0; rows--) {
            KScope kt(timer, SDR_KERNEL_FGS);
            // the last column pass writes the filter's outputs itself (fin_g / fin_o)
            const bool fin = !rows && fin_g && R1 && it == iters - 1;
            if (launch_pcr(R0, R1, rows ? s.ChT : s.Cv, w, h, F, rows, lam, st, fin ? fin_g : nullptr,
                           fin ? fin_o : nullptr))
                return -1;
        }
        lam = lam * fa;  // FastGlobalSmootherFilterImpl::filter: lambda *= lambda_attenuation
    }
    return 0;
}

// ComputeLUT_ParBody: LUT[i] = -exp(-sqrt((float)i) / sigmaColor), float math on the host
static void fgs_lut_host(double sigma, std::vector<float>* lut) {
    lut->resize(kFgsLevels);
    const float s = (float)sigma;
    for (int i = 0; i < kFgsLevels; i++) (*lut)[i] = -expf(-sqrtf((float)i) / s);
}

}  // namespace sdr

// ===========================================================================================
// C ABI (include/sdr/sdr.h)
// ===========================================================================================
struct sdr_wls {
    sdr_wls_params p{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    sdr::Buf rdisc, conf, A, B, Ac, Bc, ChT, Cv, lut, out, hbuf, coef;
    double lut_sigma = -1.0;
};

namespace {

// The sequential solver's exact division needs every pass's pivots in [1, 2^126): each pass's
// lambda (lambda * attenuation^k, in launch_fgs's float arithmetic) in [0, kFgsThomasMaxLambda]
// (an attenuation above 1 or below 0 used to pass with only the first checked)
bool thomas_lambdas_ok(double lambda, double att, int iters) {
    float lam = (float)lambda;
    const float fa = (float)att;
    for (int it = 0; it < iters; it++, lam = lam * fa)
        if (!(lam >= 0.0f) || !((double)lam <= sdr::kFgsThomasMaxLambda)) return false;
    return true;
}
constexpr const char* kThomasLambdaMsg =
    "SDR_FGS_THOMAS needs every pass's lambda * attenuation^k in [0, 2^100] (its pivots stay in [1, 2^126))";

int check_wls_params(const sdr_wls_params& p) {
    if (!(p.lambda >= 0.0) || !(p.sigma_color >= 0.0) || p.num_iter < 1)
        return sdr::set_error(SDR_ERR_ARG, "FGS needs lambda >= 0, sigma_color >= 0, num_iter >= 1");
    if (p.fgs_solver == SDR_FGS_THOMAS && !thomas_lambdas_ok(p.lambda, p.lambda_attenuation, p.num_iter))
        return sdr::set_error(SDR_ERR_ARG, kThomasLambdaMsg);
    if (p.fgs_solver != SDR_FGS_PCR && p.fgs_solver != SDR_FGS_THOMAS)
        return sdr::set_error(SDR_ERR_ARG, "fgs_solver must be SDR_FGS_PCR or SDR_FGS_THOMAS");
    if (p.depth_discontinuity_radius < 0 || p.left_offset < 0 || p.right_offset < 0 ||
        p.top_offset < 0 || p.bottom_offset < 0)
        return sdr::set_error(SDR_ERR_ARG, "negative WLS radius or offset");
    return SDR_OK;
}

int upload_lut(sdr_wls* h, double sigma, const float** out) {
    int rc;
    if ((rc = sdr::ensure(h->lut, sizeof(float) * sdr::kFgsLevels))) return rc;
    if (h->lut_sigma != sigma) {
        std::vector<float> lut;
        sdr::fgs_lut_host(sigma, &lut);
        SDR_HIP(hipMemcpy(h->lut.p, lut.data(), sizeof(float) * lut.size(), hipMemcpyHostToDevice));
        h->lut_sigma = sigma;
    }
    *out = (const float*)h->lut.p;
    return SDR_OK;
}

}  // namespace

extern "C" {

void sdr_wls_params_for_sgbm(sdr_sgbm_params* m, sdr_wls_params* p) {
    if (!m || !p) return;
    // createDisparityWLSFilter(Ptr<StereoMatcher>) [ximgproc disparity_filters.cpp]:
    // setDisp12MaxDiff(1000000), setSpeckleWindowSize(0), and for SGBM setUniquenessRatio(0);
    // offsets (max(0, minD+numD), max(0, -minD), 0, 0); radius ceil(0.5 * blockSize)
    m->disp12MaxDiff = 1000000;
    m->speckleWindowSize = 0;
    m->uniquenessRatio = 0;
    const int l = m->minDisparity + m->numDisparities;
    p->lambda = 8000.0;
    p->sigma_color = 1.5;
    p->lrc_thresh = 24;
    p->depth_discontinuity_radius = (int)std::ceil(0.5 * m->blockSize);
    p->roll_off = 0.001f;
    p->lambda_attenuation = 0.25;
    p->num_iter = 3;
    p->left_offset = l > 0 ? l : 0;
    p->right_offset = m->minDisparity < 0 ? -m->minDisparity : 0;
    p->top_offset = 0;
    p->bottom_offset = 0;
    p->min_disp = m->minDisparity;
    p->fgs_solver = SDR_FGS_THOMAS;  // ximgproc's own elimination order (sdr.h)
}

int sdr_wls_create(const sdr_wls_params* p, int device, sdr_wls** out) {
    if (!p || !out) return sdr::set_error(SDR_ERR_ARG, "null argument");
    int rc = check_wls_params(*p);
    if (rc) return rc;
    SDR_HIP(hipSetDevice(device));
    sdr_wls* h = new sdr_wls();
    h->p = *p;
    h->device = device;
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return sdr::set_error(SDR_ERR_DEVICE, "hipStreamCreate failed");
    }
    h->stream = h->own_stream;
    *out = h;
    return SDR_OK;
}

int sdr_wls_destroy(sdr_wls* h) {
    if (!h) return SDR_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (sdr::Buf* b : {&h->rdisc, &h->conf, &h->A, &h->B, &h->Ac, &h->Bc, &h->ChT, &h->Cv,
                        &h->lut, &h->out, &h->hbuf, &h->coef})
        if (b->p) (void)hipFree(b->p);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return SDR_OK;
}

int sdr_wls_set_params(sdr_wls* h, const sdr_wls_params* p) {
    if (!h || !p) return sdr::set_error(SDR_ERR_ARG, "null argument");
    int rc = check_wls_params(*p);
    if (rc) return rc;
    h->p = *p;
    return SDR_OK;
}

int sdr_wls_get_params(const sdr_wls* h, sdr_wls_params* p) {
    if (!h || !p) return sdr::set_error(SDR_ERR_ARG, "null argument");
    *p = h->p;
    return SDR_OK;
}

int sdr_wls_set_stream(sdr_wls* h, void* stream) {
    if (!h) return sdr::set_error(SDR_ERR_ARG, "null handle");
    h->stream = (hipStream_t)stream;  // NULL = the HIP null (legacy default) stream
    return SDR_OK;
}

int sdr_wls_reset_stream(sdr_wls* h) {
    if (!h) return sdr::set_error(SDR_ERR_ARG, "null handle");
    h->stream = h->own_stream;
    return SDR_OK;
}

void* sdr_wls_get_stream(const sdr_wls* h) { return h ? (void*)h->stream : nullptr; }

int sdr_wls_get_roi(const sdr_wls* h, int W, int H, int roi[4]) {
    if (!h || !roi) return sdr::set_error(SDR_ERR_ARG, "null argument");
    roi[0] = h->p.left_offset;
    roi[1] = h->p.top_offset;
    roi[2] = W - h->p.left_offset - h->p.right_offset;
    roi[3] = H - h->p.top_offset - h->p.bottom_offset;
    return SDR_OK;
}

}  // extern "C"

// DisparityWLSFilter::filter on device with the class path's optional fused epilogue (fout =
// out / 16, xyz = reprojectImageTo3D(fout, Q)); sdr_wls_filter_device is this with neither.
// ROIs up to kPcrMaxN columns take the fused front end (k_wls_prep: discontinuity maps, LR check,
// confidence, FGS weights in one launch); wider ones the per-pixel k_wls_disc / k_wls_conf /
// k_fgs_weights kernels.
int sdr::wls_filter_enqueue(sdr_wls* h, const int16_t* dl, const int16_t* dr, const uint8_t* guide,
                            int W, int H, size_t gstride, size_t gfstride, int F, int16_t* out,
                            float* conf, float* fout, const double* Q, float* xyz, sdr_sgbm* timer) {
    if (!h || !dl || !dr || !guide || !out) return sdr::set_error(SDR_ERR_ARG, "null argument");
    if (W <= 0 || H <= 0 || F <= 0 || gstride < (size_t)W || (F > 1 && gfstride < gstride * H))
        return sdr::set_error(SDR_ERR_ARG, "bad size/stride");
    if (xyz && (!fout || !Q)) return sdr::set_error(SDR_ERR_ARG, "the fused reprojection needs fout and Q");
    SDR_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const sdr_wls_params& p = h->p;
    sdr::WlsGeom g{};
    g.W = W;
    g.H = H;
    g.rx = p.left_offset;
    g.ry = p.top_offset;
    g.rw = W - p.left_offset - p.right_offset;
    g.rh = H - p.top_offset - p.bottom_offset;
    g.rrx = W - (g.rx + g.rw);
    g.radius = p.depth_discontinuity_radius;
    const int k = 2 * g.radius + 1;
    g.scale = 1.0 / (double)(k * k);
    g.roll_off = p.roll_off;
    g.lrc_thresh = p.lrc_thresh;
    g.fill = 16 * (p.min_disp - 1);
    const size_t px = (size_t)W * H;
    const bool roi = g.rw > 0 && g.rh > 0;
    if (roi && p.fgs_solver == SDR_FGS_PCR && (g.rw > sdr::kPcrMaxN || g.rh > sdr::kPcrMaxN))
        return sdr::set_error(SDR_ERR_SIZE, "SDR_FGS_PCR solves lines of at most 4096 samples "
                                            "(use SDR_FGS_THOMAS for larger ROIs)");
    const bool fused = roi && g.rw <= sdr::kPcrMaxN && g.radius <= 9;
    const size_t cpx = roi ? (size_t)g.rw * g.rh : 0;
    int rc;
    const float* lut = nullptr;
    if (!fused && (rc = sdr::ensure(h->rdisc, F * px * 4))) return rc;
    // the sequential solver's k-major arrays: sample rows padded to 4 lines (fgs_pad4), and room
    // for its loaders' reads past the last row (kFgsOverread)
    const size_t cpp = roi ? (size_t)sdr::fgs_pad4(g.rw) * sdr::fgs_pad4(g.rh) : 0;
    const size_t ov = sdr::kFgsOverread;
    for (sdr::Buf* b : {&h->A, &h->B})
        if ((rc = sdr::ensure(*b, F * cpx * 4 + 4))) return rc;
    for (sdr::Buf* b : {&h->ChT, &h->Cv})
        if ((rc = sdr::ensure(*b, F * cpp * 4 + ov))) return rc;
    if (p.fgs_solver == SDR_FGS_THOMAS) {
        // the two pass layouts (both right-hand sides interleaved) and every pass's elimination
        // coefficients (float4 (a, den, 1/den, t) and t: 20 bytes a sample and pass)
        for (sdr::Buf* b : {&h->Ac, &h->Bc})
            if ((rc = sdr::ensure(*b, F * cpp * 8 + ov))) return rc;
        if ((rc = sdr::ensure(h->coef, (size_t)std::max(2 * p.num_iter, 0) * F * cpp * 20 + ov))) return rc;
    }
    if ((rc = upload_lut(h, p.sigma_color, &lut))) return rc;
    float* A = (float*)h->A.p;
    float* B = (float*)h->B.p;
    const dim3 blk(256);
    const bool rowmajor = p.fgs_solver == SDR_FGS_PCR;
    // the sequential solver's first pass (rows) reads the right-hand sides transposed: the fused
    // front end writes them there directly
    float* Ain = rowmajor ? A : (float*)h->Ac.p;
    float* Bin = rowmajor ? B : nullptr;
    const dim3 grid((W + 63) / 64, (H + 3) / 4, F);
    sdr::WlsOut wo{out, fout, xyz, {}};
    if (Q)
        for (int t = 0; t < 16; t++) wo.Q.q[t] = Q[t];
    // with the default solver the outputs need no pass of their own: k_wls_prep writes the pixels
    // outside the ROI and the last FGS column pass the ROI's (k_wls_final otherwise)
    const bool fin_fused = fused && roi && p.fgs_solver == SDR_FGS_PCR;
    if (fused) {
        sdr::KScope kt(timer, SDR_KERNEL_WLS_PREP);
        // the window radius is ceil(blockSize / 2) <= 9 for every valid SGBM block; wider ones
        // (setDepthDiscontinuityRadius) take the per-pixel kernels below
        auto* prep = g.radius <= 4 ? sdr::k_wls_prep<4> : sdr::k_wls_prep<9>;
        hipLaunchKernelGGL(prep, dim3(H, F), blk, (size_t)g.rw * 32, st, dl, dr, g, guide, gstride, gfstride, lut,
                           rowmajor ? 1 : 0, conf, Ain, Bin, (float*)h->ChT.p, (float*)h->Cv.p, fin_fused ? 1 : 0, wo);
    } else {
        sdr::KScope kt(timer, SDR_KERNEL_WLS_PREP);
        if (roi)
            hipLaunchKernelGGL(sdr::k_wls_disc, dim3((g.rw + 63) / 64, (g.rh + 3) / 4, F), blk, 0, st,
                               dr, g, (float*)h->rdisc.p);
        hipLaunchKernelGGL(sdr::k_wls_conf, grid, blk, 0, st, dl, dr, (const float*)h->rdisc.p, g,
                           conf, A, B);
    }
    if (roi) {
        const uint8_t* g0 = guide + (size_t)g.ry * gstride + g.rx;
        const sdr::FgsScratch fs{(float*)h->Ac.p, (float*)h->Bc.p, (float*)h->ChT.p,
                                 (float*)h->Cv.p, (float*)h->coef.p};
        if (sdr::launch_fgs(g0, gstride, gfstride, lut, A, B, g.rw, g.rh, F, p.lambda,
                            p.lambda_attenuation, p.num_iter, p.fgs_solver, fs, st, fused, timer,
                            fin_fused ? &g : nullptr, fin_fused ? &wo : nullptr, fused && !rowmajor))
            return sdr::set_error(SDR_ERR_SIZE, "SDR_FGS_PCR solves lines of at most 4096 samples "
                                                "(use SDR_FGS_THOMAS for larger ROIs)");
        if (fin_fused) {
            SDR_HIP(hipGetLastError());
            return SDR_OK;
        }
    }
    {
        sdr::KScope kt(timer, SDR_KERNEL_WLS_FINAL);
        hipLaunchKernelGGL(sdr::k_wls_final, grid, blk, 0, st, A, B, g, wo);
    }
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

extern "C" {

int sdr_wls_filter_device(sdr_wls* h, const int16_t* dl, const int16_t* dr, const uint8_t* guide,
                          int W, int H, size_t gstride, size_t gfstride, int F, int16_t* out,
                          float* conf) {
    return sdr::wls_filter_enqueue(h, dl, dr, guide, W, H, gstride, gfstride, F, out, conf, nullptr,
                                   nullptr, nullptr);
}

int sdr_wls_filter(sdr_wls* h, const int16_t* dl, const int16_t* dr, const uint8_t* guide, int W,
                   int H, size_t gstride, int16_t* out, float* conf) {
    if (!h || !dl || !dr || !guide || !out) return sdr::set_error(SDR_ERR_ARG, "null argument");
    if (W <= 0 || H <= 0 || gstride < (size_t)W) return sdr::set_error(SDR_ERR_ARG, "bad size/stride");
    SDR_HIP(hipSetDevice(h->device));
    const size_t px = (size_t)W * H;
    // device staging: dl, dr, guide, out (int16), conf (float)
    int rc;
    if ((rc = sdr::ensure(h->hbuf, px * (2 + 2 + 1 + 2 + 4) + 64))) return rc;
    uint8_t* base = (uint8_t*)h->hbuf.p;
    float* dconf = (float*)base;
    int16_t* ddl = (int16_t*)(base + px * 4);
    int16_t* ddr = ddl + px;
    int16_t* dout = ddr + px;
    uint8_t* dg = (uint8_t*)(dout + px);
    hipStream_t st = h->stream;
    SDR_HIP(hipMemcpyAsync(ddl, dl, px * 2, hipMemcpyHostToDevice, st));
    SDR_HIP(hipMemcpyAsync(ddr, dr, px * 2, hipMemcpyHostToDevice, st));
    SDR_HIP(hipMemcpy2DAsync(dg, W, guide, gstride, W, H, hipMemcpyHostToDevice, st));
    if ((rc = sdr_wls_filter_device(h, ddl, ddr, dg, W, H, W, px, 1, dout, conf ? dconf : nullptr)))
        return rc;
    SDR_HIP(hipMemcpyAsync(out, dout, px * 2, hipMemcpyDeviceToHost, st));
    if (conf) SDR_HIP(hipMemcpyAsync(conf, dconf, px * 4, hipMemcpyDeviceToHost, st));
    SDR_HIP(hipStreamSynchronize(st));
    return SDR_OK;
}

int sdr_fgs_filter_device(const uint8_t* d_guide, size_t gstride, int w, int h, double lambda,
                          double sigma, double att, int iters, float* d_img, int nimg,
                          int solver, void* stream) {
    if (!d_guide || !d_img) return sdr::set_error(SDR_ERR_ARG, "null argument");
    if (w <= 0 || h <= 0 || nimg <= 0 || gstride < (size_t)w)
        return sdr::set_error(SDR_ERR_ARG, "bad size/stride");
    if (!(lambda >= 0.0) || !(sigma >= 0.0) || iters < 1)
        return sdr::set_error(SDR_ERR_ARG, "FGS needs lambda >= 0, sigma_color >= 0, num_iter >= 1");
    if (solver == SDR_FGS_THOMAS && !thomas_lambdas_ok(lambda, att, iters))
        return sdr::set_error(SDR_ERR_ARG, kThomasLambdaMsg);
    if (solver != SDR_FGS_PCR && solver != SDR_FGS_THOMAS)
        return sdr::set_error(SDR_ERR_ARG, "solver must be SDR_FGS_PCR or SDR_FGS_THOMAS");
    if (solver == SDR_FGS_PCR && (w > sdr::kPcrMaxN || h > sdr::kPcrMaxN))
        return sdr::set_error(SDR_ERR_SIZE, "SDR_FGS_PCR solves lines of at most 4096 samples "
                                            "(use SDR_FGS_THOMAS for larger images)");
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> lut;
    sdr::fgs_lut_host(sigma, &lut);
    // stream-ordered scratch: LUT, column-major copies, coefficients, weights
    float* dlut = nullptr;
    float* scr = nullptr;
    const size_t px = (size_t)w * h;
    // (frames of the sequential solver's padded layouts: fgs_pad4(w) * fgs_pad4(h) >= px samples)
    const size_t fp = (size_t)sdr::fgs_pad4(w) * sdr::fgs_pad4(h);
    SDR_HIP(sdr::scratch_alloc((void**)&dlut, sizeof(float) * lut.size(), st));
    // (FgsScratch: the sequential solver's two interleaved pass layouts, the weights, and 5 floats
    // a sample for each of its 2 * iters passes' coefficients; its loaders read up to
    // kFgsOverread bytes past an array)
    const size_t ncoef = solver == SDR_FGS_THOMAS ? (size_t)5 * (2 * iters) : 0;
    SDR_HIP(sdr::scratch_alloc((void**)&scr, sizeof(float) * fp * (6 + ncoef) + sdr::kFgsOverread, st));
    SDR_HIP(hipMemcpyAsync(dlut, lut.data(), sizeof(float) * lut.size(), hipMemcpyHostToDevice, st));
    const sdr::FgsScratch fs{scr, scr + 2 * fp, scr + 4 * fp, scr + 5 * fp, scr + 6 * fp};
    // images are filtered in pairs (two right-hand sides of one system per line)
    for (int i = 0; i < nimg; i += 2) {
        const int m = nimg - i >= 2 ? 2 : 1;
        (void)sdr::launch_fgs(d_guide, gstride, 0, dlut, d_img + i * px, m == 2 ? d_img + (i + 1) * px : nullptr,
                              w, h, 1, lambda, att, iters, solver, fs, st);
    }
    SDR_HIP(hipGetLastError());
    SDR_HIP(sdr::scratch_free(dlut, st));
    SDR_HIP(sdr::scratch_free(scr, st));
    // the host LUT vector dies here: wait for its upload before returning
    SDR_HIP(hipStreamSynchronize(st));
    return SDR_OK;
}

int sdr_fgs_plan_query(int w, int h, int nframes, int nimg, int num_iter, int solver, int cus,
                       sdr_fgs_plan* out) {
    if (!out) return sdr::set_error(SDR_ERR_ARG, "null argument");
    if (w <= 0 || h <= 0 || nframes <= 0 || num_iter < 1 || cus < 0 || (nimg != 1 && nimg != 2))
        return sdr::set_error(SDR_ERR_ARG, "bad size, nimg other than 1 or 2, num_iter < 1 or cus < 0");
    if (solver != SDR_FGS_PCR && solver != SDR_FGS_THOMAS)
        return sdr::set_error(SDR_ERR_ARG, "solver must be SDR_FGS_PCR or SDR_FGS_THOMAS");
    *out = sdr_fgs_plan{};
    if (solver == SDR_FGS_PCR) {
        if (w > sdr::kPcrMaxN || h > sdr::kPcrMaxN)
            return sdr::set_error(SDR_ERR_SIZE, "SDR_FGS_PCR solves lines of at most 4096 samples");
        out->row_pass = {SDR_FGS_KERNEL_PCR, sdr::pcr_lines(w, h)};
        out->col_pass = {SDR_FGS_KERNEL_PCR, sdr::pcr_lines(h, w)};
        return SDR_OK;
    }
    if (!cus) cus = sdr::device_cus();
    out->cus = cus;
    // the plan launch_fgs runs: its first row and column pass, and their jobs in the first job launch
    const sdr::FgsPlan plan = sdr::fgs_plan(w, h, nframes, nimg == 2, num_iter, cus);
    out->row_pass = plan.pass[0];
    out->col_pass = plan.pass[1];
    out->row_job = plan.job[0];
    out->col_job = plan.job[1];
    return SDR_OK;
}

}  // extern "C"
