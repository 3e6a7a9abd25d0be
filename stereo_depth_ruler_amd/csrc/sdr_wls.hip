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
//   k_wls_final    FGS(conf*d) / FGS(conf) -> saturate_cast<short>, 16*(min_disp-1) outside ROI
// The FGS line solves are in sdr_fgs_seq.hip (SDR_FGS_THOMAS, the default) and sdr_fgs_pcr.hip
// (SDR_FGS_PCR).  After the kernels come the stage launchers of a planned call (sdr_wls_plan.hpp):
// wls_front, launch_fgs, wls_back; the handle and the C ABI that run them are in
// sdr_wls_entries.hip.
#include "sdr_internal.hpp"
#include "sdr_wls_plan.hpp"

#pragma clang fp contract(off)

namespace sdr {

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

// ---- the stages of a planned call (sdr_wls_plan.hpp), in launch order ----

// The front end: the confidence map and the FGS right-hand sides.  Fused (k_wls_prep) it also
// writes the row's FGS weights and, when the outputs are fused too, the pixels outside the ROI.
void wls_front(const WlsPlan& pl, const WlsBufs& b, hipStream_t st, sdr_sgbm* timer) {
    const WlsGeom& g = pl.g;
    const dim3 blk(256);
    KScope kt(timer, SDR_KERNEL_WLS_PREP);
    if (pl.fused) {
        auto* prep = g.radius <= 4 ? k_wls_prep<4> : k_wls_prep<9>;
        // the sequential solver's first pass (rows) reads the right-hand sides transposed and
        // interleaved: k_wls_prep writes them into its pass buffer directly
        float* Ain = pl.rowmajor ? b.R0 : b.s.A;
        float* Bin = pl.rowmajor ? b.R1 : nullptr;
        hipLaunchKernelGGL(prep, dim3(g.H, pl.F), blk, (size_t)g.rw * 32, st, b.dl, b.dr, g, b.guide, b.gstride,
                           b.gfstride, b.lut, pl.rowmajor ? 1 : 0, b.conf, Ain, Bin, b.s.ChT, b.s.Cv,
                           pl.fin_fused ? 1 : 0, b.out);
        return;
    }
    if (pl.roi)
        hipLaunchKernelGGL(k_wls_disc, dim3((g.rw + 63) / 64, (g.rh + 3) / 4, pl.F), blk, 0, st, b.dr, g, b.rdisc);
    hipLaunchKernelGGL(k_wls_conf, dim3((g.W + 63) / 64, (g.H + 3) / 4, pl.F), blk, 0, st, b.dl, b.dr,
                       (const float*)b.rdisc, g, b.conf, b.R0, b.R1);
}

// Pass p of the sequential solver: iteration p / 2, rows (even p: lines = rows, k = column) or
// columns (odd p); k-major arrays with sample rows of fgs_pad4(lines)
static FgsThArgs pass_args(const WlsPlan& pl, const WlsBufs& b, int p) {
    const int w = pl.g.rw, h = pl.g.rh, wp = fgs_pad4(w), hp = fgs_pad4(h);
    FgsThArgs a{};
    const bool rows = (p & 1) == 0;
    fgs_pass_shape(p, w, h, &a.nl, &a.n);
    a.st = rows ? hp : wp;
    a.onp = rows ? wp : hp;
    a.fs = pl.fsp;
    a.ost = (size_t)w;
    a.ofs = (size_t)w * h;
    // rows: transposed (s.A) -> row-major (s.B); columns: row-major (s.B) -> transposed (s.A),
    // the last pass split back into R0 / R1
    a.U = rows ? b.s.A : b.s.B;
    const bool last = p == 2 * pl.iters - 1;
    a.O = last ? nullptr : rows ? b.s.B : b.s.A;
    a.O0 = last ? b.R0 : nullptr;
    a.O1 = last ? b.R1 : nullptr;
    // the pass's coefficient block: float4 (a, den, 1/den, t), then t alone
    float* cb = b.s.coef + pl.coef_off(p);
    a.coef = (const float4*)cb;
    a.tt = cb + 4 * pl.F * pl.fsp;
    return a;
}

// SDR_FGS_THOMAS: the right-hand sides transposed into s.A (fused: k_wls_prep already wrote them
// there), the coefficient jobs of every pass ((a, den, 1/den, t), kFgsMaxJobs a launch), then the
// passes alternating between the two layouts (row pass: s.A -> s.B, column pass: s.B -> s.A; the
// last column pass into R0 / R1): 2 * iters + 1 launches, each on the kernel the plan names
// (sdr_fgs_seq.hip)
static void fgs_thomas(const WlsPlan& pl, const WlsBufs& b, hipStream_t st, sdr_sgbm* timer) {
    const int w = pl.g.rw, h = pl.g.rh, F = pl.F, npass = 2 * pl.iters;
    if (!pl.fused)
        hipLaunchKernelGGL(k_fgs_pack, dim3((w + 63) / 64, (h + 63) / 64, F), dim3(256), 0, st, b.R0, b.R1, b.s.A, h, w);
    for (int p0 = 0; p0 < npass; p0 += kFgsMaxJobs) {
        FgsThArgs c{};
        c.fs = pl.fsp;
        for (int p = p0; p < npass && c.njobs < kFgsMaxJobs; p++) {
            const FgsThArgs q = pass_args(pl, b, p);
            FgsCoefJob& j = c.job[c.njobs++];
            j.Cw = (p & 1) == 0 ? b.s.ChT : b.s.Cv;
            j.coef = (float4*)q.coef;
            j.tt = (float*)q.tt;
            j.lam = pl.lam[p / 2];
            j.nl = q.nl;
            j.n = q.n;
            j.st = q.st;
        }
        KScope kt(timer, SDR_KERNEL_FGS_COEF);
        launch_fgs_jobs(c, &pl.fgs.job[p0], pl.two, F, st);
    }
    for (int p = 0; p < npass; p++) {
        KScope kt(timer, SDR_KERNEL_FGS);
        launch_fgs_pass(pass_args(pl, b, p), pl.fgs.pass[p], pl.two, F, st);
    }
}

// SDR_FGS_PCR: per iteration k_fgs_pcr over the rows and over the columns of the images themselves
// (2 launches per iteration); fused, the last column pass writes the filter's outputs itself.
// launch_pcr's -1 is left for its fallback when the device's LDS attribute cannot be read (64 KiB
// assumed): no size the plan accepts reaches it on gfx950, whose 160 KiB hold kPcrMaxN samples.
static int fgs_pcr(const WlsPlan& pl, const WlsBufs& b, hipStream_t st, sdr_sgbm* timer) {
    for (int it = 0; it < pl.iters; it++)
        for (int rows = 1; rows >= 0; rows--) {
            KScope kt(timer, SDR_KERNEL_FGS);
            const bool fin = !rows && pl.fin_fused && it == pl.iters - 1;
            if (launch_pcr(b.R0, b.R1, rows ? b.s.ChT : b.s.Cv, pl.g.rw, pl.g.rh, pl.F, rows, pl.lam[it], st,
                           fin ? &pl.g : nullptr, fin ? &b.out : nullptr))
                return -1;
        }
    return 0;
}

// FastGlobalSmootherFilter::filter on R0 (and R1 when the plan has two right-hand sides of the same
// systems), row-major rw x rh per frame, F frames with per-frame guides, in place: the weights
// (where k_wls_prep has not written them: ChT column-major = the sequential row pass's k-major, or
// row-major for k_fgs_pcr; Cv row-major), then the plan's solver.
int launch_fgs(const WlsPlan& pl, const WlsBufs& b, hipStream_t st, sdr_sgbm* timer) {
    const WlsGeom& g = pl.g;
    if (!pl.fused)
        hipLaunchKernelGGL(k_fgs_weights, dim3((g.rw + 63) / 64, (g.rh + 3) / 4, pl.F), dim3(256), 0, st,
                           b.guide + (size_t)g.ry * b.gstride + g.rx, b.gstride, b.gfstride, b.lut, g.rw, g.rh,
                           pl.rowmajor ? 1 : 0, b.s.ChT, b.s.Cv);
    if (pl.rowmajor) return fgs_pcr(pl, b, st, timer);
    fgs_thomas(pl, b, st, timer);
    return 0;
}

// The back end, where the last FGS pass has not written the outputs itself.
void wls_back(const WlsPlan& pl, const WlsBufs& b, hipStream_t st, sdr_sgbm* timer) {
    const WlsGeom& g = pl.g;
    KScope kt(timer, SDR_KERNEL_WLS_FINAL);
    hipLaunchKernelGGL(k_wls_final, dim3((g.W + 63) / 64, (g.H + 3) / 4, pl.F), dim3(256), 0, st, b.R0, b.R1, g, b.out);
}

}  // namespace sdr
