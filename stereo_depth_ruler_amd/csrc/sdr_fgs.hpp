// sdr_fgs.hpp -- what the units of the WLS / FGS filter share: the filter's geometry and outputs,
// the sequential solver's launch arguments, and the host entry points the units call on each other.
// No kernels: every kernel is launched from the unit that defines it
//   sdr_wls_plan.hip     the plan of a call (sdr_wls_plan.hpp): refusals, path, lambdas, scratch layout
//   sdr_wls.hip          the WLS front and back ends, the FGS weights and layouts; the stage launchers
//   sdr_fgs_seq.hip      the sequential solver (SDR_FGS_THOMAS): k_fgs_th, k_fgs_lr, k_fgs_lrjob
//   sdr_fgs_pcr.hip      the opt-in solver (SDR_FGS_PCR): k_fgs_pcr
//   sdr_wls_entries.hip  the filter's handle and C ABI: a call's stages over (handle, plan)
#pragma once
#include "../../include/sdr/sdr.h"
#include "sdr_device.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

namespace sdr {

// the sequential solver's k-major arrays keep their sample rows 16-byte aligned: line counts and
// line lengths rounded up to 4 (frames fgs_pad4(w) * fgs_pad4(h) samples apart)
__host__ __device__ __forceinline__ int fgs_pad4(int x) { return (x + 3) & ~3; }

struct WlsGeom {
    int W, H;
    int rx, ry, rw, rh;      // left ROI
    int rrx;                 // right ROI x (same y, w, h)
    int radius;
    double scale;            // 1 / (2r+1)^2
    float roll_off;
    int lrc_thresh;
    int fill;                // 16 * (min_disp - 1)
};

// The filter's outputs (the class path's epilogue: fout = out / 16, xyz = reprojectImageTo3D(fout,
// Q), both nullable), written by whichever kernel holds a pixel's final value: k_wls_final, or,
// with SDR_FGS_PCR, k_wls_prep (pixels outside the ROI) and the last FGS column pass (the ROI).
struct WlsOut {
    int16_t* out;
    float* fout;
    float* xyz;
    Q16 Q;
};

// saturate_cast<short>(FGS(conf*d) / FGS(conf)) (cv::divide of floats: 0 for a zero divisor;
// cvRound = cvtss2si: NaN / |v| >= 2^31 give INT_MIN, which saturates to -32768)
__device__ __forceinline__ int16_t wls_value(float a, float c) {
    const float v = c != 0.0f ? a / c : 0.0f;
    float q = rintf(v);
    q = fminf(fmaxf(q, -32768.0f), 32767.0f);
    return fabsf(v) < 2147483648.0f ? (int16_t)(int)q : (int16_t)-32768;
}

// pixel (x, y) of frame f: the int16 value and the epilogue
__device__ __forceinline__ void wls_emit(const WlsOut& o, const WlsGeom& g, int f, int x, int y, int16_t r) {
    const size_t p = (size_t)f * g.W * g.H + (size_t)y * g.W + x;
    o.out[p] = r;
    if (o.fout) {
        const float df = (float)r * 0.0625f;
        o.fout[p] = df;
        if (o.xyz) reproject_px(o.Q, x, y, (double)df, 0.0, 0, o.xyz + 3 * p);
    }
}

// FastGlobalSmootherFilter::filter's scratch, in frames of fsp = fgs_pad4(w) * fgs_pad4(h) samples
// (SDR_FGS_PCR uses ChT and Cv only, w * h a frame):
struct FgsScratch {
    float *A, *B;    // the sequential solver's two pass layouts (2 floats a sample), F frames each
    float *ChT, *Cv; // the weights, F frames each
    float* coef;     // the sequential solver's coefficients of each of the 2 * iters passes:
                     // [F * fsp] float4 (a, den, 1/den, t) then [F * fsp] t (5 * F * fsp floats)
};

constexpr int kFgsMaxJobs = 8;         // coefficient jobs in one launch
constexpr size_t kFgsOverread = 4096;  // bytes past a k-major array the loaders may read (the
                                       // last workgroup's lines beyond st, at the last sample)
constexpr double kFgsThomasMaxLambda = 0x1p100;  // pivots below 2^126 (fgs_rcp)
constexpr int kPcrMaxN = 4096;  // k_fgs_pcr's samples per block (G * n): 4 equations per thread of 1024

struct FgsCoefJob {
    const float* Cw;  // the pass's weights, k-major
    float4* coef;     // [F] frames of (a, den, 1/den, t), k-major
    float* tt;        // [F] frames of t, k-major (the back substitution's stream)
    float lam;
    int nl, n;
    int st;           // k-major sample stride (nl rounded up to 4)
    int blocks;
    int lpb;          // k_fgs_lrjob: lines a workgroup (16, 8 or 4)
};

struct FgsThArgs {
    void* U;                // k-major right-hand sides: float, or float2 (two, interleaved); the
                            // forward values are written back in place
    const float4* coef;     // this pass's (a, den, 1/den, t) ...
    const float* tt;        // ... and t
    void* O;                // line-major results (same element type as U; line stride onp), or
                            // null: ...
    float* O0;              // ... k-major results split into two arrays (the last pass; sample
    float* O1;              // stride ost, frames ofs apart)
    int nl, n;
    int st;                 // k-major sample stride of U, coef, tt
    int onp;                // O's line stride (n rounded up to 4: the next pass's st)
    size_t fs;              // frame stride of U, coef, tt, O
    size_t ost, ofs;
    int dbg;                // diagnostic builds (SDR_TH_STAMPS): the k_fgs_lr stamp slot
    int main_blocks;        // blocks of the pass itself; blocks past them run coefficient jobs
    int njobs;
    FgsCoefJob job[kFgsMaxJobs];
};

// ---- the sequential solver's dispatch plan (sdr_fgs_seq.hip) ----
// The kernel and lines a workgroup of every launch of one filter call: launch_fgs launches what
// the plan says and sdr_fgs_plan_query copies its first entries out.
struct FgsPlan {
    std::vector<sdr_fgs_launch> pass;  // pass p: k_fgs_lr or k_fgs_th
    std::vector<sdr_fgs_launch> job;   // pass p's coefficient job; a launch holds kFgsMaxJobs of them,
                                       // all on k_fgs_lrjob (each its own lines) or all on k_fgs_th
};
// pass p: a row pass (even p: nl = h lines of n = w samples) or a column pass
inline void fgs_pass_shape(int p, int w, int h, int* nl, int* n) {
    const bool rows = (p & 1) == 0;
    *nl = rows ? h : w;
    *n = rows ? w : h;
}
// pure host code (F frames a launch, a chip of `cus` CUs); the SDR_FGS_LR, SDR_FGS_LR_MAXL and
// SDR_FGS_LRJOB knobs are read once per process
FgsPlan fgs_plan(int w, int h, int F, bool two, int iters, int cus);
// one job launch (c.job[0 .. c.njobs), k[j] the plan's entry of job j) and one pass, as planned
void launch_fgs_jobs(FgsThArgs c, const sdr_fgs_launch* k, bool two, int F, hipStream_t st);
void launch_fgs_pass(FgsThArgs a, const sdr_fgs_launch& k, bool two, int F, hipStream_t st);

// ---- the opt-in solver (sdr_fgs_pcr.hip) ----
// k_fgs_pcr's lines a workgroup: short lines share one, up to 1024 samples together
inline int pcr_lines(int n, int nlines) { return std::max(1, std::min(nlines, 1024 / n)); }
// one pass over the rows (rows != 0) or columns of U0 (and U1 when non-null), in place; with fin_g /
// fin_o the pass writes the filter's outputs instead.  -1: lines too long (kPcrMaxN, the LDS).
int launch_pcr(float* U0, float* U1, const float* Cw, int w, int h, int F, int rows, float lam,
               hipStream_t st, const WlsGeom* fin_g = nullptr, const WlsOut* fin_o = nullptr);

// ---- the stages of a planned call (sdr_wls.hip) ----
struct WlsPlan;  // sdr_wls_plan.hpp
// What a call's stages read and write; the sizes are the plan's (WlsLayout).
struct WlsBufs {
    const int16_t *dl, *dr;      // the two disparity maps (null: FGS alone)
    const uint8_t* guide;        // the full frame's guide, rows gstride and frames gfstride apart
    size_t gstride, gfstride;
    const float* lut;            // the FGS weight table
    float* conf;                 // the full-size confidence map, nullable
    WlsOut out;
    float* rdisc;                // the per-pixel front end's right discontinuity map
    float *R0, *R1;              // the FGS right-hand sides, row-major over the ROI (R1 null: one)
    FgsScratch s;
};
// timer (nullable): the matcher handle whose per-kernel timing records the launches
void wls_front(const WlsPlan& pl, const WlsBufs& b, hipStream_t st, sdr_sgbm* timer);
// the plan's solver on R0 / R1 in place; fused, its last pass writes b.out.  -1: see fgs_pcr
int launch_fgs(const WlsPlan& pl, const WlsBufs& b, hipStream_t st, sdr_sgbm* timer);
void wls_back(const WlsPlan& pl, const WlsBufs& b, hipStream_t st, sdr_sgbm* timer);

}  // namespace sdr
