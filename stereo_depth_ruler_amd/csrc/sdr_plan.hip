// sdr_plan.hip -- builds the plan of a matcher call (sdr_plan.hpp).  Host only: no HIP call.
#include "sdr_plan.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

namespace sdr {
namespace {

int refuse(Plan* pl, int code, const char* why) {
    pl->rc = code;
    pl->why = why;
    return code;
}

// OpenCV's parameter defaulting (stereosgbm.cpp computeDisparitySGBM / SGBM3WayMainLoop ctor).
int make_eff(Plan* pl, const sdr_sgbm_params& p, int W, int H, int cost) {
    Eff* e = &pl->e;
    if (cost != SDR_COST_BT && cost != SDR_COST_CENSUS_9X7) return refuse(pl, SDR_ERR_ARG, "unknown cost type");
    e->cost = cost;
    if (p.numDisparities <= 0 || p.numDisparities % 16 != 0)
        return refuse(pl, SDR_ERR_NUMDISP, "numDisparities must be positive and divisible by 16");
    if (p.numDisparities > 512) return refuse(pl, SDR_ERR_LIMIT, "numDisparities > 512 is not supported");
    if (p.mode != SDR_MODE_SGBM && p.mode != SDR_MODE_HH && p.mode != SDR_MODE_SGBM_3WAY &&
        p.mode != SDR_MODE_HH4)
        return refuse(pl, SDR_ERR_MODE, "unknown mode");
    Geometry& g = e->g;
    g.W = W;
    g.H = H;
    g.D = p.numDisparities;
    g.minD = p.minDisparity;
    int maxD = g.minD + g.D;
    g.minX1 = std::max(maxD, 0);
    g.W1 = W + std::min(g.minD, 0) - g.minX1;
    g.split = 1 << 30;  // unpaired (see sdr::Geometry)
    g.minDb = g.minD;
    g.minX1b = g.minX1;
    if (p.mode == SDR_MODE_SGBM_3WAY) {
        g.SW2 = g.SH2 = p.blockSize > 0 ? p.blockSize / 2 : 1;
    } else {
        int bs = p.blockSize > 0 ? p.blockSize : 5;
        g.SW2 = g.SH2 = bs / 2;
    }
    g.P1 = p.P1 > 0 ? p.P1 : 2;
    g.P2 = std::max(p.P2 > 0 ? p.P2 : 5, g.P1 + 1);
    e->mode = p.mode;
    e->uniq = p.uniquenessRatio >= 0 ? p.uniquenessRatio : 10;
    if (e->uniq >= 100) return refuse(pl, SDR_ERR_ARG, "uniquenessRatio must be < 100");
    e->disp12MaxDiff = p.disp12MaxDiff > 0 ? p.disp12MaxDiff : 1;
    e->ftzero = std::max(p.preFilterCap, 15) | 1;  // any size: the clip table wraps mod 256 (k_prefilter)
    e->nstripes = p.nstripes > 0 ? p.nstripes : 4;
    e->uniq_simd = p.uniq_rule == SDR_UNIQ_SIMD ? 1
                 : p.uniq_rule == SDR_UNIQ_SCALAR ? 0
                 : (p.mode == SDR_MODE_SGBM_3WAY ? 1 : 0);
    e->invalid = (g.minD - 1) * 16;
    e->speckle_ws = p.speckleWindowSize;
    e->speckle_diff = 16 * p.speckleRange;
    e->blockSize = p.blockSize;
    // The int16 domain of OpenCV's own arithmetic: C = P2 + block cost and delta = minLp + P2
    // (minLp <= C) must fit a short.  Past it OpenCV's SIMD build wraps (short)delta0 and
    // saturates C while its scalar build computes them in int, so the reference's output is not
    // defined by the algorithm alone; the engine refuses instead of picking one of the two.
    if (cost == SDR_COST_CENSUS_9X7) {
        // the census pixel cost is a Hamming distance of 62-bit descriptors, whatever preFilterCap
        if (2L * g.P2 + 62L * (2 * g.SW2 + 1) * (2 * g.SH2 + 1) > 32767)
            return refuse(pl, SDR_ERR_LIMIT, "2*P2 + 62*blockSize^2 exceeds the int16 cost range");
        return SDR_OK;
    }
    // the largest pixel cost: BT of the prefiltered channel (values in [0, min(2*ftzero, 255)],
    // the uchar clip table) + BT of the raw one >> 2
    const long bmax = (long)(std::min(2 * e->ftzero, 255) + 63) * (2 * g.SW2 + 1) * (2 * g.SH2 + 1);
    if (2L * g.P2 + bmax > 32767)
        return refuse(pl, SDR_ERR_LIMIT, "2*P2 + (2*preFilterCap+63)*blockSize^2 exceeds the int16 cost "
                                         "range (OpenCV's SIMD and scalar builds disagree there)");
    return SDR_OK;
}

// Channel count of the input pair (OpenCV: CV_8UC1 or CV_8UC3; calcPixelCostBT's cn == 3 branch
// sums each channel's Sobel and raw costs, so the int16 domain bound grows with it).
int check_channels(Plan* pl, int cn) {
    const Eff& e = pl->e;
    if (cn != 1 && cn != 3) return refuse(pl, SDR_ERR_TYPE, "images must have 1 or 3 channels");
    if (cn == 1) return SDR_OK;
    if (e.cost == SDR_COST_CENSUS_9X7) return refuse(pl, SDR_ERR_TYPE, "the census cost takes single-channel images");
    const Geometry& g = e.g;
    const long bmax = (long)cn * (std::min(2 * e.ftzero, 255) + 63) * (2 * g.SW2 + 1) * (2 * g.SH2 + 1);
    if (2L * g.P2 + bmax > 32767)
        return refuse(pl, SDR_ERR_LIMIT, "2*P2 + 3*(2*preFilterCap+63)*blockSize^2 exceeds the int16 cost "
                                         "range (OpenCV's SIMD and scalar builds disagree there)");
    if ((size_t)g.H * g.W * 24 * cn > (size_t)INT32_MAX)
        return refuse(pl, SDR_ERR_SIZE, "frame too large: the right image's cost planes span more than 2 GiB");
    return SDR_OK;
}

// Frame-size limits of a matched frame (W1 > 0).
int check_frame(Plan* pl) {
    const Eff& e = pl->e;
    const Geometry& g = e.g;
    if (g.W1 <= g.SW2) return refuse(pl, SDR_ERR_SIZE, "image too narrow for numDisparities/blockSize");
    if (g.W > 8192) return refuse(pl, SDR_ERR_SIZE, "width > 8192 is not supported");
    // k_paths addresses a whole chain through one buffer resource and a 32-bit SGPR offset that
    // stays below 2^31 (num_records): the longest chain span, slack rows included, must fit
    if ((size_t)(g.H + 2 * kSouthPad) * (size_t)(g.W1 + 1) * g.D * 2 > (size_t)INT32_MAX)
        return refuse(pl, SDR_ERR_SIZE, "frame too large: a path chain spans more than 2 GiB of cost volume");
    // k_cost addresses a frame's right-image planes (3 x 8 B per pixel) the same way
    if ((size_t)g.H * g.W * 24 > (size_t)INT32_MAX)
        return refuse(pl, SDR_ERR_SIZE, "frame too large: the right image's cost planes span more than 2 GiB");
    if (!cost_supported(g)) return refuse(pl, SDR_ERR_ARG, "unsupported block shape");
    if (e.cost == SDR_COST_CENSUS_9X7) {
        // the shapes the BT cost sends to the two-pass launch_cost_generic
        if (g.SH2 > 5) return refuse(pl, SDR_ERR_LIMIT, "the census cost supports blockSize <= 11");
        if (g.D > 256) return refuse(pl, SDR_ERR_LIMIT, "the census cost supports numDisparities <= 256");
    }
    return SDR_OK;
}

// SGBM3WayMainLoop's stripes of a frame's rows, with the limits of the launches that run them:
// one top-to-bottom direction a stripe (kMaxStripes) and one extra cost band, and at most one
// row redirect, for each stripe that keeps start rows of its own (kMaxCostAux).
int lay_stripes(Plan* pl) {
    const Eff& e = pl->e;
    const int H = e.g.H;
    const int n = e.nstripes;
    const int sz = (int)std::ceil(H / (double)n);
    const int overlap = (e.blockSize / 2 + 1) + (int)std::ceil(0.1 * sz);
    int naux = 0;
    for (int s = 0; s < n; s++) {
        Stripe st;
        st.out0 = s * sz;
        if (st.out0 >= H) break;
        st.s0 = std::max(std::min(s * sz - overlap, H), 0);
        st.end = std::min((s + 1) * sz, H);
        st.ylim = std::max(H - 1 - e.g.SH2, st.s0);
        if (st.s0 == 0) st.aux_rows = 0;
        else if (st.ylim >= st.s0 + e.g.SH2) st.aux_rows = e.g.SH2;
        else st.aux_rows = st.end - st.s0;
        if (pl->nstr == kMaxStripes) return refuse(pl, SDR_ERR_ARG, "too many 3WAY stripes");
        pl->stripes[pl->nstr++] = st;
        pl->amax = std::max(pl->amax, st.aux_rows);
        naux += st.aux_rows != 0;
    }
    if (naux > kMaxCostAux) return refuse(pl, SDR_ERR_ARG, "too many 3WAY stripes");
    pl->aux_fstride = (size_t)pl->nstr * pl->amax * e.g.W1 * e.g.D;
    return SDR_OK;
}

int npaths_of(int mode) {
    return mode == SDR_MODE_HH ? 8 : mode == SDR_MODE_SGBM ? 5 : mode == SDR_MODE_HH4 ? 4 : 3;
}

}  // namespace

Plan make_plan(const sdr_sgbm_params& p, int cost, int W, int H, int F, int cn) {
    Plan pl;
    pl.F = F;
    pl.cn = cn;
    if (make_eff(&pl, p, W, H, cost)) return pl;
    pl.defaulted = true;
    if (check_channels(&pl, cn)) return pl;
    const Geometry& g = pl.e.g;
    pl.px = (size_t)W * H;
    pl.npaths = npaths_of(pl.e.mode);
    pl.empty = g.W1 <= 0;
    if (pl.empty || check_frame(&pl)) return pl;
    if (pl.e.mode == SDR_MODE_SGBM_3WAY && lay_stripes(&pl)) return pl;
    pl.cells = (size_t)H * g.W1 * g.D;
    pl.slack = (size_t)kSouthPad * g.W1 * g.D;
    pl.aux_slack = (size_t)kSouthPad * g.D;
    pl.lr_skipped = !pl.speckle() && pl.e.disp12MaxDiff >= g.D;
    return pl;
}

bool can_pair(const Eff& a, const Eff& b) {
    return a.g.W1 == b.g.W1 && a.g.W1 > 0 && a.g.D == b.g.D && a.g.SW2 == b.g.SW2 && a.g.P1 == b.g.P1 &&
           a.g.P2 == b.g.P2 && a.mode == b.mode && a.uniq == b.uniq && a.uniq_simd == b.uniq_simd &&
           a.disp12MaxDiff == b.disp12MaxDiff && a.ftzero == b.ftzero && a.nstripes == b.nstripes &&
           a.speckle_ws == 0 && b.speckle_ws == 0 && a.blockSize == b.blockSize && a.cost == b.cost;
}

Plan plan_pair(const Plan& a, const Plan& b) {
    if (!a.defaulted) return a;
    if (!b.defaulted) return b;
    Plan pl = a;
    if (!can_pair(a.e, b.e) || a.F != b.F) {
        refuse(&pl, SDR_ERR_ARG, "matchers cannot be paired");
        return pl;
    }
    pl.F = a.F + b.F;
    pl.e.g.split = a.F;
    pl.e.g.minDb = b.e.g.minD;
    pl.e.g.minX1b = b.e.g.minX1;
    return pl;
}

void plan_sweep(Plan* pl, const SweepShape shp[2]) {
    pl->shp[0] = shp[0];
    pl->shp[1] = shp[1];
    pl->sweep = shp[0].nslots > 0 && shp[1].nslots > 0;
    pl->nrec = pl->sweep ? 3 : pl->npaths - 1;
    pl->lslack = pl->slack * pl->nrec;
    pl->lfs = (size_t)pl->nrec * pl->cells;
    pl->edge_bytes = 0;
    for (int up = 0; up < 2; up++) {
        pl->flags_n[up] = (size_t)shp[up].nslots * shp[up].ntiles * 2 * shp[up].npub;
        pl->edge_bytes = std::max(pl->edge_bytes, (size_t)shp[up].nslots * shp[up].ntiles * 4 * shp[up].entry_words * 4);
    }
    pl->sweep_flags = (pl->flags_n[0] + pl->flags_n[1]) * sizeof(int);
}

size_t plan_scratch_bytes(const Plan& pl) {
    const size_t px = pl.px, cn = pl.cn;
    return (size_t)pl.F * (3 * px * 4 * cn + 3 * px * 8 * cn + pl.cells * 2 * pl.npaths + pl.aux_fstride * 2 +
                           px * 2 * 3 + px * 4 + px * 4 * 2);
}

}  // namespace sdr
