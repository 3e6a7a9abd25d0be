// sdr_wls_plan.hip -- builds the plan of a filter call (sdr_wls_plan.hpp).  Host only: no HIP call.
#include "sdr_wls_plan.hpp"

#include <algorithm>

namespace sdr {

WlsGeom wls_geom(const sdr_wls_params& p, int W, int H) {
    WlsGeom g{};
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
    return g;
}

// The sequential solver's exact division needs every pass's pivots in [1, 2^126): each pass's
// lambda (lambda * attenuation^k, in the plan's float arithmetic) in [0, kFgsThomasMaxLambda]
// (an attenuation above 1 or below 0 used to pass with only the first checked)
static bool thomas_lambdas_ok(double lambda, double att, int iters) {
    float lam = (float)lambda;
    const float fa = (float)att;
    for (int it = 0; it < iters; it++, lam = lam * fa)
        if (!(lam >= 0.0f) || !((double)lam <= kFgsThomasMaxLambda)) return false;
    return true;
}

WlsRefusal wls_refusal(const sdr_wls_params& p, const WlsGeom* g) {
    if (!(p.lambda >= 0.0) || !(p.sigma_color >= 0.0) || p.num_iter < 1)
        return {SDR_ERR_ARG, "FGS needs lambda >= 0, sigma_color >= 0, num_iter >= 1"};
    if (p.fgs_solver == SDR_FGS_THOMAS && !thomas_lambdas_ok(p.lambda, p.lambda_attenuation, p.num_iter))
        return {SDR_ERR_ARG, "SDR_FGS_THOMAS needs every pass's lambda * attenuation^k in [0, 2^100] (its pivots "
                             "stay in [1, 2^126))"};
    if (p.fgs_solver != SDR_FGS_PCR && p.fgs_solver != SDR_FGS_THOMAS)
        return {SDR_ERR_ARG, "fgs_solver must be SDR_FGS_PCR or SDR_FGS_THOMAS"};
    if (p.depth_discontinuity_radius < 0 || p.left_offset < 0 || p.right_offset < 0 || p.top_offset < 0 ||
        p.bottom_offset < 0)
        return {SDR_ERR_ARG, "negative WLS radius or offset"};
    if (g && g->rw > 0 && g->rh > 0 && p.fgs_solver == SDR_FGS_PCR && (g->rw > kPcrMaxN || g->rh > kPcrMaxN))
        return kPcrLineLimit;
    return {SDR_OK, ""};
}

sdr_wls_params fgs_params(double lambda, double sigma, double att, int iters, int solver) {
    sdr_wls_params p{};
    p.lambda = lambda;
    p.sigma_color = sigma;
    p.lambda_attenuation = att;
    p.num_iter = iters;
    p.fgs_solver = solver;
    return p;
}

WlsPlan make_wls_plan(const sdr_wls_params& p, int W, int H, int F, int nimg, int cus, bool front) {
    WlsPlan pl;
    pl.g = wls_geom(p, W, H);
    const WlsRefusal no = wls_refusal(p, &pl.g);
    pl.rc = no.rc;
    pl.why = no.why;
    if (pl.rc) return pl;
    const WlsGeom& g = pl.g;
    pl.F = F;
    pl.iters = p.num_iter;
    pl.front = front;
    pl.roi = g.rw > 0 && g.rh > 0;
    pl.rowmajor = p.fgs_solver == SDR_FGS_PCR;
    pl.two = nimg == 2;
    // ROIs up to kPcrMaxN columns take the fused front end; its window radius is ceil(blockSize / 2)
    // <= 9 for every valid SGBM block, and wider ones (setDepthDiscontinuityRadius) take the
    // per-pixel kernels.  With SDR_FGS_PCR the outputs then need no pass of their own.
    pl.fused = front && pl.roi && g.rw <= kPcrMaxN && g.radius <= 9;
    pl.fin_fused = pl.fused && pl.rowmajor;
    float lam = (float)p.lambda;
    const float fa = (float)p.lambda_attenuation;
    pl.lam.resize(pl.iters);
    for (int it = 0; it < pl.iters; it++, lam = lam * fa) pl.lam[it] = lam;  // lambda *= attenuation
    // the sequential solver's k-major arrays: sample rows padded to 4 lines (fgs_pad4), and room
    // for its loaders' reads past the last row
    pl.fsp = pl.roi ? (size_t)fgs_pad4(g.rw) * fgs_pad4(g.rh) : 0;
    const size_t cpx = pl.roi ? (size_t)g.rw * g.rh : 0, ov = kFgsOverread / sizeof(float);
    if (front) {
        pl.n.rdisc = pl.fused ? 0 : (size_t)F * W * H;
        pl.n.R0 = pl.n.R1 = F * cpx + 1;
    }
    pl.n.ChT = pl.n.Cv = F * pl.fsp + ov;
    if (!pl.rowmajor) {
        pl.n.thA = pl.n.thB = 2 * F * pl.fsp + ov;
        pl.n.coef = pl.coef_off(2 * pl.iters) + ov;
    }
    if (cus > 0) plan_dispatch(&pl, cus);
    return pl;
}

void plan_dispatch(WlsPlan* pl, int cus) {
    if (pl->roi && !pl->rowmajor) pl->fgs = fgs_plan(pl->g.rw, pl->g.rh, pl->F, pl->two, pl->iters, cus);
}

FgsScratch carve_fgs(const WlsPlan& pl, float* base) {
    FgsScratch s{};
    s.A = base;
    s.B = s.A + pl.n.thA;
    s.ChT = s.B + pl.n.thB;
    s.Cv = s.ChT + pl.n.ChT;
    s.coef = s.Cv + pl.n.Cv;
    return s;
}

}  // namespace sdr
