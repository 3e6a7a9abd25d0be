// sdr_wls_entries.hip -- the WLS / FGS filter's handle and C ABI (include/sdr/sdr.h).  Every call
// is planned once (sdr_wls_plan.hpp: the one refusal rule, the path, the scratch layout) and then
// runs its stages (sdr_wls.hip) over (handle, plan): reserve, front end, solver, back end.  The
// handle's device, stream binding and buffer release are sdr_host.hpp's Bound.  No kernels.
#include "sdr_host.hpp"
#include "sdr_wls_plan.hpp"

#include <cmath>
#include <vector>

struct sdr_wls : sdr::Bound {
    sdr_wls_params p{};
    sdr::Buf rdisc, A, B, Ac, Bc, ChT, Cv, lut, hbuf, coef;
    double lut_sigma = -1.0;
    sdr_wls() : Bound{&rdisc, &A, &B, &Ac, &Bc, &ChT, &Cv, &lut, &hbuf, &coef} {}
};

namespace {

using sdr::WlsBufs;
using sdr::WlsPlan;

constexpr int kFgsLevels = 65026;  // 255^2 + 1 squared differences of two 8-bit gray levels

int refuse(const sdr::WlsRefusal& no) { return sdr::set_error(no.rc, no.why); }

// The plan of a call on the current device (cus = 0).  Only an accepted plan of the sequential
// solver asks the device for its CUs: a refusal makes no HIP call.
WlsPlan plan_here(const sdr_wls_params& p, int W, int H, int F, int nimg, bool front, int cus = 0) {
    WlsPlan pl = sdr::make_wls_plan(p, W, H, F, nimg, cus, front);
    if (!pl.rc && !cus && !pl.rowmajor) sdr::plan_dispatch(&pl, sdr::device_cus());
    return pl;
}

// ComputeLUT_ParBody: LUT[i] = -exp(-sqrt((float)i) / sigmaColor), float math on the host (the
// same expf the oracle uses)
void fgs_lut_host(double sigma, std::vector<float>* lut) {
    lut->resize(kFgsLevels);
    const float s = (float)sigma;
    for (int i = 0; i < kFgsLevels; i++) (*lut)[i] = -expf(-sqrtf((float)i) / s);
}

int upload_lut(sdr_wls* h, double sigma, const float** out) {
    int rc;
    if ((rc = sdr::ensure(h->lut, sizeof(float) * kFgsLevels))) return rc;
    if (h->lut_sigma != sigma) {
        std::vector<float> lut;
        fgs_lut_host(sigma, &lut);
        SDR_HIP(hipMemcpy(h->lut.p, lut.data(), sizeof(float) * lut.size(), hipMemcpyHostToDevice));
        h->lut_sigma = sigma;
    }
    *out = (const float*)h->lut.p;
    return SDR_OK;
}

// The handle's grow-only buffers at the plan's sizes (SDR_FGS_PCR leaves the sequential solver's
// alone), the weight table, and the stages' view of them.
int wls_reserve(sdr_wls* h, const WlsPlan& pl, WlsBufs* b) {
    const struct {
        sdr::Buf* buf;
        size_t n;
    } need[] = {{&h->rdisc, pl.n.rdisc}, {&h->A, pl.n.R0},  {&h->B, pl.n.R1},   {&h->ChT, pl.n.ChT},
                {&h->Cv, pl.n.Cv},       {&h->Ac, pl.n.thA}, {&h->Bc, pl.n.thB}, {&h->coef, pl.n.coef}};
    int rc;
    for (const auto& r : need)
        if (r.n && (rc = sdr::ensure(*r.buf, r.n * sizeof(float)))) return rc;
    if ((rc = upload_lut(h, h->p.sigma_color, &b->lut))) return rc;
    b->rdisc = (float*)h->rdisc.p;
    b->R0 = (float*)h->A.p;
    b->R1 = (float*)h->B.p;
    b->s = {(float*)h->Ac.p, (float*)h->Bc.p, (float*)h->ChT.p, (float*)h->Cv.p, (float*)h->coef.p};
    return SDR_OK;
}

}  // namespace

// DisparityWLSFilter::filter on device with the class path's optional fused epilogue (fout =
// out / 16, xyz = reprojectImageTo3D(fout, Q)); sdr_wls_filter_device is this with neither.
int sdr::wls_filter_enqueue(sdr_wls* h, const int16_t* dl, const int16_t* dr, const uint8_t* guide, int W, int H,
                            size_t gstride, size_t gfstride, int F, int16_t* out, float* conf, float* fout,
                            const double* Q, float* xyz, hipStream_t st, sdr_sgbm* timer) {
    if (!h || !dl || !dr || !guide || !out) return sdr::set_error(SDR_ERR_ARG, "null argument");
    if (W <= 0 || H <= 0 || F <= 0 || gstride < (size_t)W || (F > 1 && gfstride < gstride * H))
        return sdr::set_error(SDR_ERR_ARG, "bad size/stride");
    if (xyz && (!fout || !Q)) return sdr::set_error(SDR_ERR_ARG, "the fused reprojection needs fout and Q");
    SDR_HIP(hipSetDevice(h->device));
    const WlsPlan pl = plan_here(h->p, W, H, F, 2, true);
    if (pl.rc) return sdr::set_error(pl.rc, pl.why);
    WlsBufs b{dl, dr, guide, gstride, gfstride, nullptr, conf, {out, fout, xyz, {}}};
    if (Q)
        for (int t = 0; t < 16; t++) b.out.Q.q[t] = Q[t];
    int rc;
    if ((rc = wls_reserve(h, pl, &b))) return rc;
    sdr::wls_front(pl, b, st, timer);
    // (the solver's only failure is the line limit, which the plan has refused already: fgs_pcr)
    if (pl.roi && sdr::launch_fgs(pl, b, st, timer)) return refuse(sdr::kPcrLineLimit);
    if (!pl.fin_fused) sdr::wls_back(pl, b, st, timer);
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

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
    if (const sdr::WlsRefusal no = sdr::wls_refusal(*p); no.rc) return refuse(no);
    sdr_wls* h = new sdr_wls();
    h->p = *p;
    if (const int rc = h->open(device)) {
        delete h;
        return rc;
    }
    *out = h;
    return SDR_OK;
}

int sdr_wls_destroy(sdr_wls* h) {
    if (!h) return SDR_OK;
    h->close();
    delete h;
    return SDR_OK;
}

int sdr_wls_set_params(sdr_wls* h, const sdr_wls_params* p) {
    if (!h || !p) return sdr::set_error(SDR_ERR_ARG, "null argument");
    if (const sdr::WlsRefusal no = sdr::wls_refusal(*p); no.rc) return refuse(no);
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
    h->bind(stream);
    return SDR_OK;
}

int sdr_wls_reset_stream(sdr_wls* h) {
    if (!h) return sdr::set_error(SDR_ERR_ARG, "null handle");
    h->unbind();
    return SDR_OK;
}

void* sdr_wls_get_stream(const sdr_wls* h) { return h ? (void*)h->stream : nullptr; }

int sdr_wls_get_roi(const sdr_wls* h, int W, int H, int roi[4]) {
    if (!h || !roi) return sdr::set_error(SDR_ERR_ARG, "null argument");
    const sdr::WlsGeom g = sdr::wls_geom(h->p, W, H);
    roi[0] = g.rx;
    roi[1] = g.ry;
    roi[2] = g.rw;
    roi[3] = g.rh;
    return SDR_OK;
}

int sdr_wls_filter_device(sdr_wls* h, const int16_t* dl, const int16_t* dr, const uint8_t* guide,
                          int W, int H, size_t gstride, size_t gfstride, int F, int16_t* out,
                          float* conf) {
    return sdr::wls_filter_enqueue(h, dl, dr, guide, W, H, gstride, gfstride, F, out, conf, nullptr, nullptr,
                                   nullptr, h ? h->stream : nullptr);
}

int sdr_wls_filter(sdr_wls* h, const int16_t* dl, const int16_t* dr, const uint8_t* guide, int W,
                   int H, size_t gstride, int16_t* out, float* conf) {
    if (!h || !dl || !dr || !guide || !out) return sdr::set_error(SDR_ERR_ARG, "null argument");
    if (W <= 0 || H <= 0 || gstride < (size_t)W) return sdr::set_error(SDR_ERR_ARG, "bad size/stride");
    SDR_HIP(hipSetDevice(h->device));
    // what the device call would refuse, before the staging is allocated and filled
    const sdr::WlsGeom g = sdr::wls_geom(h->p, W, H);
    if (const sdr::WlsRefusal no = sdr::wls_refusal(h->p, &g); no.rc) return refuse(no);
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
    // images are filtered in pairs (two right-hand sides of one system per line); an odd one is
    // left over with a plan of its own
    const sdr_wls_params p = sdr::fgs_params(lambda, sigma, att, iters, solver);
    const WlsPlan pair = plan_here(p, w, h, 1, nimg >= 2 ? 2 : 1, false);
    if (pair.rc) return sdr::set_error(pair.rc, pair.why);
    const WlsPlan last = nimg >= 2 && (nimg & 1) ? plan_here(p, w, h, 1, 1, false) : pair;
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> lut;
    fgs_lut_host(sigma, &lut);
    // stream-ordered scratch, one block: the weight table, then the plan's FGS arrays
    const size_t px = (size_t)w * h;
    sdr::ScratchLayout lay;
    const auto s_lut = lay.take<float>(lut.size()), s_fgs = lay.take<float>(pair.n.fgs_total());
    sdr::Scratch sc(st);
    if (const int rc = sc.open(lay)) return rc;
    float* dlut = sc.at(s_lut);
    SDR_HIP(hipMemcpyAsync(dlut, lut.data(), s_lut.bytes(), hipMemcpyHostToDevice, st));
    WlsBufs b{nullptr, nullptr, d_guide, gstride, 0, dlut};
    b.s = sdr::carve_fgs(pair, sc.at(s_fgs));
    int bad = 0;
    for (int i = 0; i < nimg; i += 2) {
        const bool two = nimg - i >= 2;
        b.R0 = d_img + i * px;
        b.R1 = two ? d_img + (i + 1) * px : nullptr;
        bad |= sdr::launch_fgs(two ? pair : last, b, st, nullptr);
    }
    if (const int rc = sc.finish()) return rc;
    // the host LUT vector dies here: wait for its upload before returning
    SDR_HIP(hipStreamSynchronize(st));
    return bad ? refuse(sdr::kPcrLineLimit) : SDR_OK;
}

int sdr_fgs_plan_query(int w, int h, int nframes, int nimg, int num_iter, int solver, int cus,
                       sdr_fgs_plan* out) {
    if (!out) return sdr::set_error(SDR_ERR_ARG, "null argument");
    if (w <= 0 || h <= 0 || nframes <= 0 || num_iter < 1 || cus < 0 || (nimg != 1 && nimg != 2))
        return sdr::set_error(SDR_ERR_ARG, "bad size, nimg other than 1 or 2, num_iter < 1 or cus < 0");
    // the plan a filter call of this shape runs: its first row and column pass, and their jobs in
    // the first job launch
    const WlsPlan pl = plan_here(sdr::fgs_params(0.0, 0.0, 0.0, num_iter, solver), w, h, nframes, nimg, false, cus);
    if (pl.rc != SDR_ERR_ARG) *out = sdr_fgs_plan{};  // (a size refusal has always left a zeroed record)
    if (pl.rc) return sdr::set_error(pl.rc, pl.why);
    if (pl.rowmajor) {
        out->row_pass = {SDR_FGS_KERNEL_PCR, sdr::pcr_lines(w, h)};
        out->col_pass = {SDR_FGS_KERNEL_PCR, sdr::pcr_lines(h, w)};
        return SDR_OK;
    }
    out->cus = cus ? cus : sdr::device_cus();
    out->row_pass = pl.fgs.pass[0];
    out->col_pass = pl.fgs.pass[1];
    out->row_job = pl.fgs.job[0];
    out->col_job = pl.fgs.job[1];
    return SDR_OK;
}

}  // extern "C"
