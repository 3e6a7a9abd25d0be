// sdr_wls_plan.hpp -- the plan of one WLS / FGS filter call: what the call will do, derived once
// on the host.
//
// make_wls_plan() refuses what the filter cannot run, lays out the ROI, decides the path (fused
// front end, fused outputs, the solver's layouts), lists every iteration's lambda and sizes every
// scratch array; it makes no HIP call.  Everything that reserves scratch or launches a stage
// (sdr_wls_entries.hip, the stage launchers of sdr_wls.hip) reads this record, not the parameters.
#pragma once
#include "sdr_fgs.hpp"

#include <vector>

namespace sdr {

struct WlsRefusal {
    int rc;           // SDR_OK: the call runs
    const char* why;  // its text (sdr_last_error)
};

// the shape refusal: k_fgs_pcr holds a whole line in a workgroup (kPcrMaxN samples)
constexpr WlsRefusal kPcrLineLimit{
    SDR_ERR_SIZE, "SDR_FGS_PCR solves lines of at most 4096 samples (use SDR_FGS_THOMAS for longer lines)"};

// Floats of every scratch array of a call, the solver's loaders' overread (kFgsOverread) included.
// The sequential solver's arrays hold frames of fsp = fgs_pad4(rw) * fgs_pad4(rh) samples.
struct WlsLayout {
    size_t rdisc = 0;         // the right view's discontinuity map, full frames (per-pixel front end only)
    size_t R0 = 0, R1 = 0;    // conf * d and conf, ROI-compact and row-major: the FGS right-hand sides
    size_t thA = 0, thB = 0;  // FgsScratch::A, B: 2 floats a sample (SDR_FGS_THOMAS only)
    size_t ChT = 0, Cv = 0;   // FgsScratch::ChT, Cv
    size_t coef = 0;          // FgsScratch::coef: 5 floats a sample and pass (SDR_FGS_THOMAS only)
    size_t fgs_total() const { return thA + thB + ChT + Cv + coef; }
};

struct WlsPlan {
    int rc = SDR_OK;       // the refusal, SDR_OK when the call runs
    const char* why = "";
    WlsGeom g{};           // FGS alone: the image is its own ROI
    int F = 0, iters = 0;
    bool front = false;    // the WLS front and back end run (false: FastGlobalSmootherFilter alone)
    bool roi = false;      // the ROI is not empty: the solver runs
    bool fused = false;    // k_wls_prep is the front end: it writes the weights and the solver's inputs
    bool fin_fused = false;  // no k_wls_final: k_wls_prep and the last FGS column pass write the outputs
    bool rowmajor = false;   // SDR_FGS_PCR: weights and right-hand sides stay row-major
    bool two = false;        // two right-hand sides a line
    size_t fsp = 0;          // samples of a frame in the sequential solver's padded layouts
    std::vector<float> lam;  // every iteration's lambda (lambda *= attenuation, in float)
    FgsPlan fgs;             // SDR_FGS_THOMAS: the kernel of every pass and job (plan_dispatch)
    WlsLayout n;

    // floats from FgsScratch::coef to pass p's block: [F * fsp] float4 (a, den, 1/den, t), then
    // [F * fsp] t
    size_t coef_off(int p) const { return (size_t)p * 5 * F * fsp; }
};

// The ROI and the front end's constants of a W x H frame under p.
WlsGeom wls_geom(const sdr_wls_params& p, int W, int H);
// The one refusal rule, in the order the refusals win: lambda, sigma and num_iter; the sequential
// solver's lambda range; the solver; negative radius or offsets (all SDR_ERR_ARG); then, with a
// geometry, the SDR_FGS_PCR line limit on its ROI (SDR_ERR_SIZE).
WlsRefusal wls_refusal(const sdr_wls_params& p, const WlsGeom* g = nullptr);
// The parameters of FastGlobalSmootherFilter alone: no front end, the whole image the ROI.
sdr_wls_params fgs_params(double lambda, double sigma, double att, int iters, int solver);
// The plan of F frames of W x H under p, nimg (1 or 2) right-hand sides a line, on a chip of cus
// CUs.  cus = 0: the caller asks the device once the plan is accepted and completes the dispatch
// with plan_dispatch (a refusal then needs no device).
WlsPlan make_wls_plan(const sdr_wls_params& p, int W, int H, int F, int nimg, int cus, bool front = true);
void plan_dispatch(WlsPlan* pl, int cus);
// The FGS scratch arrays of one block of pl.n.fgs_total() floats, in FgsScratch's order.
FgsScratch carve_fgs(const WlsPlan& pl, float* base);

}  // namespace sdr
