// wls_plan_check.hip -- the filter's plan builder (csrc/sdr_wls_plan.hip) as a stand-alone host
// program, for a sanitizer build: it compiles the plan unit into itself, builds the plan of every
// case of the grid below and of every refusal, and checks what each plan promises the stages that
// index by it.  Prints "wls_plan_check: N checks, M failures"; exit status 1 on a failure.
//
//   hipcc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -std=c++17 \
//         -I include tests/cpp/wls_plan_check.hip -L stereo_depth_ruler_amd/lib -lsdr \
//         -Wl,-rpath,$PWD/stereo_depth_ruler_amd/lib -o wls_plan_check
// (the library only supplies sdr::fgs_plan, which lives beside the sequential solver's kernels)
#include "../../stereo_depth_ruler_amd/csrc/sdr_wls_plan.hip"

#include <cmath>
#include <cstdio>
#include <cstring>

namespace {

int checks = 0, failures = 0;

void check(bool ok, const char* what, int line) {
    checks++;
    if (ok) return;
    failures++;
    std::printf("FAILED line %d: %s\n", line, what);
}
#define CHECK(x) check((x), #x, __LINE__)

constexpr int kCus = 256;
constexpr size_t kOv = sdr::kFgsOverread / sizeof(float);

sdr_wls_params params(int solver, int iters, int radius, int left, int right, int top, int bottom) {
    sdr_wls_params p{};
    p.lambda = 8000.0;
    p.sigma_color = 1.5;
    p.lrc_thresh = 24;
    p.depth_discontinuity_radius = radius;
    p.roll_off = 0.001f;
    p.lambda_attenuation = 0.25;
    p.num_iter = iters;
    p.left_offset = left;
    p.right_offset = right;
    p.top_offset = top;
    p.bottom_offset = bottom;
    p.fgs_solver = solver;
    return p;
}

// the refusal rule, restated
int status_of(const sdr_wls_params& p, int W, int H) {
    if (!(p.lambda >= 0.0) || !(p.sigma_color >= 0.0) || p.num_iter < 1) return SDR_ERR_ARG;
    if (p.fgs_solver == SDR_FGS_THOMAS) {
        float lam = (float)p.lambda;
        for (int it = 0; it < p.num_iter; it++, lam = lam * (float)p.lambda_attenuation)
            if (!(lam >= 0.0f) || !((double)lam <= std::ldexp(1.0, 100))) return SDR_ERR_ARG;
    }
    if (p.fgs_solver != SDR_FGS_PCR && p.fgs_solver != SDR_FGS_THOMAS) return SDR_ERR_ARG;
    if (p.depth_discontinuity_radius < 0 || p.left_offset < 0 || p.right_offset < 0 || p.top_offset < 0 ||
        p.bottom_offset < 0)
        return SDR_ERR_ARG;
    const int rw = W - p.left_offset - p.right_offset, rh = H - p.top_offset - p.bottom_offset;
    if (rw > 0 && rh > 0 && p.fgs_solver == SDR_FGS_PCR && (rw > 4096 || rh > 4096)) return SDR_ERR_SIZE;
    return SDR_OK;
}

// an accepted plan: what reserve, the front end, pass_args and the solvers rely on
void check_accepted(const sdr::WlsPlan& pl, const sdr_wls_params& p, int W, int H, int F, int nimg, bool front) {
    const sdr::WlsGeom& g = pl.g;
    const bool pcr = p.fgs_solver == SDR_FGS_PCR;
    CHECK(g.W == W && g.H == H && g.rx == p.left_offset && g.ry == p.top_offset);
    CHECK(g.rw == W - p.left_offset - p.right_offset && g.rh == H - p.top_offset - p.bottom_offset);
    CHECK(g.rrx == p.right_offset && g.radius == p.depth_discontinuity_radius);
    CHECK(pl.F == F && pl.iters == p.num_iter && pl.two == (nimg == 2) && pl.rowmajor == pcr && pl.front == front);
    CHECK(pl.roi == (g.rw > 0 && g.rh > 0));
    CHECK(!pl.fin_fused || (pl.fused && pl.roi && pcr));
    CHECK(pl.fused == (front && pl.roi && g.rw <= 4096 && g.radius <= 9));
    CHECK(pl.fin_fused == (pl.fused && pcr));
    // the lambda of every iteration: the float recurrence
    CHECK((int)pl.lam.size() == p.num_iter);
    float lam = (float)p.lambda;
    for (int it = 0; it < p.num_iter; it++, lam = lam * (float)p.lambda_attenuation)
        CHECK(std::memcmp(&pl.lam[it], &lam, sizeof lam) == 0);
    // the layout: padded frames, every array with the overread behind its last frame
    const size_t fsp = pl.roi ? (size_t)((g.rw + 3) & ~3) * ((g.rh + 3) & ~3) : 0;
    CHECK(pl.fsp == fsp);
    CHECK(pl.n.ChT >= F * fsp + kOv && pl.n.Cv >= F * fsp + kOv);
    if (pcr) {
        CHECK(pl.n.thA == 0 && pl.n.thB == 0 && pl.n.coef == 0);
        CHECK(pl.fgs.pass.empty() && pl.fgs.job.empty());
    } else {
        CHECK(pl.n.thA >= 2 * F * fsp + kOv && pl.n.thB >= 2 * F * fsp + kOv);
        for (int ps = 0; ps < 2 * p.num_iter; ps++) {
            CHECK(pl.coef_off(ps) == (size_t)ps * 5 * F * fsp);
            CHECK(pl.coef_off(ps + 1) + kOv <= pl.n.coef);
        }
        const size_t np = pl.roi ? 2 * (size_t)p.num_iter : 0;
        CHECK(pl.fgs.pass.size() == np && pl.fgs.job.size() == np);
    }
    if (front) {
        const size_t cpx = pl.roi ? (size_t)g.rw * g.rh : 0;
        CHECK(pl.n.R0 >= F * cpx && pl.n.R1 >= F * cpx && pl.n.R0 > 0 && pl.n.R1 > 0);
        CHECK(pl.n.rdisc == (pl.fused ? 0 : (size_t)F * W * H));
    } else {
        CHECK(pl.n.R0 == 0 && pl.n.R1 == 0 && pl.n.rdisc == 0);
    }
    // one block carved in FgsScratch's order ends where the last array ends
    std::vector<float> block(pl.n.fgs_total() + 1);
    const sdr::FgsScratch s = sdr::carve_fgs(pl, block.data());
    CHECK(s.A == block.data() && s.B == s.A + pl.n.thA && s.ChT == s.B + pl.n.thB && s.Cv == s.ChT + pl.n.ChT);
    CHECK(s.coef == s.Cv + pl.n.Cv && s.coef + pl.n.coef == block.data() + pl.n.fgs_total());
}

void one(const sdr_wls_params& p, int W, int H, int F, int nimg, bool front) {
    const sdr::WlsPlan pl = sdr::make_wls_plan(p, W, H, F, nimg, kCus, front);
    const int want = status_of(p, W, H);
    CHECK(pl.rc == want);
    CHECK((pl.rc == SDR_OK) == (pl.why[0] == 0));
    const sdr::WlsGeom g = sdr::wls_geom(p, W, H);
    CHECK(sdr::wls_refusal(p, &g).rc == want);
    if (pl.rc == SDR_OK) check_accepted(pl, p, W, H, F, nimg, front);
    // a plan without the CU count is the same plan with the dispatch left out
    sdr::WlsPlan q = sdr::make_wls_plan(p, W, H, F, nimg, 0, front);
    CHECK(q.rc == pl.rc && q.fgs.pass.empty() && q.n.coef == pl.n.coef && q.fused == pl.fused);
    if (q.rc == SDR_OK) {
        sdr::plan_dispatch(&q, kCus);
        CHECK(q.fgs.pass.size() == pl.fgs.pass.size() && q.fgs.job.size() == pl.fgs.job.size());
    }
}

void grid() {
    // H x W, and the ROI's inset (left, right, top, bottom)
    const int shapes[][6] = {{1, 1, 0, 0, 0, 0},      {1, 37, 0, 0, 0, 0},    {29, 1, 0, 0, 0, 0},
                             {61, 150, 16, 5, 3, 2},  {6, 4200, 64, 0, 0, 0},  // an ROI past 4096 columns
                             {61, 150, 150, 0, 0, 0}, {61, 150, 100, 60, 0, 0}};  // empty ROIs
    for (auto& s : shapes)
        for (int solver : {SDR_FGS_PCR, SDR_FGS_THOMAS})
            for (int nimg : {1, 2})
                for (int F : {1, 3})
                    for (int iters : {1, 3, 5})
                        for (int radius : {4, 9, 10}) {
                            const sdr_wls_params p = params(solver, iters, radius, s[2], s[3], s[4], s[5]);
                            if (nimg == 2) one(p, s[1], s[0], F, 2, true);  // the filter solves both at once
                            // FastGlobalSmootherFilter alone: the image is the ROI
                            one(sdr::fgs_params(p.lambda, p.sigma_color, p.lambda_attenuation, iters, solver), s[1], s[0], F,
                                nimg, false);
                        }
}

void refusals() {
    const int T = SDR_FGS_THOMAS, P = SDR_FGS_PCR;
    auto with = [](sdr_wls_params p, double lambda, double sigma, double att) {
        p.lambda = lambda;
        p.sigma_color = sigma;
        p.lambda_attenuation = att;
        return p;
    };
    for (int solver : {P, T}) {
        one(with(params(solver, 3, 3, 0, 0, 0, 0), -1.0, 1.5, 0.25), 40, 30, 1, 2, true);
        one(with(params(solver, 3, 3, 0, 0, 0, 0), NAN, 1.5, 0.25), 40, 30, 1, 2, true);
        one(with(params(solver, 3, 3, 0, 0, 0, 0), 8000.0, -0.5, 0.25), 40, 30, 1, 2, true);
        one(params(solver, 0, 3, 0, 0, 0, 0), 40, 30, 1, 2, true);
        // 8000 * 4^44 is the first lambda past 2^100; SDR_FGS_PCR has no such range
        one(with(params(solver, 44, 3, 0, 0, 0, 0), 8000.0, 1.5, 4.0), 40, 30, 1, 2, true);
        one(with(params(solver, 45, 3, 0, 0, 0, 0), 8000.0, 1.5, 4.0), 40, 30, 1, 2, true);
        one(with(params(solver, 2, 3, 0, 0, 0, 0), 8000.0, 1.5, -0.25), 40, 30, 1, 2, true);
        one(params(solver, 3, -1, 0, 0, 0, 0), 40, 30, 1, 2, true);
        one(params(solver, 3, 3, -1, 0, 0, 0), 40, 30, 1, 2, true);
        one(params(solver, 3, 3, 0, 0, 0, -1), 40, 30, 1, 2, true);
        // the line limit, on either side and in either direction
        one(params(solver, 3, 3, 0, 0, 0, 0), 4096, 3, 1, 2, true);
        one(params(solver, 3, 3, 0, 0, 0, 0), 4097, 3, 1, 2, true);
        one(params(solver, 3, 3, 0, 0, 0, 0), 3, 4097, 1, 2, true);
        one(params(solver, 3, 3, 1, 0, 0, 0), 4097, 3, 1, 2, true);  // the ROI counts, not the frame
    }
    one(params(7, 3, 3, 0, 0, 0, 0), 40, 30, 1, 2, true);
    // the order the refusals win in: parameters, solver, negative offsets, then the size
    sdr_wls_params p = with(params(7, 3, 3, -1, 0, 0, 0), -1.0, 1.5, 0.25);
    CHECK(std::strstr(sdr::wls_refusal(p).why, "FGS needs"));
    p.lambda = 8000.0;
    CHECK(std::strstr(sdr::wls_refusal(p).why, "fgs_solver must be"));
    p.fgs_solver = P;
    const sdr::WlsGeom g = sdr::wls_geom(p, 5000, 3);
    CHECK(std::strstr(sdr::wls_refusal(p, &g).why, "negative WLS radius or offset"));
    p.left_offset = 0;
    const sdr::WlsGeom g2 = sdr::wls_geom(p, 5000, 3);
    CHECK(sdr::wls_refusal(p, &g2).rc == SDR_ERR_SIZE && sdr::wls_refusal(p).rc == SDR_OK);
}

}  // namespace

int main() {
    grid();
    refusals();
    std::printf("wls_plan_check: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
