// plan_check.hip -- the plan builder (csrc/sdr_plan.hip) as a stand-alone host program, for a
// sanitizer build: it compiles the plan unit into itself, builds the plan of every case of
// tests/test_plan_cpu.py's grid and of every refusal, and checks what each plan promises the
// stages that index by it.  Prints "plan_check: N checks, M failures"; exit status 1 on a failure.
//
//   hipcc -Xarch_host -fsanitize=address,undefined -std=c++17 -I include tests/cpp/plan_check.hip \
//         -L stereo_depth_ruler_amd/lib -lsdr -Wl,-rpath,$PWD/stereo_depth_ruler_amd/lib -o plan_check
// (the library only supplies sdr::cost_supported, which lives beside the cost kernels)
#include "../../stereo_depth_ruler_amd/csrc/sdr_plan.hip"

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

sdr_sgbm_params params(int minD, int D, int bs, int P1, int P2, int cap, int uniq, int mode, int nstripes) {
    sdr_sgbm_params p{};
    p.minDisparity = minD;
    p.numDisparities = D;
    p.blockSize = bs;
    p.P1 = P1;
    p.P2 = P2;
    p.disp12MaxDiff = 1;
    p.preFilterCap = cap;
    p.uniquenessRatio = uniq;
    p.mode = mode;
    p.nstripes = nstripes;
    return p;
}

// an accepted plan: what size_scratch, the stages and the debug read-back rely on
void check_accepted(const sdr::Plan& pl, int H) {
    const sdr::Geometry& g = pl.e.g;
    CHECK(pl.rc == SDR_OK && pl.defaulted && !pl.empty);
    CHECK(pl.cells == (size_t)H * g.W1 * g.D && pl.slack == (size_t)sdr::kSouthPad * g.W1 * g.D);
    CHECK(pl.nstr <= sdr::kMaxStripes);
    int naux = 0, amax = 0, row = 0;
    for (int s = 0; s < pl.nstr; s++) {
        const sdr::Stripe& st = pl.stripes[s];
        CHECK(st.out0 == row && st.s0 <= st.out0 && st.out0 < st.end && st.end <= H);
        CHECK(st.aux_rows >= 0 && st.aux_rows <= st.end - st.s0);
        row = st.end;
        naux += st.aux_rows != 0;
        amax = std::max(amax, st.aux_rows);
    }
    CHECK(pl.nstr == 0 || row == H);
    CHECK((pl.e.mode == SDR_MODE_SGBM_3WAY) == (pl.nstr > 0));
    CHECK(naux <= sdr::kMaxCostAux && amax == pl.amax);
    CHECK(pl.aux_fstride == (size_t)pl.nstr * amax * g.W1 * g.D);
    // the last stripe's band ends where the frame's stripe-start rows end
    CHECK(pl.nstr == 0 || pl.aux_off(pl.nstr - 1) + (size_t)amax * g.W1 * g.D == pl.aux_fstride);
    sdr::Plan q = pl;
    const sdr::SweepShape none[2] = {};
    sdr::plan_sweep(&q, none);
    CHECK(!q.sweep && q.nrec == q.npaths - 1 && q.lslack == q.slack * q.nrec && q.sweep_flags == 0);
    CHECK(sdr::plan_scratch_bytes(pl) > 0);
}

void grid() {
    const int shapes[2][2] = {{320, 100}, {205, 37}};
    for (auto& wh : shapes)
        for (int D : {64, 128})
            for (int mode = 0; mode < 4; mode++)
                for (int ns : {1, 4, 7})
                    for (int cn : {1, 3})
                        for (int F : {1, 2, 8})
                            check_accepted(sdr::make_plan(params(0, D, 5, 50, 300, 31, 10, mode, ns), SDR_COST_BT,
                                                          wh[0], wh[1], F, cn), wh[1]);
    for (int mode = 0; mode < 4; mode++)
        check_accepted(sdr::make_plan(params(-24, 64, 5, 50, 300, 31, 10, mode, 4), SDR_COST_BT, 320, 100, 2, 1), 100);
    check_accepted(sdr::make_plan(params(0, 64, 5, 50, 300, 31, 10, SDR_MODE_SGBM, 4), SDR_COST_CENSUS_9X7, 320, 100, 1, 1), 100);
}

void refused(const sdr_sgbm_params& p, int cost, int W, int H, int cn, int code, const char* text, int line) {
    const sdr::Plan pl = sdr::make_plan(p, cost, W, H, 1, cn);
    check(pl.rc == code && std::strstr(pl.why, text), text, line);
}
#define REFUSED(p, cost, W, H, cn, code, text) refused(p, cost, W, H, cn, code, text, __LINE__)

void refusals() {
    const int BT = SDR_COST_BT, CENSUS = SDR_COST_CENSUS_9X7, M = SDR_MODE_SGBM, W3 = SDR_MODE_SGBM_3WAY;
    REFUSED(params(0, 64, 5, 50, 300, 31, 10, M, 4), 2, 320, 100, 1, SDR_ERR_ARG, "unknown cost type");
    REFUSED(params(0, 0, 5, 50, 300, 31, 10, M, 4), BT, 320, 100, 1, SDR_ERR_NUMDISP, "divisible by 16");
    REFUSED(params(0, 24, 5, 50, 300, 31, 10, M, 4), BT, 320, 100, 1, SDR_ERR_NUMDISP, "divisible by 16");
    REFUSED(params(0, 528, 5, 50, 300, 31, 10, M, 4), BT, 700, 100, 1, SDR_ERR_LIMIT, "numDisparities > 512");
    REFUSED(params(0, 64, 5, 50, 300, 31, 10, 7, 4), BT, 320, 100, 1, SDR_ERR_MODE, "unknown mode");
    REFUSED(params(0, 64, 5, 50, 300, 31, 100, M, 4), BT, 320, 100, 1, SDR_ERR_ARG, "uniquenessRatio");
    REFUSED(params(0, 64, 11, 10, 12633, 63, 10, M, 4), CENSUS, 320, 100, 1, SDR_ERR_LIMIT, "62*blockSize^2");
    REFUSED(params(0, 64, 11, 10, 5000, 63, 10, M, 4), BT, 320, 100, 1, SDR_ERR_LIMIT, "2*P2 + (2*preFilterCap+63)");
    REFUSED(params(0, 64, 5, 50, 300, 31, 10, M, 4), BT, 320, 100, 2, SDR_ERR_TYPE, "1 or 3 channels");
    REFUSED(params(0, 64, 5, 50, 300, 31, 10, M, 4), CENSUS, 320, 100, 3, SDR_ERR_TYPE, "single-channel");
    REFUSED(params(0, 64, 5, 50, 9500, 63, 10, M, 4), BT, 320, 100, 3, SDR_ERR_LIMIT, "2*P2 + 3*(2*preFilterCap+63)");
    REFUSED(params(0, 64, 5, 50, 300, 31, 10, M, 4), BT, 8000, 4000, 3, SDR_ERR_SIZE, "cost planes span");
    REFUSED(params(0, 64, 5, 50, 300, 31, 10, M, 4), BT, 66, 100, 1, SDR_ERR_SIZE, "too narrow");
    REFUSED(params(0, 16, 5, 50, 300, 31, 10, M, 4), BT, 8200, 10, 1, SDR_ERR_SIZE, "width > 8192");
    REFUSED(params(0, 512, 5, 50, 300, 31, 10, M, 4), BT, 8192, 200, 1, SDR_ERR_SIZE, "path chain spans");
    REFUSED(params(8000, 16, 5, 50, 300, 31, 10, M, 4), BT, 8192, 11000, 1, SDR_ERR_SIZE, "cost planes span");
    REFUSED(params(0, 64, 13, 50, 300, 31, 10, M, 4), CENSUS, 320, 100, 1, SDR_ERR_LIMIT, "blockSize <= 11");
    REFUSED(params(0, 272, 5, 50, 300, 31, 10, M, 4), CENSUS, 400, 100, 1, SDR_ERR_LIMIT, "numDisparities <= 256");
    // 25 stripes: more directions than a path launch holds; 20 stripes, 19 with rows of their own:
    // more than the cost launch's extra bands
    REFUSED(params(0, 64, 3, 50, 300, 31, 10, W3, 30), BT, 320, 100, 1, SDR_ERR_ARG, "too many 3WAY stripes");
    REFUSED(params(0, 64, 3, 50, 300, 31, 10, W3, 20), BT, 320, 100, 1, SDR_ERR_ARG, "too many 3WAY stripes");
    // nothing to match is no refusal
    const sdr::Plan none = sdr::make_plan(params(0, 64, 5, 50, 300, 31, 10, M, 4), BT, 60, 100, 1, 1);
    CHECK(none.rc == SDR_OK && none.empty && none.cells == 0 && sdr::plan_scratch_bytes(none) > 0);
}

void pairing() {
    sdr_sgbm_params l = params(0, 64, 5, 50, 300, 31, 10, SDR_MODE_SGBM, 4), r{};
    l.disp12MaxDiff = 1000000;
    r = l;
    r.minDisparity = -(l.minDisparity + l.numDisparities) + 1;  // createRightMatcher
    const sdr::Plan a = sdr::make_plan(l, SDR_COST_BT, 320, 100, 3, 1), b = sdr::make_plan(r, SDR_COST_BT, 320, 100, 3, 1);
    CHECK(a.rc == SDR_OK && b.rc == SDR_OK && sdr::can_pair(a.e, b.e));
    const sdr::Plan ab = sdr::plan_pair(a, b);
    CHECK(ab.rc == SDR_OK && ab.F == 6 && ab.e.g.split == 3 && ab.e.g.minDb == -63 && ab.e.g.minX1b == b.e.g.minX1);
    CHECK(ab.lr_skipped && ab.cells == a.cells);
    r.P2 = 301;
    const sdr::Plan c = sdr::make_plan(r, SDR_COST_BT, 320, 100, 3, 1);
    const sdr::Plan ac = sdr::plan_pair(a, c);
    CHECK(!sdr::can_pair(a.e, c.e) && ac.rc == SDR_ERR_ARG && std::strstr(ac.why, "cannot be paired"));
    const sdr::Plan b2 = sdr::make_plan(r = l, SDR_COST_BT, 320, 100, 4, 1);
    CHECK(sdr::plan_pair(a, b2).rc == SDR_ERR_ARG);  // frame counts differ
    l.numDisparities = 24;
    const sdr::Plan bad = sdr::make_plan(l, SDR_COST_BT, 320, 100, 3, 1);
    CHECK(sdr::plan_pair(bad, b).rc == SDR_ERR_NUMDISP && sdr::plan_pair(b, bad).rc == SDR_ERR_NUMDISP);
}

}  // namespace

int main() {
    grid();
    refusals();
    pairing();
    std::printf("plan_check: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
