// sdr_plan.hpp -- the plan of one matcher call: what the call will do, derived once on the host.
//
// make_plan() defaults the parameters as OpenCV does, lays out the 3WAY stripes and refuses what
// the engine cannot run; it makes no HIP call.  Everything that sizes scratch, launches a stage or
// reads a stage back (sdr_sgbm_scratch_bytes*, enqueue_compute, sdr_sgbm_debug_stage) reads this
// record, not the parameters.  The two decisions that depend on the device -- the sweep shapes and
// the 12-bit record format -- are completed into it by the enqueue, once per call.
#pragma once
#include "sdr_internal.hpp"

namespace sdr {

// The parameters as the algorithm uses them.
struct Eff {
    Geometry g;
    int mode, uniq, uniq_simd, disp12MaxDiff, ftzero, nstripes, invalid;
    int speckle_ws, speckle_diff, blockSize;
    int cost;  // SDR_COST_*
};

// One MODE_SGBM_3WAY stripe: chain rows [s0, end), output rows [out0, end), its first aux_rows
// cost rows in the stripe's own band of Caux, the box frozen below row ylim.
struct Stripe {
    int s0, end, out0, aux_rows, ylim;
};

// the top-to-bottom direction of every stripe plus E and W must fit one PathLaunch
constexpr int kMaxStripes = kMaxPathDirs - 2;
// batches from this many frames run MODE_HH's N/NE/NW and SE/SW as row sweeps (k_sweep): a sweep
// walks a frame's rows in order, so it pays one cross-tile hand-over per row per frame and only
// amortises that latency over several frames in flight
constexpr int kSweepMinFrames = 8;

struct Plan {
    int rc = SDR_OK;        // the refusal, SDR_OK when the call runs
    const char* why = "";   // its text (sdr_last_error)
    bool defaulted = false; // e is complete (the refusal, if any, came after the defaulting)
    Eff e{};                // e.g.split / minDb / minX1b describe the pairing
    int F = 0, cn = 1;      // frames (both matchers' when paired), channels
    bool empty = false;     // W1 <= 0: nothing is matched, the output is all INVALID
    size_t px = 0;          // W * H
    size_t cells = 0;       // H * W1 * D: elements of a frame's cost volume
    int npaths = 0;         // directions of the mode
    // MODE_SGBM_3WAY: stripe s keeps its start rows at Caux + s * amax * W1 * D of every frame
    int nstr = 0, amax = 0;
    Stripe stripes[kMaxStripes];
    size_t aux_fstride = 0; // elements per frame of Caux
    // elements of slack in front of C and of Caux (the path kernels' loads overrun a chain's ends
    // by up to kSouthPad rows; the E/W chains redirected into Caux by a lookahead past a row's ends)
    size_t slack = 0, aux_slack = 0;
    // A.9 can only invalidate a pixel when |disp2 - d| > disp12MaxDiff; both lie in [minD, maxD),
    // so from disp12MaxDiff >= D on (ximgproc's WLS filter sets 1000000 on the class path's left
    // matcher, createRightMatcher on the right one) the check is the identity on the matched
    // columns and INVALID elsewhere: the median reads the WTA map with that column mask instead,
    // and no right-view keys are built
    bool lr_skipped = false;

    // ---- completed by the enqueue (plan_sweep, then the record format) ----
    // batched MODE_HH: N/NE/NW and S/SE/SW as two row-synchronous sweeps (when every tile of the
    // frames in flight fits the resident grid); the records are then E, W and up -- saturated sums
    // of non-negative path costs, so the grouping is exact -- and the down sweep runs the WTA
    SweepShape shp[2] = {};  // [0]: down (S, SE, SW + WTA), [1]: up (N, NE, NW)
    bool sweep = false;
    int nrec = 0;            // L records per pixel
    // elements of slack in front of the L records and behind them: kSouthPad records a column in the
    // larger of the two orders' y strides (W1 * nrec * D; by column a y step is one record)
    size_t lslack = 0;
    size_t lfs = 0;          // L elements per frame, [H][W1][nrec][D] or [W1][H][nrec][D] (records)
    // [pass][slots][tiles][2] counters, then the edge ring (sized for either pass)
    size_t flags_n[2] = {0, 0}, sweep_flags = 0, edge_bytes = 0;
    bool rec12 = false;      // 12-bit path-cost records (PathLaunch::rec12)
    // the records' order (PathLaunch::l_xs, l_ys): by column, [F][W1][H][nrec]..., where the fused
    // pass is the one-column k_south_wta fed by one-chain k_paths; by row, [F][H][W1][nrec]..., else
    sdr_sgbm_records records{};
    // the kernel of every launch, as the launchers switch on it (sdr_sgbm_last_plan)
    sdr_sgbm_launches launches{};

    bool census() const { return e.cost == SDR_COST_CENSUS_9X7; }
    bool speckle() const { return e.speckle_ws > 0; }
    // the census descriptors [F][2][H][W] take 16 of planesR's 24 bytes a pixel (0: the BT cost)
    size_t census_bytes() const { return census() ? (size_t)F * 2 * px * 8 : 0; }
    // a batch that could take the sweep (it does not inside a graph capture)
    bool sweep_batch() const { return e.mode == SDR_MODE_HH && F >= kSweepMinFrames; }
    // elements from a frame's start in Caux to stripe s's band
    size_t aux_off(int s) const { return (size_t)s * amax * e.g.W1 * e.g.D; }
};

// The plan of F frames of W x H x cn under p and the cost type.  Refusals keep the order of the
// checks: defaulting, channels, then -- for a frame that matches anything -- the frame size and
// the stripe limits.
Plan make_plan(const sdr_sgbm_params& p, int cost, int W, int H, int F, int cn);
// Paired matchers (the class path): frames [0, a.F) run a's parameters on (L, R), frames
// [a.F, 2 a.F) the right matcher's, b's, on (R, L) -- right_matcher->compute(R, L) -- in the same
// launches.  Only when the two differ in minDisparity alone and match the same number of columns
// (createRightMatcher + the WLS filter's mutations give exactly that).
bool can_pair(const Eff& a, const Eff& b);
Plan plan_pair(const Plan& a, const Plan& b);
// Decides the sweep (shp: sweep_shape() of both passes, all zero when the batch takes none) and
// what follows from it: the records per pixel, their slack and the sweep's flag and ring sizes.
void plan_sweep(Plan* pl, const SweepShape shp[2]);
// Device bytes a call of this plan needs (sdr_sgbm_scratch_bytes*): the planes, the cost volume
// and one L volume a direction, the stripe-start rows, the maps and keys.
size_t plan_scratch_bytes(const Plan& pl);

}  // namespace sdr
