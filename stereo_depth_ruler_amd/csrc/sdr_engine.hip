// sdr_engine.hip -- scheduling of the stage kernels: the compute entries and the class path of
// the C ABI (include/sdr/sdr.h).
//
// compute_device() enqueues the whole hot path of cv::StereoSGBM::compute on the handle's stream:
//   prefilter -> cost volume (+ 3WAY stripe-start rows) -> path kernels (first writes S, middle
//   ones accumulate, last one fuses WTA/uniqueness/subpixel) -> disp2 + LR check -> median3
//   -> speckle CCL [-> min -> reprojectImageTo3D]
// What a call does is decided once, by its plan (sdr_plan.hpp); the stages below read it.
// No host synchronisation, allocation or copy happens inside the enqueue once scratch is sized,
// so the sequence can be captured into a hipGraph by the caller.
#include "sdr_device.hpp"
#include "sdr_handle.hpp"

#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>

using sdr::ensure;
using sdr::KTimer;
using sdr::Plan;
using sdr::retire;
using sdr::stage_bytes;

namespace {

int fail(int code, const char* msg) { return sdr::set_error(code, msg); }
int refuse(const Plan& pl) { return sdr::set_error(pl.rc, pl.why); }

// A sweep's workgroups wait on each other, so its grid must become resident as a whole: other
// kernels only delay that (they finish without waiting on anything), but two sweeps in flight at
// once could each hold part of the chip while waiting for the rest.  Sweeps of every handle and
// stream of a device are therefore chained in submission order through one event per device.
std::mutex g_sweep_mu;
std::map<int, hipEvent_t> g_sweep_last;

// What a call reads and writes besides the handle's scratch: F frames already on the device,
//   out (nullable): dense [F][H][W] int16 destination for the final map (else internal buffer)
//   out_min (nullable): per-frame minimum of the final map (reprojectImageTo3D handleMissing)
struct Io {
    const uint8_t *L, *R;
    size_t stride, fstride;
    int16_t* out;
    int* out_min;
};

// the call's volumes inside the handle's buffers, behind their front slack
int16_t* vol_C(const sdr_sgbm* h, const Plan& p) { return (int16_t*)h->C.p + p.slack; }
int16_t* vol_Caux(const sdr_sgbm* h, const Plan& p) { return (int16_t*)h->Caux.p + p.aux_slack; }
int16_t* vol_L(const sdr_sgbm* h, const Plan& p) { return (int16_t*)h->Lr.p + p.lslack; }  // [F][H][W1][nrec][D], or by column (record_order)
// the right-view WTA keys; none are built when the LR check is skipped
uint32_t* keys_of(const sdr_sgbm* h, const Plan& p) { return p.lr_skipped ? nullptr : (uint32_t*)h->keys2.p; }

// Completes the plan's sweep decision and sizes the handle's scratch for it; from its return on
// the handle's buffers belong to this call (h->last).
int size_scratch(sdr_sgbm* h, Plan* pl) {
    const sdr::Geometry& g = pl->e.g;
    const size_t F = pl->F, px = pl->px, cn = pl->cn;
    sdr::SweepShape shp[2] = {};
    // (not inside a graph capture: its replays could overlap another sweep's, which the event
    // chain of the sweep stage orders for directly enqueued sweeps only)
    if (pl->sweep_batch() && !sdr::capturing(h->stream))
        for (int up = 0; up < 2; up++) shp[up] = sdr::sweep_shape(g, pl->F, up != 0);
    sdr::plan_sweep(pl, shp);
    int rc;
    if ((rc = ensure(h->planesL, F * 3 * px * 4 * cn))) return rc;
    if ((rc = ensure(h->planesR, F * 3 * px * 8 * cn))) return rc;
    if ((rc = ensure(h->sink, sdr::cost_sink_bytes(g)))) return rc;
    // a batch that can take the sweep sizes L for the chains' P - 1 records too, so a graph
    // capture of the same shape (chains only) allocates nothing
    const size_t lrec = pl->sweep_batch() ? (size_t)(pl->npaths - 1) : (size_t)pl->nrec;
    if ((rc = ensure(h->C, (F * pl->cells + 2 * pl->slack) * 2))) return rc;
    if ((rc = ensure(h->Lr, (F * pl->cells + 2 * pl->slack) * lrec * 2))) return rc;
    if ((rc = ensure(h->keys2, F * px * 4))) return rc;
    if ((rc = ensure(h->Caux, (F * pl->aux_fstride + 2 * pl->aux_slack) * 2))) return rc;
    if ((rc = ensure(h->draw, F * px * 2))) return rc;
    if ((rc = ensure(h->dlr, F * px * 2))) return rc;
    if (pl->speckle()) {
        if ((rc = ensure(h->labels, F * px * 4))) return rc;
        if ((rc = ensure(h->sizes, F * px * 4))) return rc;
    }
    h->last = *pl;
    return SDR_OK;
}

// The sweep's flags, error word and edge ring, and the handle's status word with its host copy.
int size_sweep(sdr_sgbm* h, const Plan& p) {
    int rc;
    if ((rc = ensure(h->sweep, p.sweep_flags + 256 + p.edge_bytes))) return rc;
    if (h->status_host) return SDR_OK;
    if ((rc = ensure(h->status, 256))) return rc;
    SDR_HIP(hipMemsetAsync(h->status.p, 0, 256, h->stream));
    if (hipHostMalloc((void**)&h->status_host, sizeof(int), hipHostMallocDefault) != hipSuccess) {
        h->status_host = nullptr;
        return fail(SDR_ERR_NOMEM, "hipHostMalloc failed");
    }
    *h->status_host = 0;
    return SDR_OK;
}

// Prefilter, or the census transform: the cost kernel's operand planes (and the keys' fill).
sdr::Planes stage_planes(sdr_sgbm* h, const Plan& p, const Io& io) {
    const sdr::Geometry& g = p.e.g;
    sdr::Planes pl;
    pl.L = (uint32_t*)h->planesL.p;
    pl.R = (uint64_t*)h->planesR.p;
    pl.fstrideL = pl.fstrideR = 3 * p.px * p.cn;
    pl.cn = p.cn;
    if (p.census()) {
        // the descriptors [F][2][H][W] take 16 of planesR's 24 bytes a pixel
        uint64_t* desc = (uint64_t*)h->planesR.p;
        pl.L = (uint32_t*)desc;
        pl.R = desc + p.px;
        pl.fstrideL = pl.fstrideR = 2 * p.px;
        KTimer kt(h, SDR_KERNEL_PREFILTER);
        sdr::launch_census(io.L, io.R, io.stride, io.fstride, g.W, g.H, p.F, desc, h->stream, g.split, keys_of(h, p));
    } else {
        KTimer kt(h, SDR_KERNEL_PREFILTER);
        sdr::launch_prefilter(io.L, io.R, io.stride, io.fstride, g.W, g.H, p.F, p.e.ftzero, pl, h->stream, g.split,
                              keys_of(h, p));
    }
    return pl;
}

// The cost volume, with the 3WAY stripe-start rows as extra row bands of the same launch.  Returns
// the rows a band and the main bands of a one-pass launch ({0, 0}: the generic cost, or no launch).
sdr::CostBands stage_cost(sdr_sgbm* h, const Plan& p, const sdr::Planes& planes) {
    const sdr::Geometry& g = p.e.g;
    sdr::CostArgs ca{};
    ca.pl = planes;
    ca.out = vol_C(h, p);
    ca.out_fstride = p.cells;
    ca.out_row0 = 0;
    ca.row_begin = 0;
    ca.row_end = g.H;
    ca.s0 = 0;
    ca.ylim = std::max(g.H - 1 - g.SH2, 0);
    // the full-DP cost buffers of MODE_HH and MODE_HH4 keep P2 on the rows the running sum never reaches
    ca.hh_bottom = p.e.mode == SDR_MODE_HH || p.e.mode == SDR_MODE_HH4;
    // 0: sized by the launcher for one full pass of resident blocks (SDR_DEBUG_COST_ROWS: a test's own)
    ca.TY = h->cost_rows;
    ca.sink = (int16_t*)h->sink.p;
    ca.naux = 0;
    ca.aux_fstride = p.aux_fstride;
    for (int s = 0; s < p.nstr; s++) {
        const sdr::Stripe& sp = p.stripes[s];
        if (!sp.aux_rows) continue;
        sdr::CostAux& x = ca.aux[ca.naux++];  // at most kMaxCostAux: the plan's stripe limit
        x.out = vol_Caux(h, p) + p.aux_off(s);
        x.row0 = sp.s0;
        x.rows = sp.aux_rows;
        x.s0 = sp.s0;
        x.ylim = sp.ylim;
    }
    KTimer kt(h, SDR_KERNEL_COST);
    // blockSize 13..17 (within the int16 domain) or D > 256: the two-pass cost through the
    // idle L records
    const sdr::CostChoice cc = sdr::cost_choice(g, p.cn, p.census());
    if (cc.kernel == SDR_SGBM_COST_CENSUS) return sdr::launch_cost_census(g, ca, cc, p.F, h->stream);
    if (cc.kernel == SDR_SGBM_COST_GENERIC) {
        sdr::launch_cost_generic(g, ca, p.F, (uint32_t*)h->Lr.p, h->stream);
        return {0, 0};
    }
    return sdr::launch_cost(g, ca, cc, p.F, h->stream);
}

void add_dir(sdr::PathLaunch& pl, int dir, int nch, int H, int16_t* out) {
    sdr::PathDir d{};
    d.dir = dir;
    d.nchains = nch;
    d.ybeg = 0;
    d.yend = H;
    d.write_from = 0;
    d.out = out;
    pl.d[pl.ndirs++] = d;
}

// The directions of the two path launches.  pls, k_paths: every direction except the
// top-to-bottom one, each into its own L record (in the order E, W, [S], SE, SW, N, NE, NW that
// k_wta_lr's sum uses); plS, k_south_wta: the top-to-bottom chains fused with the WTA, reading
// the other P-1 records.  v: the call's volumes (all null for a plan query, which reads the
// launches' shapes alone).
struct Volumes {
    int16_t *C, *Lr, *Caux;
};
int16_t* at(int16_t* base, size_t off) { return base ? base + off : nullptr; }

void path_dirs(const Volumes& v, const Plan& p, sdr::PathLaunch& pls, sdr::PathLaunch& plS) {
    const sdr::Geometry& g = p.e.g;
    const int H = g.H;
    int16_t* Lr = v.Lr;
    int16_t* Caux = v.Caux;
    pls.C = plS.C = v.C;
    pls.cs_fstride = plS.cs_fstride = p.cells;
    pls.l_fstride = plS.l_fstride = p.lfs;
    pls.l_pix = plS.l_pix = p.nrec * g.D;
    pls.aux_fstride = plS.aux_fstride = p.aux_fstride;
    int nbuf = 0;
    auto buf = [&]() { return at(Lr, (size_t)(nbuf++) * g.D); };
    const int nE = H, nS = g.W1, nD = g.W1 + H - 1;
    // longest chains first: the E/W rows (W1 steps) are dispatched before the shorter ones
    add_dir(pls, sdr::DIR_E, nE, H, buf());
    add_dir(pls, sdr::DIR_W, nE, H, buf());
    if (p.e.mode == SDR_MODE_SGBM_3WAY) {
        for (int s = 0; s < p.nstr; s++) {
            const sdr::Stripe& sp = p.stripes[s];
            add_dir(plS, sdr::DIR_S, nS, H, nullptr);
            sdr::PathDir& d = plS.d[plS.ndirs - 1];
            d.ybeg = sp.s0;
            d.yend = sp.end;
            d.write_from = sp.out0;
            if (sp.aux_rows) {
                d.Caux = at(Caux, p.aux_off(s));
                d.aux_row0 = sp.s0;
                d.aux_rows = sp.aux_rows;
            }
        }
    } else if (p.e.mode == SDR_MODE_HH4) {
        // computeDisparitySGBM_HH4: the two vertical and the two horizontal directions
        add_dir(plS, sdr::DIR_S, nS, H, nullptr);
        add_dir(pls, sdr::DIR_N, nS, H, buf());
    } else if (p.sweep) {
        // record 2: the up sweep; S, SE and SW run in the down sweep with the WTA
    } else {
        add_dir(plS, sdr::DIR_S, nS, H, nullptr);
        if (p.e.mode == SDR_MODE_HH) add_dir(pls, sdr::DIR_N, nS, H, buf());
        add_dir(pls, sdr::DIR_SE, nD, H, buf());
        add_dir(pls, sdr::DIR_SW, nD, H, buf());
        if (p.e.mode == SDR_MODE_HH) {
            add_dir(pls, sdr::DIR_NE, nD, H, buf());
            add_dir(pls, sdr::DIR_NW, nD, H, buf());
        }
    }
    for (int s = 0; s < p.nstr; s++) {
        const sdr::Stripe& sp = p.stripes[s];
        // every row of the stripe comes from its own buffer: its output rows differ from C too
        if (sp.aux_rows == 0 || sp.aux_rows != sp.end - sp.s0 || sp.out0 >= sp.end) continue;
        sdr::RowRedirect& r = pls.redir[pls.nredir++];  // at most kMaxCostAux: the plan's stripe limit
        r.lo = sp.out0;
        r.hi = sp.end;
        r.s0 = sp.s0;
        r.aux = at(Caux, p.aux_off(s));
    }
    for (sdr::PathLaunch* pl : {&pls, &plS}) {
        pl->prefix[0] = 0;
        for (int i = 0; i < pl->ndirs; i++) pl->prefix[i + 1] = pl->prefix[i] + pl->d[i].nchains;
    }
}

// The record format of this call, for both launches: e = C - L lies in [0, P2], so with P2 <=
// 4095 the chains' records take 12 bits a value (1.5 B instead of 2 B per cell and direction,
// written once and read once) and the fused pass rebuilds L = C - e exactly.  Not the sweep
// (k_sweep16 reads int16 records, and its up record is a sum of three), not 3WAY, and only
// where both launchers dispatch a kernel that implements it; the buffer keeps its int16 size.
// rec16: SDR_PATH_REC=16 (sdr_sgbm::rec16); cus: the compute units of the launchers' thresholds.
void record_format(const Volumes& v, Plan& p, sdr::PathLaunch& pls, sdr::PathLaunch& plS, bool rec16, int cus) {
    const sdr::Geometry& g = p.e.g;
    p.rec12 = !rec16 && !p.sweep && g.P2 >= 0 && g.P2 <= 4095 &&
              (p.e.mode == SDR_MODE_SGBM || p.e.mode == SDR_MODE_HH || p.e.mode == SDR_MODE_HH4) &&
              sdr::path_rec12_supported(g, pls, plS, p.nrec + 1, p.F, cus);
    if (!p.rec12) return;
    const int recel = g.D * 3 / 4;  // int16 elements of one direction's record
    pls.rec12 = plS.rec12 = 1;
    pls.l_pix = plS.l_pix = p.nrec * recel;
    for (int i = 0; i < pls.ndirs; i++) pls.d[i].out = at(v.Lr, (size_t)i * recel);
}

// The order of the records, for both launches, through PathLaunch's two strides.  By column,
// [F][W1][H][nrec]...: the fused pass's workgroup then reads its column's records -- a block of
// rows, a consumer wave's four rows -- as one contiguous run instead of pieces a frame row apart.
// Only where that pass is the one-column k_south_wta fed by one-chain k_paths, without 3WAY's
// stripes (either record format); the two-column and two-chain kernels, whose second column or
// chain is a neighbour along x, 3WAY and the sweeps keep row order, [F][H][W1][nrec]....  C stays
// row-major.  col: the handle's SDR_PATH_ORDER.  A frame so tall that a diagonal chain's stores
// between two re-basings would span 2^31 bytes by column keeps row order as well.
void record_order(Plan& p, sdr::PathLaunch& pls, sdr::PathLaunch& plS, const sdr::PathsChoice& pc,
                  const sdr::SouthChoice& sc, bool col) {
    const sdr::Geometry& g = p.e.g;
    auto set = [&](ptrdiff_t xs, ptrdiff_t ys) {
        pls.l_xs = plS.l_xs = xs;
        pls.l_ys = plS.l_ys = ys;
    };
    col = col && !p.sweep && p.nstr == 0 && pls.nredir == 0 && pc.kernel == SDR_SGBM_PATHS_CHAIN &&
          sc.kernel == SDR_SGBM_SOUTH_WTA && !sc.tc;
    if (col) {
        set((ptrdiff_t)g.H * pls.l_pix, pls.l_pix);
        col = sdr::paths_store_span(pls) <= (size_t)INT32_MAX;
    }
    if (!col) set(pls.l_pix, (ptrdiff_t)g.W1 * pls.l_pix);
    sdr_sgbm_records& r = p.records;
    r = sdr_sgbm_records{};
    r.order = col ? SDR_SGBM_RECORDS_BY_COLUMN : SDR_SGBM_RECORDS_BY_ROW;
    r.r12 = p.rec12;
    r.nrec = p.nrec;
    r.pix = pls.l_pix;
    r.xs = pls.l_xs, r.ys = pls.l_ys;
    r.frame = (int64_t)p.lfs;
    r.slack = (int64_t)p.lslack;
    r.reach = (int64_t)sdr::south_reach(g, plS, sc);
}

// The two path launches of a plan whose sweep decision is made (plan_sweep), the record format and
// order and the kernel of every launch; p.launches is the record sdr_sgbm_last_plan and sdr_sgbm_plan_query
// hand out, and pc / sc -- the same values -- are what the launchers switch on.  cus holds for
// the chain-count thresholds alone (SDR_DEBUG_PLAN_CUS): nothing here sizes a grid.
struct PathChoices {
    sdr::PathsChoice pc;
    sdr::SouthChoice sc;
};
PathChoices plan_launches(const Volumes& v, Plan& p, sdr::PathLaunch& pls, sdr::PathLaunch& plS, bool rec16,
                          bool col, int cus) {
    const sdr::Geometry& g = p.e.g;
    path_dirs(v, p, pls, plS);
    record_format(v, p, pls, plS, rec16, cus);
    PathChoices ch;
    ch.pc = sdr::paths_choice(g, pls, p.F, cus);
    ch.sc = sdr::south_choice(g, plS, p.nrec + 1, p.F, cus);
    record_order(p, pls, plS, ch.pc, ch.sc, col);
    const sdr::CostChoice cc = sdr::cost_choice(g, p.cn, p.census());
    sdr_sgbm_launches& o = p.launches;
    o = sdr_sgbm_launches{};
    o.cost_kernel = cc.kernel, o.cost_nr = cc.nr, o.cost_k = cc.k, o.cost_cn = cc.cn;
    o.paths_kernel = ch.pc.kernel, o.paths_dpl = ch.pc.dpl, o.paths_pad = ch.pc.pad, o.paths_r12 = ch.pc.r12;
    o.paths_chains = ch.pc.chains;
    o.south_kernel = ch.sc.kernel, o.south_dpl = ch.sc.dpl, o.south_pad = ch.sc.pad, o.south_np = ch.sc.np;
    o.south_tc = ch.sc.tc, o.south_r12 = ch.sc.r12, o.south_chains = ch.sc.chains;
    if (p.sweep) {
        o.south_kernel = SDR_SGBM_SOUTH_SWEEP;
        o.sweep_dw = g.D <= 128 ? 4 : 8;  // launch_sweep's classes
        o.sweep_pad = g.D < 32 * o.sweep_dw;
        for (int up = 0; up < 2; up++) o.sweep_nslots[up] = p.shp[up].nslots, o.sweep_ntiles[up] = p.shp[up].ntiles;
    }
    o.post = p.speckle() ? SDR_SGBM_POST_SPECKLE : p.lr_skipped ? SDR_SGBM_POST_MEDIAN_COLS : SDR_SGBM_POST_MEDIAN_LR;
    o.cus = cus;
    return ch;
}

// Batched MODE_HH: the up sweep into record 2, then the down sweep with the WTA.
int stage_sweep(sdr_sgbm* h, const Plan& p) {
    const sdr::Geometry& g = p.e.g;
    hipStream_t st = h->stream;
    char* sb = (char*)h->sweep.p;
    SDR_HIP(hipMemsetAsync(sb, 0, p.sweep_flags + sizeof(int), st));
    sdr::SweepArgs sa{};
    sa.C = vol_C(h, p);
    sa.cs_fstride = p.cells;
    sa.l_fstride = p.lfs;
    sa.l_pix = p.nrec * g.D;
    sa.flags = (int*)sb;
    sa.err = (int*)(sb + p.sweep_flags);
    sa.edge = (uint32_t*)(sb + p.sweep_flags + 256);
    sa.spin = h->sweep_spin;
    sdr::SweepWta sw{};
    sw.recs = vol_L(h, p);
    sw.disp_raw = (int16_t*)h->draw.p;
    sw.d2 = keys_of(h, p);
    sw.disp_fstride = p.px;
    sw.uniq = p.e.uniq;
    sw.uniq_simd = p.e.uniq_simd;
    std::lock_guard<std::mutex> lk(g_sweep_mu);
    hipEvent_t& last = g_sweep_last[h->device];
    if (last) SDR_HIP(hipStreamWaitEvent(st, last, 0));
    else SDR_HIP(hipEventCreateWithFlags(&last, sdr::kOrderEvent));
    for (int up = 1; up >= 0; up--) {
        sa.up = up;
        sa.ntiles = p.shp[up].ntiles;
        sa.nslots = p.shp[up].nslots;
        sa.rec = vol_L(h, p) + (size_t)2 * g.D;
        KTimer kt(h, up ? SDR_KERNEL_SWEEP : SDR_KERNEL_SWEEP_DOWN);
        sdr::launch_sweep(g, sa, sw, p.F, st);
        sa.flags += p.flags_n[up];
    }
    SDR_HIP(hipEventRecord(last, st));
    return SDR_OK;
}

// The top-to-bottom chains fused with the WTA (a batch that swept has run it in the down sweep).
void stage_south_wta(sdr_sgbm* h, const Plan& p, const sdr::PathLaunch& plS, const sdr::SouthChoice& sc) {
    sdr::SouthWtaArgs wa{};
    wa.L = vol_L(h, p);
    wa.npaths = p.nrec + 1;
    wa.disp_raw = (int16_t*)h->draw.p;
    wa.d2 = keys_of(h, p);
    wa.disp_fstride = p.px;
    wa.uniq = p.e.uniq;
    wa.uniq_simd = p.e.uniq_simd;
    KTimer kt(h, SDR_KERNEL_WTA_LR);
    sdr::launch_south_wta(p.e.g, plS, wa, sc, p.F, h->stream);
}

// LR check, median and speckle filter into dst, the frame minima, and the sweep's verdict.
int stage_post(sdr_sgbm* h, const Plan& p, int16_t* dst, int* out_min) {
    const sdr::Geometry& g = p.e.g;
    const sdr::Eff& e = p.e;
    hipStream_t st = h->stream;
    int16_t* draw = (int16_t*)h->draw.p;
    int16_t* dfin = (int16_t*)h->dfin.p;
    const sdr::LrSrc lr{g, draw, keys_of(h, p), p.px, e.disp12MaxDiff};
    if (p.speckle()) {
        // the LR check and the median filter run inside the labelling's first pass (dfin = median
        // of the LR-checked map, computed per tile from draw and d2)
        KTimer kt(h, SDR_KERNEL_SPECKLE);
        sdr::launch_speckle(dfin, dst, g.W, g.H, p.F, e.invalid, e.speckle_ws, e.speckle_diff,
                            (int*)h->labels.p, (int*)h->sizes.p, out_min, st, &lr, dfin);
    } else {
        {
            KTimer kt(h, SDR_KERNEL_MEDIAN);
            if (p.lr_skipped) sdr::launch_median3_cols(draw, dst, g, p.F, st);
            else sdr::launch_median3_lr(lr, dst, p.F, st);
        }
        if (out_min) {
            KTimer kt(h, SDR_KERNEL_REPROJECT);
            sdr::launch_min_s16(dst, p.px, p.px, p.F, out_min, st);
        }
    }
    if (p.sweep) {
        // a timed-out wait made this batch's frames wrong: they become INVALID (and the handle's
        // status says so) before anything downstream reads them
        sdr::launch_sweep_verdict((const int*)((char*)h->sweep.p + p.sweep_flags), dst, p.px, p.F,
                                  (int16_t)e.invalid, out_min, (int*)h->status.p, st);
        SDR_HIP(hipMemcpyAsync(h->status_host, h->status.p, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    return SDR_OK;
}

// Enqueues the full compute of a planned call whose inputs are already on the device.
//   prefilter -> cost volume (+ 3WAY stripe-start rows) -> the P-1 directions other than
//   top-to-bottom in one launch, each into its own L buffer -> top-to-bottom chains fused with
//   WTA/uniqueness/subpixel/disp2 -> LR check -> median3 -> speckle
// Per cell this moves 2 (C write) + 4(P-1) (paths: C read + L write) + 2 + 2(P-1) (fused pass:
// C read + the other L reads) = 6P - 2 bytes, 4 fewer than the canonical 2 + 6P of SURVEY.md 8(d).
// planned: the caller's plan (refused ones included: the refusal is reported here, in its place
// among the call's other checks); the enqueue completes it.
int enqueue_compute(sdr_sgbm* h, Plan& planned, const Io& io, int16_t** final_disp) {
    // a batch of an earlier call whose sweep wait gave up (its frames were written as INVALID):
    // reported here, by the next call, if no sdr_sgbm_last_status has reported it yet.  The
    // host copy is refreshed asynchronously after every sweep batch, so this check never waits
    // (a timeout still in flight is reported by the call after)
    // (a count of timed-out batches: each is reported once, whatever copies are still in flight)
    if (h->status_host && __atomic_load_n(h->status_host, __ATOMIC_ACQUIRE) != h->status_reported) {
        h->status_reported = __atomic_load_n(h->status_host, __ATOMIC_ACQUIRE);
        return fail(SDR_ERR_DEVICE, "an earlier MODE_HH batch's row sweep timed out waiting for a neighbouring "
                                    "tile: that batch's frames were written as INVALID (this call did not run)");
    }
    SDR_HIP(sdr::begin_call(h));
    if (planned.rc) return refuse(planned);
    hipStream_t st = h->stream;
    int rc;
    if ((rc = ensure(h->dfin, planned.F * planned.px * 2))) return rc;
    int16_t* dst = io.out ? io.out : (int16_t*)h->dfin.p;
    *final_disp = dst;
    if (planned.empty) {
        sdr::launch_fill_s16(dst, (int16_t)planned.e.invalid, planned.F * planned.px, st);
        if (io.out_min) sdr::launch_min_s16(dst, planned.px, planned.px, planned.F, io.out_min, st);
        return SDR_OK;
    }
    if ((rc = size_scratch(h, &planned))) return rc;
    Plan& p = h->last;
    if (h->timing) SDR_HIP(hipEventRecord(h->ev[0], st));
    if (p.sweep && (rc = size_sweep(h, p))) return rc;

    const sdr::Planes planes = stage_planes(h, p, io);
    const sdr::CostBands cb = stage_cost(h, p, planes);
    if (cb.rows < 0) return fail(SDR_ERR_LIMIT, "no cost kernel is compiled for this plan's block size and channels");
    if (h->timing) SDR_HIP(hipEventRecord(h->ev[1], st));

    sdr::PathLaunch pls{}, plS{};
    // (the debug knob's compute units reach the two chain-count thresholds, nothing else)
    const int cus = h->plan_cus > 0 ? h->plan_cus : sdr::device_cus();
    const PathChoices ch = plan_launches({vol_C(h, p), vol_L(h, p), vol_Caux(h, p)}, p, pls, plS, h->rec16, h->rec_col, cus);
    p.launches.cost_rows = cb.rows, p.launches.cost_bands = cb.bands;
    { KTimer kt(h, SDR_KERNEL_PATHS); sdr::launch_paths(p.e.g, pls, ch.pc, p.F, st); }
    if (p.sweep && (rc = stage_sweep(h, p))) return rc;
    if (h->timing) SDR_HIP(hipEventRecord(h->ev[2], st));

    if (!p.sweep) stage_south_wta(h, p, plS, ch.sc);
    if ((rc = stage_post(h, p, dst, io.out_min))) return rc;
    if (h->timing) SDR_HIP(hipEventRecord(h->ev[3], st));
    SDR_HIP(retire(h));
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

Plan plan_of(const sdr_sgbm* h, int W, int H, int F, int cn) { return sdr::make_plan(h->p, h->cost, W, H, F, cn); }

}  // namespace

// ===========================================================================================
// C ABI: the compute entries
// ===========================================================================================
extern "C" {

size_t sdr_sgbm_scratch_bytes(const sdr_sgbm_params* p, int width, int height, int nframes) {
    return sdr_sgbm_scratch_bytes_cn(p, width, height, 1, nframes);
}

size_t sdr_sgbm_scratch_bytes_cn(const sdr_sgbm_params* p, int width, int height, int channels,
                                 int nframes) {
    return sdr_sgbm_scratch_bytes_ex(p, SDR_COST_BT, width, height, channels, nframes);
}

size_t sdr_sgbm_scratch_bytes_ex(const sdr_sgbm_params* p, int cost, int width, int height, int channels,
                                 int nframes) {
    if (!p) return 0;
    const Plan pl = sdr::make_plan(*p, cost, width, height, std::max(nframes, 1), channels);
    if (pl.rc) {
        refuse(pl);
        return 0;
    }
    return sdr::plan_scratch_bytes(pl);
}

}  // extern "C"

namespace {

// sdr_sgbm_plan_query and sdr_sgbm_records_query: one plan, the launches and (recs) the records
int plan_query(const sdr_sgbm_params* p, int cost, int width, int height, int nframes, int channels, int cus,
               sdr_sgbm_launches* out, sdr_sgbm_records* recs) {
    if (!p || !out) return fail(SDR_ERR_ARG, "null argument");
    if (width <= 0 || height <= 0 || nframes <= 0 || cus < 0) return fail(SDR_ERR_ARG, "bad size, frame count or cus");
    Plan pl = sdr::make_plan(*p, cost, width, height, nframes, channels);
    if (pl.rc) return refuse(pl);
    *out = sdr_sgbm_launches{};
    out->cus = cus ? cus : sdr::device_cus();
    if (pl.empty) return SDR_OK;
    const sdr::Geometry& g = pl.e.g;
    // the sweep decision of size_scratch: on the device its tiling, off it the batch's eligibility
    // (sweep_shape asks the device for the kernels' occupancy; it takes no batch past D = 256)
    sdr::SweepShape shp[2] = {};
    const bool eligible = pl.sweep_batch() && g.D <= 256;
    for (int up = 0; up < 2 && eligible; up++)
        shp[up] = cus ? sdr::SweepShape{0, 0, 1, 0, 0} : sdr::sweep_shape(g, pl.F, up != 0);
    sdr::plan_sweep(&pl, shp);
    sdr::PathLaunch pls{}, plS{};
    const char* rec = getenv("SDR_PATH_REC");
    plan_launches({nullptr, nullptr, nullptr}, pl, pls, plS, rec && atoi(rec) == 16, sdr::path_order_col(), out->cus);
    *out = pl.launches;
    if (cus) out->sweep_nslots[0] = out->sweep_nslots[1] = 0;  // eligible, shape unknown
    if (recs) *recs = pl.records;
    return SDR_OK;
}

}  // namespace

extern "C" {

int sdr_sgbm_plan_query(const sdr_sgbm_params* p, int cost, int width, int height, int nframes, int channels,
                        int cus, sdr_sgbm_launches* out) {
    return plan_query(p, cost, width, height, nframes, channels, cus, out, nullptr);
}

int sdr_sgbm_records_query(const sdr_sgbm_params* p, int cost, int width, int height, int nframes, int channels,
                           int cus, sdr_sgbm_records* out) {
    sdr_sgbm_launches l;
    if (out) *out = sdr_sgbm_records{};
    return plan_query(p, cost, width, height, nframes, channels, cus, out ? &l : nullptr, out);
}

int sdr_sgbm_last_records(const sdr_sgbm* h, sdr_sgbm_records* out) {
    if (!h || !out) return fail(SDR_ERR_ARG, "null argument");
    if (!h->last.launches.cost_kernel) return fail(SDR_ERR_ARG, "no call has run the stages on this handle yet");
    *out = h->last.records;
    return SDR_OK;
}

int sdr_sgbm_last_plan(const sdr_sgbm* h, sdr_sgbm_launches* out) {
    if (!h || !out) return fail(SDR_ERR_ARG, "null argument");
    if (!h->last.launches.cost_kernel) return fail(SDR_ERR_ARG, "no call has run the stages on this handle yet");
    *out = h->last.launches;
    return SDR_OK;
}

int sdr_sgbm_compute_device(sdr_sgbm* h, const uint8_t* dL, const uint8_t* dR, int W, int H,
                            size_t stride, size_t fstride, int F, int16_t* dDisp,
                            size_t disp_stride, size_t disp_fstride) {
    return sdr_sgbm_compute_device_cn(h, dL, dR, W, H, 1, stride, fstride, F, dDisp, disp_stride,
                                      disp_fstride);
}

int sdr_sgbm_compute_device_cn(sdr_sgbm* h, const uint8_t* dL, const uint8_t* dR, int W, int H,
                               int channels, size_t stride, size_t fstride, int F, int16_t* dDisp,
                               size_t disp_stride, size_t disp_fstride) {
    if (!h || !dL || !dR || !dDisp) return fail(SDR_ERR_ARG, "null argument");
    if (channels != 1 && channels != 3) return fail(SDR_ERR_TYPE, "images must have 1 or 3 channels");
    int rc = sdr::check_dims(W * channels, H, stride, F);
    if (rc) return rc;
    if (disp_stride < (size_t)W) return fail(SDR_ERR_ARG, "disp_stride < width");
    if (F > 1 && fstride < stride * H) return fail(SDR_ERR_ARG, "frame_stride too small");
    SDR_HIP(hipSetDevice(h->device));
    int16_t* fin = nullptr;
    const size_t px = (size_t)W * H;
    const bool dense = disp_stride == (size_t)W && (F == 1 || disp_fstride == px);
    Plan pl = plan_of(h, W, H, F, channels);
    if ((rc = enqueue_compute(h, pl, {dL, dR, stride, fstride, dense ? dDisp : nullptr, nullptr}, &fin))) return rc;
    if (!dense) {
        for (int f = 0; f < F; f++)
            SDR_HIP(hipMemcpy2DAsync(dDisp + f * disp_fstride, disp_stride * 2, fin + f * px, W * 2,
                                     W * 2, H, hipMemcpyDeviceToDevice, h->stream));
        SDR_HIP(retire(h));
    }
    return SDR_OK;
}

int sdr_sgbm_compute_reproject_device(sdr_sgbm* h, const uint8_t* dL, const uint8_t* dR, int W,
                                      int H, size_t stride, size_t fstride, int F, int16_t* dDisp,
                                      const double Q[16], int handle_missing, float* dXYZ) {
    if (!h || !dL || !dR || !Q || !dXYZ) return fail(SDR_ERR_ARG, "null argument");
    int rc = sdr::check_dims(W, H, stride, F);
    if (rc) return rc;
    if (F > 1 && fstride < stride * H) return fail(SDR_ERR_ARG, "frame_stride too small");
    SDR_HIP(hipSetDevice(h->device));
    int16_t* fin = nullptr;
    const size_t px = (size_t)W * H;
    if ((rc = ensure(h->mins, (size_t)F * 4 * sdr::kMinSlots))) return rc;
    int* mins = handle_missing ? (int*)h->mins.p : nullptr;
    Plan pl = plan_of(h, W, H, F, 1);
    if ((rc = enqueue_compute(h, pl, {dL, dR, stride, fstride, dDisp, mins}, &fin))) return rc;
    {
        KTimer kt(h, SDR_KERNEL_REPROJECT);
        sdr::launch_reproject_s16(fin, W, H, W, px, Q, handle_missing, mins, dXYZ, (size_t)W * 3,
                                  px * 3, F, h->stream);
    }
    SDR_HIP(retire(h));
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

// The host-pointer entries plan the call before they stage or upload anything: a refusal then
// leaves no DMA in flight from the staging buffer.
int sdr_sgbm_compute(sdr_sgbm* h, const uint8_t* left, const uint8_t* right, int W, int H,
                     int channels, size_t stride, int16_t* disp, size_t disp_stride) {
    if (!h || !left || !right || !disp) return fail(SDR_ERR_ARG, "null argument");
    if (channels != 1 && channels != 3) return fail(SDR_ERR_TYPE, "images must have 1 or 3 channels");
    const int cn = channels;
    int rc = sdr::check_dims(W * cn, H, stride, 1);
    if (rc) return rc;
    if (disp_stride < (size_t)W) return fail(SDR_ERR_ARG, "disp_stride < width");
    Plan pl = plan_of(h, W, H, 1, cn);
    if (pl.rc) return refuse(pl);
    SDR_HIP(hipSetDevice(h->device));
    const size_t px = (size_t)W * H, ib = px * cn;
    if ((rc = ensure(h->hin, 2 * ib))) return rc;
    if ((rc = h->hx.begin(2 * stage_bytes(ib) + stage_bytes(px * 2)))) return rc;
    uint8_t* dL = (uint8_t*)h->hin.p;
    uint8_t* dR = dL + ib;
    if ((rc = h->hx.upload(dL, (size_t)W * cn, left, stride, (size_t)W * cn, H, h->stream))) return rc;
    if ((rc = h->hx.upload(dR, (size_t)W * cn, right, stride, (size_t)W * cn, H, h->stream))) return rc;
    int16_t* fin = nullptr;
    if ((rc = enqueue_compute(h, pl, {dL, dR, (size_t)W * cn, ib, nullptr, nullptr}, &fin))) {
        (void)hipStreamSynchronize(h->stream);  // the uploads from the staging buffer have landed
        return rc;
    }
    if ((rc = h->hx.download(disp, disp_stride * 2, fin, (size_t)W * 2, (size_t)W * 2, H, h->stream))) return rc;
    return h->hx.drain();
}

int sdr_sgbm_compute_reproject(sdr_sgbm* h, const uint8_t* left, const uint8_t* right, int W, int H,
                               size_t stride, int16_t* disp, size_t disp_stride, const double Q[16],
                               int handle_missing, float* xyz, size_t xyz_stride) {
    if (!h || !left || !right || !Q || !xyz) return fail(SDR_ERR_ARG, "null argument");
    int rc = sdr::check_dims(W, H, stride, 1);
    if (rc) return rc;
    if (disp && disp_stride < (size_t)W) return fail(SDR_ERR_ARG, "disp_stride < width");
    if (xyz_stride < (size_t)W * 3) return fail(SDR_ERR_ARG, "xyz_stride < 3*width");
    Plan pl = plan_of(h, W, H, 1, 1);
    if (pl.rc) return refuse(pl);
    SDR_HIP(hipSetDevice(h->device));
    const size_t px = (size_t)W * H;
    if ((rc = ensure(h->hin, 2 * px))) return rc;
    if ((rc = ensure(h->hxyz, px * 12))) return rc;
    if ((rc = ensure(h->mins, 4 * sdr::kMinSlots))) return rc;
    if ((rc = h->hx.begin(2 * stage_bytes(px) + stage_bytes(px * 2) + stage_bytes(px * 12)))) return rc;
    uint8_t* dL = (uint8_t*)h->hin.p;
    uint8_t* dR = dL + px;
    float* dX = (float*)h->hxyz.p;
    if ((rc = h->hx.upload(dL, W, left, stride, W, H, h->stream))) return rc;
    if ((rc = h->hx.upload(dR, W, right, stride, W, H, h->stream))) return rc;
    int16_t* fin = nullptr;
    int* mins = handle_missing ? (int*)h->mins.p : nullptr;
    if ((rc = enqueue_compute(h, pl, {dL, dR, (size_t)W, px, nullptr, mins}, &fin))) {
        (void)hipStreamSynchronize(h->stream);  // the uploads from the staging buffer have landed
        return rc;
    }
    // the disparity's copy-out overlaps the reprojection
    if (disp && (rc = h->hx.download(disp, disp_stride * 2, fin, (size_t)W * 2, (size_t)W * 2, H, h->stream)))
        return rc;
    {
        KTimer kt(h, SDR_KERNEL_REPROJECT);
        sdr::launch_reproject_s16(fin, W, H, W, px, Q, handle_missing, mins, dX, (size_t)W * 3, px * 3, 1,
                                  h->stream);
    }
    SDR_HIP(hipGetLastError());
    SDR_HIP(retire(h));
    if ((rc = h->hx.download(xyz, xyz_stride * 4, dX, (size_t)W * 12, (size_t)W * 12, H, h->stream))) return rc;
    return h->hx.drain();
}

}  // extern "C"

// ===========================================================================================
// The class path
// ===========================================================================================
namespace {

// matcher->compute(L, R) (stereo_disparity.cpp:27) and right_matcher->compute(R, L) (:28) are
// independent until the WLS filter.  When the right matcher differs from the left one in
// minDisparity alone (createRightMatcher after createDisparityWLSFilter: always on the class
// path) both run as ONE batch of 2F frames through the same launches: at 640x360 a matcher's
// row chains fill under a third of the chip, and no stream fork/join is needed.  Otherwise
// the right one runs on a side stream forked from the caller's and joined back before the filter.
struct ClassPlans {
    Plan l, r;  // paired: l is the plan of both matchers' 2F frames
    bool paired = false;
};

ClassPlans plan_class(const sdr_sgbm* left, const sdr_sgbm* right, int w2, int h2, int F) {
    ClassPlans cp;
    cp.l = plan_of(left, w2, h2, F, 1);
    if (!right) return cp;
    cp.r = plan_of(right, w2, h2, F, 1);
    cp.paired = cp.l.defaulted && cp.r.defaulted && sdr::can_pair(cp.l.e, cp.r.e);
    if (cp.paired) cp.l = sdr::plan_pair(cp.l, cp.r);
    return cp;
}

// The unpaired right matcher on the left handle's side stream, forked from st and joined to it
// by left->join.
int class_right_on_side(sdr_sgbm* left, sdr_sgbm* right, Plan& pr, const Io& io, hipStream_t st) {
    int rc;
    if (!left->side) {
        SDR_HIP(hipStreamCreateWithFlags(&left->side, hipStreamNonBlocking));
        SDR_HIP(hipEventCreateWithFlags(&left->fork, sdr::kOrderEvent));
        SDR_HIP(hipEventCreateWithFlags(&left->join, sdr::kOrderEvent));
    }
    SDR_HIP(hipEventRecord(left->fork, st));
    SDR_HIP(hipStreamWaitEvent(left->side, left->fork, 0));
    // the right matcher runs on the side stream and returns to its own stream binding without
    // touching that stream now (a transient one may already be gone): its work is relayed
    // through its own stream and its stream waits on it at its next call (begin_call)
    hipStream_t rs = right->stream;
    const bool rp = right->persistent;
    if ((rc = sdr::use_stream(right, left->side, true))) return rc;
    int16_t* fin = nullptr;
    rc = enqueue_compute(right, pr, io, &fin);
    const hipError_t re = sdr::relay(right, left->side);
    right->pending = false;
    right->stream = rs;
    right->persistent = rp;
    right->needs_wait = true;
    if (rc) return rc;
    SDR_HIP(re);
    SDR_HIP(hipEventRecord(left->join, left->side));
    return SDR_OK;
}

// StereoDisparity::computeDisparity from the half-size gray pair on the device, and optionally
// computeDepth (Q, d_xyz non-null) fused into the WLS epilogue.  given (nullable): the call's
// plans, when the caller has made them already.
int class_enqueue(sdr_sgbm* left, sdr_sgbm* right, sdr_wls* wls, const uint8_t* sl,
                  const uint8_t* sr, int w2, int h2, int F, float* d_out,
                  int16_t* d_filtered, float* d_conf, const double* Q, float* d_xyz,
                  ClassPlans* given = nullptr) {
    if (!left || !sl || !sr || !d_out) return fail(SDR_ERR_ARG, "null argument");
    if (w2 <= 0 || h2 <= 0 || F <= 0) return fail(SDR_ERR_ARG, "bad size");
    if (right && right->device != left->device) return fail(SDR_ERR_ARG, "matchers on different devices");
    if (wls && !right) return fail(SDR_ERR_ARG, "the WLS filter needs the right matcher's disparity");
    SDR_HIP(hipSetDevice(left->device));
    hipStream_t st = left->stream;
    const size_t px2 = (size_t)w2 * h2;
    int rc;
    // dl and dr are one buffer [2F][h][w]: the paired launch writes both
    if ((rc = ensure(left->cls_dl, 2 * F * px2 * 2))) return rc;
    if ((rc = ensure(left->cls_wls, d_filtered ? 0 : F * px2 * 2))) return rc;
    int16_t* dl = (int16_t*)left->cls_dl.p;
    int16_t* dr = dl + F * px2;
    int16_t* dw = d_filtered ? d_filtered : (int16_t*)left->cls_wls.p;
    ClassPlans own;
    if (!given) own = plan_class(left, right, w2, h2, F);
    ClassPlans& cp = given ? *given : own;
    int16_t* fin = nullptr;
    // (the paired plan's frames [F, 2F) take the images swapped: one Io serves both matchers)
    if (!cp.paired && right && (rc = class_right_on_side(left, right, cp.r, {sr, sl, (size_t)w2, px2, dr, nullptr}, st)))
        return rc;
    if ((rc = enqueue_compute(left, cp.l, {sl, sr, (size_t)w2, px2, dl, nullptr}, &fin))) return rc;
    if (!cp.paired && right) SDR_HIP(hipStreamWaitEvent(st, left->join, 0));
    if (wls) {
        // wls_filter->filter(disp_left, left_small, filtered, disp_right) (stereo_disparity.cpp:31)
        // with filtered_disp.convertTo(CV_32F, 1/16) (:34) and computeDepth (:76-80) in its epilogue
        if ((rc = sdr::wls_filter_enqueue(wls, dl, dr, sl, w2, h2, w2, px2, F, dw, d_conf, d_out, Q, d_xyz, st, left)))
            return rc;
    } else {
        if (d_filtered) SDR_HIP(hipMemcpyAsync(d_filtered, dl, F * px2 * 2, hipMemcpyDeviceToDevice, st));
        sdr::launch_disp16_to_f32(dl, d_out, F * px2, st);
        if (d_xyz)
            sdr::launch_reproject_f32(d_out, w2, h2, w2, px2, Q, 0, nullptr, d_xyz, (size_t)w2 * 3, px2 * 3, F, st);
    }
    SDR_HIP(retire(left));
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

}  // namespace

extern "C" {

int sdr_stereo_class_compute_device(sdr_sgbm* left, sdr_sgbm* right, sdr_wls* wls,
                                    const uint8_t* sl, const uint8_t* sr, int w2, int h2, int F,
                                    float* d_out, int16_t* d_filtered, float* d_conf) {
    return class_enqueue(left, right, wls, sl, sr, w2, h2, F, d_out, d_filtered, d_conf, nullptr, nullptr);
}

int sdr_stereo_class_depth_device(sdr_sgbm* left, sdr_sgbm* right, sdr_wls* wls,
                                  const uint8_t* sl, const uint8_t* sr, int w2, int h2, int F,
                                  float* d_out, int16_t* d_filtered, float* d_conf,
                                  const double Q[16], float* d_xyz) {
    if (!Q || !d_xyz) return fail(SDR_ERR_ARG, "null argument");
    return class_enqueue(left, right, wls, sl, sr, w2, h2, F, d_out, d_filtered, d_conf, Q, d_xyz);
}

int sdr_stereo_class_compute(sdr_sgbm* left, sdr_sgbm* right, sdr_wls* wls,
                             const uint8_t* bgr_left, const uint8_t* bgr_right, int W, int H,
                             size_t bgr_stride, float* out, size_t out_stride, int16_t* disp_left,
                             int16_t* disp_right, int16_t* filtered, float* conf) {
    if (!left || !bgr_left || !bgr_right || !out) return fail(SDR_ERR_ARG, "null argument");
    if (W <= 0 || H <= 0 || bgr_stride < (size_t)W * 3) return fail(SDR_ERR_ARG, "bad size/stride");
    if ((W & 1) || (H & 1)) return fail(SDR_ERR_SIZE, "INTER_AREA 0.5x needs even width and height");
    const int w2 = W / 2, h2 = H / 2;
    if (out_stride < (size_t)w2) return fail(SDR_ERR_ARG, "out_stride < width/2");
    int rc;
    ClassPlans cp = plan_class(left, right, w2, h2, 1);
    if (cp.l.rc) return refuse(cp.l);
    if (right && cp.r.rc) return refuse(cp.r);
    SDR_HIP(hipSetDevice(left->device));
    hipStream_t st = left->stream;
    const size_t px = (size_t)W * H, px2 = (size_t)w2 * h2;
    if ((rc = ensure(left->cls_bgr, 2 * px * 3))) return rc;
    if ((rc = ensure(left->cls_gray, 2 * px))) return rc;
    if ((rc = ensure(left->cls_small, 2 * px2))) return rc;
    if ((rc = ensure(left->cls_f, px2 * 4))) return rc;
    if ((rc = ensure(left->cls_conf, conf ? px2 * 4 : 0))) return rc;
    if ((rc = ensure(left->cls_filt, px2 * 2))) return rc;
    uint8_t* bgr = (uint8_t*)left->cls_bgr.p;
    uint8_t* gray = (uint8_t*)left->cls_gray.p;
    uint8_t* small = (uint8_t*)left->cls_small.p;
    float* f = (float*)left->cls_f.p;
    int16_t* filt = (int16_t*)left->cls_filt.p;
    float* dconf = conf ? (float*)left->cls_conf.p : nullptr;
    // host copies through the handle's page-locked staging (DMA straight from/to sdr_host_alloc
    // buffers, e.g. the facade's Mats)
    sdr::HostXfer& hx = left->hx;
    if ((rc = hx.begin(2 * stage_bytes(px * 3) + stage_bytes(px2 * 4) * 3 + stage_bytes(px2 * 2) * 3)))
        return rc;
    if ((rc = hx.upload(bgr, (size_t)W * 3, bgr_left, bgr_stride, (size_t)W * 3, H, st))) return rc;
    if ((rc = hx.upload(bgr + px * 3, (size_t)W * 3, bgr_right, bgr_stride, (size_t)W * 3, H, st))) return rc;
    // cvtColor(BGR2GRAY) x2, resize(0.5, INTER_AREA) x2 (stereo_disparity.cpp:19-24)
    sdr::launch_bgr2gray(bgr, W, H, (size_t)W * 3, gray, W, 2, st);
    sdr::launch_area_half(gray, W, H, W, small, w2, 2, st);
    if ((rc = class_enqueue(left, right, wls, small, small + px2, w2, h2, 1, f, filt, dconf, nullptr, nullptr, &cp))) {
        (void)hipStreamSynchronize(st);  // the uploads from the staging buffer have landed
        return rc;
    }
    if ((rc = hx.download(out, out_stride * 4, f, (size_t)w2 * 4, (size_t)w2 * 4, h2, st))) return rc;
    if (disp_left && (rc = hx.download(disp_left, (size_t)w2 * 2, left->cls_dl.p, (size_t)w2 * 2, (size_t)w2 * 2, h2, st)))
        return rc;
    if (disp_right && right &&
        (rc = hx.download(disp_right, (size_t)w2 * 2, (int16_t*)left->cls_dl.p + px2, (size_t)w2 * 2, (size_t)w2 * 2, h2, st)))
        return rc;
    if (filtered && (rc = hx.download(filtered, (size_t)w2 * 2, filt, (size_t)w2 * 2, (size_t)w2 * 2, h2, st))) return rc;
    if (conf && wls && (rc = hx.download(conf, (size_t)w2 * 4, dconf, (size_t)w2 * 4, (size_t)w2 * 4, h2, st))) return rc;
    return hx.drain();
}

}  // extern "C"
