// sdr_handle.hpp -- the matcher handle and its stream binding, shared by the handle unit
// (sdr_handle.hip) and the scheduling unit (sdr_engine.hip).
//
// One handle = one HIP stream + device scratch sized for the largest (W, H, D, frames) seen.
#pragma once
#include "sdr_host.hpp"
#include "sdr_plan.hpp"
#include "sdr_staging.hpp"

#include <vector>

struct sdr_sgbm {
    sdr_sgbm_params p{};
    int cost = SDR_COST_BT;  // SDR_COST_* (sdr_sgbm_set_cost)
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    sdr::Buf planesL, planesR, sink, C, Lr, Caux, draw, dlr, dfin, labels, sizes, mins, hin, hxyz, keys2;
    // The plan of the last call that ran the stages, as enqueue_compute completed it: what the
    // scratch buffers hold now (sdr_sgbm_debug_stage finds its data with it)
    sdr::Plan last;
    // MODE_HH row sweeps: [2 passes][slots][tiles][2] counters, the call's error word, the edge
    // rings.  status: the handle's sticky status word on the device (set by a batch whose sweep
    // wait timed out, never cleared by a call; sdr_sgbm_last_status reports and clears it),
    // status_host: its page-locked copy, refreshed after every sweep batch
    sdr::Buf sweep, status;
    int* status_host = nullptr;
    int sweep_spin = sdr::kSweepSpin;  // debug knob SDR_DEBUG_SWEEP_SPIN
    // debug knob SDR_DEBUG_PLAN_CUS: the compute units paths_two_chain and south_two_col count
    // with (0: the device's).  Read by enqueue_compute's plan_launches alone -- never by anything
    // that sizes a resident grid (the sweeps' tiling, the cost kernels' row bands)
    int plan_cus = 0;
    // debug knob SDR_DEBUG_COST_ROWS: the rows of a row band of the one-pass cost kernels (0: the
    // launcher's own rule).  The kernels take any band height; nothing here waits on a resident grid
    int cost_rows = 0;
    // SDR_PATH_REC=16 in the environment when the handle was created: int16 path-cost records
    // always (A/B and tests; the default takes 12-bit records where enqueue_compute can)
    bool rec16 = false;
    // SDR_PATH_ORDER in the environment when the handle was created (path_order_col): the records
    // by column where record_order() can (the default), or by row always (=row: A/B and tests)
    bool rec_col = true;
    sdr::HostXfer hx;  // pinned staging of the host-pointer entry points
    sdr::Buf cls_bgr, cls_gray, cls_small, cls_dl, cls_wls, cls_f, cls_conf, cls_filt;
    int timing = 0;  // 0 off, 1 stage events, 2 stage + per-kernel events
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // per-kernel event pairs (timing level 2), harvested by sdr_sgbm_kernel_time
    std::vector<hipEvent_t> kev;
    std::vector<int> kkind;
    size_t kused = 0;
    // class path: the right matcher runs on a side stream forked from / joined to this one
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    // recorded after the last kernel that touches this handle's scratch; a stream switch makes
    // the new stream wait for it, so one matcher used from two streams never overlaps itself
    hipEvent_t done = nullptr;
    bool pending = false;  // work enqueued on a persistent stream since the last switch, not yet recorded
    // the current stream outlives the handle's use of it: the handle's own stream, or a caller's
    // stream declared persistent (sdr_sgbm_set_stream_ex).  Only such a stream is touched after
    // the call that used it has returned (the lazy retire record at a switch, destroy's sync).
    bool persistent = true;
    // `done` was recorded after the handle's last call on a transient stream, relayed through the
    // handle's own stream so that it refers to no caller stream: the next stream waits on it
    bool relayed = false;
    bool needs_wait = false;  // the current stream has not waited on `done` yet (begin_call)
    // sweep timeouts reported so far (the device word counts them; its copy, status_host, is
    // refreshed after every sweep batch)
    int status_reported = 0;
};

namespace sdr {

// Events that only order streams on this device (the handle's retire event, the sweep
// serialisation, the class path's fork / join) and the per-kernel timers: a device-scope release.
// The default event's system-scope release writes back and invalidates the caches at every record:
// on the class path's frame that was a ~5 us idle gap between the matchers and the WLS filter, and
// the kernels after it started on cold caches.  (The host-staging events of drain() keep the
// default: the host reads what they order.)
constexpr unsigned kOrderEvent = hipEventDisableTiming | hipEventReleaseToDevice;
constexpr unsigned kTimerEvent = hipEventReleaseToDevice;

// The stream-binding rules (sdr_handle.hip).
bool capturing(hipStream_t s);
hipError_t relay(sdr_sgbm* h, hipStream_t from);
hipError_t retire(sdr_sgbm* h);
hipError_t begin_call(sdr_sgbm* h);
int use_stream(sdr_sgbm* h, hipStream_t s, bool persistent);
// SDR_PATH_ORDER of the environment now: false for "row", true for anything else (by column is
// the default: k_south_wta 173 -> 160 us on C2, profiles/rec_order/README.md)
bool path_order_col();

// RAII event pair around one kernel launch when per-kernel timing is on.
using KTimer = KScope;

}  // namespace sdr
