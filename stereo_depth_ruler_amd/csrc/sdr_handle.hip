// sdr_handle.hip -- the matcher handle: its life, parameters, stream binding, timers, status and
// debug read-back (the handle's part of include/sdr/sdr.h; the struct: sdr_handle.hpp).
#include "sdr_handle.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace sdr {

// A stream being captured into a graph (hipStreamBeginCapture, torch.cuda.graph).
bool capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}
// The handle's last enqueue, for the next stream that uses its scratch (h->done).
//  * On a persistent stream (the handle's own, or a caller's declared so: torch's pooled streams)
//    the record is lazy: only when the handle moves to another stream does its old stream get the
//    event (after everything queued there so far, the handle's work included), and the new stream
//    wait on it.  An event record is a queue barrier: recorded after every call it left a ~6 us
//    idle gap per class-path frame (rounds 4 and 5).
//  * On a transient caller stream (sdr_sgbm_set_stream; the caller may destroy it as soon as its
//    work is done) the event is recorded at the end of every call, and relayed through the
//    handle's own stream (that stream waits on it, then the event is recorded again there), so
//    neither a later switch nor destroy touches the caller's stream: HIP does not validate a
//    destroyed stream's handle, and an event whose last record was on one crashes a later wait
//    (round 5, gpurun_out/r5b/tests.log).
// Nothing is recorded into or waited on from a graph capture: the capture's replays order
// themselves.
// `done` after everything queued on `from`, re-recorded on the handle's own stream
hipError_t relay(sdr_sgbm* h, hipStream_t from) {
    hipError_t e = hipEventRecord(h->done, from);
    if (e == hipSuccess) e = hipStreamWaitEvent(h->own_stream, h->done, 0);
    if (e == hipSuccess) e = hipEventRecord(h->done, h->own_stream);
    h->relayed = e == hipSuccess;
    return e;
}
hipError_t retire(sdr_sgbm* h) {
    if (h->persistent) {
        h->pending = true;
        return hipSuccess;
    }
    if (!h->done || capturing(h->stream)) return hipSuccess;
    return relay(h, h->stream);
}
// At the start of a call: the handle's stream waits for work the handle queued elsewhere and
// has not been ordered before it yet (the class path's unpaired right matcher, run on a side stream)
hipError_t begin_call(sdr_sgbm* h) {
    if (!h->needs_wait) return hipSuccess;
    h->needs_wait = false;
    if (capturing(h->stream)) return hipSuccess;
    return hipStreamWaitEvent(h->stream, h->done, 0);
}
int use_stream(sdr_sgbm* h, hipStream_t s, bool persistent) {
    // a stream being captured neither queries nor waits on an event recorded outside the capture
    // (both invalidate a global-mode capture); torch.cuda.graph synchronises before it captures,
    // and a caller capturing by hand orders the handle's earlier work before the capture itself
    persistent = persistent || s == h->own_stream;
    if (s == h->stream) {
        // the same stream, now declared transient: record what the persistent form left pending
        // (the stream exists: this call names it)
        hipError_t e = hipSuccess;
        if (h->persistent && !persistent && h->pending) {
            h->persistent = false;
            h->pending = false;
            e = retire(h);
        }
        h->persistent = persistent;
        if (e != hipSuccess)
            return set_error(SDR_ERR_DEVICE, std::string("ordering the handle's work on its stream: ") + hipGetErrorString(e));
        return SDR_OK;
    }
    hipError_t e = hipSuccess;
    bool wait = false;
    if (h->pending && h->done && !capturing(h->stream) && !capturing(s)) {
        // h->pending implies a persistent previous stream: it still exists
        e = hipEventRecord(h->done, h->stream);
        wait = true;
    } else if (h->relayed && !capturing(s)) {
        wait = true;  // recorded on the handle's own stream: no caller stream is touched
    }
    if (wait && e == hipSuccess) e = hipStreamWaitEvent(s, h->done, 0);
    // the handle moves to s even when the ordering failed: the error is reported once and the
    // handle stays usable on s
    h->pending = false;
    h->relayed = false;
    h->needs_wait = false;
    h->stream = s;
    h->persistent = persistent;
    if (e != hipSuccess)
        return set_error(SDR_ERR_DEVICE, std::string("ordering the handle's previous stream before the new one: ") +
                                             hipGetErrorString(e));
    return SDR_OK;
}

bool ktimer_begin(sdr_sgbm* h, int kind) {
    if (h->timing < 2) return false;
    if (h->kused * 2 + 2 > h->kev.size()) {
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreateWithFlags(&a, kTimerEvent) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&b, kTimerEvent) != hipSuccess) {
            (void)hipEventDestroy(a);
            return false;
        }
        h->kev.push_back(a);
        h->kev.push_back(b);
        h->kkind.push_back(kind);
    }
    h->kkind[h->kused] = kind;
    (void)hipEventRecord(h->kev[2 * h->kused], h->stream);
    return true;
}

bool path_order_col() {
    const char* o = getenv("SDR_PATH_ORDER");
    return !(o && std::string(o) == "row");
}

void ktimer_end(sdr_sgbm* h) {
    (void)hipEventRecord(h->kev[2 * h->kused + 1], h->stream);
    h->kused++;
}

}  // namespace sdr

using sdr::Buf;
using sdr::set_error;

extern "C" {

int sdr_sgbm_create(const sdr_sgbm_params* p, int device, sdr_sgbm** out) {
    if (!p || !out) return set_error(SDR_ERR_ARG, "null argument");
    *out = nullptr;
    int ndev = 0;
    SDR_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return set_error(SDR_ERR_DEVICE, "invalid device index");
    SDR_HIP(hipSetDevice(device));
    sdr_sgbm* h = new sdr_sgbm();
    h->p = *p;
    h->device = device;
    const char* rec = getenv("SDR_PATH_REC");
    h->rec16 = rec && atoi(rec) == 16;
    h->rec_col = sdr::path_order_col();
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return set_error(SDR_ERR_DEVICE, "hipStreamCreate failed");
    }
    h->stream = h->own_stream;
    for (auto& ev : h->ev) (void)hipEventCreateWithFlags(&ev, sdr::kTimerEvent);
    (void)hipEventCreateWithFlags(&h->done, sdr::kOrderEvent);
    *out = h;
    return SDR_OK;
}

int sdr_sgbm_destroy(sdr_sgbm* h) {
    if (!h) return SDR_OK;
    (void)hipSetDevice(h->device);
    // a transient caller stream is never touched after its call: the relay put its work on own_stream
    if (h->stream && h->persistent) (void)hipStreamSynchronize(h->stream);
    if (h->own_stream && h->own_stream != h->stream) (void)hipStreamSynchronize(h->own_stream);
    if (h->status_host) (void)hipHostFree(h->status_host);
    for (Buf* b : {&h->sweep, &h->status, &h->planesL, &h->planesR, &h->sink, &h->C, &h->Lr, &h->Caux, &h->draw, &h->dlr, &h->dfin, &h->keys2,
                   &h->labels, &h->sizes, &h->mins, &h->hin, &h->hxyz, &h->cls_bgr,
                   &h->cls_gray, &h->cls_small, &h->cls_dl, &h->cls_wls, &h->cls_f,
                   &h->cls_conf, &h->cls_filt})
        if (b->p) (void)hipFree(b->p);
    h->hx.release();
    for (auto ev : h->ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto ev : h->kev) (void)hipEventDestroy(ev);
    if (h->side) (void)hipStreamSynchronize(h->side);
    if (h->fork) (void)hipEventDestroy(h->fork);
    if (h->join) (void)hipEventDestroy(h->join);
    if (h->done) (void)hipEventDestroy(h->done);
    if (h->side) (void)hipStreamDestroy(h->side);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return SDR_OK;
}

int sdr_sgbm_set_params(sdr_sgbm* h, const sdr_sgbm_params* p) {
    if (!h || !p) return set_error(SDR_ERR_ARG, "null argument");
    h->p = *p;
    return SDR_OK;
}

int sdr_sgbm_get_params(const sdr_sgbm* h, sdr_sgbm_params* p) {
    if (!h || !p) return set_error(SDR_ERR_ARG, "null argument");
    *p = h->p;
    return SDR_OK;
}

int sdr_sgbm_set_cost(sdr_sgbm* h, int cost) {
    if (!h) return set_error(SDR_ERR_ARG, "null handle");
    if (cost != SDR_COST_BT && cost != SDR_COST_CENSUS_9X7) return set_error(SDR_ERR_ARG, "unknown cost type");
    h->cost = cost;
    return SDR_OK;
}

int sdr_sgbm_get_cost(const sdr_sgbm* h) { return h ? h->cost : set_error(SDR_ERR_ARG, "null handle"); }

int sdr_sgbm_set_stream(sdr_sgbm* h, void* stream) {
    if (!h) return set_error(SDR_ERR_ARG, "null handle");
    (void)hipSetDevice(h->device);
    // NULL = the HIP null (legacy default) stream, which always exists
    return sdr::use_stream(h, (hipStream_t)stream, stream == nullptr);
}

int sdr_sgbm_set_stream_ex(sdr_sgbm* h, void* stream, int flags) {
    if (!h) return set_error(SDR_ERR_ARG, "null handle");
    if (flags & ~SDR_STREAM_PERSISTENT) return set_error(SDR_ERR_ARG, "unknown stream flags");
    (void)hipSetDevice(h->device);
    return sdr::use_stream(h, (hipStream_t)stream, stream == nullptr || (flags & SDR_STREAM_PERSISTENT));
}

int sdr_sgbm_reset_stream(sdr_sgbm* h) {
    if (!h) return set_error(SDR_ERR_ARG, "null handle");
    (void)hipSetDevice(h->device);
    return sdr::use_stream(h, h->own_stream, true);
}

void* sdr_sgbm_get_stream(const sdr_sgbm* h) { return h ? (void*)h->stream : nullptr; }

int sdr_sgbm_enable_timing(sdr_sgbm* h, int enable) {
    if (!h) return set_error(SDR_ERR_ARG, "null handle");
    h->timing = enable < 0 ? 0 : enable;
    h->kused = 0;
    return SDR_OK;
}

int sdr_sgbm_last_timing(const sdr_sgbm* h, float* cost_ms, float* paths_ms, float* post_ms) {
    if (!h || !h->timing) return set_error(SDR_ERR_ARG, "timing not enabled");
    SDR_HIP(hipEventSynchronize(h->ev[3]));
    float a = 0, b = 0, c = 0;
    SDR_HIP(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
    SDR_HIP(hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
    SDR_HIP(hipEventElapsedTime(&c, h->ev[2], h->ev[3]));
    if (cost_ms) *cost_ms = a;
    if (paths_ms) *paths_ms = b;
    if (post_ms) *post_ms = c;
    return SDR_OK;
}

int sdr_sgbm_kernel_time(sdr_sgbm* h, int kind, int reset, float* total_ms, int* count) {
    if (!h) return set_error(SDR_ERR_ARG, "null handle");
    float tot = 0;
    int n = 0;
    if (h->kused) {
        SDR_HIP(hipEventSynchronize(h->kev[2 * h->kused - 1]));
        for (size_t i = 0; i < h->kused; i++) {
            if (kind >= 0 && h->kkind[i] != kind) continue;
            float ms = 0;
            SDR_HIP(hipEventElapsedTime(&ms, h->kev[2 * i], h->kev[2 * i + 1]));
            tot += ms;
            n++;
        }
    }
    if (total_ms) *total_ms = tot;
    if (count) *count = n;
    if (reset) h->kused = 0;
    return SDR_OK;
}

int sdr_sgbm_last_status(sdr_sgbm* h) {
    if (!h) return set_error(SDR_ERR_ARG, "null handle");
    if (!h->status_host) return SDR_OK;  // no sweep batch has run on this handle
    SDR_HIP(hipSetDevice(h->device));
    if (h->persistent) SDR_HIP(hipStreamSynchronize(h->stream));
    SDR_HIP(hipStreamSynchronize(h->own_stream));  // relayed work (transient streams, side stream)
    const int n = __atomic_load_n(h->status_host, __ATOMIC_ACQUIRE);
    if (n == h->status_reported) return SDR_OK;
    h->status_reported = n;  // the device word counts timeouts and is never cleared
    return set_error(SDR_ERR_DEVICE, "a MODE_HH row sweep timed out waiting for a neighbouring tile: that "
                                     "batch's frames were written as INVALID");
}

int sdr_sgbm_debug_knob(sdr_sgbm* h, int knob, int value) {
    if (!h) return set_error(SDR_ERR_ARG, "null handle");
    if (knob == SDR_DEBUG_PLAN_CUS) {
        h->plan_cus = value > 0 ? value : 0;
        return SDR_OK;
    }
    if (knob == SDR_DEBUG_COST_ROWS) {
        h->cost_rows = value > 0 ? value : 0;
        return SDR_OK;
    }
    if (knob != SDR_DEBUG_SWEEP_SPIN) return set_error(SDR_ERR_ARG, "unknown knob");
    h->sweep_spin = value > 0 ? value : sdr::kSweepSpin;
    return SDR_OK;
}

int sdr_sgbm_debug_stage(const sdr_sgbm* h, int stage, void* dst, size_t bytes) {
    if (!h || !dst) return set_error(SDR_ERR_ARG, "null argument");
    const Buf* b = stage == 0 ? &h->C : stage == 1 ? &h->draw : stage == 2 ? &h->dlr
                 : stage == 3 ? &h->dfin : stage == 4 ? &h->Lr : stage == 5 ? &h->keys2
                 : stage == 6 ? &h->Caux : stage == 7 ? &h->planesR : stage == 8 ? &h->planesL
                 : stage == 9 ? &h->planesR : nullptr;
    if (!b) return set_error(SDR_ERR_ARG, "bad stage");
    const sdr::Plan& pl = h->last;
    if (stage == 8 || stage == 9) {
        // the prefilter's operands: the census cost keeps its descriptors in the same buffer
        if (pl.census()) return set_error(SDR_ERR_ARG, "the last compute used the census cost");
        const size_t have = (size_t)pl.F * 3 * pl.px * pl.cn * (stage == 8 ? 4 : 8);
        if (bytes > have) return set_error(SDR_ERR_ARG, "stage buffer smaller than requested");
    }
    if (stage == 7 && !pl.census_bytes()) return set_error(SDR_ERR_ARG, "the last compute did not use the census cost");
    if (stage == 7 && bytes > pl.census_bytes()) return set_error(SDR_ERR_ARG, "stage buffer smaller than requested");
    // front slack (the L records' is P-1 times C's)
    const size_t skip = stage == 0 ? pl.slack * 2 : stage == 4 ? pl.lslack * 2
                      : stage == 6 ? pl.aux_slack * 2 : 0;
    if (!b->p || bytes + skip > b->n) return set_error(SDR_ERR_ARG, "stage buffer smaller than requested");
    SDR_HIP(hipSetDevice(h->device));
    // the LR-checked map is never written by the pipeline: materialise it for this stage (when the
    // last compute skipped the no-op LR check, from the WTA map alone)
    if (stage == 2 && h->draw.p && h->dlr.p) {
        const sdr::Geometry& g = pl.e.g;
        if (pl.lr_skipped)
            sdr::launch_mask_cols((const int16_t*)h->draw.p, (int16_t*)h->dlr.p, g, pl.F, h->stream);
        else
            sdr::launch_lr_apply(g, (const int16_t*)h->draw.p, (const uint32_t*)h->keys2.p,
                                 (int16_t*)h->dlr.p, pl.px, pl.e.disp12MaxDiff, pl.F, h->stream);
    }
    SDR_HIP(hipStreamSynchronize(h->stream));
    const sdr_sgbm_records& rc = pl.records;
    if (stage == 4 && rc.order == SDR_SGBM_RECORDS_BY_COLUMN) {
        // the stage's documented layout is by row: copy the frames the request touches whole and
        // turn each frame's [W1][H] records to [H][W1] here; the rest of a frame's span (unused by
        // 12-bit records) goes out as it is
        const size_t fb = (size_t)rc.frame * 2, rb = (size_t)rc.pix * 2;
        const size_t W1 = pl.e.g.W1, H = pl.e.g.H;
        const size_t nf = std::min((bytes + fb - 1) / fb, (size_t)pl.F);
        if (bytes > nf * fb) return set_error(SDR_ERR_ARG, "stage buffer smaller than requested");
        std::vector<char> dev(nf * fb), out(nf * fb);
        SDR_HIP(hipMemcpy(dev.data(), (const char*)b->p + skip, nf * fb, hipMemcpyDeviceToHost));
        out = dev;
        for (size_t f = 0; f < nf; f++)
            for (size_t y = 0; y < H; y++)
                for (size_t x = 0; x < W1; x++)
                    memcpy(&out[f * fb + (y * W1 + x) * rb], &dev[f * fb + (x * H + y) * rb], rb);
        memcpy(dst, out.data(), bytes);
        return SDR_OK;
    }
    SDR_HIP(hipMemcpy(dst, (const char*)b->p + skip, bytes, hipMemcpyDeviceToHost));
    return SDR_OK;
}

}  // extern "C"
