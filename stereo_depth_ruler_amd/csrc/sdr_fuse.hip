// sdr_fuse.hip -- the ruler over time: one disparity map from the last frames of a still scene
// (the `f` freeze of stereo_displayer.cpp:191-196, after which every click reads one map).  A
// pixel's valid values over the F frames of a stack vote: their lower median, the values within
// `tol` of it, and with enough of those their ordered double mean or the median itself.  The
// definition is in include/sdr/sdr.h.
//
// k_fuse<T, KMAX> is a pure stream: a thread owns 8 bytes of adjacent pixels of a row (two float,
// four int16; two int16 at KMAX 32) and holds their F <= KMAX values in registers (every loop over the frames is unrolled
// over KMAX with compile-time indices: no register is indexed dynamically), all loads of the thread
// are issued before the first value is used, the median is selected by counting, and the record's
// counts are summed over the wave and the workgroup before one atomic a counter a workgroup, into
// one of kFuseSlots partial records that k_fuse_record adds up (atomics on one 64-byte line run one
// behind another: 225 workgroups on one record cost the 640x360 call 5 us).
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <cmath>

#include "sdr_device.hpp"
#include "sdr_internal.hpp"
#include "sdr_ruler_shared.hpp"

namespace sdr {

static_assert(sizeof(sdr_fuse_params) == 32, "sdr_fuse_params is 32 bytes");
static_assert(sizeof(sdr_fusion) == 64, "sdr_fusion is 64 bytes");
static_assert(offsetof(sdr_fusion, n_fused) == 16 && offsetof(sdr_fusion, sum_support) == 40,
              "sdr_fusion: six counts from byte 16, the 64-bit sums from byte 40");

constexpr int kFuseThreads = 256;
constexpr int kFuseWaves = kFuseThreads / 64;
constexpr int kFuseSlots = 64;  // partial records, one a lane of k_fuse_record's wave
// pixels a thread: 8 bytes of the stack, but two int16 at 32 frames, where four pixels' values take
// every register and leave one wave a SIMD.  16 bytes (four float) were measured too: 57600 threads
// do not fill the device at 640x360, and the kernel took 1.2 to 1.6 times as long
template <typename T, int KMAX>
constexpr int kFusePx = (sizeof(T) == 2 && KMAX == 32) ? 2 : 8 / (int)sizeof(T);

// which of a call's arrays take one vector access for a thread's pixels (the host decides from the
// pointers and strides; the rest, and the row's tail, go pixel by pixel)
enum { kFuseVecDisp = 1, kFuseVecConf = 2, kFuseVecOut = 4 };

struct FuseOut {
    float* out;
    uint8_t* support;
    float* spread;
    sdr_fusion* slots;  // kFuseSlots zeroed partial records, or null for a call without a record
};

// N elements in one access
template <typename E, int N>
using FuseVec = E __attribute__((ext_vector_type(N)));

// a thread's N values of one frame: one vector load, or one load a pixel of the row
template <int N, typename E>
__device__ __forceinline__ void fuse_load(const E* p, bool vec, int left, float (&v)[N]) {
    if (vec) {
        const FuseVec<E, N> q = *reinterpret_cast<const FuseVec<E, N>*>(p);
#pragma unroll
        for (int i = 0; i < N; i++) {
            const E e = q[i];
            v[i] = load_disp(&e);
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = i < left ? load_disp(p + i) : 0.f;
    }
}

// what a pixel adds to the record, packed for the wave sums: six counts of 10 bits (a wave adds at
// most 64 * 4 to each) and the two sums in 32 bits each
struct FuseTally {
    long long classes;  // n_fused, n_empty, n_sparse, n_unstable, n_filled, n_replaced
    long long sums;     // sum_support, n_disagree << 32
};

// One pixel: v the F values (slots >= F hold anything and are not valid), ok their validity.
// Returns the value written to d_out; *support and *spread are the other two maps' values.
template <int KMAX>
__device__ __forceinline__ float fuse_pixel(const float (&v)[KMAX], unsigned ok, int F, const sdr_fuse_params& P,
                                            int* support, float* spread, FuseTally* tally) {
#pragma clang fp contract(off)
    // an invalid value becomes +inf: it sorts behind every valid one and agrees with nothing
    float w[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++) w[k] = ((ok >> k) & 1u) ? v[k] : INFINITY;
    const int n = __popc(ok);
    *support = 0;
    *spread = ruler_nan();
    if (n == 0) {
        tally->classes += 1ll << 10;
        return P.fill;
    }
    // rank by counting: the valid values before w[i] by `<`, equal ones in frame order
    int rank[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++) rank[k] = 0;
#pragma unroll
    for (int i = 1; i < KMAX; i++) {
#pragma unroll
        for (int j = 0; j < i; j++) {
            const bool first = w[j] <= w[i];  // j < i: w[j] sorts first unless w[i] < w[j]
            rank[i] += first ? 1 : 0;
            rank[j] += first ? 0 : 1;
        }
    }
    const int want = (n - 1) >> 1;
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; k++)
        if (((ok >> k) & 1u) && rank[k] == want) m = w[k];
    // the values that agree with the median, in frame order: their count, their double sum, the
    // smallest and the largest by `<` (of equal ones the earliest)
    unsigned agree = 0;
    double s = 0.0;
    float lo = 0.f, hi = 0.f;
    bool any = false;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const bool a = fabsf(w[k] - m) <= P.tol;
        if (a) {
            agree |= 1u << k;
            s += (double)w[k];
            lo = (!any || w[k] < lo) ? w[k] : lo;
            hi = (!any || hi < w[k]) ? w[k] : hi;
            any = true;
        }
    }
    const int n_in = __popc(agree);
    if (n_in < P.min_count) {
        tally->classes += n < P.min_count ? 1ll << 20 : 1ll << 30;
        return P.fill;
    }
    const unsigned last = 1u << (F - 1);
    tally->classes += 1ll + (!(ok & last) ? 1ll << 40 : 0ll) + (((ok & last) && !(agree & last)) ? 1ll << 50 : 0ll);
    tally->sums += (long long)n_in + ((long long)(n - n_in) << 32);
    *support = n_in;
    *spread = hi - lo;
    return P.mode == SDR_FUSE_MEDIAN ? m : (float)(s / (double)n_in);
}

template <typename T, int KMAX>
__global__ __launch_bounds__(kFuseThreads) void k_fuse(RegionMaps<T> maps, sdr_fuse_params P, FuseOut o, int vecs,
                                                       int groups_row, int groups) {
    constexpr int PX = kFusePx<T, KMAX>;
    __shared__ long long sh[kFuseWaves][2];
    const int tid = threadIdx.x;
    const int g = blockIdx.x * kFuseThreads + tid;  // the thread's group of PX pixels
    const int W = maps.W, F = maps.F;
    FuseTally tally{0, 0};
    if (g < groups) {
        const int y = g / groups_row, x = (g - y * groups_row) * PX;
        const int left = min(W - x, PX);
        const bool whole = left == PX;
        const T* pd = maps.disp + (size_t)y * maps.stride + (size_t)x;
        const size_t px = (size_t)y * (size_t)W + (size_t)x;
        const float* pc = maps.conf ? maps.conf + px : nullptr;
        const size_t cf = (size_t)maps.H * (size_t)W;
        // every load of the thread before the first use: F frames of disparities, then of confidences
        float v[KMAX][PX], c[KMAX][PX];
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            if (k < F) {
                fuse_load<PX>(pd + (size_t)k * maps.fstride, whole && (vecs & kFuseVecDisp), left, v[k]);
            } else {
#pragma unroll
                for (int i = 0; i < PX; i++) v[k][i] = 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            if (pc && k < F) {
                fuse_load<PX>(pc + (size_t)k * cf, whole && (vecs & kFuseVecConf), left, c[k]);
            } else {
#pragma unroll
                for (int i = 0; i < PX; i++) c[k][i] = 0.f;
            }
        }
        float r[PX], sp[PX];
        int su[PX];
#pragma unroll
        for (int i = 0; i < PX; i++) {
            float col[KMAX];
            unsigned ok = 0;
#pragma unroll
            for (int k = 0; k < KMAX; k++) {
                col[k] = v[k][i];
                const bool good = k < F && i < left && isfinite(col[k]) && col[k] > P.min_disp &&
                                  (!pc || c[k][i] >= P.conf_min);
                ok |= good ? 1u << k : 0u;
            }
            if (i < left)
                r[i] = fuse_pixel<KMAX>(col, ok, F, P, &su[i], &sp[i], &tally);
            else
                r[i] = 0.f, su[i] = 0, sp[i] = 0.f;
        }
        if (whole && (vecs & kFuseVecOut)) {
            FuseVec<float, PX> qr, qs;
            FuseVec<uint8_t, PX> qu;
#pragma unroll
            for (int i = 0; i < PX; i++) qr[i] = r[i], qs[i] = sp[i], qu[i] = (uint8_t)su[i];
            *reinterpret_cast<FuseVec<float, PX>*>(o.out + px) = qr;
            if (o.support) *reinterpret_cast<FuseVec<uint8_t, PX>*>(o.support + px) = qu;
            if (o.spread) *reinterpret_cast<FuseVec<float, PX>*>(o.spread + px) = qs;
        } else {
#pragma unroll
            for (int i = 0; i < PX; i++) {
                if (i >= left) continue;
                o.out[px + i] = r[i];
                if (o.support) o.support[px + i] = (uint8_t)su[i];
                if (o.spread) o.spread[px + i] = sp[i];
            }
        }
    }
    if (!o.slots) return;  // uniform
    // the record: the wave's sums, the workgroup's through LDS, then one atomic a counter from the
    // workgroup's first eight lanes into the workgroup's partial record (zeroed on the stream before
    // the launch)
    const long long wc = wave_sum(tally.classes), ws = wave_sum(tally.sums);
    if ((tid & 63) == 0) {
        sh[tid >> 6][0] = wc;
        sh[tid >> 6][1] = ws;
    }
    __syncthreads();
    if (tid >= 8) return;
    sdr_fusion* slot = o.slots + blockIdx.x % kFuseSlots;
    long long cls[kFuseWaves], sums[kFuseWaves];
#pragma unroll
    for (int w = 0; w < kFuseWaves; w++) cls[w] = sh[w][0], sums[w] = sh[w][1];
    if (tid < 6) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < kFuseWaves; w++) t += (int)((cls[w] >> (10 * tid)) & 1023);
        // n_fused .. n_unstable, n_filled, n_replaced: six consecutive int32 from byte 16
        if (t) atomicAdd(reinterpret_cast<int*>(slot) + 4 + tid, t);
    } else {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < kFuseWaves; w++)
            t += tid == 6 ? (unsigned long long)(sums[w] & 0xffffffffll) : (unsigned long long)(sums[w] >> 32);
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(tid == 6 ? &slot->sum_support : &slot->n_disagree);
        if (t) atomicAdd(dst, t);
    }
}

// The record from the partial records: one wave, a slot a lane.
__global__ __launch_bounds__(kFuseSlots) void k_fuse_record(const sdr_fusion* __restrict__ slots, int F, int W, int H,
                                                            int mode, sdr_fusion* __restrict__ out) {
    const sdr_fusion s = slots[threadIdx.x];
    sdr_fusion r;
    r.frames = F, r.width = W, r.height = H, r.mode = mode;
    r.n_fused = (int32_t)wave_sum((long long)s.n_fused);
    r.n_empty = (int32_t)wave_sum((long long)s.n_empty);
    r.n_sparse = (int32_t)wave_sum((long long)s.n_sparse);
    r.n_unstable = (int32_t)wave_sum((long long)s.n_unstable);
    r.n_filled = (int32_t)wave_sum((long long)s.n_filled);
    r.n_replaced = (int32_t)wave_sum((long long)s.n_replaced);
    r.sum_support = wave_sum((long long)s.sum_support);
    r.n_disagree = wave_sum((long long)s.n_disagree);
    r.reserved = 0;
    if (threadIdx.x == 0) *out = r;
}

}  // namespace sdr

namespace {

using namespace sdr::ruler_host;

// argument guards of the two entries (host only)
int check_fuse_args(const void* disp, int disp_type, size_t stride, size_t fstride, int W, int H, int F,
                    const sdr_fuse_params* p, const void* out) {
    if (!disp || !out || !p) return rfail(SDR_ERR_ARG, "null argument");
    if (int rc = sdr::check_dims(W, H, stride, F)) return rc;
    if (F > 1 && fstride < stride * (size_t)H) return rfail(SDR_ERR_ARG, "bad stride");
    if (disp_type != SDR_DISP_F32 && disp_type != SDR_DISP_S16)
        return rfail(SDR_ERR_ARG, "disp_type must be SDR_DISP_F32 or SDR_DISP_S16");
    if (p->mode != SDR_FUSE_MEAN && p->mode != SDR_FUSE_MEDIAN)
        return rfail(SDR_ERR_ARG, "mode must be SDR_FUSE_MEAN or SDR_FUSE_MEDIAN");
    if (!std::isfinite(p->tol) || p->tol < 0.f) return rfail(SDR_ERR_ARG, "tol must be finite and >= 0");
    if (p->min_count < 1 || p->min_count > SDR_FUSE_MAX_FRAMES)
        return rfail(SDR_ERR_ARG, "min_count must be in 1..32");
    if (p->reserved[0] || p->reserved[1]) return rfail(SDR_ERR_ARG, "reserved fields must be 0");
    if (std::isfinite(p->fill) && p->fill > p->min_disp)
        return rfail(SDR_ERR_ARG, "fill must not be a valid disparity (finite and > min_disp)");
    if (F > SDR_FUSE_MAX_FRAMES) return rfail(SDR_ERR_LIMIT, "at most SDR_FUSE_MAX_FRAMES frames a stack");
    if ((size_t)W * (size_t)H > (size_t)INT32_MAX) return rfail(SDR_ERR_LIMIT, "width * height > INT32_MAX");
    return SDR_OK;
}

bool aligned(const void* p, size_t bytes) { return ((uintptr_t)p % bytes) == 0; }

template <typename T, int KMAX>
void launch_fuse(const sdr::RegionMaps<T>& maps, const sdr_fuse_params& P, const sdr::FuseOut& o, hipStream_t st) {
    // the vector paths: a thread's pixels in one access, where every row of every frame keeps the
    // access's alignment (the dense maps: where the width does)
    constexpr size_t px = sdr::kFusePx<T, KMAX>;
    int vecs = 0;
    if (aligned(maps.disp, px * sizeof(T)) && maps.stride % px == 0 && (maps.F == 1 || maps.fstride % px == 0))
        vecs |= sdr::kFuseVecDisp;
    const bool dense = maps.W % px == 0;
    if (dense && maps.conf && aligned(maps.conf, px * sizeof(float))) vecs |= sdr::kFuseVecConf;
    if (dense && aligned(o.out, px * sizeof(float)) && (!o.support || aligned(o.support, px)) &&
        (!o.spread || aligned(o.spread, px * sizeof(float))))
        vecs |= sdr::kFuseVecOut;
    const int groups_row = (maps.W + (int)px - 1) / (int)px;
    const long long groups = (long long)groups_row * maps.H;  // <= INT32_MAX pixels: fits an int
    const unsigned blocks = (unsigned)((groups + sdr::kFuseThreads - 1) / sdr::kFuseThreads);
    hipLaunchKernelGGL((sdr::k_fuse<T, KMAX>), dim3(blocks), dim3(sdr::kFuseThreads), 0, st, maps, P, o, vecs, groups_row,
                       (int)groups);
}

}  // namespace

extern "C" {

void sdr_fuse_params_default(sdr_fuse_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->min_disp = -1.0f;
    p->conf_min = 0.0f;
    p->tol = 1.0f;
    p->fill = -1.0f;
    p->min_count = 2;
    p->mode = SDR_FUSE_MEAN;
}

int sdr_fuse_disp_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride, int W, int H, int F,
                         const float* d_conf, const sdr_fuse_params* params, float* d_out, uint8_t* d_support,
                         float* d_spread, sdr_fusion* d_rec, void* stream) {
    if (int rc = check_fuse_args(d_disp, disp_type, stride, frame_stride, W, H, F, params, d_out)) return rc;
    hipStream_t st = (hipStream_t)stream;
    // with a record: kFuseSlots partial records in stream-ordered scratch, cleared on the stream
    sdr::Scratch sc(st);
    sdr_fusion* slots = nullptr;
    if (d_rec) {
        sdr::ScratchLayout lay;
        const auto s_slots = lay.take<sdr_fusion>(sdr::kFuseSlots);
        if (int rc = sc.open(lay)) return rc;
        slots = sc.at(s_slots);
        SDR_HIP(hipMemsetAsync(slots, 0, sdr::kFuseSlots * sizeof(sdr_fusion), st));
    }
    const sdr::FuseOut o{d_out, d_support, d_spread, slots};
    with_maps(d_disp, disp_type, stride, frame_stride, W, H, F, d_conf, nullptr, [&](auto maps) {
        using T = disp_elem_t<decltype(maps)>;
        if (F <= 4)
            launch_fuse<T, 4>(maps, *params, o, st);
        else if (F <= 8)
            launch_fuse<T, 8>(maps, *params, o, st);
        else if (F <= 16)
            launch_fuse<T, 16>(maps, *params, o, st);
        else
            launch_fuse<T, 32>(maps, *params, o, st);
    });
    if (d_rec)
        hipLaunchKernelGGL(sdr::k_fuse_record, dim3(1), dim3(sdr::kFuseSlots), 0, st, (const sdr_fusion*)slots, F, W, H,
                           params->mode, d_rec);
    return sc.finish();
}

int sdr_fuse_disp(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H, int F,
                  const float* conf, const sdr_fuse_params* params, float* out, uint8_t* support, float* spread,
                  sdr_fusion* rec) {
    int rc = check_fuse_args(disp, disp_type, stride, frame_stride, W, H, F, params, out);
    if (rc) return rc;
    HostCall c;
    const HostCall::Maps m = c.maps(disp, disp_type, stride, frame_stride, W, H, F, conf);
    const size_t n = (size_t)W * H;
    const auto s_out = c.output(out, n);
    const auto s_spread = c.output(spread, spread ? n : 0);
    const auto s_rec = c.output(rec, rec ? 1 : 0);
    const auto s_support = c.output(support, support ? n : 0);
    if ((rc = c.ready())) return rc;
    rc = sdr_fuse_disp_device(m.disp, disp_type, m.stride, m.fstride, W, H, F, m.conf, params, c.at(s_out),
                              support ? c.at(s_support) : nullptr, spread ? c.at(s_spread) : nullptr,
                              rec ? c.at(s_rec) : nullptr, c.stream());
    return rc ? rc : c.finish();
}

}  // extern "C"
