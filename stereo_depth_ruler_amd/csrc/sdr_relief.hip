// sdr_relief.hip -- the relief of a region: the heights of a rectangle's pixels above a fitted
// plane, their counts, exact sums and extremes, and order statistics by a radix selection over a
// monotone 32-bit key of the height in three passes of 11, 11 and 10 bits.  The definition is in
// include/sdr/sdr.h ("the relief of a region").
#include <math.h>
#include <string.h>

#include <cmath>

#include <algorithm>
#include <string>
#include <type_traits>

#include "sdr_device.hpp"
#include "sdr_internal.hpp"
#include "sdr_region.hpp"
#include "sdr_ruler_shared.hpp"

namespace sdr {

static_assert(sizeof(sdr_relief_query) == 32, "sdr_relief_query is 32 bytes");
static_assert(sizeof(sdr_relief_params) == 64, "sdr_relief_params is 64 bytes");
static_assert(sizeof(sdr_relief) == 128, "sdr_relief is 128 bytes");

constexpr int kReliefBins = 2048;      // passes 1 and 2: 11 bits
constexpr int kReliefLastBins = 1024;  // pass 3: 10 bits
constexpr int kReliefQ = 8;            // quantiles a call, and so distinct prefixes a pass
constexpr int kReliefSums = 7;         // n_masked, n_valid, n, n_above, n_below, sum256, sum256_above

// A query's state, zeroed with its histograms before the first sweep.
struct ReliefState {
    long long acc[kReliefSums];
    unsigned kmax, kmin_inv;        // the largest key and the largest ~key (zero: none yet)
    int status;                     // pick 1 has written the record (refused or empty): the rest leaves
    int nslot[2];                   // distinct prefixes behind pass 1 / pass 2
    unsigned prefix[2][kReliefQ];   // the key's top 11 / 22 bits of each slot
    int slot[2][kReliefQ];          // quantile j's slot behind pass 1 / pass 2
    unsigned rank[2][kReliefQ];     // and its rank among the keys that share the slot's prefix
    int pad;
};
static_assert(sizeof(ReliefState) == 272, "ReliefState is 272 bytes");

// One sweep over the queries' pixels: grid (slices of a W x H frame, queries), `hist` the pass's
// histograms of the batch.  Pass 1 sums the counts and the integer sums, takes the extremes on the
// ordered key and counts the key's top 11 bits; pass 2 counts the next 11 bits of the keys whose
// top bits are one of pick 1's prefixes, pass 3 the last 10 bits of those that match one of pick
// 2's.  A workgroup counts into LDS (pass 1: one histogram; passes 2 and 3: one a prefix, nq of
// them at most, which the launch sizes the LDS for) and adds its non-zero bins to the query's.  A
// query that is refused or empty and a slice past the area leave at once (block-uniform); no
// workgroup waits on another.
template <typename T, int PASS>
__global__ __launch_bounds__(kRegionThreads) void k_relief_sweep(
    RegionMaps<T> maps, Q16 Q, sdr_relief_params P, const sdr_plane* __restrict__ planes, int NP,
    const sdr_relief_query* __restrict__ queries, ReliefState* __restrict__ states, unsigned* __restrict__ hist) {
#pragma clang fp contract(off)
    extern __shared__ unsigned lh[];
    constexpr int kBins = PASS == 3 ? kReliefLastBins : kReliefBins;
    const int k = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    ReliefState* S = states + k;
    if (PASS > 1 && S->status) return;  // block-uniform
    const sdr_relief_query q = queries[k];
    RegionPlane pl;
    RegionSlice<T> sl;
    if (!query_slice(maps, planes, NP, q, &pl, &sl)) return;
    const int nslot = PASS == 1 ? 1 : S->nslot[PASS - 2];  // 1..nq
    const int slots = PASS == 1 ? 1 : P.nq;                 // the query's histograms of this pass
    unsigned pre[kReliefQ];
#pragma unroll
    for (int s = 0; s < kReliefQ; s++) pre[s] = (PASS > 1 && s < nslot) ? S->prefix[PASS - 2][s] : 0u;
    for (int i = tid; i < nslot * kBins; i += kRegionThreads) lh[i] = 0;
    __syncthreads();

    long long m[kReliefSums];
#pragma unroll
    for (int i = 0; i < kReliefSums; i++) m[i] = 0;
    unsigned kmax = 0, kmin_inv = 0;
    sl.each([&](unsigned u, unsigned v) __attribute__((always_inline)) {
        const RegionPix px = region_pixel(sl, Q, pl, P.min_disp, P.conf_min, q.label, u, v);
        const unsigned key = ordered_key(px.hf);
        if (PASS == 1) {
            m[0] += px.masked ? 1 : 0;
            m[1] += px.valid ? 1 : 0;
            if (!px.member) return;
            const bool above = px.hf > P.band;
            const long long e = llrint((double)px.hf * 256.0);
            m[2] += 1;
            m[3] += above ? 1 : 0;
            m[4] += px.hf < -P.band ? 1 : 0;
            m[5] += e;
            m[6] += above ? e : 0;
            kmax = max(kmax, key);
            kmin_inv = max(kmin_inv, ~key);
            atomicAdd(&lh[key >> 21], 1u);
        } else {
            if (!px.member) return;
            const unsigned top = PASS == 2 ? key >> 21 : key >> 10;
            const unsigned bin = PASS == 2 ? (key >> 10) & 2047u : key & 1023u;
#pragma unroll
            for (int s = 0; s < kReliefQ; s++)  // the prefixes differ: one slot at most
                if (s < nslot && top == pre[s]) atomicAdd(&lh[s * kBins + (int)bin], 1u);
        }
    });
    if constexpr (PASS == 1) {
        // wave butterflies, then the waves' sums through LDS, as the plane fit's sweep
        __shared__ long long red[kRegionWaves][kReliefSums];
        __shared__ unsigned redk[kRegionWaves][2];
#pragma unroll
        for (int i = 0; i < kReliefSums; i++) {
            const long long s = wave_sum(m[i]);
            if (lane == 0) red[wave][i] = s;
        }
        kmax = wave_max(kmax);
        kmin_inv = wave_max(kmin_inv);
        if (lane == 0) {
            redk[wave][0] = kmax;
            redk[wave][1] = kmin_inv;
        }
        __syncthreads();
        if (tid < kReliefSums) {
            long long s = 0;
#pragma unroll
            for (int w = 0; w < kRegionWaves; w++) s += red[w][tid];
            if (s) atomicAdd((unsigned long long*)S->acc + tid, (unsigned long long)s);
        } else if (tid < kReliefSums + 2) {
            const int i = tid - kReliefSums;
            unsigned b = 0;
#pragma unroll
            for (int w = 0; w < kRegionWaves; w++) b = max(b, redk[w][i]);
            if (b) atomicMax(i ? &S->kmin_inv : &S->kmax, b);  // a member's key and ~key are never 0
        }
    }
    __syncthreads();
    unsigned* gh = hist + (size_t)k * (size_t)slots * kBins;
    for (int i = tid; i < nslot * kBins; i += kRegionThreads) {
        const unsigned c = lh[i];
        if (c) atomicAdd(gh + i, c);
    }
}

// Element k (0-based, below the histogram's total) of a histogram's multiset by the whole
// workgroup: its bin and its rank among the bin's elements, in every thread.
template <int BINS>
__device__ __forceinline__ void relief_locate(const unsigned* __restrict__ h, unsigned k, unsigned* sh_wave,
                                              unsigned* sh_res, unsigned* bin, unsigned* rank) {
    constexpr int kPer = BINS / kRegionThreads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned c[kPer], sum = 0;
#pragma unroll
    for (int i = 0; i < kPer; i++) {
        c[i] = h[tid * kPer + i];
        sum += c[i];
    }
    unsigned inc = sum;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sh_wave[wave] = inc;
    if (tid == 0) sh_res[0] = sh_res[1] = 0;
    __syncthreads();
    unsigned before = inc - sum;
    for (int w = 0; w < wave; w++) before += sh_wave[w];
    if (k >= before && k - before < sum) {  // one thread
        unsigned r = k - before;
        bool found = false;
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            if (!found && r < c[i]) {
                sh_res[0] = (unsigned)(tid * kPer + i);
                sh_res[1] = r;
                found = true;
            }
            if (!found) r -= c[i];
        }
    }
    __syncthreads();
    *bin = sh_res[0];
    *rank = sh_res[1];
    __syncthreads();
}

// quantile j's prefix joins the slots (thread 0): ranks that fall in one bin share a slot
__device__ __forceinline__ void relief_slot(ReliefState* S, int pass, int j, unsigned prefix, unsigned rank,
                                            int* nslot) {
    int s = 0;
    while (s < *nslot && S->prefix[pass][s] != prefix) s++;
    if (s == *nslot) {
        S->prefix[pass][s] = prefix;
        *nslot = s + 1;
    }
    S->slot[pass][j] = s;
    S->rank[pass][j] = rank;
}

// the record of a query (one thread); qv: the nq quantiles of a valid one
__device__ __forceinline__ void relief_write(sdr_relief* o, const sdr_relief_query& q, uint32_t flags, int area,
                                             const ReliefState* S, const sdr_relief_params& P, const float* qv) {
#pragma clang fp contract(off)
    const bool valid = flags == SDR_RELIEF_VALID;
    const bool counted = valid || flags == SDR_RELIEF_EMPTY;
    sdr_relief r;
    for (int j = 0; j < kReliefQ; j++) r.q[j] = (valid && j < P.nq) ? qv[j] : ruler_nan();
    r.h_min = r.h_max = ruler_nan();
    r.mean = r.mean_above = __builtin_nan("");
    r.sum256 = r.sum256_above = 0;
    r.area = area;
    r.n_masked = counted ? (int)S->acc[0] : 0;
    r.n_valid = counted ? (int)S->acc[1] : 0;
    r.n = r.n_above = r.n_below = 0;
    r.n_rejected = r.n_valid;
    if (valid) {
        r.n = (int)S->acc[2];
        r.n_above = (int)S->acc[3];
        r.n_below = (int)S->acc[4];
        r.n_rejected = r.n_valid - r.n;
        r.sum256 = S->acc[5];
        r.sum256_above = S->acc[6];
        r.h_max = ordered_unkey(S->kmax);
        r.h_min = ordered_unkey(~S->kmin_inv);
        r.mean = ((double)r.sum256 / (double)r.n) / 256.0;
        if (r.n_above > 0) r.mean_above = ((double)r.sum256_above / (double)r.n_above) / 256.0;
    }
    r.frame = q.frame;
    r.plane = q.plane;
    r.label = q.label;
    r.flags = flags;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    *o = r;
}

// Behind sweep 1, a workgroup a query: the record of a query that is refused or has no member
// (the later kernels then leave it), else for each quantile the bin of the first histogram its
// rank falls in and the rank inside the bin.
__global__ __launch_bounds__(kRegionThreads) void k_relief_pick1(RegionDims dims, sdr_relief_params P,
                                                                 const sdr_plane* __restrict__ planes, int NP,
                                                                 const sdr_relief_query* __restrict__ queries,
                                                                 ReliefState* __restrict__ states,
                                                                 const unsigned* __restrict__ hist1,
                                                                 sdr_relief* __restrict__ out) {
    __shared__ unsigned sh_wave[kRegionWaves], sh_res[2];
    const int k = blockIdx.x, tid = threadIdx.x;
    const sdr_relief_query q = queries[k];
    ReliefState* S = states + k;
    RegionPlane pl;
    uint32_t flags = query_refusal(dims, planes, NP, q, &pl);
    const long long n = S->acc[2];
    if (!flags && n == 0) flags = SDR_RELIEF_EMPTY;
    if (flags) {  // block-uniform
        if (tid == 0) {
            const PlaneRect R = plane_rect(region_segment(q));
            relief_write(out + k, q, flags, flags == SDR_RELIEF_OUT_OF_RANGE ? 0 : R.rw * R.rh, S, P, nullptr);
            S->status = 1;
        }
        return;
    }
    int nslot = 0;
    for (int j = 0; j < P.nq; j++) {
        const unsigned kk = (unsigned)(((n - 1) * (long long)P.permille[j]) / 1000);
        unsigned bin, rank;
        relief_locate<kReliefBins>(hist1 + (size_t)k * kReliefBins, kk, sh_wave, sh_res, &bin, &rank);
        if (tid == 0) relief_slot(S, 0, j, bin, rank, &nslot);
    }
    if (tid == 0) S->nslot[0] = nslot;
}

// Behind sweep 2: the next 11 bits of each quantile from its slot's histogram.
__global__ __launch_bounds__(kRegionThreads) void k_relief_pick2(sdr_relief_params P,
                                                                 ReliefState* __restrict__ states,
                                                                 const unsigned* __restrict__ hist2) {
    __shared__ unsigned sh_wave[kRegionWaves], sh_res[2];
    const int k = blockIdx.x, tid = threadIdx.x;
    ReliefState* S = states + k;
    if (S->status) return;  // block-uniform
    int nslot = 0;
    for (int j = 0; j < P.nq; j++) {
        const int s = S->slot[0][j];
        unsigned bin, rank;
        relief_locate<kReliefBins>(hist2 + ((size_t)k * P.nq + s) * kReliefBins, S->rank[0][j], sh_wave, sh_res,
                                   &bin, &rank);
        if (tid == 0) relief_slot(S, 1, j, (S->prefix[0][s] << 11) | bin, rank, &nslot);
    }
    if (tid == 0) S->nslot[1] = nslot;
}

// Behind sweep 3: the last 10 bits, each quantile's float from its 32 key bits, the record.
__global__ __launch_bounds__(kRegionThreads) void k_relief_finish(sdr_relief_params P,
                                                                  const sdr_relief_query* __restrict__ queries,
                                                                  const ReliefState* __restrict__ states,
                                                                  const unsigned* __restrict__ hist3,
                                                                  sdr_relief* __restrict__ out) {
    __shared__ unsigned sh_wave[kRegionWaves], sh_res[2];
    __shared__ float qv[kReliefQ];
    const int k = blockIdx.x, tid = threadIdx.x;
    const ReliefState* S = states + k;
    if (S->status) return;  // block-uniform: pick 1 has written the record
    for (int j = 0; j < P.nq; j++) {
        const int s = S->slot[1][j];
        unsigned bin, rank;
        relief_locate<kReliefLastBins>(hist3 + ((size_t)k * P.nq + s) * kReliefLastBins, S->rank[1][j], sh_wave,
                                       sh_res, &bin, &rank);
        if (tid == 0) qv[j] = ordered_unkey((S->prefix[1][s] << 10) | bin);
    }
    if (tid != 0) return;
    const sdr_relief_query q = queries[k];
    const PlaneRect R = plane_rect(region_segment(q));
    relief_write(out + k, q, SDR_RELIEF_VALID, R.rw * R.rh, S, P, qv);
}

}  // namespace sdr

namespace {

using namespace sdr::ruler_host;

// queries a batch: the batches run one behind another on the stream through one scratch block
// (272 B of state and 8 KB + nq * 12 KB of histograms a query)
constexpr int kReliefBatch = 256;

int check_relief_params(const sdr_relief_params* p, const void* planes, int P) {
    if (int rc = check_planes_arg(planes, P)) return rc;
    if (p->nq < 0 || p->nq > 8) return rfail(SDR_ERR_ARG, "nq must be in 0..8");
    for (int j = 0; j < p->nq; j++)
        if (p->permille[j] < 0 || p->permille[j] > 1000) return rfail(SDR_ERR_ARG, "permille must be in 0..1000");
    if (!(std::isfinite(p->band) && p->band >= 0.0f)) return rfail(SDR_ERR_ARG, "band must be finite and >= 0");
    for (int i = 0; i < 4; i++)
        if (p->reserved[i]) return rfail(SDR_ERR_ARG, "reserved fields must be 0");
    return SDR_OK;
}

}  // namespace

extern "C" {

void sdr_relief_params_default(sdr_relief_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->min_disp = -1.0f;
    p->conf_min = 0.0f;
    p->band = 0.0f;
    p->nq = 3;
    p->permille[0] = 50;
    p->permille[1] = 500;
    p->permille[2] = 950;
}

int sdr_plane_relief_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride, int W, int H,
                            int F, const float* d_conf, const uint8_t* d_labels, const double Q[16],
                            const sdr_relief_params* params, const sdr_plane* d_planes, int P,
                            const sdr_relief_query* d_queries, int K, sdr_relief* d_out, void* stream) {
    int rc = check_plane_maps(d_disp, disp_type, stride, frame_stride, W, H, F, Q, params, d_queries, K, d_out);
    if (rc || (rc = check_relief_params(params, d_planes, P))) return rc;
    if (K == 0) return SDR_OK;
    hipStream_t st = (hipStream_t)stream;
    const sdr::Q16 q = make_q16(Q);
    const sdr_relief_params RP = *params;
    const int nq = RP.nq, KB = std::min(K, kReliefBatch);
    // scratch of a batch, all of it zeroed: {states, pass 1's histograms, pass 2's, pass 3's}
    sdr::ScratchLayout lay;
    const auto s_states = lay.take<sdr::ReliefState>((size_t)KB);
    const auto s_h1 = lay.take<unsigned>((size_t)KB * sdr::kReliefBins);
    const auto s_h2 = lay.take<unsigned>((size_t)KB * nq * sdr::kReliefBins);
    const auto s_h3 = lay.take<unsigned>((size_t)KB * nq * sdr::kReliefLastBins);
    sdr::Scratch sc(st);
    if ((rc = sc.open(lay))) return rc;
    sdr::ReliefState* states = sc.at(s_states);
    unsigned* h1 = sc.at(s_h1);
    unsigned* h2 = sc.at(s_h2);
    unsigned* h3 = sc.at(s_h3);
    const unsigned slices = sdr::region_slices(W, H);
    const dim3 block(sdr::kRegionThreads);
    const size_t lds1 = sdr::kReliefBins * sizeof(unsigned), lds2 = (size_t)nq * lds1,
                 lds3 = (size_t)nq * sdr::kReliefLastBins * sizeof(unsigned);
    hipError_t e = hipSuccess;
    auto batch = [&](auto maps, int k0, int kb) {
        using T = disp_elem_t<decltype(maps)>;
        const sdr_relief_query* qs = d_queries + k0;
        const dim3 sgrid(slices, (unsigned)kb), pgrid((unsigned)kb);
        if ((e = hipMemsetAsync(sc.base, 0, lay.total, st)) != hipSuccess) return;
        hipLaunchKernelGGL((sdr::k_relief_sweep<T, 1>), sgrid, block, lds1, st, maps, q, RP, d_planes, P, qs, states, h1);
        hipLaunchKernelGGL(sdr::k_relief_pick1, pgrid, block, 0, st, maps.dims(), RP, d_planes, P, qs, states,
                           (const unsigned*)h1, d_out + k0);
        if (nq > 0) {
            hipLaunchKernelGGL((sdr::k_relief_sweep<T, 2>), sgrid, block, lds2, st, maps, q, RP, d_planes, P, qs, states,
                               h2);
            hipLaunchKernelGGL(sdr::k_relief_pick2, pgrid, block, 0, st, RP, states, (const unsigned*)h2);
            hipLaunchKernelGGL((sdr::k_relief_sweep<T, 3>), sgrid, block, lds3, st, maps, q, RP, d_planes, P, qs, states,
                               h3);
        }
        hipLaunchKernelGGL(sdr::k_relief_finish, pgrid, block, 0, st, RP, qs, (const sdr::ReliefState*)states,
                           (const unsigned*)h3, d_out + k0);
    };
    for (int k0 = 0; k0 < K && e == hipSuccess; k0 += KB)
        with_maps(d_disp, disp_type, stride, frame_stride, W, H, F, d_conf, d_labels,
                  [&](auto maps) { batch(maps, k0, std::min(K - k0, KB)); });
    return sc.finish(e);
}

int sdr_plane_relief(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H, int F,
                     const float* conf, const uint8_t* labels, const double Q[16], const sdr_relief_params* params,
                     const sdr_plane* planes, int P, const sdr_relief_query* queries, int K, sdr_relief* out) {
    return region_host_call(check_relief_params, sdr_plane_relief_device, disp, disp_type, stride, frame_stride, W, H,
                            F, conf, labels, Q, params, planes, P, queries, K, out);
}

}  // extern "C"
