// sdr_plane.hip -- the ruler against a surface: the robust plane fit of a rectangle's disparities
// (exact integer moments, a coarse-to-fine inlier refit), the seeded search for a region's dominant
// planes, and the signed distance of sampled points to fitted planes.  The definitions are in
// include/sdr/sdr.h ("the ruler against a surface", "the dominant planes of a region").
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "sdr_device.hpp"
#include "sdr_internal.hpp"
#include "sdr_region.hpp"
#include "sdr_ruler_shared.hpp"

namespace sdr {

// ---- the plane fit (the definition: sdr.h, "the ruler against a surface") ----
static_assert(sizeof(sdr_plane_params) == 32, "sdr_plane_params is 32 bytes");
static_assert(sizeof(sdr_plane) == 128, "sdr_plane is 128 bytes");
static_assert(sizeof(sdr_plane_query) == 16, "sdr_plane_query is 16 bytes");
static_assert(sizeof(struct sdr_plane_distance) == 32, "sdr_plane_distance is 32 bytes");

// accumulators of a region: [iterations + 2 sweeps][kPlaneSlots] int64.  Sweeps 0..iterations hold
// the nine moments of their fit's pixel set {n, Su, Sv, Sq, Suu, Suv, Svv, Suq, Svq}, the last
// sweep {n_inliers, See, the bits of max |r|}
constexpr int kPlaneSlots = 16;
constexpr int kPlaneMoments = 9;

struct PlaneFit {
    double a, b, c;  // in 1/16 px
    bool ok;
};

// The solve of sdr.h from a set's moments.  Every workgroup of a sweep and the record writer
// repeat it from the same integers: the same bits everywhere.
__device__ __forceinline__ PlaneFit plane_solve(const long long* __restrict__ m, int min_inliers) {
#pragma clang fp contract(off)
    const long long n = m[0];
    const double N = (double)n, su = (double)m[1], sv = (double)m[2], sq = (double)m[3];
    const double cuu = N * (double)m[4] - su * su;
    const double cuv = N * (double)m[5] - su * sv;
    const double cvv = N * (double)m[6] - sv * sv;
    const double cuq = N * (double)m[7] - su * sq;
    const double cvq = N * (double)m[8] - sv * sq;
    const double det = cuu * cvv - cuv * cuv;
    PlaneFit f;
    f.a = (cuq * cvv - cvq * cuv) / det;
    f.b = (cvq * cuu - cuq * cuv) / det;
    f.c = ((sq - f.a * su) - f.b * sv) / N;
    f.ok = n >= (long long)min_inliers && det > 0.0 && isfinite(f.a) && isfinite(f.b) && isfinite(f.c);
    return f;
}

__device__ __forceinline__ double plane_at(const PlaneFit& f, double u, double v) {
#pragma clang fp contract(off)
    return (f.a * u + f.b * v) + f.c;
}

// the valid pixel's value on the 1/16 px grid
__device__ __forceinline__ bool plane_q(const float* p, float min_disp, int* q) {
    const float d = *p;
    *q = (int)rint((double)d * 16.0);
    return isfinite(d) && d > min_disp && fabsf(d) < 2048.f;
}
__device__ __forceinline__ bool plane_q(const int16_t* p, float min_disp, int* q) {
    const int v = *p;
    *q = v;
    return (float)v * 0.0625f > min_disp;
}

// The plane search's state (sdr_find_planes*), written by its one-workgroup kernels and read by the
// kernels behind them on the stream.
struct SearchState {
    int stopped;      // a round has stopped the search (or the region is out of range)
    int winner;       // the round's winning hypothesis
    int score, voids;
    double a, b, c;   // its seed plane, in 1/16 px
};
constexpr uint8_t kFreeLabel = 255;

// Pixel (u, v) of the slice's region on the 1/16 px grid; true when it counts: valid, confident
// and, in the search (kFree), not yet claimed by a plane.
template <bool kFree, typename T, typename L>
__device__ __forceinline__ bool plane_pixel(const RegionView<T, L>& sl, const sdr_plane_params& P, unsigned u,
                                            unsigned v, int* q) {
    bool ok = plane_q(sl.fd + (size_t)v * sl.stride + u, P.min_disp, q);
    if (sl.fc) ok = ok && sl.fc[(size_t)v * sl.W + u] >= P.conf_min;
    if (kFree) ok = ok && sl.fl[(size_t)v * sl.W + u] == kFreeLabel;
    return ok;
}

// One sweep over the regions' pixels: grid (slices of a W x H frame, regions).  Sweep 0 sums the
// moments of the valid pixels, sweep s = 1..iterations those of the pixels within the scheduled
// band of fit s - 1, sweep iterations + 1 the statistics against the last fit.  A region that is
// out of range, a slice past its area and a chain that a degenerate fit has stopped leave at once
// (block-uniform); no workgroup waits on another.
//
// kSearch (sdr_find_planes*): one region, `acc` its round's accumulators, the sweeps 1..iterations + 1
// only; a pixel counts only while it is free (its label 255), sweep 1's previous plane is the
// round's seed plane, and a stopped search leaves at once.  The sums and the residual are the
// same code either way.
template <typename T, bool kSearch>
__global__ __launch_bounds__(kRegionThreads) void k_plane_sweep(RegionMaps<T> maps, sdr_plane_params P,
                                                               const sdr_segment* __restrict__ regs,
                                                               long long* __restrict__ acc, int sweep,
                                                               const uint8_t* __restrict__ labels,
                                                               const SearchState* __restrict__ state) {
#pragma clang fp contract(off)
    __shared__ long long red[kRegionWaves][kPlaneMoments];
    const int k = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (kSearch && state->stopped) return;  // block-uniform
    const sdr_segment sg = regs[k];
    if (!maps.holds(sg)) return;
    RegionSlice<T> sl;
    if (!region_cut(maps.view(sg, kSearch ? labels : nullptr), &sl)) return;
    long long* A = acc + (size_t)k * (size_t)(P.iterations + 2) * kPlaneSlots;
    const bool last = sweep == P.iterations + 1;
    PlaneFit fit = {0.0, 0.0, 0.0, true};
    double band = 0.0;
    if (sweep > 0) {
        if (kSearch && sweep == 1)
            fit = PlaneFit{state->a, state->b, state->c, true};
        else
            fit = plane_solve(A + (size_t)(sweep - 1) * kPlaneSlots, P.min_inliers);
        if (!fit.ok) return;  // the chain has stopped: the later sweeps' accumulators stay 0
        band = (double)P.inlier_px * 16.0 * (double)(1 << (last ? 0 : P.iterations - sweep));
    }

    long long m[kPlaneMoments];
#pragma unroll
    for (int i = 0; i < kPlaneMoments; i++) m[i] = 0;
    double rmax = 0.0;
    sl.each([&](unsigned u, unsigned v) __attribute__((always_inline)) {
        int q;
        bool ok = plane_pixel<kSearch>(sl, P, u, v, &q);
        double r = 0.0;
        if (sweep > 0) {
            r = (double)q - plane_at(fit, (double)u, (double)v);
            ok = ok && fabs(r) <= band;
        }
        if (!ok) return;
        if (last) {
            const long long e = llrint(r * 16.0);
            m[0] += 1;
            m[1] += e * e;
            rmax = fmax(rmax, fabs(r));
        } else {
            const long long lu = u, lv = v, lq = q;
            m[0] += 1;
            m[1] += lu;
            m[2] += lv;
            m[3] += lq;
            m[4] += lu * lu;
            m[5] += lu * lv;
            m[6] += lv * lv;
            m[7] += lu * lq;
            m[8] += lv * lq;
        }
    });
    // wave butterflies, then the waves' sums through LDS; a maximum of non-negative doubles is
    // the maximum of their bits
    const int nsum = last ? 2 : kPlaneMoments;
#pragma unroll
    for (int i = 0; i < kPlaneMoments; i++) {
        if (i < nsum) {  // block-uniform
            const long long s = wave_sum(m[i]);
            if (lane == 0) red[wave][i] = s;
        }
    }
    if (last) {
        const long long b = wave_max(__double_as_longlong(rmax));
        if (lane == 0) red[wave][2] = b;
    }
    __syncthreads();
    long long* dst = A + (size_t)sweep * kPlaneSlots;
    if (tid < nsum) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < kRegionWaves; w++) s += red[w][tid];
        if (s) atomicAdd((unsigned long long*)dst + tid, (unsigned long long)s);
    } else if (last && tid == 2) {
        long long b = 0;
#pragma unroll
        for (int w = 0; w < kRegionWaves; w++) b = max(b, red[w][2]);
        if (b) atomicMax((unsigned long long*)dst + 2, (unsigned long long)b);
    }
}

// reprojectImageTo3D's row sums at a real-valued pixel, the point kept in double
__device__ __forceinline__ void plane_reproject(const Q16& Q, double x, double y, double d, double* o) {
#pragma clang fp contract(off)
    double h[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double s = 0.0;
        s += Q.q[i * 4 + 0] * x;
        s += Q.q[i * 4 + 1] * y;
        s += Q.q[i * 4 + 2] * d;
        s += Q.q[i * 4 + 3] * 1.0;
        h[i] = s;
    }
    o[0] = h[0] / h[3];
    o[1] = h[1] / h[3];
    o[2] = h[2] / h[3];
}

// The statistics, coefficients and 3-D plane of a record from the last fit, its moment set M and
// the statistics sweep's sums L = {n_inliers, See, the bits of max |r|}; o.flags becomes
// SDR_PLANE_OK or SDR_PLANE_NONFINITE.
__device__ __forceinline__ void plane_record(sdr_plane& o, const PlaneRect& R, const PlaneFit& fit,
                                             const long long* __restrict__ M,
                                             const long long* __restrict__ L, const Q16& Q) {
#pragma clang fp contract(off)
    o.n_inliers = (int)L[0];
    if (L[0] > 0) {
        o.rms_px = canon(sqrt((double)L[1] / (double)L[0]) / 256.0);
        o.max_abs_px = (float)(__longlong_as_double(L[2]) / 16.0);
    }
    o.coef[0] = fit.a * 0.0625;
    o.coef[1] = fit.b * 0.0625;
    o.coef[2] = fit.c * 0.0625;
    const double ue = (double)(R.rw - 1), ve = (double)(R.rh - 1);
    const double xs = (double)R.xs, ys = (double)R.ys;
    double p0[3], p1[3], p2[3], ce[3];
    plane_reproject(Q, xs, ys, plane_at(fit, 0.0, 0.0) * 0.0625, p0);
    plane_reproject(Q, (double)(R.xs + R.rw - 1), ys, plane_at(fit, ue, 0.0) * 0.0625, p1);
    plane_reproject(Q, xs, (double)(R.ys + R.rh - 1), plane_at(fit, 0.0, ve) * 0.0625, p2);
    const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    const double mx = e1y * e2z - e1z * e2y;
    const double my = e1z * e2x - e1x * e2z;
    const double mz = e1x * e2y - e1y * e2x;
    const double len = sqrt((mx * mx + my * my) + mz * mz);
    double nx = mx / len, ny = my / len, nz = mz / len;
    double off = -((nx * p0[0] + ny * p0[1]) + nz * p0[2]);
    if (off < 0.0) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
        off = -off;
    }
    const double N = (double)M[0];
    const double cu = (double)M[1] / N, cv = (double)M[2] / N;
    plane_reproject(Q, xs + cu, ys + cv, plane_at(fit, cu, cv) * 0.0625, ce);
    if (isfinite(nx) && isfinite(ny) && isfinite(nz) && isfinite(off) && isfinite(ce[0]) && isfinite(ce[1]) &&
        isfinite(ce[2])) {
        o.normal[0] = nx;
        o.normal[1] = ny;
        o.normal[2] = nz;
        o.offset = off;
        for (int i = 0; i < 3; i++) o.centroid[i] = ce[i];
        o.flags = SDR_PLANE_OK;
    } else {
        o.flags = SDR_PLANE_NONFINITE;
    }
}

// The records, one lane a region, from the accumulators the sweeps have left.
__global__ __launch_bounds__(64) void k_plane_finish(const sdr_segment* __restrict__ regs, int K,
                                                     RegionDims dims, Q16 Q, sdr_plane_params P,
                                                     const long long* __restrict__ acc,
                                                     sdr_plane* __restrict__ out) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    const sdr_segment sg = regs[k];
    const double qn = __builtin_nan("");
    sdr_plane o;
    for (int i = 0; i < 3; i++) o.coef[i] = o.normal[i] = o.centroid[i] = qn;
    o.offset = o.rms_px = qn;
    o.max_abs_px = ruler_nan();
    o.x0 = min(sg.x0, sg.x1);
    o.y0 = min(sg.y0, sg.y1);
    o.frame = sg.frame;
    o.area = o.n_valid = o.n_inliers = o.fits = 0;
    o.flags = SDR_PLANE_OUT_OF_RANGE;
    o.reserved = 0;
    if (!dims.holds(sg)) {
        out[k] = o;
        return;
    }
    const PlaneRect R = plane_rect(sg);
    const long long* A = acc + (size_t)k * (size_t)(P.iterations + 2) * kPlaneSlots;
    o.area = R.rw * R.rh;
    o.n_valid = (int)A[0];
    PlaneFit fit = {0.0, 0.0, 0.0, false};
    const long long* M = A;
    for (int s = 0; s <= P.iterations; s++) {
        M = A + (size_t)s * kPlaneSlots;
        fit = plane_solve(M, P.min_inliers);
        if (!fit.ok) break;
        o.fits++;
    }
    if (!fit.ok) {
        o.flags = SDR_PLANE_DEGENERATE;
        out[k] = o;
        return;
    }
    plane_record(o, R, fit, M, A + (size_t)(P.iterations + 1) * kPlaneSlots, Q);
    out[k] = o;
}

// ---- the plane search (the definition: sdr.h, "the dominant planes of a region") ----
static_assert(sizeof(sdr_plane_search_params) == 64, "sdr_plane_search_params is 64 bytes");
static_assert(sizeof(sdr_plane_search_round) == 16, "sdr_plane_search_round is 16 bytes");
static_assert(sizeof(SearchState) == 40, "SearchState is 40 bytes");

// A hypothesis: the plane A*u + B*v + C*q = D through its three points; C == 0: void.
struct SearchHyp {
    int A, B, C, pad;
    long long D;
    long long pad2;
};
static_assert(sizeof(SearchHyp) == 32, "SearchHyp is 32 bytes");

constexpr int kSearchTries = 16;
constexpr int kSearchChunk = 64;  // hypotheses a workgroup of the score kernel (grid y)

__device__ __forceinline__ uint32_t search_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// the record of a round that did not run, or of a region out of range (flags)
__device__ __forceinline__ void search_empty_record(sdr_plane* o, const sdr_segment& sg, int area, uint32_t flags) {
    const double qn = __builtin_nan("");
    for (int i = 0; i < 3; i++) o->coef[i] = o->normal[i] = o->centroid[i] = qn;
    o->offset = o->rms_px = qn;
    o->max_abs_px = ruler_nan();
    o->x0 = min(sg.x0, sg.x1);
    o->y0 = min(sg.y0, sg.y1);
    o->frame = sg.frame;
    o->area = area;
    o->n_valid = o->n_inliers = o->fits = 0;
    o->flags = flags;
    o->reserved = 0;
}

__device__ __forceinline__ void search_round(sdr_plane_search_round* rounds, int r, int h, int score, int voids,
                                             uint32_t stop) {
    if (!rounds) return;
    rounds[r].hypothesis = h;
    rounds[r].score = score;
    rounds[r].voids = voids;
    rounds[r].stop = stop;
}

// One thread stops the search in round r: the count, the records r.., the rounds r..
__device__ __forceinline__ void search_stop(SearchState* st, const sdr_segment& sg, int area, int r, int max_planes,
                                            int h, int score, int voids, uint32_t code, uint32_t rec_flags,
                                            sdr_plane* planes, int32_t* count, sdr_plane_search_round* rounds) {
    st->stopped = 1;
    *count = r;
    for (int i = r; i < max_planes; i++) {
        search_empty_record(planes + i, sg, area, rec_flags);
        if (i == r && code != SDR_SEARCH_NOT_RUN)
            search_round(rounds, i, h, score, voids, code);
        else
            search_round(rounds, i, -1, 0, 0, SDR_SEARCH_NOT_RUN);
    }
}

// Before round 0: a region out of range stops the search with its records.
__global__ __launch_bounds__(64) void k_search_init(const sdr_segment* __restrict__ reg, RegionDims dims,
                                                    int max_planes, SearchState* __restrict__ st,
                                                    sdr_plane* __restrict__ planes, int32_t* __restrict__ count,
                                                    sdr_plane_search_round* __restrict__ rounds) {
    if (threadIdx.x != 0) return;
    const sdr_segment sg = reg[0];
    *count = 0;
    if (!dims.holds(sg))
        search_stop(st, sg, 0, 0, max_planes, -1, 0, 0, SDR_SEARCH_NOT_RUN, SDR_PLANE_OUT_OF_RANGE, planes, count,
                    rounds);
}

// The draws of round r, a thread a hypothesis.
template <typename T>
__global__ __launch_bounds__(64) void k_search_draw(RegionMaps<T> maps, sdr_plane_params P, const sdr_segment* __restrict__ reg,
                                                    const uint8_t* __restrict__ labels, int r, int M, uint32_t seed,
                                                    const SearchState* __restrict__ st,
                                                    SearchHyp* __restrict__ hyp) {
    if (st->stopped) return;
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= M) return;
    const sdr_segment sg = reg[0];
    const RegionView<T> vw = maps.view(sg, labels);  // in range: k_search_init
    const PlaneRect R = vw.R;
    const unsigned area = (unsigned)R.rw * (unsigned)R.rh;
    const uint32_t key = search_mix(search_mix(seed ^ (0x9E3779B9u * (uint32_t)(r + 1))) ^ (uint32_t)h);
    int pu[3], pv[3], pq[3];
    bool found = true;
    for (int j = 0; j < 3; j++) {
        bool got = false;
        for (int t = 0; t < kSearchTries && !got; t++) {
            const uint32_t x = search_mix(key ^ (uint32_t)(16 * j + t));
            const unsigned p = (unsigned)(((unsigned long long)x * area) >> 32);  // < area
            const unsigned v = p / (unsigned)R.rw, u = p - v * (unsigned)R.rw;
            int q;
            const bool ok = plane_pixel<true>(vw, P, u, v, &q);
            if (ok) {
                pu[j] = (int)u;
                pv[j] = (int)v;
                pq[j] = q;
                got = true;
            }
        }
        found = found && got;
        if (!got) pu[j] = pv[j] = pq[j] = 0;
    }
    SearchHyp o = {0, 0, 0, 0, 0, 0};
    if (found) {
        const long long du1 = pu[1] - pu[0], dv1 = pv[1] - pv[0], dq1 = pq[1] - pq[0];
        const long long du2 = pu[2] - pu[0], dv2 = pv[2] - pv[0], dq2 = pq[2] - pq[0];
        const long long A = dv1 * dq2 - dq1 * dv2, B = dq1 * du2 - du1 * dq2, C = du1 * dv2 - dv1 * du2;
        if (C != 0) {  // |A|, |B| < 2^31, |C| < 2^25 (sdr.h)
            o.A = (int)A;
            o.B = (int)B;
            o.C = (int)C;
            o.D = A * pu[0] + B * pv[0] + C * pq[0];
        }
    }
    hyp[h] = o;
}

// The scores of round r: grid (slices of a W x H frame, chunks of kSearchChunk hypotheses).  A
// workgroup keeps its slice's pixels in registers and walks its chunk's hypotheses (their index is
// wave-uniform: scalar loads).  A wave counts a hypothesis' pixels by
// ballots, the waves' counts meet in LDS, and one integer atomic a (workgroup, hypothesis with a
// count) goes to the score array: neither the slices' order nor the grid shows in the result.  It
// also counts the round's free pixels (the record's n_valid) into acc[0].
template <typename T>
__global__ __launch_bounds__(kRegionThreads) void k_search_score(RegionMaps<T> maps, sdr_plane_params P,
                                                                const sdr_segment* __restrict__ reg,
                                                                const uint8_t* __restrict__ labels, int M,
                                                                const SearchState* __restrict__ st,
                                                                const SearchHyp* __restrict__ hyp,
                                                                unsigned* __restrict__ scores,
                                                                long long* __restrict__ acc) {
    __shared__ unsigned cnt[kRegionWaves][kSearchChunk];
    if (st->stopped) return;  // block-uniform
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    RegionSlice<T> sl;
    if (!region_cut(maps.view(reg[0], labels), &sl)) return;
    const long long Tq = (long long)floor((double)P.inlier_px * 16.0);

    // the loop is written out: every lane takes part in a step's ballot, past the area too
    int pu[kRegionPix], pv[kRegionPix], pq[kRegionPix];
    bool pf[kRegionPix];
    int nfree = 0;
#pragma unroll
    for (int j = 0; j < kRegionPix; j++) {
        const unsigned p = sl.base + (unsigned)(j * kRegionThreads + tid);
        pu[j] = pv[j] = pq[j] = 0;
        pf[j] = false;
        if (p < sl.area) {
            const unsigned v = p / (unsigned)sl.R.rw, u = p - v * (unsigned)sl.R.rw;
            int q;
            const bool ok = plane_pixel<true>(sl, P, u, v, &q);
            pu[j] = (int)u;
            pv[j] = (int)v;
            pq[j] = ok ? q : 0;
            pf[j] = ok;
        }
        nfree += __popcll(__ballot(pf[j]));  // the wave's count, in every lane
    }
    const int c0 = (int)blockIdx.y * kSearchChunk;  // < M: the grid
    if (c0 == 0 && lane == 0 && nfree) atomicAdd((unsigned long long*)acc, (unsigned long long)nfree);
    {
        const int nh = min(M - c0, kSearchChunk);
        for (int i = 0; i < nh; i++) {  // at most kSearchChunk
            const SearchHyp hp = hyp[c0 + i];  // wave-uniform
            unsigned c = 0;
            if (hp.C != 0) {
                const long long thr = Tq * (long long)abs(hp.C);
#pragma unroll
                for (int j = 0; j < kRegionPix; j++) {
                    const long long e = ((long long)hp.A * pu[j] + (long long)hp.B * pv[j] +
                                         (long long)hp.C * pq[j]) - hp.D;
                    const bool in = pf[j] && (e < 0 ? -e : e) <= thr;
                    c += (unsigned)__popcll(__ballot(in));
                }
            }
            if (lane == 0) cnt[wave][i] = c;
        }
        __syncthreads();
        if (tid < nh) {
            unsigned s = 0;
#pragma unroll
            for (int w = 0; w < kRegionWaves; w++) s += cnt[w][tid];
            if (s) atomicAdd(scores + c0 + tid, s);
        }
    }
}

// The pick of round r by one workgroup: the highest score among the hypotheses that are not void,
// ties to the lowest index (the maximum of (score << 32) | ~h), the stop decision, the seed plane.
__global__ __launch_bounds__(kRegionThreads) void k_search_pick(const sdr_segment* __restrict__ reg, int r,
                                                               int max_planes, int M, int min_inliers,
                                                               const SearchHyp* __restrict__ hyp,
                                                               const unsigned* __restrict__ scores,
                                                               SearchState* __restrict__ st,
                                                               sdr_plane* __restrict__ planes,
                                                               int32_t* __restrict__ count,
                                                               sdr_plane_search_round* __restrict__ rounds) {
#pragma clang fp contract(off)
    __shared__ unsigned long long best[kRegionWaves];
    __shared__ int nvoid[kRegionWaves];
    if (st->stopped) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long key = 0;
    int voids = 0;
    for (int h = tid; h < M; h += kRegionThreads) {  // at most 16 passes
        if (hyp[h].C == 0) {
            voids++;
        } else {
            const unsigned long long k = ((unsigned long long)scores[h] << 32) | (unsigned long long)(0xffffffffu - (unsigned)h);
            key = max(key, k);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        key = max(key, (unsigned long long)__shfl_xor((long long)key, o, 64));
        voids += __shfl_xor(voids, o, 64);
    }
    if (lane == 0) {
        best[wave] = key;
        nvoid[wave] = voids;
    }
    __syncthreads();
    if (tid != 0) return;
    key = 0;
    voids = 0;
    for (int w = 0; w < kRegionWaves; w++) {
        key = max(key, best[w]);
        voids += nvoid[w];
    }
    const sdr_segment sg = reg[0];
    const PlaneRect R = plane_rect(sg);
    const int area = R.rw * R.rh;
    if (voids == M) {
        search_stop(st, sg, area, r, max_planes, -1, 0, voids, SDR_SEARCH_NO_HYPOTHESIS, SDR_PLANE_DEGENERATE, planes,
                    count, rounds);
        return;
    }
    const int h = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    const int score = (int)(key >> 32);
    if (score < min_inliers) {
        search_stop(st, sg, area, r, max_planes, h, score, voids, SDR_SEARCH_LOW_SCORE, SDR_PLANE_DEGENERATE, planes,
                    count, rounds);
        return;
    }
    const SearchHyp hp = hyp[h];
    st->winner = h;
    st->score = score;
    st->voids = voids;
    st->a = -(double)hp.A / (double)hp.C;
    st->b = -(double)hp.B / (double)hp.C;
    st->c = (double)hp.D / (double)hp.C;
}

// The record of round r from its accumulators, or the stop the refits or the statistics call for.
__global__ __launch_bounds__(64) void k_search_finish(const sdr_segment* __restrict__ reg, int r, int max_planes,
                                                      Q16 Q, sdr_plane_params P, const long long* __restrict__ A,
                                                      SearchState* __restrict__ st, sdr_plane* __restrict__ planes,
                                                      int32_t* __restrict__ count,
                                                      sdr_plane_search_round* __restrict__ rounds) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || st->stopped) return;
    const sdr_segment sg = reg[0];
    const PlaneRect R = plane_rect(sg);
    const int area = R.rw * R.rh;
    const int h = st->winner, score = st->score, voids = st->voids;
    PlaneFit fit = {0.0, 0.0, 0.0, false};
    const long long* M = A;
    for (int s = 1; s <= P.iterations; s++) {
        M = A + (size_t)s * kPlaneSlots;
        fit = plane_solve(M, P.min_inliers);
        if (!fit.ok) break;
    }
    const long long* L = A + (size_t)(P.iterations + 1) * kPlaneSlots;
    if (!fit.ok || L[0] < (long long)P.min_inliers) {
        search_stop(st, sg, area, r, max_planes, h, score, voids,
                    fit.ok ? SDR_SEARCH_FEW_INLIERS : SDR_SEARCH_REFIT_DEGENERATE, SDR_PLANE_DEGENERATE, planes,
                    count, rounds);
        return;
    }
    sdr_plane o;
    search_empty_record(&o, sg, area, 0);
    o.n_valid = (int)A[0];
    o.fits = P.iterations + 1;
    plane_record(o, R, fit, M, L, Q);
    planes[r] = o;
    *count = r + 1;
    search_round(rounds, r, h, score, voids, SDR_SEARCH_RAN);
}

// The claim of round r: the statistics sweep's inliers (the same residual against the same plane)
// get the round's label.  A pass of its own behind k_search_finish: a round that stops claims
// nothing, and no sweep can see a partly claimed map.
template <typename T>
__global__ __launch_bounds__(kRegionThreads) void k_search_claim(RegionMaps<T> maps, sdr_plane_params P,
                                                                const sdr_segment* __restrict__ reg,
                                                                uint8_t* __restrict__ labels, int r,
                                                                const SearchState* __restrict__ st,
                                                                const long long* __restrict__ A) {
#pragma clang fp contract(off)
    if (st->stopped) return;  // block-uniform
    RegionSlice<T, uint8_t> sl;
    if (!region_cut(maps.view(reg[0], labels), &sl)) return;
    const int W = maps.W;
    const PlaneFit fit = plane_solve(A + (size_t)P.iterations * kPlaneSlots, P.min_inliers);  // ok: not stopped
    const double band = (double)P.inlier_px * 16.0;
    sl.each([&](unsigned u, unsigned v) __attribute__((always_inline)) {
        int q;
        const bool ok = plane_pixel<true>(sl, P, u, v, &q);
        const double res = (double)q - plane_at(fit, (double)u, (double)v);
        if (ok && fabs(res) <= band) sl.fl[(size_t)v * W + u] = (uint8_t)r;
    });
}

// Point queries, one wave a query: the ruler's sample and its distance to a fitted plane.
template <typename T>
__global__ __launch_bounds__(kRegionThreads) void k_plane_distance(RegionMaps<T> maps, Q16 Q, sdr_ruler_params P,
                                                                  const sdr_plane* __restrict__ planes, int NP,
                                                                  const sdr_plane_query* __restrict__ qs, int K,
                                                                  struct sdr_plane_distance* __restrict__ out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * kRegionWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (k >= K) return;  // wave-uniform
    const sdr_plane_query q = qs[k];
    const bool inside = maps.holds(q.frame, q.x, q.y);
    uint32_t flags = inside ? 0 : SDR_PDIST_OUT_OF_RANGE;
    RegionPlane pl = {{0.0, 0.0, 0.0}, 0.0};
    const bool plane_ok = query_plane(planes, NP, q.plane, &pl);
    if (!plane_ok) flags |= SDR_PDIST_NO_PLANE;
    RulerSample s;
    s.d = s.xyz[0] = s.xyz[1] = s.xyz[2] = ruler_nan();
    s.n = 0;
    s.valid = false;
    if (inside) s = ruler_sample(maps.frame(q.frame), Q, P, q.x, q.y, lane);
    if (lane != 0) return;
    double dist = __builtin_nan("");
    if (s.valid && plane_ok) {
        dist = canon(((pl.n[0] * (double)s.xyz[0] + pl.n[1] * (double)s.xyz[1]) + pl.n[2] * (double)s.xyz[2]) + pl.off);
        flags |= SDR_PDIST_VALID;
    }
    struct sdr_plane_distance* o = out + k;
    o->p[0] = canon(s.xyz[0]);
    o->p[1] = canon(s.xyz[1]);
    o->p[2] = canon(s.xyz[2]);
    o->d = s.d;
    o->distance = dist;
    o->n = s.n;
    o->flags = flags;
}

}  // namespace sdr

namespace {

using namespace sdr::ruler_host;

int check_plane_params(const sdr_plane_params* p) {
    if (p->iterations < 0 || p->iterations > 8) return rfail(SDR_ERR_ARG, "iterations must be in 0..8");
    if (p->min_inliers < 3) return rfail(SDR_ERR_ARG, "min_inliers must be >= 3");
    if (!(p->inlier_px > 0.0f && p->inlier_px <= 64.0f)) return rfail(SDR_ERR_ARG, "inlier_px must be in (0, 64]");
    return SDR_OK;
}

int check_search_params(const sdr_plane_search_params* p) {
    const int rc = check_plane_params(&p->fit);
    if (rc) return rc;
    if (p->fit.iterations < 1) return rfail(SDR_ERR_ARG, "the plane search takes iterations in 1..8");
    if (p->max_planes < 1 || p->max_planes > 8) return rfail(SDR_ERR_ARG, "max_planes must be in 1..8");
    if (p->hypotheses < 1 || p->hypotheses > 4096) return rfail(SDR_ERR_ARG, "hypotheses must be in 1..4096");
    return SDR_OK;
}

int check_query_params(const sdr_ruler_params* p, const void* planes, int P) {
    if (p->radius < 0 || p->radius > 4) return rfail(SDR_ERR_ARG, "radius must be in 0..4");
    if (p->min_count < 1) return rfail(SDR_ERR_ARG, "min_count must be >= 1");
    return check_planes_arg(planes, P);
}

}  // namespace

extern "C" {

void sdr_plane_params_default(sdr_plane_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->iterations = 3;
    p->min_inliers = 16;
    p->inlier_px = 1.0f;
    p->min_disp = -1.0f;
    p->conf_min = 0.0f;
}

int sdr_fit_planes_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride, int W,
                          int H, int F, const float* d_conf, const double Q[16],
                          const sdr_plane_params* params, const sdr_segment* d_regions, int K,
                          sdr_plane* d_planes, void* stream) {
    int rc = check_plane_maps(d_disp, disp_type, stride, frame_stride, W, H, F, Q, params, d_regions, K, d_planes);
    if (rc || (rc = check_plane_params(params))) return rc;
    if (K == 0) return SDR_OK;
    hipStream_t st = (hipStream_t)stream;
    const sdr::Q16 q = make_q16(Q);
    const int sweeps = params->iterations + 2;
    const size_t per = (size_t)sweeps * sdr::kPlaneSlots;
    sdr::ScratchLayout lay;
    const auto s_acc = lay.take<long long>((size_t)K * per);
    sdr::Scratch sc(st);
    if ((rc = sc.open(lay))) return rc;
    long long* acc = sc.at(s_acc);
    SDR_HIP(hipMemsetAsync(acc, 0, s_acc.bytes(), st));
    const unsigned slices = sdr::region_slices(W, H);
    for (int s = 0; s < sweeps; s++)
        for (int k0 = 0; k0 < K; k0 += 65535) {  // the grid's y extent
            const dim3 grid(slices, (unsigned)std::min(K - k0, 65535)), block(sdr::kRegionThreads);
            with_maps(d_disp, disp_type, stride, frame_stride, W, H, F, d_conf, nullptr, [&](auto maps) {
                hipLaunchKernelGGL((sdr::k_plane_sweep<disp_elem_t<decltype(maps)>, false>), grid, block, 0, st, maps,
                                   *params, d_regions + k0, acc + k0 * per, s, (const uint8_t*)nullptr,
                                   (const sdr::SearchState*)nullptr);
            });
        }
    hipLaunchKernelGGL(sdr::k_plane_finish, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, st, d_regions, K,
                       sdr::RegionDims{W, H, F, 0}, q, *params, (const long long*)acc, d_planes);
    return sc.finish();
}

void sdr_plane_search_params_default(sdr_plane_search_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    sdr_plane_params_default(&p->fit);
    p->fit.min_inliers = 64;
    p->max_planes = 4;
    p->hypotheses = 256;
    p->seed = 0;
}

int sdr_find_planes_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride, int W, int H,
                           int F, const float* d_conf, const double Q[16], const sdr_plane_search_params* params,
                           const sdr_segment* d_region, sdr_plane* d_planes, int32_t* d_count,
                           sdr_plane_search_round* d_rounds, uint8_t* d_labels, void* stream) {
    int rc = check_plane_maps(d_disp, disp_type, stride, frame_stride, W, H, F, Q, params, d_region, 1, d_planes);
    if (rc) return rc;
    if (!d_count) return rfail(SDR_ERR_ARG, "null argument");
    if ((rc = check_search_params(params))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const sdr::Q16 q = make_q16(Q);
    const sdr_plane_params P = params->fit;
    const int NP = params->max_planes, M = params->hypotheses;
    const size_t px = (size_t)W * H;
    // scratch: {state, the rounds' accumulators, the rounds' scores} zeroed, the hypotheses of one
    // round (every round writes all M before it reads them), the claim map when the caller has none
    const size_t per = (size_t)(P.iterations + 2) * sdr::kPlaneSlots;
    sdr::ScratchLayout lay;
    const auto s_state = lay.take<sdr::SearchState>(1);
    const auto s_acc = lay.take<long long>((size_t)NP * per);
    const auto s_scores = lay.take<unsigned>((size_t)NP * M);
    const auto s_hyp = lay.take<sdr::SearchHyp>((size_t)M);
    const auto s_lab = lay.take<uint8_t>(d_labels ? 0 : px);
    sdr::Scratch sc(st);
    if ((rc = sc.open(lay))) return rc;
    sdr::SearchState* state = sc.at(s_state);
    long long* acc = sc.at(s_acc);
    unsigned* scores = sc.at(s_scores);
    sdr::SearchHyp* hyp = sc.at(s_hyp);
    uint8_t* labels = d_labels ? d_labels : sc.at(s_lab);
    SDR_HIP(hipMemsetAsync(state, 0, s_hyp.off, st));  // everything ahead of the hypotheses
    SDR_HIP(hipMemsetAsync(labels, 0xff, px, st));
    const unsigned slices = sdr::region_slices(W, H);
    const dim3 sgrid(slices), sblock(sdr::kRegionThreads), dgrid((unsigned)((M + 63) / 64)), one(1), wave(64);
    const dim3 cgrid(slices, (unsigned)((M + sdr::kSearchChunk - 1) / sdr::kSearchChunk));
    hipLaunchKernelGGL(sdr::k_search_init, one, wave, 0, st, d_region, sdr::RegionDims{W, H, F, 0}, NP, state, d_planes,
                       d_count, d_rounds);
    // the maps carry no label map: the search's claim map is one frame's and goes beside them
    auto round = [&](auto maps, int r) {
        using T = disp_elem_t<decltype(maps)>;
        long long* A = acc + (size_t)r * per;
        unsigned* S = scores + (size_t)r * M;
        hipLaunchKernelGGL(sdr::k_search_draw<T>, dgrid, wave, 0, st, maps, P, d_region, (const uint8_t*)labels, r, M,
                           params->seed, (const sdr::SearchState*)state, hyp);
        hipLaunchKernelGGL(sdr::k_search_score<T>, cgrid, sblock, 0, st, maps, P, d_region, (const uint8_t*)labels, M,
                           (const sdr::SearchState*)state, (const sdr::SearchHyp*)hyp, S, A);
        hipLaunchKernelGGL(sdr::k_search_pick, one, sblock, 0, st, d_region, r, NP, M, P.min_inliers,
                           (const sdr::SearchHyp*)hyp, (const unsigned*)S, state, d_planes, d_count, d_rounds);
        for (int s = 1; s <= P.iterations + 1; s++)
            hipLaunchKernelGGL((sdr::k_plane_sweep<T, true>), sgrid, sblock, 0, st, maps, P, d_region, A, s,
                               (const uint8_t*)labels, (const sdr::SearchState*)state);
        hipLaunchKernelGGL(sdr::k_search_finish, one, wave, 0, st, d_region, r, NP, q, P, (const long long*)A, state,
                           d_planes, d_count, d_rounds);
        hipLaunchKernelGGL(sdr::k_search_claim<T>, sgrid, sblock, 0, st, maps, P, d_region, labels, r,
                           (const sdr::SearchState*)state, (const long long*)A);
    };
    for (int r = 0; r < NP; r++)
        with_maps(d_disp, disp_type, stride, frame_stride, W, H, F, d_conf, nullptr, [&](auto maps) { round(maps, r); });
    return sc.finish();
}

int sdr_find_planes(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H, int F,
                    const float* conf, const double Q[16], const sdr_plane_search_params* params,
                    const sdr_segment* region, sdr_plane* planes, int32_t* count, sdr_plane_search_round* rounds,
                    uint8_t* labels) {
    int rc = check_plane_maps(disp, disp_type, stride, frame_stride, W, H, F, Q, params, region, 1, planes);
    if (rc) return rc;
    if (!count) return rfail(SDR_ERR_ARG, "null argument");
    if ((rc = check_search_params(params))) return rc;
    const size_t NP = (size_t)params->max_planes;
    HostCall c;
    const HostCall::Maps m = c.maps(disp, disp_type, stride, frame_stride, W, H, F, conf);
    const sdr_segment* d_region = c.input(c.S->rows, region, 1);
    const auto s_planes = c.output(planes, NP);
    const auto s_count = c.output(count, 1);
    const auto s_rounds = c.output(rounds, NP);  // the device form always writes them
    const auto s_labels = c.output(labels, labels ? (size_t)W * H : 0);
    if ((rc = c.ready())) return rc;
    rc = sdr_find_planes_device(m.disp, disp_type, m.stride, m.fstride, W, H, F, m.conf, Q, params, d_region,
                                c.at(s_planes), c.at(s_count), c.at(s_rounds), labels ? c.at(s_labels) : nullptr,
                                c.stream());
    return rc ? rc : c.finish();
}

int sdr_plane_distance_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride, int W,
                              int H, int F, const float* d_conf, const double Q[16],
                              const sdr_ruler_params* params, const sdr_plane* d_planes, int P,
                              const sdr_plane_query* d_queries, int K,
                              struct sdr_plane_distance* d_out,
                              void* stream) {
    int rc = check_plane_maps(d_disp, disp_type, stride, frame_stride, W, H, F, Q, params, d_queries, K, d_out);
    if (rc || (rc = check_query_params(params, d_planes, P))) return rc;
    if (K == 0) return SDR_OK;
    const sdr::Q16 q = make_q16(Q);
    const dim3 grid((unsigned)((K + sdr::kRegionWaves - 1) / sdr::kRegionWaves)), block(sdr::kRegionThreads);
    with_maps(d_disp, disp_type, stride, frame_stride, W, H, F, d_conf, nullptr, [&](auto maps) {
        hipLaunchKernelGGL(sdr::k_plane_distance<disp_elem_t<decltype(maps)>>, grid, block, 0, (hipStream_t)stream, maps,
                           q, *params, d_planes, P, d_queries, K, d_out);
    });
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

int sdr_fit_planes(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H, int F,
                   const float* conf, const double Q[16], const sdr_plane_params* params,
                   const sdr_segment* regions, int K, sdr_plane* planes) {
    int rc = check_plane_maps(disp, disp_type, stride, frame_stride, W, H, F, Q, params, regions, K, planes);
    if (rc || (rc = check_plane_params(params))) return rc;
    if (K == 0) return SDR_OK;
    HostCall c;
    const HostCall::Maps m = c.maps(disp, disp_type, stride, frame_stride, W, H, F, conf);
    const sdr_segment* d_regions = c.input(c.S->rows, regions, (size_t)K);
    const auto s_planes = c.output(planes, (size_t)K);
    if ((rc = c.ready())) return rc;
    rc = sdr_fit_planes_device(m.disp, disp_type, m.stride, m.fstride, W, H, F, m.conf, Q, params, d_regions, K,
                               c.at(s_planes), c.stream());
    return rc ? rc : c.finish();
}

int sdr_plane_distance(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H,
                       int F, const float* conf, const double Q[16], const sdr_ruler_params* params,
                       const sdr_plane* planes, int P, const sdr_plane_query* queries, int K,
                       struct sdr_plane_distance* out) {
    int rc = check_plane_maps(disp, disp_type, stride, frame_stride, W, H, F, Q, params, queries, K, out);
    if (rc || (rc = check_query_params(params, planes, P))) return rc;
    if (K == 0) return SDR_OK;
    HostCall c;
    const HostCall::Maps m = c.maps(disp, disp_type, stride, frame_stride, W, H, F, conf);
    const sdr_plane* d_planes = c.input(c.S->planes, planes, (size_t)P);
    const sdr_plane_query* d_queries = c.input(c.S->rows, queries, (size_t)K);
    const auto s_out = c.output(out, (size_t)K);
    if ((rc = c.ready())) return rc;
    rc = sdr_plane_distance_device(m.disp, disp_type, m.stride, m.fstride, W, H, F, m.conf, Q, params, d_planes, P,
                                   d_queries, K, c.at(s_out), c.stream());
    return rc ? rc : c.finish();
}

}  // extern "C"
