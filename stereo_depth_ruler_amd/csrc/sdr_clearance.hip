// sdr_clearance.hip -- the clearance of two labelled things: the members of two labels in a
// rectangle, each member's point (the ruler's sample over its own set), and the closest pair of
// points, one of each set, by all pairs block against block with an exact prune on the blocks'
// bounds.  The definition is in include/sdr/sdr.h ("the clearance of two labelled things").
#include <math.h>
#include <string.h>

#include <cmath>

#include <algorithm>
#include <atomic>
#include <string>
#include <type_traits>

#include "sdr_device.hpp"
#include "sdr_internal.hpp"
#include "sdr_region.hpp"
#include "sdr_ruler_shared.hpp"

namespace sdr {

static_assert(sizeof(sdr_clearance_query) == 32, "sdr_clearance_query is 32 bytes");
static_assert(sizeof(sdr_clearance_params) == 64, "sdr_clearance_params is 64 bytes");
static_assert(sizeof(struct sdr_clearance) == 128, "sdr_clearance is 128 bytes");

constexpr int kClrBlock = 256;                     // points a block: the unit of the bounds and of the prune
constexpr int kClrPer = 4;                         // A's points a lane of the pair kernel's one wave
constexpr int kClrWave = kClrBlock / kClrPer;      // its threads
static_assert(kClrWave == 64, "the pair kernel is one wave");
constexpr int kClrGroups = 16;                     // workgroups a block of A: each takes every 16th block of B
constexpr unsigned long long kClrInf = 0x7ff0000000000000ull;  // +inf: the bits of a non-negative double order as it does

// A query's state, zeroed (best: +inf) before its first sweep.
struct ClrState {
    int n[2];                 // members of A, of B
    int m[2];                 // points appended to A's list, to B's
    unsigned long long best;  // the bits of the smallest s a workgroup has found so far
    int pad[10];
};
static_assert(sizeof(ClrState) == 64, "ClrState is 64 bytes");

// a point of a list: XYZ and the index v * rw + u of its pixel
struct ClrPoint {
    float x, y, z;
    int idx;
};
static_assert(sizeof(ClrPoint) == 16, "ClrPoint is 16 bytes");

struct ClrBounds {
    float lo[3], hi[3];
};

// a workgroup's best pair: s's bits, the indices of p and q (ip < 0: it ran no pair)
struct ClrCand {
    unsigned long long s;
    int ip, iq;
};

// One array holds both lists: A's point j at [j], B's point j at [cap - 1 - j] (the sets are
// disjoint, so m_a + m_b <= area <= cap).
__device__ __forceinline__ size_t clr_at(int set, int j, int cap) { return set ? (size_t)(cap - 1 - j) : (size_t)j; }

__device__ __forceinline__ unsigned long long clr_shfl(unsigned long long v, int o) {
    return (unsigned long long)__shfl_xor((long long)v, o, 64);
}

// (s, ip, iq) before (t, jp, jq) in the result's order; s and t are bits of non-negative doubles
__device__ __forceinline__ bool clr_before(unsigned long long s, int ip, int iq, unsigned long long t, int jp, int jq) {
    return s < t || (s == t && (ip < jp || (ip == jp && iq < jq)));
}

// Sweep 1, a workgroup a slice: mark[v * rw + u] = 1 for a member of A, 2 for a member of B, 0 for
// the rest; the members' counts.  A refused query and a slice past the area leave at once.
template <typename T>
__global__ __launch_bounds__(kRegionThreads) void k_clr_mark(
    RegionMaps<T> maps, Q16 Q, sdr_clearance_params P, const sdr_plane* __restrict__ planes, int NP,
    const sdr_clearance_query* __restrict__ query, ClrState* __restrict__ S, uint8_t* __restrict__ mark) {
#pragma clang fp contract(off)
    const sdr_clearance_query q = *query;
    RegionPlane pl;
    RegionSlice<T> sl;
    if (!query_slice(maps, planes, NP, q, &pl, &sl)) return;  // block-uniform
    const int W = maps.W;
    int na = 0, nb = 0;
    sl.each([&](unsigned u, unsigned v) __attribute__((always_inline)) {
        const int l = sl.fl[(size_t)v * W + u];
        uint8_t m = 0;
        if (l == q.label_a || l == q.label_b) {
            const RegionPix px = region_pixel(sl, Q, pl, P.min_disp, P.conf_min, l, u, v);
            if (px.member && P.h_lo <= px.hf && px.hf <= P.h_hi) m = l == q.label_a ? 1 : 2;
        }
        mark[(size_t)v * sl.R.rw + u] = m;
        na += m == 1 ? 1 : 0;
        nb += m == 2 ? 1 : 0;
    });
    const long long ca = wave_sum((long long)na), cb = wave_sum((long long)nb);
    if ((threadIdx.x & 63) == 0) {
        if (ca) atomicAdd(&S->n[0], (int)ca);
        if (cb) atomicAdd(&S->n[1], (int)cb);
    }
}

// Sweep 2, a workgroup a slice, a wave a member at a time: the member's window of the rectangle, the
// disparities of its pixels of the same set, the ruler's selection, the reprojection.  The slice's
// points are gathered in LDS (A's from the front, B's from the back) and appended to the lists with
// one reservation a set, so a list's blocks stay slices' neighbours whatever order the workgroups
// finish in; that order shows in no output.  dmed[v * rw + u]: a point's median.
template <typename T>
__global__ __launch_bounds__(kRegionThreads) void k_clr_sample(
    RegionMaps<T> maps, Q16 Q, sdr_clearance_params P, const sdr_plane* __restrict__ planes, int NP,
    const sdr_clearance_query* __restrict__ query,
    ClrState* __restrict__ S, const uint8_t* __restrict__ mark, float* __restrict__ dmed, ClrPoint* __restrict__ pts,
    int cap) {
#pragma clang fp contract(off)
    __shared__ ClrPoint buf[kRegionSlice];
    __shared__ int cnt[2], base[2];
    const sdr_clearance_query q = *query;
    RegionPlane pl;
    RegionSlice<T> sl;
    if (!query_slice(maps, planes, NP, q, &pl, &sl)) return;  // block-uniform
    const size_t stride = maps.stride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    const int rw = sl.R.rw, rh = sl.R.rh, r = P.radius;
    // the wave's 512 pixels of the slice, 64 at a time: the members among them, one after another
    for (int c = 0; c < kRegionSlice / kRegionThreads; c++) {
        const unsigned p0 = sl.base + (unsigned)((wave * (kRegionSlice / kRegionThreads) + c) * 64);
        if (p0 >= sl.area) break;  // wave-uniform
        const unsigned p = p0 + (unsigned)lane;
        const int mine = p < sl.area ? mark[p] : 0;
        unsigned long long todo = __ballot(mine != 0);
        ClrPoint pt = {0.f, 0.f, 0.f, -1};  // the point of this lane's pixel
        while (todo) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const unsigned pm = p0 + (unsigned)l;
            const int set = __builtin_amdgcn_readlane(mine, l);
            const int v = (int)(pm / (unsigned)rw), u = (int)(pm - (unsigned)v * (unsigned)rw);
            const int us = max(u - r, 0), ue = min(u + r, rw - 1);
            const int vs = max(v - r, 0), ve = min(v + r, rh - 1);
            const int ww = ue - us + 1, wc = ww * (ve - vs + 1);
            float val[2];
            bool ok[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int j = lane + 64 * k;
                val[k] = 0.f;
                ok[k] = false;
                if (j < wc) {
                    const int wy = j / ww, wx = j - wy * ww;
                    const size_t py = (size_t)(vs + wy), px = (size_t)(us + wx);
                    val[k] = load_disp(sl.fd + py * stride + px);
                    ok[k] = mark[py * (size_t)rw + px] == set;
                }
            }
            float d = 0.f;
            const int n = ruler_select(val, ok, wc, P.min_count, lane, &d);
            if (n < P.min_count) continue;  // wave-uniform (n >= 1: the member itself)
            float xyz[3];
            reproject_px(Q, sl.R.xs + u, sl.R.ys + v, (double)d, 0.0, 0, xyz);
            if (!finite3(xyz)) continue;
            if (lane == l) {
                pt = ClrPoint{xyz[0], xyz[1], xyz[2], (int)pm};
                dmed[pm] = d;
            }
        }
        // the chunk's points into the slice's buffer, in lane order
#pragma unroll
        for (int set = 0; set < 2; set++) {
            const bool has = pt.idx >= 0 && mine == set + 1;
            const unsigned long long hm = __ballot(has);
            if (!hm) continue;
            int b = 0;
            if (lane == 0) b = atomicAdd(&cnt[set], __popcll(hm));
            b = __builtin_amdgcn_readfirstlane(b);
            if (has) {
                const int j = b + __popcll(hm & ((1ull << lane) - 1ull));
                buf[set ? kRegionSlice - 1 - j : j] = pt;
            }
        }
    }
    __syncthreads();
    if (tid < 2) base[tid] = cnt[tid] ? atomicAdd(&S->m[tid], cnt[tid]) : 0;
    __syncthreads();
#pragma unroll
    for (int set = 0; set < 2; set++)
        for (int j = tid; j < cnt[set]; j += kRegionThreads)
            pts[clr_at(set, base[set] + j, cap)] = buf[set ? kRegionSlice - 1 - j : j];
}

// The bounds of every block of kClrBlock points of the two lists: grid (blocks a list at most, 2),
// one wave a block.
__global__ __launch_bounds__(kClrWave) void k_clr_bounds(const ClrState* __restrict__ S,
                                                         const ClrPoint* __restrict__ pts, int cap,
                                                         ClrBounds* __restrict__ bounds, int maxblocks) {
    const int set = blockIdx.y, jb = blockIdx.x, lane = threadIdx.x;
    const int m = S->m[set];
    if (jb * kClrBlock >= m) return;  // block-uniform
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
#pragma unroll
    for (int k = 0; k < kClrPer; k++) {
        const int j = jb * kClrBlock + k * kClrWave + lane;
        if (j < m) {
            const ClrPoint p = pts[clr_at(set, j, cap)];
            lo[0] = fminf(lo[0], p.x), hi[0] = fmaxf(hi[0], p.x);
            lo[1] = fminf(lo[1], p.y), hi[1] = fmaxf(hi[1], p.y);
            lo[2] = fminf(lo[2], p.z), hi[2] = fmaxf(hi[2], p.z);
        }
    }
    ClrBounds b;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            lo[i] = fminf(lo[i], __shfl_xor(lo[i], o, 64));
            hi[i] = fmaxf(hi[i], __shfl_xor(hi[i], o, 64));
        }
        b.lo[i] = lo[i];
        b.hi[i] = hi[i];
    }
    if (lane == 0) bounds[(size_t)set * maxblocks + jb] = b;
}

// A lower bound of every pair's s between two blocks, as bits: per axis the gap of the bounds as a
// float subtraction (not below 0), squared and summed in double in s's order.  Float subtraction,
// the exact squares and the rounded additions are monotone, so no pair's computed s is below it.
__device__ __forceinline__ unsigned long long clr_gap(const ClrBounds& a, const ClrBounds& b) {
#pragma clang fp contract(off)
    double g[3];
#pragma unroll
    for (int i = 0; i < 3; i++) g[i] = (double)fmaxf(0.f, fmaxf(b.lo[i] - a.hi[i], a.lo[i] - b.hi[i]));
    const double s = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    return (unsigned long long)__double_as_longlong(s);
}

// The pairs, kClrGroups workgroups (one wave each) a block of A's list: its points kClrPer a lane in
// registers, the group's blocks of B (every kClrGroups-th) through LDS one after another (every lane
// reads the same point of B: a broadcast), the best (s, iq) of each of the lane's points.  The block
// of the group nearest by the bounds runs first; after it a block runs unless its lower bound is
// STRICTLY greater than the smallest s this workgroup or any other has found, so every pair that
// ties the minimum runs and the result is the brute force's whatever order the workgroups run in.
// No workgroup waits on another.
__global__ __launch_bounds__(kClrWave) void k_clr_pairs(ClrState* __restrict__ S, const ClrPoint* __restrict__ pts,
                                                        int cap, const ClrBounds* __restrict__ bounds, int maxblocks,
                                                        int prune, ClrCand* __restrict__ cand) {
#pragma clang fp contract(off)
    __shared__ ClrPoint qb[kClrBlock];
    const int ja = blockIdx.x, grp = blockIdx.y, lane = threadIdx.x;
    const int ma = S->m[0], mb = S->m[1];
    const int nb = (mb + kClrBlock - 1) / kClrBlock;
    if (ja * kClrBlock >= ma || grp >= nb) return;  // block-uniform
    const int mine_n = (nb - grp + kClrGroups - 1) / kClrGroups;  // the group's blocks: grp + t * kClrGroups
    ClrPoint a[kClrPer];
    double bs[kClrPer];
    int bq[kClrPer];
#pragma unroll
    for (int k = 0; k < kClrPer; k++) {
        const int j = ja * kClrBlock + k * kClrWave + lane;
        // a slot past the list holds NaN: every comparison with its s fails
        a[k] = j < ma ? pts[clr_at(0, j, cap)] : ClrPoint{ruler_nan(), ruler_nan(), ruler_nan(), -1};
        bs[k] = __builtin_inf();
        bq[k] = 0x7fffffff;
    }
    const ClrBounds ba = bounds[ja];
    const ClrBounds* bb = bounds + maxblocks;
    // the group's nearest block of B by the bounds (ties to the first)
    unsigned long long g0 = ~0ull;
    int first = grp;
    for (int jb = grp + lane * kClrGroups; jb < nb; jb += kClrWave * kClrGroups) {
        const unsigned long long g = clr_gap(ba, bb[jb]);
        if (g < g0) g0 = g, first = jb;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long g = clr_shfl(g0, o);
        const int f = __shfl_xor(first, o, 64);
        if (g < g0 || (g == g0 && f < first)) g0 = g, first = f;
    }
    unsigned long long mine = kClrInf;  // the smallest s of this workgroup's pairs
    for (int t = -1; t < mine_n; t++) {
        const int jb = t < 0 ? first : grp + t * kClrGroups;
        if (t >= 0 && jb == first) continue;
        if (t >= 0 && prune) {
            const unsigned long long seen = min(mine, __atomic_load_n(&S->best, __ATOMIC_RELAXED));
            if (clr_gap(ba, bb[jb]) > seen) continue;  // wave-uniform
        }
        const int nq = min(kClrBlock, mb - jb * kClrBlock);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kClrPer; k++) {
            const int j = k * kClrWave + lane;
            if (j < nq) qb[j] = pts[clr_at(1, jb * kClrBlock + j, cap)];
        }
        __syncthreads();
        for (int j = 0; j < nq; j++) {
            const ClrPoint qp = qb[j];
#pragma unroll
            for (int k = 0; k < kClrPer; k++) {
                const float v0 = qp.x - a[k].x, v1 = qp.y - a[k].y, v2 = qp.z - a[k].z;
                const double s = ((double)v0 * (double)v0 + (double)v1 * (double)v1) + (double)v2 * (double)v2;
                if (s < bs[k] || (s == bs[k] && qp.idx < bq[k])) bs[k] = s, bq[k] = qp.idx;
            }
        }
        double m = bs[0];
#pragma unroll
        for (int k = 1; k < kClrPer; k++) m = fmin(m, bs[k]);
        unsigned long long now = (unsigned long long)__double_as_longlong(m);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) now = min(now, clr_shfl(now, o));
        if (now < mine) {
            mine = now;
            if (lane == 0) atomicMin(&S->best, now);
        }
    }
    // the workgroup's best pair in the result's order
    unsigned long long s = ~0ull;
    int ip = 0x7fffffff, iq = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < kClrPer; k++) {
        const unsigned long long sk = (unsigned long long)__double_as_longlong(bs[k]);
        if (a[k].idx >= 0 && bq[k] != 0x7fffffff && clr_before(sk, a[k].idx, bq[k], s, ip, iq))
            s = sk, ip = a[k].idx, iq = bq[k];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long s2 = clr_shfl(s, o);
        const int ip2 = __shfl_xor(ip, o, 64), iq2 = __shfl_xor(iq, o, 64);
        if (clr_before(s2, ip2, iq2, s, ip, iq)) s = s2, ip = ip2, iq = iq2;
    }
    if (lane == 0) cand[(size_t)ja * kClrGroups + grp] = ClrCand{s, ip == 0x7fffffff ? -1 : ip, iq};
}

// The record, one workgroup: the smallest of the workgroups' pairs in the result's order, its two
// points again from their medians, the distance and its two parts.
__global__ __launch_bounds__(kRegionThreads) void k_clr_finish(RegionDims dims, Q16 Q,
                                                               const sdr_plane* __restrict__ planes, int NP,
                                                               const sdr_clearance_query* __restrict__ query,
                                                               const ClrState* __restrict__ S,
                                                               const float* __restrict__ dmed,
                                                               const ClrCand* __restrict__ cand,
                                                               struct sdr_clearance* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ ClrCand red[kRegionWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const sdr_clearance_query q = *query;
    RegionPlane pl;
    uint32_t flags = query_refusal(dims, planes, NP, q, &pl);
    const int ma = flags ? 0 : S->m[0], mb = flags ? 0 : S->m[1];
    if (!flags) flags = (ma == 0 || mb == 0) ? SDR_CLEARANCE_EMPTY : SDR_CLEARANCE_VALID;
    unsigned long long s = ~0ull;
    int ip = 0x7fffffff, iq = 0x7fffffff;
    if (flags == SDR_CLEARANCE_VALID) {  // block-uniform
        const int na = (ma + kClrBlock - 1) / kClrBlock, nb = (mb + kClrBlock - 1) / kClrBlock;
        for (int j = tid; j < na * kClrGroups; j += kRegionThreads) {
            if (j % kClrGroups >= nb) continue;  // a group without a block of B wrote nothing
            const ClrCand c = cand[j];
            if (c.ip >= 0 && clr_before(c.s, c.ip, c.iq, s, ip, iq)) s = c.s, ip = c.ip, iq = c.iq;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long s2 = clr_shfl(s, o);
            const int ip2 = __shfl_xor(ip, o, 64), iq2 = __shfl_xor(iq, o, 64);
            if (clr_before(s2, ip2, iq2, s, ip, iq)) s = s2, ip = ip2, iq = iq2;
        }
        if (lane == 0) red[wave] = ClrCand{s, ip, iq};
        __syncthreads();
        if (tid == 0)
            for (int w = 1; w < kRegionWaves; w++)
                if (clr_before(red[w].s, red[w].ip, red[w].iq, s, ip, iq)) s = red[w].s, ip = red[w].ip, iq = red[w].iq;
    }
    if (tid != 0) return;
    struct sdr_clearance r;
    r.distance = r.along = r.across = __builtin_nan("");
    for (int i = 0; i < 3; i++) r.p_a[i] = r.p_b[i] = ruler_nan();
    r.d_a = r.d_b = ruler_nan();
    r.xa = r.ya = r.xb = r.yb = -1;
    r.area = r.n_a = r.n_b = r.m_a = r.m_b = 0;
    if (flags != SDR_CLEARANCE_OUT_OF_RANGE) {
        const PlaneRect R = plane_rect(region_segment(q));
        r.area = R.rw * R.rh;
        if (flags != SDR_CLEARANCE_NO_PLANE) {
            r.n_a = S->n[0], r.n_b = S->n[1];
            r.m_a = ma, r.m_b = mb;
        }
        if (flags == SDR_CLEARANCE_VALID) {  // every workgroup ran its group's nearest block: a pair exists
            r.ya = R.ys + ip / R.rw, r.xa = R.xs + ip % R.rw;
            r.yb = R.ys + iq / R.rw, r.xb = R.xs + iq % R.rw;
            r.d_a = dmed[ip], r.d_b = dmed[iq];
            reproject_px(Q, r.xa, r.ya, (double)r.d_a, 0.0, 0, r.p_a);
            reproject_px(Q, r.xb, r.yb, (double)r.d_b, 0.0, 0, r.p_b);
            const float v0 = r.p_b[0] - r.p_a[0], v1 = r.p_b[1] - r.p_a[1], v2 = r.p_b[2] - r.p_a[2];
            const double sd = ((double)v0 * (double)v0 + (double)v1 * (double)v1) + (double)v2 * (double)v2;
            const double al = (pl.n[0] * (double)v0 + pl.n[1] * (double)v1) + pl.n[2] * (double)v2;
            const double t = sd - al * al;
            r.distance = canon(sqrt(sd));
            r.along = canon(al);
            r.across = canon(sqrt(t > 0.0 ? t : 0.0));
        }
    }
    r.frame = q.frame;
    r.plane = q.plane;
    r.label_a = q.label_a;
    r.label_b = q.label_b;
    r.flags = flags;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = 0;
    *out = r;
}

}  // namespace sdr

namespace {

using namespace sdr::ruler_host;

// SDR_DEBUG_CLEARANCE_PRUNE: 0 makes every block pair run
std::atomic<int> g_prune{1};

int check_clearance_params(const sdr_clearance_params* p, const void* planes, int P) {
    if (int rc = check_planes_arg(planes, P)) return rc;
    if (std::isnan(p->h_lo) || std::isnan(p->h_hi) || p->h_lo > p->h_hi)
        return rfail(SDR_ERR_ARG, "h_lo and h_hi must not be NaN, and h_lo <= h_hi");
    if (p->radius < 0 || p->radius > 4) return rfail(SDR_ERR_ARG, "radius must be in 0..4");
    if (p->min_count < 1) return rfail(SDR_ERR_ARG, "min_count must be >= 1");
    for (int i = 0; i < 10; i++)
        if (p->reserved[i]) return rfail(SDR_ERR_ARG, "reserved fields must be 0");
    return SDR_OK;
}

// what the two entries refuse beyond the maps and the parameters
int check_clearance_call(const void* labels, int K) {
    if (!labels) return rfail(SDR_ERR_ARG, "the clearance needs a label map");
    if (K > SDR_CLEARANCE_MAX_QUERIES) return rfail(SDR_ERR_ARG, "at most SDR_CLEARANCE_MAX_QUERIES queries a call");
    return SDR_OK;
}

}  // namespace

extern "C" {

void sdr_clearance_params_default(sdr_clearance_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->min_disp = -1.0f;
    p->conf_min = 0.0f;
    p->h_lo = -1048576.0f;
    p->h_hi = 1048576.0f;
    p->radius = 0;
    p->min_count = 1;
}

int sdr_clearance_debug_knob(int knob, int value) {
    if (knob != SDR_DEBUG_CLEARANCE_PRUNE) return rfail(SDR_ERR_ARG, "unknown clearance debug knob");
    g_prune.store(value != 0, std::memory_order_relaxed);
    return SDR_OK;
}

int sdr_clearance_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride, int W, int H, int F,
                         const float* d_conf, const uint8_t* d_labels, const double Q[16],
                         const sdr_clearance_params* params, const sdr_plane* d_planes, int P,
                         const sdr_clearance_query* d_queries, int K, struct sdr_clearance* d_out, void* stream) {
    int rc = check_plane_maps(d_disp, disp_type, stride, frame_stride, W, H, F, Q, params, d_queries, K, d_out);
    if (rc || (rc = check_clearance_params(params, d_planes, P)) || (rc = check_clearance_call(d_labels, K))) return rc;
    if (K == 0) return SDR_OK;
    hipStream_t st = (hipStream_t)stream;
    const sdr::Q16 q = make_q16(Q);
    const sdr_clearance_params CP = *params;
    const int prune = g_prune.load(std::memory_order_relaxed);
    // scratch of one query, which every query uses in turn: {state, marks, medians, the two lists in
    // one array, the blocks' bounds of A and of B, the workgroups' candidates}
    const int cap = W * H, maxblocks = cap / sdr::kClrBlock + 1;
    sdr::ScratchLayout lay;
    const auto s_state = lay.take<sdr::ClrState>(1);
    const auto s_mark = lay.take<uint8_t>((size_t)cap);
    const auto s_dmed = lay.take<float>((size_t)cap);
    const auto s_pts = lay.take<sdr::ClrPoint>((size_t)cap);
    const auto s_bounds = lay.take<sdr::ClrBounds>((size_t)2 * maxblocks);
    const auto s_cand = lay.take<sdr::ClrCand>((size_t)maxblocks * sdr::kClrGroups);
    sdr::Scratch sc(st);
    if ((rc = sc.open(lay))) return rc;
    sdr::ClrState* state = sc.at(s_state);
    uint8_t* mark = sc.at(s_mark);
    float* dmed = sc.at(s_dmed);
    sdr::ClrPoint* pts = sc.at(s_pts);
    sdr::ClrBounds* bounds = sc.at(s_bounds);
    sdr::ClrCand* cand = sc.at(s_cand);
    const unsigned slices = sdr::region_slices(W, H);
    const dim3 block(sdr::kRegionThreads), wave(sdr::kClrWave);
    hipError_t e = hipSuccess;
    auto one = [&](auto maps, int k) {
        using T = disp_elem_t<decltype(maps)>;
        const sdr_clearance_query* qk = d_queries + k;
        // the state's first 16 bytes are the counts (0), the next 8 the bits of +inf
        if ((e = hipMemsetAsync(state, 0, sizeof(sdr::ClrState), st)) != hipSuccess) return;
        if ((e = hipMemsetD32Async((hipDeviceptr_t)((char*)state + 20), 0x7ff00000, 1, st)) != hipSuccess) return;
        hipLaunchKernelGGL((sdr::k_clr_mark<T>), dim3(slices), block, 0, st, maps, q, CP, d_planes, P, qk, state, mark);
        hipLaunchKernelGGL((sdr::k_clr_sample<T>), dim3(slices), block, 0, st, maps, q, CP, d_planes, P, qk, state,
                           (const uint8_t*)mark, dmed, pts, cap);
        hipLaunchKernelGGL(sdr::k_clr_bounds, dim3((unsigned)maxblocks, 2), wave, 0, st, (const sdr::ClrState*)state,
                           (const sdr::ClrPoint*)pts, cap, bounds, maxblocks);
        hipLaunchKernelGGL(sdr::k_clr_pairs, dim3((unsigned)maxblocks, sdr::kClrGroups), wave, 0, st, state, (const sdr::ClrPoint*)pts,
                           cap, (const sdr::ClrBounds*)bounds, maxblocks, prune, cand);
        hipLaunchKernelGGL(sdr::k_clr_finish, dim3(1), block, 0, st, maps.dims(), q, d_planes, P, qk,
                           (const sdr::ClrState*)state, (const float*)dmed, (const sdr::ClrCand*)cand, d_out + k);
    };
    for (int k = 0; k < K && e == hipSuccess; k++)
        with_maps(d_disp, disp_type, stride, frame_stride, W, H, F, d_conf, d_labels, [&](auto maps) { one(maps, k); });
    return sc.finish(e);
}

int sdr_clearance(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H, int F,
                  const float* conf, const uint8_t* labels, const double Q[16], const sdr_clearance_params* params,
                  const sdr_plane* planes, int P, const sdr_clearance_query* queries, int K,
                  struct sdr_clearance* out) {
    auto check = [&](const sdr_clearance_params* p, const void* pl, int np) {
        const int rc = check_clearance_params(p, pl, np);
        return rc ? rc : check_clearance_call(labels, K);
    };
    return region_host_call(check, sdr_clearance_device, disp, disp_type, stride, frame_stride, W, H, F, conf, labels, Q,
                            params, planes, P, queries, K, out);
}

}  // extern "C"
