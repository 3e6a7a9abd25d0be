// sdr_footprint.hip -- the footprint of a region: the pixels of a rectangle binned on a grid of
// square cells in a fitted plane, the cells that stray pixels occupy alone dropped by a 3 x 3
// support rule, and the minimum-area bounding rectangle of the kept cells over 90 whole-degree
// directions.  The definition is in include/sdr/sdr.h ("the footprint of a region").
#include <limits.h>
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

// c_k = lrint(16384 * cos(k deg)), s_k = lrint(16384 * sin(k deg)), k = 0..89
#define SDR_FOOT_DIRS                                                                          \
    {16384, 0}, {16382, 286}, {16374, 572}, {16362, 857}, {16344, 1143},                       \
    {16322, 1428}, {16294, 1713}, {16262, 1997}, {16225, 2280}, {16182, 2563},                 \
    {16135, 2845}, {16083, 3126}, {16026, 3406}, {15964, 3686}, {15897, 3964},                 \
    {15826, 4240}, {15749, 4516}, {15668, 4790}, {15582, 5063}, {15491, 5334},                 \
    {15396, 5604}, {15296, 5872}, {15191, 6138}, {15082, 6402}, {14968, 6664},                 \
    {14849, 6924}, {14726, 7182}, {14598, 7438}, {14466, 7692}, {14330, 7943},                 \
    {14189, 8192}, {14044, 8438}, {13894, 8682}, {13741, 8923}, {13583, 9162},                 \
    {13421, 9397}, {13255, 9630}, {13085, 9860}, {12911, 10087}, {12733, 10311},               \
    {12551, 10531}, {12365, 10749}, {12176, 10963}, {11982, 11174}, {11786, 11381},            \
    {11585, 11585}, {11381, 11786}, {11174, 11982}, {10963, 12176}, {10749, 12365},            \
    {10531, 12551}, {10311, 12733}, {10087, 12911}, {9860, 13085}, {9630, 13255},              \
    {9397, 13421}, {9162, 13583}, {8923, 13741}, {8682, 13894}, {8438, 14044},                 \
    {8192, 14189}, {7943, 14330}, {7692, 14466}, {7438, 14598}, {7182, 14726},                 \
    {6924, 14849}, {6664, 14968}, {6402, 15082}, {6138, 15191}, {5872, 15296},                 \
    {5604, 15396}, {5334, 15491}, {5063, 15582}, {4790, 15668}, {4516, 15749},                 \
    {4240, 15826}, {3964, 15897}, {3686, 15964}, {3406, 16026}, {3126, 16083},                 \
    {2845, 16135}, {2563, 16182}, {2280, 16225}, {1997, 16262}, {1713, 16294},                 \
    {1428, 16322}, {1143, 16344}, {857, 16362}, {572, 16374}, {286, 16382}

namespace sdr {

static_assert(sizeof(sdr_footprint_params) == 64, "sdr_footprint_params is 64 bytes");
static_assert(sizeof(sdr_footprint) == 256, "sdr_footprint is 256 bytes");

constexpr int kFootDirs = 90;
constexpr int kFootTile = 16;               // the cell pass: a workgroup a tile of 16 x 16 cells
constexpr int kFootHalo = kFootTile + 4;    // counts two cells around it
constexpr int kFootKept = kFootTile + 2;    // kept flags one cell around it
constexpr int kFootFinish = 128;            // threads of the last launch (>= kFootDirs)
static_assert(kFootTile * kFootTile == kRegionThreads, "a thread a cell of the tile");

__constant__ int c_foot_dirs[kFootDirs][2] = {SDR_FOOT_DIRS};

struct FootBasis {
    double es[3], et[3];
    RegionPlane pl;
};

// A query's state: the setup launch writes all of it.
struct FootState {
    FootBasis b;
    unsigned flags;   // 0, or the flag that refuses the query
    unsigned cnt[3];  // n_masked, n_valid, n
    int smin, smax, tmin, tmax;
    unsigned n_outside, n_raw, n_kept, pad;
    int ext[kFootDirs][4];  // over the kept cells: min p, max p, min r, max r
};
static_assert(sizeof(FootState) == 128 + kFootDirs * 16, "FootState's layout");

// Setup, a workgroup a query: the checks, the basis, the accumulators at their start values.
__global__ __launch_bounds__(kFootFinish) void k_foot_setup(RegionDims dims, const sdr_plane* __restrict__ planes, int NP,
                                                            const sdr_relief_query* __restrict__ queries,
                                                            FootState* __restrict__ states) {
#pragma clang fp contract(off)
    const int k = blockIdx.x, tid = threadIdx.x;
    FootState* S = states + k;
    if (tid < kFootDirs) {
        S->ext[tid][0] = INT_MAX;
        S->ext[tid][1] = INT_MIN;
        S->ext[tid][2] = INT_MAX;
        S->ext[tid][3] = INT_MIN;
    }
    if (tid != 0) return;
    const sdr_relief_query q = queries[k];
    double es[3] = {0, 0, 0}, et[3] = {0, 0, 0};
    RegionPlane pl = {{0, 0, 0}, 0};
    unsigned flags = query_refusal(dims, planes, NP, q, &pl);
    if (!flags) {
        const double* n = pl.n;
        double a, b, c;
        if (fabs(n[0]) <= fabs(n[1])) {
            a = 1.0 - n[0] * n[0];
            b = -(n[0] * n[1]);
            c = -(n[0] * n[2]);
        } else {
            a = -(n[0] * n[1]);
            b = 1.0 - n[1] * n[1];
            c = -(n[1] * n[2]);
        }
        const double len = sqrt((a * a + b * b) + c * c);
        es[0] = a / len;
        es[1] = b / len;
        es[2] = c / len;
        et[0] = n[1] * es[2] - n[2] * es[1];
        et[1] = n[2] * es[0] - n[0] * es[2];
        et[2] = n[0] * es[1] - n[1] * es[0];
        for (int i = 0; i < 3; i++)
            if (!isfinite(es[i]) || !isfinite(et[i])) flags = SDR_FOOTPRINT_NO_PLANE;
    }
    for (int i = 0; i < 3; i++) {
        S->b.es[i] = es[i];
        S->b.et[i] = et[i];
        S->cnt[i] = 0;
    }
    S->b.pl = pl;
    S->flags = flags;
    S->smin = S->tmin = INT_MAX;
    S->smax = S->tmax = INT_MIN;
    S->n_outside = S->n_raw = S->n_kept = S->pad = 0;
}

struct FootPix {
    bool masked, valid, member;
    int si, ti;
};

// Pixel (u, v) of the slice's region: the region rule's member, the band of heights, the cell.
// Both sweeps repeat it: the same bits in each.
template <typename T>
__device__ __forceinline__ FootPix foot_pixel(const RegionSlice<T>& sl, const Q16& Q, const FootBasis& B,
                                              const sdr_footprint_params& P, int label, unsigned u, unsigned v) {
#pragma clang fp contract(off)
    const RegionPix px = region_pixel(sl, Q, B.pl, P.min_disp, P.conf_min, label, u, v);
    FootPix r = {px.masked, px.valid, false, 0, 0};
    if (!px.member) return r;
    if (!(P.h_lo <= px.hf && px.hf <= P.h_hi)) return r;
    const double X = (double)px.xyz[0], Y = (double)px.xyz[1], Z = (double)px.xyz[2];
    const double s = (B.es[0] * X + B.es[1] * Y) + B.es[2] * Z;
    const double t = (B.et[0] * X + B.et[1] * Y) + B.et[2] * Z;
    const double qs = s / (double)P.cell, qt = t / (double)P.cell;
    if (!(fabs(qs) < 1073741824.0 && fabs(qt) < 1073741824.0)) return r;
    r.si = (int)floor(qs);  // in [-2^30, 2^30)
    r.ti = (int)floor(qt);
    r.member = true;
    return r;
}

// One sweep over the queries' pixels: grid (slices of a W x H frame, queries).  Pass 1 counts the
// masked, valid and member pixels and takes the extremes of the members' cells; pass 2 recomputes
// the members and adds each to its cell of the query's G x G grid (cleared before), or to n_outside.
// A refused query and a slice past the area leave at once (block-uniform).
template <typename T, int PASS>
__global__ __launch_bounds__(kRegionThreads) void k_foot_sweep(
    RegionMaps<T> maps, Q16 Q, sdr_footprint_params P, const sdr_relief_query* __restrict__ queries,
    FootState* __restrict__ states, unsigned* __restrict__ grids) {
    __shared__ int red[kRegionWaves][8];
    const int k = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    FootState* S = states + k;
    if (S->flags) return;                    // block-uniform
    if (PASS == 2 && S->cnt[2] == 0) return;  // no member
    const sdr_relief_query q = queries[k];
    RegionSlice<T> sl;
    if (!region_cut(query_view(maps, q), &sl)) return;  // in range: S->flags
    const FootBasis B = S->b;
    const int si0 = PASS == 2 ? S->smin : 0, ti0 = PASS == 2 ? S->tmin : 0;  // pass 1 is complete
    const unsigned G = (unsigned)P.grid;
    unsigned* g = grids + (size_t)k * G * G;

    int m[3] = {0, 0, 0};
    int smin = INT_MAX, smax = INT_MIN, tmin = INT_MAX, tmax = INT_MIN;
    int outside = 0;
    sl.each([&](unsigned u, unsigned v) __attribute__((always_inline)) {
        const FootPix px = foot_pixel(sl, Q, B, P, q.label, u, v);
        if (PASS == 1) {
            m[0] += px.masked ? 1 : 0;
            m[1] += px.valid ? 1 : 0;
            if (!px.member) return;
            m[2] += 1;
            smin = min(smin, px.si);
            smax = max(smax, px.si);
            tmin = min(tmin, px.ti);
            tmax = max(tmax, px.ti);
        } else {
            if (!px.member) return;
            // both differences are in [0, 2^31): unsigned, and a value below G indexes the grid
            const unsigned di = (unsigned)px.si - (unsigned)si0, dj = (unsigned)px.ti - (unsigned)ti0;
            if (di < G && dj < G)
                atomicAdd(g + (size_t)di * G + dj, 1u);
            else
                outside += 1;
        }
    });
    if constexpr (PASS == 1) {
        int w[7];
        w[0] = (int)wave_sum((long long)m[0]);
        w[1] = (int)wave_sum((long long)m[1]);
        w[2] = (int)wave_sum((long long)m[2]);
        w[3] = wave_min(smin);
        w[4] = wave_max(smax);
        w[5] = wave_min(tmin);
        w[6] = wave_max(tmax);
        if (lane == 0)
            for (int i = 0; i < 7; i++) red[wave][i] = w[i];
        __syncthreads();
        if (tid < 7) {
            int a = red[0][tid];
            for (int x = 1; x < kRegionWaves; x++) {
                const int b = red[x][tid];
                a = tid < 3 ? a + b : ((tid == 3 || tid == 5) ? min(a, b) : max(a, b));
            }
            if (tid < 3) {
                if (a) atomicAdd(&S->cnt[tid], (unsigned)a);
            } else if (tid == 3) {
                if (a != INT_MAX) atomicMin(&S->smin, a);
            } else if (tid == 4) {
                if (a != INT_MIN) atomicMax(&S->smax, a);
            } else if (tid == 5) {
                if (a != INT_MAX) atomicMin(&S->tmin, a);
            } else {
                if (a != INT_MIN) atomicMax(&S->tmax, a);
            }
        }
    } else {
        const int o = (int)wave_sum((long long)outside);
        if (lane == 0) red[wave][0] = o;
        __syncthreads();
        if (tid == 0) {
            int a = 0;
            for (int x = 0; x < kRegionWaves; x++) a += red[x][0];
            if (a) atomicAdd(&S->n_outside, (unsigned)a);
        }
    }
}

// The pass over the cells: grid (tiles of 16 x 16 cells along j, along i, queries).  The counts of
// the tile and two cells around it go to LDS, the kept flags of the tile and one cell around it
// follow from them, and the tile's kept cells that have a neighbour (of the four) that is not kept
// are compacted into a list: c_k > 0 for every k, so for a kept cell whose four neighbours are
// kept each of the four extremes is reached by a neighbour too, and skipping it is exact.  Lane k
// of the first 90 threads then walks the list (broadcast LDS reads) with its direction and adds
// its four extremes to the query's with one atomic each.
__global__ __launch_bounds__(kRegionThreads) void k_foot_cells(sdr_footprint_params P,
                                                             FootState* __restrict__ states,
                                                             const unsigned* __restrict__ grids) {
    __shared__ unsigned cnt[kFootHalo][kFootHalo + 1];
    __shared__ unsigned char kept[kFootKept][kFootKept + 2];
    __shared__ unsigned list[kRegionThreads];
    __shared__ unsigned tot[3];  // raw, kept, listed
    const int k = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    FootState* S = states + k;
    if (S->flags || S->cnt[2] == 0) return;  // block-uniform
    const int G = P.grid;
    const int i0 = (int)blockIdx.y * kFootTile, j0 = (int)blockIdx.x * kFootTile;
    // the members' cells end at the spans (each at least 1, in int64: up to 2^31)
    const long long span_s = (long long)S->smax - (long long)S->smin + 1;
    const long long span_t = (long long)S->tmax - (long long)S->tmin + 1;
    if (i0 >= span_s || j0 >= span_t) return;  // an empty tile keeps no cell (block-uniform)
    const unsigned* g = grids + (size_t)k * (size_t)G * (size_t)G;
    if (tid < 3) tot[tid] = 0;
    for (int x = tid; x < kFootHalo * kFootHalo; x += kRegionThreads) {
        const int li = x / kFootHalo, lj = x - li * kFootHalo;
        const int gi = i0 + li - 2, gj = j0 + lj - 2;
        cnt[li][lj] = (gi >= 0 && gi < G && gj >= 0 && gj < G) ? g[(size_t)gi * G + gj] : 0u;
    }
    __syncthreads();
    for (int x = tid; x < kFootKept * kFootKept; x += kRegionThreads) {
        const int li = x / kFootKept, lj = x - li * kFootKept;  // cnt's (li + 1, lj + 1)
        unsigned sum = 0;  // at most 2^24 members a query
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) sum += cnt[li + a][lj + b];
        kept[li][lj] = (cnt[li + 1][lj + 1] >= 1u && sum >= (unsigned)P.support) ? 1 : 0;
    }
    __syncthreads();
    const int li = tid >> 4, lj = tid & 15;
    const bool raw = cnt[li + 2][lj + 2] >= 1u;  // a cell outside the grid holds 0
    const bool kp = kept[li + 1][lj + 1] != 0;
    const bool edge = kp && !(kept[li][lj + 1] && kept[li + 2][lj + 1] && kept[li + 1][lj] && kept[li + 1][lj + 2]);
    const unsigned long long braw = __ballot(raw), bkept = __ballot(kp), bedge = __ballot(edge);
    unsigned at = 0;
    if (lane == 0) {
        if (braw) atomicAdd(&tot[0], (unsigned)__popcll(braw));
        if (bkept) atomicAdd(&tot[1], (unsigned)__popcll(bkept));
        if (bedge) at = atomicAdd(&tot[2], (unsigned)__popcll(bedge));
    }
    at = (unsigned)__shfl((int)at, 0, 64);
    if (edge)  // at most kRegionThreads entries: one a thread
        list[at + (unsigned)__popcll(bedge & ((1ull << lane) - 1ull))] = ((unsigned)(i0 + li) << 16) | (unsigned)(j0 + lj);
    __syncthreads();
    if (tid == 0) {
        if (tot[0]) atomicAdd(&S->n_raw, tot[0]);
        if (tot[1]) atomicAdd(&S->n_kept, tot[1]);
    }
    const int nl = (int)tot[2];
    if (tid >= kFootDirs || nl == 0) return;
    const int c = c_foot_dirs[tid][0], s = c_foot_dirs[tid][1];
    int pmin = INT_MAX, pmax = INT_MIN, rmin = INT_MAX, rmax = INT_MIN;
    for (int x = 0; x < nl; x++) {
        const unsigned e = list[x];
        const int i = (int)(e >> 16), j = (int)(e & 0xffffu);
        const int p = c * i + s * j, r = c * j - s * i;  // below 2^25
        pmin = min(pmin, p);
        pmax = max(pmax, p);
        rmin = min(rmin, r);
        rmax = max(rmax, r);
    }
    atomicMin(&S->ext[tid][0], pmin);
    atomicMax(&S->ext[tid][1], pmax);
    atomicMin(&S->ext[tid][2], rmin);
    atomicMax(&S->ext[tid][3], rmax);
}

__device__ __forceinline__ int foot_sat(long long v) {
    return v > (long long)INT_MAX ? INT_MAX : (int)v;
}

// The record, a workgroup a query: the area of each direction's rectangle, the smallest one, the
// sides, the fill and the corners.
__global__ __launch_bounds__(kFootFinish) void k_foot_finish(sdr_footprint_params P,
                                                             const sdr_relief_query* __restrict__ queries,
                                                             const FootState* __restrict__ states,
                                                             sdr_footprint* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ long long areas[kFootDirs];
    const int k = blockIdx.x, tid = threadIdx.x;
    const FootState* S = states + k;
    const bool ran = S->flags == 0;
    const bool valid = ran && S->n_kept > 0;  // block-uniform
    if (valid && tid < kFootDirs) {
        const int c = c_foot_dirs[tid][0], s = c_foot_dirs[tid][1];
        const int U0 = S->ext[tid][0], U1 = S->ext[tid][1] + c + s;
        const int V0 = S->ext[tid][2] - s, V1 = S->ext[tid][3] + c;
        areas[tid] = (long long)(U1 - U0) * (long long)(V1 - V0);
    }
    __syncthreads();
    if (tid != 0) return;
    const sdr_relief_query q = queries[k];
    sdr_footprint r;
    const double nan = __builtin_nan("");
    r.side[0] = r.side[1] = r.fill = nan;
    for (int i = 0; i < 3; i++) {
        for (int x = 0; x < 4; x++) r.corner[x][i] = nan;
        r.basis_s[i] = r.basis_t[i] = nan;
    }
    r.i0 = r.j0 = 0;
    r.angle_deg = -1;
    r.span_s = r.span_t = 0;
    r.area = r.n_masked = r.n_valid = r.n = r.n_outside = r.n_cells_raw = r.n_cells = 0;
    r.frame = q.frame;
    r.plane = q.plane;
    r.label = q.label;
    r.flags = S->flags;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = 0;
    if (S->flags != SDR_FOOTPRINT_OUT_OF_RANGE) {
        const PlaneRect R = plane_rect(region_segment(q));
        r.area = R.rw * R.rh;
    }
    if (ran) {
        r.n_masked = (int)S->cnt[0];
        r.n_valid = (int)S->cnt[1];
        r.n = (int)S->cnt[2];
        r.n_outside = (int)S->n_outside;
        r.n_cells_raw = (int)S->n_raw;
        r.n_cells = (int)S->n_kept;
        if (r.n > 0) {
            r.i0 = S->smin;
            r.j0 = S->tmin;
            r.span_s = foot_sat((long long)S->smax - (long long)S->smin + 1);
            r.span_t = foot_sat((long long)S->tmax - (long long)S->tmin + 1);
        }
        r.flags = (valid ? SDR_FOOTPRINT_VALID : SDR_FOOTPRINT_EMPTY) | (r.n_outside > 0 ? SDR_FOOTPRINT_CLIPPED : 0);
    }
    if (valid) {
        int best = 0;
        for (int d = 1; d < kFootDirs; d++)
            if (areas[d] < areas[best]) best = d;
        const int c = c_foot_dirs[best][0], s = c_foot_dirs[best][1];
        const int U[2] = {S->ext[best][0], S->ext[best][1] + c + s};
        const int V[2] = {S->ext[best][2] - s, S->ext[best][3] + c};
        const double cell = (double)P.cell;
        const double du = (double)(U[1] - U[0]) / 16384.0, dv = (double)(V[1] - V[0]) / 16384.0;
        r.angle_deg = best;
        r.side[0] = canon(du * cell);
        r.side[1] = canon(dv * cell);
        r.fill = canon((double)r.n_cells / (du * dv));
        const double ch = (double)c / 16384.0, sh = (double)s / 16384.0;
        const int cu[4] = {0, 1, 1, 0}, cv[4] = {0, 0, 1, 1};
        for (int x = 0; x < 4; x++) {
            const double a = (double)U[cu[x]] / 16384.0, b = (double)V[cv[x]] / 16384.0;
            const double gi = ch * a - sh * b, gj = sh * a + ch * b;
            const double Sx = ((double)S->smin + gi) * cell, Tx = ((double)S->tmin + gj) * cell;
            for (int i = 0; i < 3; i++) r.corner[x][i] = canon((Sx * S->b.es[i] + Tx * S->b.et[i]) - S->b.pl.off * S->b.pl.n[i]);
        }
        for (int i = 0; i < 3; i++) {
            r.basis_s[i] = S->b.es[i];
            r.basis_t[i] = S->b.et[i];
        }
    }
    out[k] = r;
}

}  // namespace sdr

namespace {

using namespace sdr::ruler_host;

const int32_t kFootDirsHost[sdr::kFootDirs][2] = {SDR_FOOT_DIRS};

constexpr int kFootBatch = 256;                          // queries a batch at most
constexpr size_t kFootGridBytes = (size_t)64 << 20;      // and their grids take at most this

int check_footprint_params(const sdr_footprint_params* p, const void* planes, int P) {
    if (int rc = check_planes_arg(planes, P)) return rc;
    if (!(std::isfinite(p->cell) && p->cell >= 0.0625f && p->cell <= 65536.0f))
        return rfail(SDR_ERR_ARG, "cell must be finite and in 0.0625..65536");
    if (p->grid < 16 || p->grid > 1024) return rfail(SDR_ERR_ARG, "grid must be in 16..1024");
    if (p->support < 1 || p->support > 255) return rfail(SDR_ERR_ARG, "support must be in 1..255");
    if (std::isnan(p->h_lo) || std::isnan(p->h_hi) || p->h_lo > p->h_hi)
        return rfail(SDR_ERR_ARG, "h_lo and h_hi must not be NaN, and h_lo <= h_hi");
    for (int i = 0; i < 9; i++)
        if (p->reserved[i]) return rfail(SDR_ERR_ARG, "reserved fields must be 0");
    return SDR_OK;
}

}  // namespace

extern "C" {

void sdr_footprint_params_default(sdr_footprint_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->min_disp = -1.0f;
    p->conf_min = 0.0f;
    p->cell = 4.0f;
    p->h_lo = -1048576.0f;
    p->h_hi = 1048576.0f;
    p->grid = 512;
    p->support = 4;
}

int sdr_footprint_direction(int k, int32_t* c, int32_t* s) {
    if (k < 0 || k >= sdr::kFootDirs || !c || !s) return rfail(SDR_ERR_ARG, "direction must be in 0..89");
    *c = kFootDirsHost[k][0];
    *s = kFootDirsHost[k][1];
    return SDR_OK;
}

int sdr_plane_footprint_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride, int W, int H,
                               int F, const float* d_conf, const uint8_t* d_labels, const double Q[16],
                               const sdr_footprint_params* params, const sdr_plane* d_planes, int P,
                               const sdr_relief_query* d_queries, int K, sdr_footprint* d_out, void* stream) {
    int rc = check_plane_maps(d_disp, disp_type, stride, frame_stride, W, H, F, Q, params, d_queries, K, d_out);
    if (rc || (rc = check_footprint_params(params, d_planes, P))) return rc;
    if (K == 0) return SDR_OK;
    hipStream_t st = (hipStream_t)stream;
    const sdr::Q16 q = make_q16(Q);
    const sdr_footprint_params FP = *params;
    const size_t G = (size_t)FP.grid, gbytes = G * G * sizeof(unsigned);  // 1 KiB .. 4 MiB a query
    const int KB = std::min(K, std::min(kFootBatch, (int)(kFootGridBytes / gbytes)));  // >= 1
    // scratch of a batch: {grids, states}
    sdr::ScratchLayout lay;
    const auto s_grids = lay.take<unsigned>((size_t)KB * G * G);
    const auto s_states = lay.take<sdr::FootState>((size_t)KB);
    sdr::Scratch sc(st);
    if ((rc = sc.open(lay))) return rc;
    unsigned* grids = sc.at(s_grids);
    sdr::FootState* states = sc.at(s_states);
    const unsigned slices = sdr::region_slices(W, H);
    const unsigned tiles = (unsigned)((G + sdr::kFootTile - 1) / sdr::kFootTile);
    const dim3 block(sdr::kRegionThreads), small(sdr::kFootFinish);
    hipError_t e = hipSuccess;
    auto batch = [&](auto maps, int k0, int kb) {
        using T = disp_elem_t<decltype(maps)>;
        const sdr_relief_query* qs = d_queries + k0;
        const dim3 sgrid(slices, (unsigned)kb), cgrid(tiles, tiles, (unsigned)kb), pgrid((unsigned)kb);
        if ((e = hipMemsetAsync(grids, 0, (size_t)kb * gbytes, st)) != hipSuccess) return;
        hipLaunchKernelGGL(sdr::k_foot_setup, pgrid, small, 0, st, maps.dims(), d_planes, P, qs, states);
        hipLaunchKernelGGL((sdr::k_foot_sweep<T, 1>), sgrid, block, 0, st, maps, q, FP, qs, states, grids);
        hipLaunchKernelGGL((sdr::k_foot_sweep<T, 2>), sgrid, block, 0, st, maps, q, FP, qs, states, grids);
        hipLaunchKernelGGL(sdr::k_foot_cells, cgrid, block, 0, st, FP, states, (const unsigned*)grids);
        hipLaunchKernelGGL(sdr::k_foot_finish, pgrid, small, 0, st, FP, qs, (const sdr::FootState*)states,
                           d_out + k0);
    };
    for (int k0 = 0; k0 < K && e == hipSuccess; k0 += KB)
        with_maps(d_disp, disp_type, stride, frame_stride, W, H, F, d_conf, d_labels,
                  [&](auto maps) { batch(maps, k0, std::min(K - k0, KB)); });
    return sc.finish(e);
}

int sdr_plane_footprint(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H, int F,
                        const float* conf, const uint8_t* labels, const double Q[16],
                        const sdr_footprint_params* params, const sdr_plane* planes, int P,
                        const sdr_relief_query* queries, int K, sdr_footprint* out) {
    return region_host_call(check_footprint_params, sdr_plane_footprint_device, disp, disp_type, stride, frame_stride,
                            W, H, F, conf, labels, Q, params, planes, P, queries, K, out);
}

}  // extern "C"
