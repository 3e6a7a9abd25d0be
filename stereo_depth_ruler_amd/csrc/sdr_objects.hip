// sdr_objects.hip -- the objects of a region: the connected sets of a rectangle's pixels that stand
// in a band of heights above a fitted plane and whose disparities step by at most max_diff, the
// largest first, as records and as a label map the relief and the footprint take.  The definition
// is in include/sdr/sdr.h ("the objects of a region").
//
//   k_obj_local    32 x 32 tile of the rectangle in LDS: membership (the region rule) and disparity,
//                  horizontal runs from one ballot a row, unions across rows (and diagonals) in LDS,
//                  local sizes.  P[pixel] = tile-root pixel index (-1: no member), S[tile root] =
//                  its pixel count, 0 elsewhere; the tile's member counts for the scan record.
//   k_obj_merge    pixel pairs across tile borders (and the diagonal pairs across them) unite the
//                  tile roots: the lock-free min-root union-find of sdr_unionfind.hpp.
//   k_obj_sizes    each tile root finds its global root, adds its count there, points at it.
//   k_obj_select   a slice of the rectangle a workgroup: the slice's components and kept ones
//                  counted, its max_objects largest keys (n << 24 | 0xFFFFFF - root) listed.
//   k_obj_rank     one workgroup: the tiles' and slices' counts summed (plain stores and one
//                  reader: no atomic on a counter every workgroup shares), then the max_objects
//                  largest keys of the slices' lists, in order; a ranked root's size becomes
//                  -1 - rank.
//   k_obj_stats    P[P[pixel]] is the global root: its rank is the pixel's label; the ranked
//                  objects' sums and extremes, wave-reduced, through LDS, one atomic set a workgroup.
//   k_obj_finish   the records and the scan record.
// Indices are the rectangle's row-major v * rw + u, so a component's smallest index is its root.
// No kernel waits on another workgroup: the union-find's loops end because parents only decrease.
#include <math.h>
#include <string.h>

#include <cmath>

#include <algorithm>

#include "sdr_device.hpp"
#include "sdr_internal.hpp"
#include "sdr_region.hpp"
#include "sdr_ruler_shared.hpp"
#include "sdr_unionfind.hpp"

namespace sdr {

static_assert(sizeof(sdr_object_params) == 64, "sdr_object_params is 64 bytes");
static_assert(sizeof(sdr_object) == 64, "sdr_object is 64 bytes");
static_assert(sizeof(sdr_object_scan) == 64, "sdr_object_scan is 64 bytes");

constexpr int kObjTile = 32;         // a tile's side: a wave covers two rows
constexpr int kObjTilePix = kObjTile * kObjTile;
constexpr int kObjLocalThreads = 1024;  // a thread a pixel of the tile: 16 waves hide the region rule's doubles
constexpr int kObjMax = 64;          // max_objects at most
constexpr int kObjRankThreads = 1024;
constexpr unsigned kObjRootMask = 0xFFFFFFu;  // area <= 2^24

// A ranked object's sums, zeroed: every extreme is a maximum of a value that is never 0.
struct ObjAcc {
    long long sum_x, sum_y, sum256;
    unsigned x0i, y0i;        // max of 0x10000 - x, 0x10000 - y
    unsigned x1p, y1p;        // max of x + 1, y + 1
    unsigned kmax, kmin_inv;  // the largest ordered key of hf and the largest ~key
};
static_assert(sizeof(ObjAcc) == 48, "ObjAcc is 48 bytes");

// The call's state, zeroed before the first kernel.  The counts are k_obj_rank's sums of what the
// tiles (ObjTileCount) and the slices (ObjSliceCount) of the rectangle wrote.
struct ObjState {
    unsigned long long ranked[kObjMax];  // the ranked keys, 0 past count
    ObjAcc acc[kObjMax];
    int n_masked, n_valid, n, n_components, n_kept, largest_dropped, count, pad;
};
struct ObjTileCount {
    int n_masked, n_valid, n, pad;
};
struct ObjSliceCount {
    int n_components, n_kept, largest_dropped, pad;
};
static_assert(sizeof(ObjState) == 3616, "ObjState is 3616 bytes");

// 1024 threads = 16 waves, a thread a pixel of the tile: a wave covers two tile rows.
template <typename T>
__global__ __launch_bounds__(kObjLocalThreads) void k_obj_local(
    RegionMaps<T> maps, Q16 Q, sdr_object_params P, const sdr_plane* __restrict__ planes, int NP,
    const sdr_relief_query* __restrict__ query, ObjTileCount* __restrict__ tiles, int* __restrict__ Pa,
    int* __restrict__ Sz) {
#pragma clang fp contract(off)
    __shared__ float dv[kObjTilePix];  // a member's disparity, NaN elsewhere: no join with a NaN
    __shared__ int lab[kObjTilePix];
    __shared__ int cnt[kObjTilePix];
    __shared__ int red[kObjLocalThreads / 64][3];
    const sdr_relief_query q = *query;
    RegionPlane pl;
    RegionView<T> M;
    if (query_view(maps, planes, NP, q, &pl, &M)) return;
    const PlaneRect R = M.R;
    const size_t stride = maps.stride;
    const int tx0 = blockIdx.x * kObjTile, ty0 = blockIdx.y * kObjTile;
    if (tx0 >= R.rw || ty0 >= R.rh) return;  // block-uniform
    const int i = threadIdx.x, lane = i & 63, wave = i >> 6, lx = i & (kObjTile - 1);
    const int u = tx0 + lx, v = ty0 + (i >> 5);
    const float md = P.max_diff;
    const bool conn8 = P.connectivity == 8;

    bool mem = false, masked = false, valid = false;
    float d = ruler_nan();
    if (u < R.rw && v < R.rh) {
        const RegionPix px = region_pixel(M, Q, pl, P.min_disp, P.conf_min, q.label, (unsigned)u, (unsigned)v);
        masked = px.masked;
        valid = px.valid;
        mem = px.member && P.h_lo <= px.hf && px.hf <= P.h_hi;
        if (mem) d = load_disp(M.fd + (size_t)v * stride + (size_t)u);  // step 2's bits
    }
    dv[i] = d;
    cnt[i] = 0;
    {  // the tile's counts: ballots, the waves' counts through LDS, one plain store
        const int nm = __popcll(__ballot(masked)), nv = __popcll(__ballot(valid)), nn = __popcll(__ballot(mem));
        if (lane == 0) {
            red[wave][0] = nm;
            red[wave][1] = nv;
            red[wave][2] = nn;
        }
    }
    __syncthreads();
    if (i == 0) {
        ObjTileCount c = {0, 0, 0, 0};
        for (int w = 0; w < kObjLocalThreads / 64; w++) {
            c.n_masked += red[w][0];
            c.n_valid += red[w][1];
            c.n += red[w][2];
        }
        tiles[blockIdx.y * gridDim.x + blockIdx.x] = c;
    }
    // horizontal runs: a run starts at every member not joined to its left neighbour
    const bool hc = mem && lx > 0 && fabsf(d - dv[i - 1]) <= md;
    const unsigned long long starts = __ballot(mem && !hc);
    const unsigned long long below = starts & (~0ull >> (63 - lane));
    const int s = 63 - __clzll((long long)(below | 1ull));  // a member's row holds a start at or before it
    const int run = mem ? i - (lane - s) : -1;
    lab[i] = run;
    __syncthreads();
    // joins with the row above: the pixel above, and with 8-connectivity its two neighbours
    if (run >= 0 && i >= kObjTile) {
        const int up = i - kObjTile;
        if (fabsf(d - dv[up]) <= md) lds_unite(lab, run, up);
        if (conn8) {
            if (lx > 0 && fabsf(d - dv[up - 1]) <= md) lds_unite(lab, run, up - 1);
            if (lx < kObjTile - 1 && fabsf(d - dv[up + 1]) <= md) lds_unite(lab, run, up + 1);
        }
    }
    __syncthreads();
    // roots and local sizes (one LDS atomic per distinct root of a wave)
    const int root = run >= 0 ? lds_find(lab, run) : -1;
    unsigned long long pend = __ballot(root >= 0);
    while (pend) {
        const int src = __ffsll((long long)pend) - 1;
        const int r = __shfl(root, src);
        const unsigned long long m = __ballot(root == r) & pend;
        if (lane == src) atomicAdd(&cnt[r], __popcll(m));
        pend &= ~m;
    }
    __syncthreads();
    if (u >= R.rw || v >= R.rh) return;
    const int g = v * R.rw + u;
    Pa[g] = root >= 0 ? (ty0 + (root >> 5)) * R.rw + tx0 + (root & (kObjTile - 1)) : -1;
    Sz[g] = (root >= 0 && root == i) ? cnt[i] : 0;
}

// A thread a border pixel: the last column of a tile against the column right of it, the last row
// against the row below, each with its one (4) or three (8) neighbours across; the diagonal pairs
// at a tile corner are among them.
template <typename T>
__global__ __launch_bounds__(256) void k_obj_merge(RegionMaps<T> maps, sdr_object_params P,
                                                   const sdr_plane* __restrict__ planes, int NP,
                                                   const sdr_relief_query* __restrict__ query, int* Pa) {
#pragma clang fp contract(off)
    const sdr_relief_query q = *query;
    RegionPlane pl;
    RegionView<T> M;
    if (query_view(maps, planes, NP, q, &pl, &M)) return;
    const PlaneRect R = M.R;
    const T* fd = M.fd;
    const size_t stride = maps.stride;
    const int nvx = (R.rw - 1) / kObjTile, nhy = (R.rh - 1) / kObjTile;
    const int nv = nvx * R.rh, nh = nhy * R.rw;
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= nv + nh) return;
    int ax, ay, bx[3], by[3];
    if (t < nv) {
        ay = t / nvx;
        ax = (t - ay * nvx + 1) * kObjTile - 1;
        bx[0] = bx[1] = bx[2] = ax + 1;
        by[0] = ay;
        by[1] = ay - 1;
        by[2] = ay + 1;
    } else {
        const int w = t - nv, yb = w / R.rw;
        ax = w - yb * R.rw;
        ay = (yb + 1) * kObjTile - 1;
        by[0] = by[1] = by[2] = ay + 1;
        bx[0] = ax;
        bx[1] = ax - 1;
        bx[2] = ax + 1;
    }
    // every load a pair may need is issued up front (a pair out of the rectangle reads a itself):
    // two dependent round trips instead of up to eight
    const int a = ay * R.rw + ax;
    const int nb = P.connectivity == 8 ? 3 : 1;
    bool in[3];
    int b[3], pb[3];
    float db[3];
    const int pa = uf_load(Pa, a);
    const float da = load_disp(fd + (size_t)ay * stride + (size_t)ax);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        in[j] = j < nb && bx[j] >= 0 && bx[j] < R.rw && by[j] >= 0 && by[j] < R.rh;
        const int x = in[j] ? bx[j] : ax, y = in[j] ? by[j] : ay;
        b[j] = y * R.rw + x;
        pb[j] = uf_load(Pa, b[j]);
        db[j] = load_disp(fd + (size_t)y * stride + (size_t)x);
    }
    if (pa < 0) return;
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (in[j] && pb[j] >= 0 && fabsf(da - db[j]) <= P.max_diff) uf_unite(Pa, a, b[j]);
}

// tile roots (S > 0): the global root, the size accumulated there, a one-hop pointer for the
// sweeps behind.  Only a global root's size is added to, and a global root adds nothing.
__global__ __launch_bounds__(kRegionThreads) void k_obj_sizes(RegionDims dims, const sdr_plane* __restrict__ planes, int NP,
                                                              const sdr_relief_query* __restrict__ query, int* Pa,
                                                              int* Sz) {
    const sdr_relief_query q = *query;
    RegionPlane pl;
    if (query_refusal(dims, planes, NP, q, &pl)) return;
    const PlaneRect R = plane_rect(region_segment(q));
    const unsigned area = (unsigned)R.rw * (unsigned)R.rh, base = blockIdx.x * (unsigned)kRegionSlice;
#pragma unroll
    for (int j = 0; j < kRegionPix; j++) {
        const unsigned p = base + (unsigned)(j * kRegionThreads + (int)threadIdx.x);
        if (p >= area) continue;
        const int c = Sz[p];
        if (c <= 0) continue;
        const int r = uf_find(Pa, (int)p);
        if (r != (int)p) {
            atomicAdd(&Sz[r], c);
            Pa[p] = r;
        }
    }
}

// the largest value of a workgroup's threads, in every thread (wm: a slot a wave)
template <int WAVES>
__device__ __forceinline__ unsigned long long block_max(unsigned long long m, unsigned long long* wm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    m = wave_max(m);
    if (lane == 0) wm[wave] = m;
    __syncthreads();
    unsigned long long best = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) best = max(best, wm[w]);
    __syncthreads();
    return best;
}

// A slice of the rectangle's order a workgroup: its global roots counted (slices[slice]), and the
// slice's max_objects largest keys of kept roots into cand[slice][max_objects], zeros behind them.
__global__ __launch_bounds__(kRegionThreads) void k_obj_select(RegionDims dims, sdr_object_params P,
                                                               const sdr_plane* __restrict__ planes, int NP,
                                                               const sdr_relief_query* __restrict__ query,
                                                               ObjSliceCount* __restrict__ slices,
                                                               const int* __restrict__ Pa,
                                                               const int* __restrict__ Sz,
                                                               unsigned long long* __restrict__ cand) {
    __shared__ unsigned long long wm[kRegionWaves];
    __shared__ int red[kRegionWaves][3];
    const sdr_relief_query q = *query;
    RegionPlane pl;
    if (query_refusal(dims, planes, NP, q, &pl)) return;
    const PlaneRect R = plane_rect(region_segment(q));
    const unsigned area = (unsigned)R.rw * (unsigned)R.rh, base = blockIdx.x * (unsigned)kRegionSlice;
    if (base >= area) return;  // block-uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long key[kRegionPix];
    int ncomp = 0, nkept = 0, dropped = 0;
#pragma unroll
    for (int j = 0; j < kRegionPix; j++) {
        const unsigned p = base + (unsigned)(j * kRegionThreads + tid);
        key[j] = 0;
        if (p >= area || Pa[p] != (int)p) continue;
        const int c = Sz[p];
        ncomp++;
        if (c >= P.min_pixels) {
            nkept++;
            key[j] = ((unsigned long long)c << 24) | (unsigned long long)(kObjRootMask - p);
        } else {
            dropped = max(dropped, c);
        }
    }
    ncomp = (int)wave_sum((long long)ncomp);
    nkept = (int)wave_sum((long long)nkept);
    dropped = wave_max(dropped);
    if (lane == 0) {
        red[wave][0] = ncomp;
        red[wave][1] = nkept;
        red[wave][2] = dropped;
    }
    __syncthreads();
    if (tid == 0) {
        ObjSliceCount c = {0, 0, 0, 0};
        for (int w = 0; w < kRegionWaves; w++) {
            c.n_components += red[w][0];
            c.n_kept += red[w][1];
            c.largest_dropped = max(c.largest_dropped, red[w][2]);
        }
        slices[blockIdx.x] = c;
    }
    unsigned long long* list = cand + (size_t)blockIdx.x * (size_t)P.max_objects;
    for (int r = 0; r < P.max_objects; r++) {
        unsigned long long m = 0;
#pragma unroll
        for (int j = 0; j < kRegionPix; j++) m = max(m, key[j]);
        const unsigned long long best = block_max<kRegionWaves>(m, wm);  // the keys differ: one owner
        if (best == 0) {  // block-uniform
            for (int i = r + tid; i < P.max_objects; i += kRegionThreads) list[i] = 0;
            break;
        }
        if (tid == 0) list[r] = best;
#pragma unroll
        for (int j = 0; j < kRegionPix; j++)
            if (key[j] == best) key[j] = 0;
    }
}

// One workgroup.  First the scan record's counts: the sums of what the rectangle's tiles and slices
// wrote.  Then max_objects rounds of the largest key left in the slices' lists; a thread reads the
// same entries every round, so the zero it writes over a winner is its own to see.
__global__ __launch_bounds__(kObjRankThreads) void k_obj_rank(RegionDims dims, sdr_object_params P,
                                                              const sdr_plane* __restrict__ planes, int NP,
                                                              const sdr_relief_query* __restrict__ query,
                                                              ObjState* __restrict__ S,
                                                              const ObjTileCount* __restrict__ tiles,
                                                              const ObjSliceCount* __restrict__ slices,
                                                              int* __restrict__ Sz, unsigned long long* cand) {
    __shared__ unsigned long long wm[kObjRankThreads / 64];
    __shared__ int sh[kObjRankThreads / 64][6];
    const sdr_relief_query q = *query;
    RegionPlane pl;
    if (query_refusal(dims, planes, NP, q, &pl)) return;
    const int W = dims.W;
    const PlaneRect R = plane_rect(region_segment(q));
    const size_t area = (size_t)R.rw * (size_t)R.rh;
    const int nslices = (int)((area + kRegionSlice - 1) / kRegionSlice);
    const int total = nslices * P.max_objects;  // <= 8192 * 64
    const int tid = threadIdx.x;
    {
        const int tw = (R.rw + kObjTile - 1) / kObjTile, th = (R.rh + kObjTile - 1) / kObjTile;
        const int pitch = (W + kObjTile - 1) / kObjTile;  // k_obj_local's grid
        int c[6] = {0, 0, 0, 0, 0, 0};
        for (int i = tid; i < tw * th; i += kObjRankThreads) {
            const ObjTileCount t = tiles[(i / tw) * pitch + i % tw];
            c[0] += t.n_masked;
            c[1] += t.n_valid;
            c[2] += t.n;
        }
        for (int i = tid; i < nslices; i += kObjRankThreads) {
            const ObjSliceCount t = slices[i];
            c[3] += t.n_components;
            c[4] += t.n_kept;
            c[5] = max(c[5], t.largest_dropped);
        }
        // five sums and a maximum: the waves' values through LDS, thread 0 the rest
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const int r = j < 5 ? (int)wave_sum((long long)c[j]) : wave_max(c[j]);
            if ((tid & 63) == 0) sh[tid >> 6][j] = r;
        }
        __syncthreads();
        if (tid == 0) {
            int t[6] = {0, 0, 0, 0, 0, 0};
            for (int w = 0; w < kObjRankThreads / 64; w++)
                for (int j = 0; j < 6; j++) t[j] = j < 5 ? t[j] + sh[w][j] : max(t[j], sh[w][j]);
            S->n_masked = t[0];
            S->n_valid = t[1];
            S->n = t[2];
            S->n_components = t[3];
            S->n_kept = t[4];
            S->largest_dropped = t[5];
        }
    }
    int count = 0;
    for (int r = 0; r < P.max_objects; r++) {
        unsigned long long m = 0;
        int mi = -1;
        for (int i = tid; i < total; i += kObjRankThreads) {
            const unsigned long long v = cand[i];
            if (v > m) {
                m = v;
                mi = i;
            }
        }
        const unsigned long long best = block_max<kObjRankThreads / 64>(m, wm);
        if (best == 0) break;  // block-uniform
        if (m == best) cand[mi] = 0;
        if (tid == 0) {
            S->ranked[r] = best;
            Sz[kObjRootMask - (unsigned)(best & kObjRootMask)] = -1 - r;
        }
        count = r + 1;
    }
    if (tid == 0) S->count = count;
}

// The labels and the ranked objects' records: every lane takes part in the wave reductions, a
// lane without a ranked pixel with neutral values.
template <typename T>
__global__ __launch_bounds__(kRegionThreads) void k_obj_stats(RegionMaps<T> maps, Q16 Q, sdr_object_params P,
                                                              const sdr_plane* __restrict__ planes, int NP,
                                                              const sdr_relief_query* __restrict__ query,
                                                              ObjState* __restrict__ S, const int* __restrict__ Pa,
                                                              const int* __restrict__ Sz,
                                                              uint8_t* __restrict__ labels_out) {
#pragma clang fp contract(off)
    __shared__ ObjAcc la[kObjMax];
    const sdr_relief_query q = *query;
    RegionPlane pl;
    RegionView<T> M;
    if (query_view(maps, planes, NP, q, &pl, &M)) return;
    if (S->count == 0) return;  // block-uniform: every label stays 255
    const PlaneRect R = M.R;
    const int W = maps.W;
    const unsigned area = (unsigned)R.rw * (unsigned)R.rh, base = blockIdx.x * (unsigned)kRegionSlice;
    if (base >= area) return;  // block-uniform
    uint8_t* lo = maps.view(region_segment(q), labels_out).fl;  // the frame's label map that goes out
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < kObjMax) la[tid] = ObjAcc{0, 0, 0, 0u, 0u, 0u, 0u, 0u, 0u};
    __syncthreads();
    // the labels of the thread's pixels first, so that their dependent loads overlap
    int kj[kRegionPix];
#pragma unroll
    for (int j = 0; j < kRegionPix; j++) {
        const unsigned p = base + (unsigned)(j * kRegionThreads + tid);
        kj[j] = -1;
        if (p < area) {
            const int pp = Pa[p];
            if (pp >= 0) {
                const int s = Sz[Pa[pp]];  // the global root's size, or -1 - rank
                if (s < 0) kj[j] = -1 - s;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kRegionPix; j++) {
        const unsigned p = base + (unsigned)(j * kRegionThreads + tid);
        const int k = kj[j];
        const unsigned v = p < area ? p / (unsigned)R.rw : 0u, u = p < area ? p - v * (unsigned)R.rw : 0u;
        if (lo && p < area) lo[(size_t)v * W + u] = k < 0 ? (uint8_t)255 : (uint8_t)k;
        if (__ballot(k >= 0) == 0) continue;  // wave-uniform
        long long e = 0;
        unsigned key = 0;
        if (k >= 0) {
            const RegionPix px = region_pixel(M, Q, pl, P.min_disp, P.conf_min, q.label, u, v);
            e = llrint((double)px.hf * 256.0);
            key = ordered_key(px.hf);
        }
        const int x = R.xs + (int)u, y = R.ys + (int)v;
        unsigned long long pend = __ballot(k >= 0);
        while (pend) {  // wave-uniform
            const int src = __ffsll((long long)pend) - 1;
            const int kk = __shfl(k, src);
            const bool mine = k == kk;
            const long long sx = wave_sum(mine ? (long long)x : 0ll), sy = wave_sum(mine ? (long long)y : 0ll);
            const long long se = wave_sum(mine ? e : 0ll);
            const unsigned x0i = wave_max(mine ? 0x10000u - (unsigned)x : 0u);
            const unsigned y0i = wave_max(mine ? 0x10000u - (unsigned)y : 0u);
            const unsigned x1p = wave_max(mine ? (unsigned)x + 1u : 0u), y1p = wave_max(mine ? (unsigned)y + 1u : 0u);
            const unsigned kmax = wave_max(mine ? key : 0u), kmin_inv = wave_max(mine ? ~key : 0u);
            if (lane == src) {
                ObjAcc* a = la + kk;
                atomicAdd((unsigned long long*)&a->sum_x, (unsigned long long)sx);
                atomicAdd((unsigned long long*)&a->sum_y, (unsigned long long)sy);
                atomicAdd((unsigned long long*)&a->sum256, (unsigned long long)se);
                atomicMax(&a->x0i, x0i);
                atomicMax(&a->y0i, y0i);
                atomicMax(&a->x1p, x1p);
                atomicMax(&a->y1p, y1p);
                atomicMax(&a->kmax, kmax);
                atomicMax(&a->kmin_inv, kmin_inv);
            }
            pend &= ~__ballot(mine);
        }
    }
    __syncthreads();
    if (tid < kObjMax && la[tid].x1p != 0) {  // the slice holds pixels of object tid
        const ObjAcc l = la[tid];
        ObjAcc* a = S->acc + tid;
        atomicAdd((unsigned long long*)&a->sum_x, (unsigned long long)l.sum_x);
        atomicAdd((unsigned long long*)&a->sum_y, (unsigned long long)l.sum_y);
        atomicAdd((unsigned long long*)&a->sum256, (unsigned long long)l.sum256);
        atomicMax(&a->x0i, l.x0i);
        atomicMax(&a->y0i, l.y0i);
        atomicMax(&a->x1p, l.x1p);
        atomicMax(&a->y1p, l.y1p);
        atomicMax(&a->kmax, l.kmax);
        atomicMax(&a->kmin_inv, l.kmin_inv);
    }
}

// the max_objects records (a thread each) and the scan record
__global__ __launch_bounds__(kObjMax) void k_obj_finish(RegionDims dims, sdr_object_params P,
                                                        const sdr_plane* __restrict__ planes, int NP,
                                                        const sdr_relief_query* __restrict__ query,
                                                        const ObjState* __restrict__ S,
                                                        sdr_object* __restrict__ objects,
                                                        sdr_object_scan* __restrict__ scan) {
    const sdr_relief_query q = *query;
    RegionPlane pl;
    const uint32_t refused = query_refusal(dims, planes, NP, q, &pl);
    const PlaneRect R = plane_rect(region_segment(q));
    const int tid = threadIdx.x, count = refused ? 0 : S->count;
    if (tid < P.max_objects) {
        sdr_object o;
        o.n = 0;
        o.root = o.x0 = o.y0 = o.x1 = o.y1 = -1;
        o.sum_x = o.sum_y = o.sum256 = 0;
        o.h_min = o.h_max = ruler_nan();
        o.flags = 0;
        o.reserved = 0;
        if (tid < count) {
            const unsigned long long key = S->ranked[tid];
            const ObjAcc a = S->acc[tid];
            o.n = (int)(key >> 24);
            o.root = (int)(kObjRootMask - (unsigned)(key & kObjRootMask));
            o.x0 = 0x10000 - (int)a.x0i;
            o.y0 = 0x10000 - (int)a.y0i;
            o.x1 = (int)a.x1p - 1;
            o.y1 = (int)a.y1p - 1;
            o.sum_x = a.sum_x;
            o.sum_y = a.sum_y;
            o.sum256 = a.sum256;
            o.h_max = ordered_unkey(a.kmax);
            o.h_min = ordered_unkey(~a.kmin_inv);
            const bool cut = o.x0 == R.xs || o.x1 == R.xs + R.rw - 1 || o.y0 == R.ys || o.y1 == R.ys + R.rh - 1;
            o.flags = SDR_OBJECT_VALID | (cut ? SDR_OBJECT_CUT : 0);
        }
        objects[tid] = o;
    }
    if (tid != 0) return;
    sdr_object_scan s;
    memset(&s, 0, sizeof s);
    s.frame = q.frame;
    s.plane = q.plane;
    s.label = q.label;
    if (refused) {
        s.flags = refused;
        s.area = refused == kRegionOutOfRange ? 0 : R.rw * R.rh;
    } else {
        s.area = R.rw * R.rh;
        s.n_masked = S->n_masked;
        s.n_valid = S->n_valid;
        s.n = S->n;
        s.n_components = S->n_components;
        s.n_kept = S->n_kept;
        s.count = count;
        s.largest_dropped = S->largest_dropped;
        s.flags = (s.n_kept == 0 ? SDR_OBJECTS_EMPTY : SDR_OBJECTS_VALID) |
                  (s.n_kept > P.max_objects ? SDR_OBJECTS_TRUNCATED : 0);
    }
    *scan = s;
}

}  // namespace sdr

namespace {

using namespace sdr::ruler_host;

int check_object_params(const sdr_object_params* p, const void* planes, int P) {
    if (int rc = check_planes_arg(planes, P)) return rc;
    if (std::isnan(p->h_lo) || std::isnan(p->h_hi) || p->h_lo > p->h_hi)
        return rfail(SDR_ERR_ARG, "h_lo and h_hi must not be NaN, and h_lo <= h_hi");
    if (!(std::isfinite(p->max_diff) && p->max_diff >= 0.0f))
        return rfail(SDR_ERR_ARG, "max_diff must be finite and >= 0");
    if (p->connectivity != 4 && p->connectivity != 8) return rfail(SDR_ERR_ARG, "connectivity must be 4 or 8");
    if (p->min_pixels < 1 || p->min_pixels > (1 << 24)) return rfail(SDR_ERR_ARG, "min_pixels must be in 1..2^24");
    if (p->max_objects < 1 || p->max_objects > sdr::kObjMax) return rfail(SDR_ERR_ARG, "max_objects must be in 1..64");
    for (int i = 0; i < 8; i++)
        if (p->reserved[i]) return rfail(SDR_ERR_ARG, "reserved fields must be 0");
    return SDR_OK;
}

// the guards of both entries
int check_objects_call(const void* disp, int disp_type, size_t stride, size_t fstride, int W, int H, int F,
                       const void* labels_in, const double* Q, const sdr_object_params* params, const void* planes,
                       int P, const void* query, const void* objects, const void* scan, const void* labels_out) {
    int rc = check_plane_maps(disp, disp_type, stride, fstride, W, H, F, Q, params, query, 1, objects);
    if (rc || (rc = check_object_params(params, planes, P))) return rc;
    if (!scan) return rfail(SDR_ERR_ARG, "null argument");
    if (labels_out && labels_out == labels_in) return rfail(SDR_ERR_ARG, "labels_out must not be labels_in");
    return SDR_OK;
}

}  // namespace

extern "C" {

void sdr_object_params_default(sdr_object_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->min_disp = -1.0f;
    p->conf_min = 0.0f;
    p->h_lo = 10.0f;
    p->h_hi = 1048576.0f;
    p->max_diff = 1.0f;
    p->connectivity = 8;
    p->min_pixels = 64;
    p->max_objects = 16;
}

int sdr_find_objects_device(const void* d_disp, int disp_type, size_t stride, size_t frame_stride, int W, int H,
                            int F, const float* d_conf, const uint8_t* d_labels_in, const double Q[16],
                            const sdr_object_params* params, const sdr_plane* d_planes, int P,
                            const sdr_relief_query* d_query, sdr_object* d_objects, sdr_object_scan* d_scan,
                            uint8_t* d_labels_out, void* stream) {
    if (int rc = check_objects_call(d_disp, disp_type, stride, frame_stride, W, H, F, d_labels_in, Q, params, d_planes,
                                    P, d_query, d_objects, d_scan, d_labels_out))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const sdr::Q16 q = make_q16(Q);
    const sdr_object_params OP = *params;
    const size_t px = (size_t)W * H;
    const unsigned slices = sdr::region_slices(W, H);
    const dim3 tiles((unsigned)((W + sdr::kObjTile - 1) / sdr::kObjTile),
                     (unsigned)((H + sdr::kObjTile - 1) / sdr::kObjTile));
    // scratch, sized for the frame (the query is device memory): {parents, sizes, candidates, the
    // tiles' counts, the slices' counts, state}
    sdr::ScratchLayout lay;
    const auto s_parents = lay.take<int>(px);
    const auto s_sizes = lay.take<int>(px);
    const auto s_cand = lay.take<unsigned long long>((size_t)slices * OP.max_objects);
    const auto s_tiles = lay.take<sdr::ObjTileCount>((size_t)tiles.x * tiles.y);
    const auto s_slices = lay.take<sdr::ObjSliceCount>((size_t)slices);
    const auto s_state = lay.take<sdr::ObjState>(1);
    sdr::Scratch sc(st);
    if (int rc = sc.open(lay)) return rc;
    int* Pa = sc.at(s_parents);
    int* Sz = sc.at(s_sizes);
    unsigned long long* cand = sc.at(s_cand);
    sdr::ObjTileCount* tcnt = sc.at(s_tiles);
    sdr::ObjSliceCount* scnt = sc.at(s_slices);
    sdr::ObjState* S = sc.at(s_state);
    // border pixels of the largest rectangle: ((W - 1) / 32) * H + ((H - 1) / 32) * W <= 2^20
    const size_t borders = (size_t)((W - 1) / sdr::kObjTile) * H + (size_t)((H - 1) / sdr::kObjTile) * W;
    const dim3 block(sdr::kRegionThreads), sgrid(slices), mgrid((unsigned)((borders + 255) / 256));
    hipError_t e = hipMemsetAsync(S, 0, sizeof(sdr::ObjState), st);
    if (e == hipSuccess && d_labels_out) e = hipMemsetAsync(d_labels_out, 255, px, st);
    if (e == hipSuccess)
        with_maps(d_disp, disp_type, stride, frame_stride, W, H, F, d_conf, d_labels_in, [&](auto maps) {
            using T = disp_elem_t<decltype(maps)>;
            const sdr::RegionDims dims = maps.dims();
            hipLaunchKernelGGL((sdr::k_obj_local<T>), tiles, dim3(sdr::kObjLocalThreads), 0, st, maps, q, OP, d_planes, P,
                               d_query, tcnt, Pa, Sz);
            if (borders)
                hipLaunchKernelGGL((sdr::k_obj_merge<T>), mgrid, dim3(256), 0, st, maps, OP, d_planes, P, d_query, Pa);
            hipLaunchKernelGGL(sdr::k_obj_sizes, sgrid, block, 0, st, dims, d_planes, P, d_query, Pa, Sz);
            hipLaunchKernelGGL(sdr::k_obj_select, sgrid, block, 0, st, dims, OP, d_planes, P, d_query, scnt,
                               (const int*)Pa, (const int*)Sz, cand);
            hipLaunchKernelGGL(sdr::k_obj_rank, dim3(1), dim3(sdr::kObjRankThreads), 0, st, dims, OP, d_planes, P,
                               d_query, S, (const sdr::ObjTileCount*)tcnt, (const sdr::ObjSliceCount*)scnt, Sz, cand);
            hipLaunchKernelGGL((sdr::k_obj_stats<T>), sgrid, block, 0, st, maps, q, OP, d_planes, P, d_query, S,
                               (const int*)Pa, (const int*)Sz, d_labels_out);
            hipLaunchKernelGGL(sdr::k_obj_finish, dim3(1), dim3(sdr::kObjMax), 0, st, dims, OP, d_planes, P, d_query,
                               (const sdr::ObjState*)S, d_objects, d_scan);
        });
    return sc.finish(e);
}

int sdr_find_objects(const void* disp, int disp_type, size_t stride, size_t frame_stride, int W, int H, int F,
                     const float* conf, const uint8_t* labels_in, const double Q[16], const sdr_object_params* params,
                     const sdr_plane* planes, int P, const sdr_relief_query* query, sdr_object* objects,
                     sdr_object_scan* scan, uint8_t* labels_out) {
    int rc = check_objects_call(disp, disp_type, stride, frame_stride, W, H, F, labels_in, Q, params, planes, P, query,
                                objects, scan, labels_out);
    if (rc) return rc;
    HostCall c;
    const HostCall::Maps m = c.maps(disp, disp_type, stride, frame_stride, W, H, F, conf);
    const sdr_plane* d_planes = c.input(c.S->planes, planes, (size_t)P);
    const sdr_relief_query* d_query = c.input(c.S->rows, query, 1);
    const uint8_t* d_labels_in = c.input(c.S->labels, labels_in, (size_t)F * W * H);
    const auto s_objects = c.output(objects, (size_t)params->max_objects);
    const auto s_scan = c.output(scan, 1);
    const auto s_labels = c.output(labels_out, labels_out ? (size_t)W * H : 0);
    if ((rc = c.ready())) return rc;
    rc = sdr_find_objects_device(m.disp, disp_type, m.stride, m.fstride, W, H, F, m.conf, d_labels_in, Q, params,
                                 d_planes, P, d_query, c.at(s_objects), c.at(s_scan),
                                 labels_out ? c.at(s_labels) : nullptr, c.stream());
    return rc ? rc : c.finish();
}

}  // extern "C"
