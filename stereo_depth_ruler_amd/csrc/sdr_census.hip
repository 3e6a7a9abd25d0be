// sdr_census.hip -- the census matching cost (SDR_COST_CENSUS_9X7): the 9x7 census transform of
// both images and the cost volume of its Hamming distances (CDNA4).
//
//   descriptors  u64 [F][2][H][W]   index 0: the frame's left-role image, 1: its right-role image.
//                                   Bit k of T(y, x) (k = 0 the LSB) is 1 iff
//                                   I(clamp(y+dy, 0, H-1), clamp(x+dx, 0, W-1)) < I(y, x), k counting
//                                   (dy, dx) row-major over dy = -3..3, dx = -4..4 without the
//                                   centre; bits 62 and 63 are 0.  Raw intensities: no prefilter.
//   C            s16 [F][H][W1][D]  P2 + blockSize^2 box sum of
//                                   pc(y, x, d) = popcount(T_left(y, x) ^ T_right(y, x - d))
//
// The cost kernel is k_cost's skeleton (sdr_cost_kernel.hpp) with another pixel cost: lanes are
// disparity pairs, a block owns BCOLS output columns, each pixel cost is computed once, summed
// vertically in a register ring of the last NR rows and horizontally through LDS, one barrier
// per row, every load unconditional with clamped indices.  What differs is the operand staging:
// a lane holding disparities (d, d+1) of column x needs T_right(x-d) and T_right(x-d-1), so a
// row of right descriptors is staged split into its even-x and odd-x halves (lane p reads entry
// x - 2p of one half and x - 1 - 2p of the other: both ds_read_b64 are consecutive across lanes),
// and the left descriptor of a column is one broadcast ds_read_b64.  Per pair: 4 v_xor, 4
// v_bcnt_u32_b32 and the pack into the ring's u16x2 word.
#include "sdr_cost_kernel.hpp"

namespace sdr {

// ------------------------------------------------------------------------------------------
// Census transform.  One block per image row, both roles of all frames in one launch; the 7
// rows (replicated at the top and bottom) are staged in LDS.  Like k_prefilter it honours the
// paired matchers' swap (frames >= split take the images swapped) and starts the right-view
// keys of the WTA at kD2None.
// ------------------------------------------------------------------------------------------
constexpr int kCensusRows = 7, kCensusCols = 9;

__global__ __launch_bounds__(256) void k_census(const uint8_t* __restrict__ Limg,
                                                const uint8_t* __restrict__ Rimg, size_t stride,
                                                size_t fstride, int W, int H, uint64_t* desc,
                                                int split, uint32_t* d2fill) {
    extern __shared__ uint32_t rows32[];  // [7][WP] bytes, WP = W rounded up to 4
    uint8_t* rows = (uint8_t*)rows32;
    const int y = blockIdx.x, img = blockIdx.y, f = blockIdx.z;
    const int WP = (W + 3) & ~3;
    const bool swap = f >= split;
    const uint8_t* base = ((img != 0) != swap ? Rimg : Limg) + (size_t)(swap ? f - split : f) * fstride;
    if (((W | (int)stride | (int)fstride | (int)(uintptr_t)base) & 3) == 0) {
        // dword-aligned rows: four bytes a lane
        const int nw = W >> 2;
        for (int i = threadIdx.x; i < kCensusRows * nw; i += blockDim.x) {
            const int r = i / nw, x = i - r * nw;
            const int yy = min(max(y + r - 3, 0), H - 1);
            rows32[r * nw + x] = ((const uint32_t*)(base + (size_t)yy * stride))[x];
        }
    } else {
        for (int i = threadIdx.x; i < kCensusRows * W; i += blockDim.x) {
            const int r = i / W, x = i - r * W;
            const int yy = min(max(y + r - 3, 0), H - 1);
            rows[r * WP + x] = base[(size_t)yy * stride + x];
        }
    }
    __syncthreads();
    if (d2fill && img == 0) {
        // the right-view keys of this row start empty (k_south_wta's atomics fold into them)
        uint32_t* d2 = d2fill + ((size_t)f * H + y) * W;
        for (int x = threadIdx.x; x < W; x += blockDim.x) d2[x] = kD2None;
    }
    uint64_t* dst = desc + (((size_t)f * 2 + img) * H + y) * W;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const uint32_t c = rows[3 * WP + x];
        int xs[kCensusCols];
#pragma unroll
        for (int k = 0; k < kCensusCols; k++) xs[k] = min(max(x + k - 4, 0), W - 1);
        uint32_t lo = 0, hi = 0;  // bits 0..31 and 32..61
#pragma unroll
        for (int r = 0; r < kCensusRows; r++)
#pragma unroll
            for (int k = 0; k < kCensusCols; k++) {
                if (r == 3 && k == 4) continue;
                constexpr int centre = 3 * kCensusCols + 4;
                const int bit = r * kCensusCols + k - (r * kCensusCols + k > centre ? 1 : 0);
                const uint32_t b = rows[r * WP + xs[k]] < c ? 1u : 0u;
                if (bit < 32) lo |= b << bit;
                else hi |= b << (bit - 32);
            }
        dst[x] = (uint64_t)lo | ((uint64_t)hi << 32);
    }
}

void launch_census(const uint8_t* L, const uint8_t* R, size_t stride, size_t fstride, int W, int H,
                   int F, uint64_t* desc, hipStream_t st, int split, uint32_t* d2fill) {
    hipLaunchKernelGGL(k_census, dim3(H, 2, F), dim3(256), (size_t)kCensusRows * ((W + 3) & ~3), st, L, R,
                       stride, fstride, W, H, desc, split, d2fill);
}

// ------------------------------------------------------------------------------------------
// Cost volume of the census pixel cost: the formula and the contract of k_cost (CostArgs,
// Geometry, the C layout and sink row, row bands + stripe-start bands in one launch, hh_bottom,
// frame_geom for paired frames, the XCD block order).  a.pl.L / a.pl.R are the left-role and
// right-role descriptor planes (u64 [H][W] per frame, frames pl.fstrideL / pl.fstrideR u64 apart).
// ------------------------------------------------------------------------------------------
template <int NR, int K>
struct CensusCfg : CostCfg<NR, K, 1> {
    using B = CostCfg<NR, K, 1>;
    // LDS bytes: two staging buffers (R: 2 parity halves, L: one descriptor a column) + two
    // column-sum buffers
    static size_t lds_bytes(int D) {
        return (size_t)2 * 2 * cost_half_r(B::NLV + D) * 8 + (size_t)2 * B::NLV * 8 +
               (size_t)2 * B::NLV * K * 64 * 4;
    }
};

template <int NR, int K, bool EDGE>
__device__ __forceinline__ void census_block(const Geometry& g, const CostArgs& a, uint64_t* lds,
                                             int bx, int f, int ty0, int ty1) {
    using Cfg = CensusCfg<NR, K>;
    constexpr int SW2 = Cfg::SW2, SH2 = SW2, BCOLS = Cfg::BCOLS, CW = Cfg::CW;
    constexpr int PCW = Cfg::PCW, NLV = Cfg::NLV, PD = Cfg::PD, U = Cfg::U;
    static_assert(U % PD == 0 && U % NR == 0 && U % 2 == 0, "static slots");
    const int W = g.W, H = g.H, W1 = g.W1, D = g.D;
    const int lane = threadIdx.x & 63, tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bx0 = bx * BCOLS;
    const uint32_t P2x2 = splat16(g.P2);
    int16_t* out = a.out + (size_t)f * a.out_fstride;

    // output addressing as in cost_block: lanes past the last disparity pair alias it, every
    // store is unconditional, warm-up rows go to the sink row
    const int ox0 = bx0 + wave * CW;
    const int ncols = EDGE ? min(CW, W1 - ox0) : CW;
    const uint32_t colb = (uint32_t)D * 2, rowb = (uint32_t)W1 * colb;
    const Rsrc rO = rsrc_at(out + ((size_t)(ty0 - a.out_row0) * W1 + ox0) * D);
    const Rsrc rSink = rsrc_at(a.sink + (size_t)ox0 * D);
    int qpc[K];
    uint32_t vo[K];
#pragma unroll
    for (int i = 0; i < K; i++) {
        qpc[i] = min(lane + 64 * i, D / 2 - 1);
        vo[i] = 4 * qpc[i];
    }
    auto emit_at = [&](Rsrc r, uint32_t so, auto&& val) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < K; i++)
#pragma unroll
            for (int c = 0; c < CW; c++)
                if (!EDGE || c < ncols) __builtin_amdgcn_raw_buffer_store_b32(val(i, c), r, vo[i], so + c * colb, 0);
    };
    auto emit = [&](int y, auto&& val) __attribute__((always_inline)) { emit_at(rO, (uint32_t)(y - ty0) * rowb, val); };

    // rows [yl, ty1) of MODE_HH keep the initial P2
    int yl = ty1;
    if (a.hh_bottom) yl = max(ty0, min(ty1, max(1, H - SH2)));
    for (int y = yl; y < ty1; y++) emit(y, [&](int, int) { return P2x2; });
    if (yl <= ty0) return;

    // Virtual columns v = vlo + p, p = 0 .. NLV-1; wave w computes the pixel costs of columns
    // p = w + 4*jj.  Left descriptors are staged for image columns minX1 + clamp(v, 0, W1-1);
    // right descriptors for xr = minX1 + vlo - minD - (D-1) + e, e = 0 .. NLV+D-2: disparity 2qp of
    // column p needs e = p + D-1 - 2qp, disparity 2qp+1 the entry before it.  Entry e is staged at
    // [e & 1][e >> 1]; image columns are clamped to [0, W-1] (columns beyond [0, W1) are computed
    // from clamped data and never read, as in cost_block).
    const int vlo = bx0 - SW2;
    const int NRP = NLV + D - 1;
    const int HR = cost_half_r(NLV + D);  // entries per parity half (>= ceil(NRP / 2))
    const int BUFR = 2 * HR;
    uint64_t* LB = lds + 2 * BUFR;                       // [2][NLV] left descriptors
    uint32_t* VB = (uint32_t*)(LB + 2 * NLV);            // [2][NLV][K][64] column sums

    constexpr int NT = Cfg::NT, NW = Cfg::NW;
    static_assert(NLV <= NT, "one left descriptor a thread");
    constexpr int NPR = (NLV + 128 * K - 1 + NT - 1) / NT;  // R entries per thread (NRP <= NLV + 128 K - 1)
    const int xr0 = g.minX1 + vlo - g.minD - (D - 1);
    const Rsrc rR = rsrc_at(a.pl.R + (size_t)f * a.pl.fstrideR);  // < 2 GiB a frame (check_frame)
    const Rsrc rL = rsrc_at((const uint64_t*)a.pl.L + (size_t)f * a.pl.fstrideL);
    uint32_t gr[NPR];
    int pr[NPR];
#pragma unroll
    for (int t = 0; t < NPR; t++) {
        const int ir = min(tid + NT * t, NRP - 1);
        gr[t] = 8 * min(max(xr0 + ir, 0), W - 1);
        pr[t] = (ir & 1) * HR + (ir >> 1);
    }
    const int il = min(tid, NLV - 1);
    const uint32_t gl = 8 * (g.minX1 + min(max(vlo + il, 0), W1 - 1));
    struct Stage {
        uint64_t r[NPR];
        uint64_t l;
    };
    Stage st[PD];
    auto fetch = [&](int r, Stage& sg) __attribute__((always_inline)) {
        const uint32_t so = (uint32_t)r * W * 8;
#pragma unroll
        for (int t = 0; t < NPR; t++) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b64(rR, gr[t], so, 0);
            sg.r[t] = (uint64_t)v[0] | ((uint64_t)v[1] << 32);
        }
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(rL, gl, so, 0);
        sg.l = (uint64_t)v[0] | ((uint64_t)v[1] << 32);
    };
    auto put = [&](int b, const Stage& sg) __attribute__((always_inline)) {
        uint64_t* BR = lds + b * BUFR;
#pragma unroll
        for (int t = 0; t < NPR; t++) BR[pr[t]] = sg.r[t];
        LB[b * NLV + il] = sg.l;
    };

    // per-lane staged position of disparity 2qp of this wave's column jj: e = p + D-1 - 2qp with
    // p = wave + NW*jj, i.e. half (wave + 1) & 1, entry (wave + D-1) / 2 - qp + (NW/2)*jj; disparity
    // 2qp+1 is e - 1: the other half, entry (wave + D-2) / 2 - qp + (NW/2)*jj
    int rpa[K], rpb[K];
#pragma unroll
    for (int i = 0; i < K; i++) {
        rpa[i] = ((wave + 1) & 1) * HR + ((wave + D - 1) >> 1) - qpc[i];
        rpb[i] = (wave & 1) * HR + ((wave + D - 2) >> 1) - qpc[i];
    }
    uint32_t* Vw = VB + (wave * K) * 64 + lane;
    const int plo = SW2 - bx0, phi = W1 - 1 - vlo;

    // virtual rows and outputs
    const int ylim = a.ylim, s0 = a.s0;
    const int tfirst = min(ty0, ylim), tlast = min(yl - 1, ylim);
    const int qbeg = tfirst - SH2, qend = tlast + SH2;
    auto phys = [&](int q) { return min(max(min(q, qend), s0), H - 1); };

    // horizontal sums (+ P2) of the column sums in buffer b
    auto hsum = [&](int b, uint32_t (&hs)[K][CW]) __attribute__((always_inline)) {
        const uint32_t* V = VB + b * (NLV * K * 64) + (wave * CW) * K * 64 + lane;
#pragma unroll
        for (int i = 0; i < K; i++) {
            uint32_t v[CW + 2 * SW2];
#pragma unroll
            for (int c = 0; c < CW + 2 * SW2; c++) {
                int dc = c;  // interior: immediate offsets from one base
                if (EDGE) dc = min(max(wave * CW + c, plo), phi) - wave * CW;
                v[c] = V[(dc * K + i) * 64];
            }
            uint32_t h = P2x2;
#pragma unroll
            for (int k = 0; k < 2 * SW2 + 1; k++) h = pk_add(h, v[k]);
            hs[i][0] = h;
#pragma unroll
            for (int c = 1; c < CW; c++) {
                h = pk_sub(pk_add(h, v[c + 2 * SW2]), v[c - 1]);
                hs[i][c] = h;
            }
        }
    };

    uint32_t ring[NR][K][PCW], vs[K][PCW];
#pragma unroll
    for (int s = 0; s < NR; s++)
#pragma unroll
        for (int i = 0; i < K; i++)
#pragma unroll
            for (int jj = 0; jj < PCW; jj++) ring[s][i][jj] = 0;
#pragma unroll
    for (int i = 0; i < K; i++)
#pragma unroll
        for (int jj = 0; jj < PCW; jj++) vs[i][jj] = 0;

    fetch(phys(qbeg), st[0]);
    put(0, st[0]);
#pragma unroll
    for (int k = 1; k <= PD; k++) fetch(phys(qbeg + k), st[k % PD]);
    __syncthreads();

    // one barrier per virtual row q = qbeg + j (mod U): (A) horizontal sums + outputs of the
    // column sums row q-1 left in LDS, (B) staging of row q+1 and the fetch of row q+1+PD, (C)
    // pixel costs of row q, the vertical window, its column sums into LDS
    auto row = [&](const int q, auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        constexpr int s = j % NR, b = j & 1;
        {
            uint32_t hs[K][CW];
            hsum(b ^ 1, hs);
            const int t = q - 1 - SH2;
            const bool real = t >= ty0;
            emit_at(real ? rO : rSink, real ? (uint32_t)(t - ty0) * rowb : 0u, [&](int i, int c) { return hs[i][c]; });
        }
        put((j + 1) & 1, st[(j + 1) % PD]);
        fetch(phys(q + 1 + PD), st[(j + 1) % PD]);
        const uint64_t* BR = lds + b * BUFR;
        const uint64_t* BL = LB + b * NLV + wave;
#pragma unroll
        for (int jj = 0; jj < PCW; jj++) {
            const uint64_t tl = BL[NW * jj];  // every lane reads the column's descriptor: a broadcast
#pragma unroll
            for (int i = 0; i < K; i++) {
                const uint64_t ra = BR[rpa[i] + (NW / 2) * jj], rb = BR[rpb[i] + (NW / 2) * jj];
                const uint32_t pix = (uint32_t)__builtin_popcountll(tl ^ ra) |
                                     ((uint32_t)__builtin_popcountll(tl ^ rb) << 16);
                vs[i][jj] = pk_sub(pk_add(vs[i][jj], pix), ring[s][i][jj]);
                ring[s][i][jj] = pix;
            }
        }
        {
            uint32_t* Vb = Vw + b * (NLV * K * 64);
#pragma unroll
            for (int jj = 0; jj < PCW; jj++)
#pragma unroll
                for (int i = 0; i < K; i++) Vb[(NW * jj * K + i) * 64] = vs[i][jj];
        }
        __syncthreads();
    };
    int qq = qbeg;
    for (; qq + U - 1 <= qend; qq += U) unroll_rows(row, qq, std::make_integer_sequence<int, U>{});
    unroll_rows_tail(row, qq, qend, std::make_integer_sequence<int, U>{});
    // the last window, t = tlast: its rows [max(tlast, ty0), yl) (the frozen bottom rows repeat it)
    uint32_t hs[K][CW];
    hsum((qend - qbeg) & 1, hs);
    for (int y = max(tlast, ty0); y < yl; y++) emit(y, [&](int i, int c) { return hs[i][c]; });
}

template <int NR, int K>
__global__ __launch_bounds__((CensusCfg<NR, K>::NT)) void k_cost_census(Geometry g, CostArgs a) {
    using Cfg = CensusCfg<NR, K>;
    extern __shared__ uint64_t lds[];
    // block order and row bands as in k_cost
    const int gx = gridDim.x, gy = gridDim.y;
    const int l = xcd_block(blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z), gx * gy * gridDim.z);
    const int bx = l % gx, by = (l / gx) % gy, f = l / (gx * gy);
    const int nmain = gy - a.naux;
    CostArgs aa = a;
    int ty0, ty1;
    if (by < nmain) {
        ty0 = a.row_begin + by * a.TY;
        ty1 = min(ty0 + a.TY, a.row_end);
    } else {
        const CostAux& x = a.aux[by - nmain];
        aa.out = x.out;
        aa.out_fstride = a.aux_fstride;
        aa.out_row0 = x.row0;
        aa.s0 = x.s0;
        aa.ylim = x.ylim;
        aa.hh_bottom = 0;
        ty0 = x.row0;
        ty1 = x.row0 + x.rows;
    }
    if (ty0 >= ty1) return;
    const int bx0 = bx * Cfg::BCOLS;
    const Geometry gf = frame_geom(g, f);
    if (bx0 - Cfg::SW2 < 0 || bx0 + Cfg::BCOLS + Cfg::SW2 > g.W1) census_block<NR, K, true>(gf, aa, lds, bx, f, ty0, ty1);
    else census_block<NR, K, false>(gf, aa, lds, bx, f, ty0, ty1);
}

template <int NR, int K>
static CostBands launch_census_t(const Geometry& g, CostArgs a, int F, hipStream_t st) {
    using Cfg = CensusCfg<NR, K>;
    const int rows = max(a.row_end - a.row_begin, 0);
    const size_t lds = Cfg::lds_bytes(g.D);
    const int colblocks = (g.W1 + Cfg::BCOLS - 1) / Cfg::BCOLS;
    if (a.TY <= 0) {
        // the tallest row band that fills the chip in one pass of resident blocks (launch_cost_t)
        static thread_local size_t key = 0;
        static thread_local int per_cu = 0;
        if (key != lds) {
            per_cu = 0;
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_cost_census<NR, K>, Cfg::NT, lds);
            key = lds;
        }
        const int slots = max(1, device_cus() * max(1, per_cu));
        const int per_band = max(1, colblocks * F);
        const int avail = max(per_band, slots - a.naux * per_band);
        const int bands = max(1, avail / per_band);
        a.TY = max(4, (rows + bands - 1) / bands);
    }
    if (rows == 0) a.TY = 1;
    dim3 grid(colblocks, (rows + a.TY - 1) / a.TY + a.naux, F);
    hipLaunchKernelGGL((k_cost_census<NR, K>), grid, dim3(Cfg::NT), lds, st, g, a);
    return {a.TY, (rows + a.TY - 1) / a.TY};
}

// SH2 <= 5 and D <= 256 (check_frame refuses the rest under the census cost)
CostBands launch_cost_census(const Geometry& g, const CostArgs& a, const CostChoice& c, int F, hipStream_t st) {
    if (a.row_end <= a.row_begin && a.naux == 0) return {0, 0};
    const int NR = c.nr;
    const bool k2 = c.k == 2;
#define SDR_CENSUS(NRV) \
    case NRV: return k2 ? launch_census_t<NRV, 2>(g, a, F, st) : launch_census_t<NRV, 1>(g, a, F, st);
    switch (NR) {
        SDR_CENSUS(1) SDR_CENSUS(3) SDR_CENSUS(5) SDR_CENSUS(7) SDR_CENSUS(9) SDR_CENSUS(11)
        default: return kNoCostKernel;
    }
#undef SDR_CENSUS
}

}  // namespace sdr
