// sdr_fgs_pcr.hip -- the FGS filter's opt-in solver (SDR_FGS_PCR) and its launcher:
//   k_fgs_pcr   one FGS pass (rows or columns): every line's tridiagonal system solved by parallel
//               cyclic reduction in LDS, both right-hand sides at once, the diagonal carried as the
//               row sum (every term non-negative, ~200x closer to the exact solution than the
//               sequential elimination); contraction off and IEEE division, bit for bit
//               oracle/wls_oracle.c fgs_line_pcr
#include "sdr_fgs.hpp"

#pragma clang fp contract(off)

namespace sdr {

// FGS line solves by parallel cyclic reduction, in the operation order of
// oracle/wls_oracle.c fgs_line_pcr.  A workgroup of T threads (blockDim.x, a multiple of 64, up
// to 1024) owns G lines of n samples of one frame (G = 1 for long lines); equation e = g*n + k of
// the block lives in registers of thread e mod T (slot e / T), so a thread keeps its equations'
// (a, c, e, b, d0, d1) across the log2(n) stages and only publishes what its neighbours read:
//   X[e] = {row sum, 1/b, d0, d1} (one 16-byte LDS word), A[e] = a, Cc[e] = c
// Stage s reads X and A of e - s, X and Cc of e + s (zeros past the line's ends), then every
// equation is rewritten at once.  The published values are double-buffered by stage parity, so
// a stage costs one barrier: a thread can only overwrite a buffer two stages later, after the
// barrier every reader of it has passed.  The chip holds few lines (360 rows or 280 column pairs
// at 640x360), so the block takes as many threads as equations (EPT = 1 up to 1024 samples):
// several waves per SIMD hide the LDS and division latencies of the stage chain.  The images are
// read and written in place in their row-major layout: for rows (lines = rows) a block's loads
// are whole rows, for columns (lines = columns) G adjacent columns per row; loads and stores go
// through LDS with consecutive threads on consecutive addresses.  Weights Cw: same layout as the
// images (Ch for rows, Cv for columns, 0 on each line's last sample).

// DB: the stage buffers double-buffered (48 B of LDS per sample, one barrier per stage), or single
// (24 B per sample, two barriers per stage) for blocks whose 48 B per sample exceed the
// workgroup's LDS (160 KiB on gfx950: past 3413 samples)
// FIN (the last column pass, both right-hand sides): instead of storing the solved A, B back, the
// block writes the filter's outputs for its ROI pixels (wls_value / wls_emit; gw = the geometry)
template <int EPT, bool TWO, bool DB = true, bool FIN = false>
__global__ __launch_bounds__(1024) void k_fgs_pcr(float* U0, float* U1, const float* __restrict__ Cw,
                                                  int w, int h, size_t fstride, int rows, int G,
                                                  float lam, WlsGeom gw = {}, WlsOut wo = {}) {
    extern __shared__ float4 pcr_smem[];
    constexpr int NB = DB ? 2 : 1;
    const int T = blockDim.x;
    const int n = rows ? w : h;
    const int nlines = rows ? h : w;
    const int N = G * n;
    // NB stage buffers: X [NB][N] {row sum, 1/b, d0, d1}, then A [NB][N] (a; the weights during
    // the load), Cc [NB][N] (c)
    float4* X = pcr_smem;
    float* A = (float*)(X + NB * N);
    float* Cc = A + NB * N;
    const int tid = threadIdx.x;
    // consecutive line groups share an XCD: the column pass's G-column blocks of one row band
    // read and write parts of the same cache lines, which then meet in one L2
    const int gx = gridDim.x;
    const int lb = xcd_block(blockIdx.x + gx * blockIdx.y, gx * gridDim.y);
    const int l0 = (lb % gx) * G;
    const size_t fo = (size_t)(lb / gx) * fstride;
    auto addr = [&](int idx, int& g, int& k) -> size_t {
        if (rows) {
            g = idx / n;
            k = idx - g * n;
            return (size_t)(l0 + g) * w + k;
        }
        k = idx / G;
        g = idx - k * G;
        return (size_t)k * w + l0 + g;
    };
    // ---- coalesced load into LDS: weight -> A[e], rhs -> X[e].z/.w ----
    for (int idx = tid; idx < N; idx += T) {
        int g, k;
        const size_t off = addr(idx, g, k);
        const int e = g * n + k;
        float cw = 0.0f, r0 = 0.0f, r1 = 0.0f;
        if (l0 + g < nlines) {
            cw = Cw[fo + off];
            r0 = U0[fo + off];
            if constexpr (TWO) r1 = U1[fo + off];
        }
        A[e] = cw;
        X[e] = make_float4(0.0f, 0.0f, r0, r1);
    }
    __syncthreads();
    float a[EPT], c[EPT], rs[EPT], b[EPT], d0[EPT], d1[EPT];
    int kk[EPT];
#pragma unroll
    for (int j = 0; j < EPT; j++) {
        const int e = tid + j * T;
        kk[j] = 0;
        a[j] = c[j] = 0.0f;
        rs[j] = b[j] = 1.0f;
        d0[j] = d1[j] = 0.0f;
        if (e < N) {
            const int k = e - (e / n) * n;
            kk[j] = k;
            c[j] = lam * A[e];
            a[j] = k > 0 ? lam * A[e - 1] : 0.0f;
            rs[j] = 1.0f;
            b[j] = (1.0f - a[j]) - c[j];
            d0[j] = X[e].z;
            d1[j] = X[e].w;
        }
    }
    __syncthreads();
    int buf = 0;
    for (int s = 1; s < n; s <<= 1, buf ^= DB ? N : 0) {
        float4* Xb = X + buf;
        float* Ab = A + buf;
        float* Cb = Cc + buf;
#pragma unroll
        for (int j = 0; j < EPT; j++) {
            const int e = tid + j * T;
            if (e < N) {
                Xb[e] = make_float4(rs[j], 1.0f / b[j], d0[j], d1[j]);
                Ab[e] = a[j];
                Cb[e] = c[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EPT; j++) {
            // branch-free: all four reads in flight at once, missing neighbours selected to zero
            // (threads past N compute on a clamped equation and never publish)
            const int e = min(tid + j * T, N - 1);
            {
                const bool hm = kk[j] >= s, hp = kk[j] + s < n;
                const int em = hm ? e - s : e, ep = hp ? e + s : e;
                float4 xm = Xb[em], xp = Xb[ep];
                float am = Ab[em], cp = Cb[ep];
                const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (!hm) {
                    xm = z4;
                    am = 0.0f;
                }
                if (!hp) {
                    xp = z4;
                    cp = 0.0f;
                }
                const float k1 = a[j] * xm.y;
                const float k2 = c[j] * xp.y;
                const float na = -(am * k1);
                const float nc = -(cp * k2);
                const float ne = (rs[j] - xm.x * k1) - xp.x * k2;
                b[j] = (ne - na) - nc;
                a[j] = na;
                c[j] = nc;
                rs[j] = ne;
                d0[j] = (d0[j] - xm.z * k1) - xp.z * k2;
                if constexpr (TWO) d1[j] = (d1[j] - xm.w * k1) - xp.w * k2;
            }
        }
        if constexpr (!DB) __syncthreads();  // every read of the one buffer done before the next writes
    }
    // ---- decoupled: u = d / b, staged in LDS (buffer `buf`, untouched since two stages back) for
    // the coalesced store ----
    float4* Xo = X + buf;
#pragma unroll
    for (int j = 0; j < EPT; j++) {
        const int e = tid + j * T;
        if (e < N) Xo[e] = make_float4(0.0f, 0.0f, d0[j] / b[j], TWO ? d1[j] / b[j] : 0.0f);
    }
    __syncthreads();
    for (int idx = tid; idx < N; idx += T) {
        int g, k;
        const size_t off = addr(idx, g, k);
        if (l0 + g >= nlines) continue;
        const float4 x = Xo[g * n + k];
        if constexpr (FIN) {
            // columns pass: line l0 + g is ROI column j, sample k its ROI row i
            wls_emit(wo, gw, lb / gx, gw.rx + l0 + g, gw.ry + k, wls_value(x.z, x.w));
        } else {
            U0[fo + off] = x.z;
            if constexpr (TWO) U1[fo + off] = x.w;
        }
    }
}

// k_fgs_pcr instance for G*n samples per block: one equation per thread up to 1024 samples
// (T = the samples rounded up to whole waves), 2 or 4 per thread of 1024 beyond
template <bool TWO, bool FIN>
static int launch_pcr_as(float* U0, float* U1, const float* Cw, int w, int h, int F, int rows,
                         float lam, hipStream_t st, const WlsGeom& gw, const WlsOut& wo) {
    const int n = rows ? w : h, nlines = rows ? h : w;
    if (n > kPcrMaxN) return -1;
    // short lines: G per block so that a block holds up to 1024 samples
    const int G = pcr_lines(n, nlines);
    const int N = G * n;
    // (one equation per thread: 2 or 4 per thread at 640x360 measured 12.8 -> 15.0 / 16.8 us a pass)
    const int ept = N <= 1024 ? 1 : N <= 2048 ? 2 : 4;
    const int T = std::min(1024, ((N + ept - 1) / ept + 63) / 64 * 64);
    const dim3 grid((nlines + G - 1) / G, F), blk(T);
    const size_t fs = (size_t)w * h;
    // the workgroup's LDS (160 KiB on gfx950) holds double-buffered stages up to 3413 samples
    static thread_local int max_lds = 0;
    if (!max_lds) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
            max_lds <= 0)
            max_lds = 64 * 1024;
    }
    const bool db = (size_t)N * 48 <= (size_t)max_lds;
    if (!db && (size_t)N * 24 > (size_t)max_lds) return -1;
    auto* k = !db ? k_fgs_pcr<4, TWO, false, FIN>
              : ept == 1 ? k_fgs_pcr<1, TWO, true, FIN> : ept == 2 ? k_fgs_pcr<2, TWO, true, FIN> : k_fgs_pcr<4, TWO, true, FIN>;
    hipLaunchKernelGGL(k, grid, blk, (size_t)N * (db ? 48 : 24), st, U0, U1, Cw, w, h, fs, rows, G, lam, gw, wo);
    return 0;
}

int launch_pcr(float* U0, float* U1, const float* Cw, int w, int h, int F, int rows, float lam,
               hipStream_t st, const WlsGeom* fin_g, const WlsOut* fin_o) {
    if (fin_g && fin_o && U1) return launch_pcr_as<true, true>(U0, U1, Cw, w, h, F, rows, lam, st, *fin_g, *fin_o);
    return U1 ? launch_pcr_as<true, false>(U0, U1, Cw, w, h, F, rows, lam, st, {}, {})
              : launch_pcr_as<false, false>(U0, U1, Cw, w, h, F, rows, lam, st, {}, {});
}

}  // namespace sdr

