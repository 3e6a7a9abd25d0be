// sdr_fgs_seq.hip -- the FGS filter's sequential solver (SDR_FGS_THOMAS, the default: ximgproc's
// own elimination order, bit-exact with oracle/wls_oracle.c fgs_line), contraction off:
//   k_fgs_th         one FGS pass, or the coefficient jobs of up to kFgsMaxJobs passes: a chain on
//                    one solver wave a workgroup (lane = line, 16, 32 or 64 lines) fed through an
//                    LDS ring by two loader waves, a writer wave doing every store; any line length
//   k_fgs_lr         one FGS pass of two right-hand sides, its L = 16, 8, 4 or 2 lines resident in
//                    LDS (up to 6 * 1024 / L samples), a solver wave per image, lane = (row, line)
//   k_fgs_lrjob      the coefficient jobs the k_fgs_lr way (L = 16, 8 or 4)
//   k_fgs_rcp_check  fgs_rcp against the IEEE division (sdr_fgs_rcp_selftest)
// and fgs_plan, which names the kernel of every launch of a filter call, with its launchers.
#include "sdr_fgs.hpp"
#include "sdr_internal.hpp"

#include <cstdlib>
#include <string>

#pragma clang fp contract(off)

namespace sdr {

// ---- diagnostic stamps (SDR_TH_STAMPS builds only; results unchanged): the macros the kernels
// call (TH_* in k_fgs_th, LR_STAMP in k_fgs_lr, LJ_STAMP in k_fgs_lrjob; empty in the product
// build), their buffers, the launchers' arming, the readers of scripts/*_stamps.py and th_counts.py
#ifdef SDR_TH_STAMPS
// s_memtime stamps of workgroup (0, 0) of one k_fgs_th launch (scripts/th_stamps.py)
__device__ unsigned long long* g_th_stamps;
#define TH_STAMP(role, idx)                                                                       \
    do {                                                                                          \
        if (g_th_stamps && blockIdx.x == 0 && blockIdx.y == 0 && (threadIdx.x & 63) == 0)         \
            g_th_stamps[(role) * 1024 + (idx)] = __builtin_amdgcn_s_memtime();                    \
    } while (0)
constexpr int kThStampRoles = 6;
__device__ unsigned long long g_th_blk[512][3];  // per workgroup of the stamped launch: start, fwd end, end
#define TH_BLK(i)                                                                                  \
    do {                                                                                           \
        if (g_th_stamps && blockIdx.y == 0 && (threadIdx.x & 63) == 0 && blockIdx.x < 512)         \
            g_th_blk[blockIdx.x][i] = __builtin_amdgcn_s_memtime();                                \
    } while (0)
__device__ unsigned int g_th_counts[4];  // pass chunks: reciprocal form, exact from the start, redone
#define TH_COUNT(i)                                                                                \
    do {                                                                                           \
        if ((threadIdx.x & 63) == 0) atomicAdd(&g_th_counts[i], 1u);                               \
    } while (0)
// k_fgs_lr, per workgroup of the first 512 of each of 16 launch slots (scripts/lr_stamps.py):
// 0 entry, 1 first chunk landed, 2 forward done, 3 back done (solver 0), 4 writer done, 5 solver exit,
// 6 entry s_memrealtime (100 MHz)
__device__ unsigned long long g_lr_blk[16][512][8];
#define LR_STAMP(cond, slot, i)                                                                      \
    do {                                                                                             \
        if ((cond) && (slot) >= 0 && (threadIdx.x & 63) == 0 && blockIdx.x < 512 && blockIdx.y == 0) { \
            g_lr_blk[(slot) & 15][blockIdx.x][i] = __builtin_amdgcn_s_memtime();                     \
            if ((i) == 0) g_lr_blk[(slot) & 15][blockIdx.x][6] = __builtin_amdgcn_s_memrealtime();    \
            if ((i) == 5) g_lr_blk[(slot) & 15][blockIdx.x][7] = __builtin_amdgcn_s_memrealtime();    \
        }                                                                                            \
    } while (0)
// k_fgs_lrjob's per-workgroup stamps of the last launch (frame 0, the first 512 workgroups;
// scripts/lj_stamps.py): 0 entry, 1 chunk 0 prepared (prep), 2 solver past its first barrier,
// 3 solver done, 4 writer 0 done, 5 prep done, 6 / 7 s_memrealtime at 0 / 3
__device__ unsigned long long g_lj_blk[512][8];
#define LJ_STAMP(cond, i)                                                                            \
    do {                                                                                             \
        if ((cond) && (threadIdx.x & 63) == 0 && blockIdx.x < 512 && blockIdx.y == 0) {              \
            g_lj_blk[blockIdx.x][i] = __builtin_amdgcn_s_memtime();                                  \
            if ((i) == 0) g_lj_blk[blockIdx.x][6] = __builtin_amdgcn_s_memrealtime();                 \
            if ((i) == 3) g_lj_blk[blockIdx.x][7] = __builtin_amdgcn_s_memrealtime();                 \
        }                                                                                            \
    } while (0)

// arms TH_STAMP for the k_fgs_th launch SDR_TH_STAMP_LAUNCH names (counted from 0), disarms it for
// every other
static unsigned long long* th_stamp_buf = nullptr;
static void th_stamps_arm(hipStream_t st) {
    static int launches = 0;
    static const int want = getenv("SDR_TH_STAMP_LAUNCH") ? atoi(getenv("SDR_TH_STAMP_LAUNCH")) : -1;
    if (!th_stamp_buf) (void)hipMalloc((void**)&th_stamp_buf, kThStampRoles * 1024 * 8);
    unsigned long long* v = launches++ == want ? th_stamp_buf : nullptr;
    (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_th_stamps), &v, sizeof(v), 0, hipMemcpyHostToDevice, st);
}
// a k_fgs_lr launch's LR_STAMP slot (FgsThArgs::dbg)
static int lr_stamp_slot() { static int slot = 0; return slot++ & 15; }

// the readers; sdr_th_stamps: the stamps of the launch SDR_TH_STAMP_LAUNCH names ([kThStampRoles][1024] u64)
extern "C" {
int sdr_th_stamps(unsigned long long* host) {
    if (!th_stamp_buf) return -1;
    return hipMemcpy(host, th_stamp_buf, kThStampRoles * 1024 * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int sdr_th_blocks(unsigned long long* host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_th_blk), 512 * 3 * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int sdr_th_counts(unsigned int* host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_th_counts), 16, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int sdr_lr_blocks(unsigned long long* host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_lr_blk), 16 * 512 * 8 * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int sdr_lj_blocks(unsigned long long* host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_lj_blk), 512 * 8 * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
}  // extern "C"
#else
#define TH_STAMP(role, idx) \
    do {                    \
    } while (0)
#define TH_COUNT(i) \
    do {            \
    } while (0)
#define TH_BLK(i) \
    do {          \
    } while (0)
#define LR_STAMP(cond, slot, i) \
    do {                        \
    } while (0)
#define LJ_STAMP(cond, i) \
    do {                  \
    } while (0)
static void th_stamps_arm(hipStream_t) {}
static int lr_stamp_slot() { return -1; }
#endif

// ---- k_fgs_th: the sequential pass and coefficient jobs through an LDS ring ------------------
// FGS line solve, per line of n samples with weights C[k] = lut[(g[k] - g[k+1])^2] (0 at the
// last sample):  (1 - lam*(C[k-1] + C[k])) u_k + lam*C[k-1] u_{k-1} + lam*C[k] u_{k+1} = f_k
// (C = -w <= 0), Thomas forward elimination then back substitution, in the oracle's order
// (oracle/wls_oracle.c fgs_line, ximgproc's fgs_filter.cpp sweep):
//   k=0:  den = 1 - lam*C0;  t0 = lam*C0 / den;  u0 = u0 / den
//   k>0:  a = lam*C[k-1];  c = lam*C[k];  den = (1 - c) - a*(1 + t[k-1]);
//         t[k] = c / den;  u_k = (u_k - a*u_{k-1}) / den
//   back: u_k = u_k - t[k]*u_{k+1}
// The elimination coefficients (den, t) depend on the guide's weights and lambda only, not on the
// right-hand sides: one launch of coefficient jobs computes them for every pass of a filter first
// (the t recurrence, ~13 dependent operations a sample with its IEEE division, and 1/den beside
// it), and the passes then run only the right-hand sides' recurrence, with the division x / den
// done from the correctly rounded reciprocal r = 1/den:
//   q0 = x*r,  rem = -fma(q0, den, -x) (exact),  q = fma(rem, r, q0)
// which is the correctly rounded quotient (Markstein's theorem: r within half an ulp of 1/den and
// q0 within an ulp of x/den; den >= 1 here) as long as nothing underflows: for 0 < |q0| < 2^-96 a
// chunk runs again with real divisions; scripts/markstein_check.c finds no difference at or above
// that threshold in 2e9 random pairs (den up to 2^60).  Five dependent operations a sample.
//
// A pass of F frames x nl lines runs as a chain on one wave per workgroup (lane = line, LPB = 16,
// 32 or 64 lines a workgroup), which touches nothing but LDS, with three helper waves:
//   wave 0    the solver: the recurrence of its LPB lines sample by sample, each sample's operands
//             read from the LDS ring kThPF samples ahead (ds_read latency off the chain), each
//             result written to an LDS row for the writer
//   waves 1-2 loaders: LDS-DMA (global_load_lds_dwordx4, 1 KiB a wave-instruction) of the next
//             chunks (CH = 1024 / LPB samples x LPB lines of every operand stream) into a ring of
//             kThNB buffers, up to kThNB - 2 chunks in flight
//   wave 3    the writer: every global store of the pass -- the forward values (k-major, in place)
//             and the results (line-major: the next pass's k-major layout, the transpose between
//             passes done by reading the rows transposed; or k-major into the two outputs)
// One s_barrier per chunk orders them: chunk c + 2 has landed (loaders' counted vmcnt), the solver
// is done with chunk c - 1's buffer and has written chunk c's rows before the barrier that ends
// iteration c.  Measured at 640x360 (a 560x360 ROI, two right-hand sides): 64 lines a workgroup
// with the solver storing its own results, 96 us a pass; 16 lines, 77 us; 16 lines with the
// stores on the writer wave, 39 us (the solver's stores queued behind the loaders' DMA in the
// CU's memory pipeline: a variant without them ran 45 us at 77).
// Layout: every k-major array (element (line l, sample k) at k * st + l, st = nl rounded up to 4)
// has 16-byte aligned sample rows, which the 16-byte DMA needs; the frames are fs apart.
constexpr int kThNB = 5;          // LDS ring buffers
constexpr int kThPF = 8;          // the solver's LDS lookahead (samples)
constexpr int kThBuf = 1024 * 24; // a chunk (1024 line-samples) of the largest stream set
template <int LPB, int ES> struct ThRows {
    // the solver's back-substitution rows: CH samples x LPB lines, double-buffered; the row stride
    // S (dwords) is = E * LPB / 16 (mod 64), so that the writer's transposed reads (CH samples of
    // 64 / CH lines a wave-instruction) fall on distinct banks
    static constexpr int CH = 1024 / LPB, E = ES / 4;
    static constexpr int S = LPB * E + (64 - (LPB * E) % 64) % 64 + E * LPB / 16;
    static constexpr int bytes = 2 * CH * S * 4;
};
constexpr int kThRows = ThRows<16, 8>::bytes;  // the rows area (the largest use)
constexpr int kThLds = kThNB * kThBuf + kThRows;
static_assert(ThRows<32, 8>::bytes <= kThRows && ThRows<64, 8>::bytes <= kThRows, "rows");
static_assert(kThRows >= 2 * 1024 * 16, "the forward and job rows fit the rows area");
// two flag words (chunk parity) in the rows area's last bytes -- padding of the back substitution's
// last row, clear of the job rows: a job chunk to run with IEEE divisions
constexpr int kThFlags = kThRows - 16;

static_assert(2 * 1024 * 16 <= kThFlags && ThRows<16, 8>::S * 4 - 16 >= 16 * 8, "flags in the rows' padding");
static_assert(kThLds <= 160 * 1024, "one workgroup's LDS");
constexpr uint32_t kFgsTinyKey = 0x1EFFFFFFu;  // fgs_tiny_key(q) < this <=> 0 < |q| < 2^-96

// The correctly rounded 1/d for 1 <= d < 2^126: v_rcp_f32 and one Newton step, equal to the IEEE
// quotient 1.0f / d for every mantissa of d at every exponent checked (sdr_fgs_rcp_selftest,
// tests/test_gpu_wls.py; at 2^126 and beyond 1/d is subnormal and it is not) -- 3 operations
// instead of the IEEE division's ~11.  Every pivot is at most 1 + 2 * lambda, hence
// kFgsThomasMaxLambda.
__device__ __forceinline__ float fgs_rcp(float d) {
    const float r0 = __builtin_amdgcn_rcpf(d);
    return __builtin_fmaf(__builtin_fmaf(-d, r0, 1.0f), r0, r0);
}

// 2|q| - 1 as an integer (the sign bit shifted out): below kFgsTinyKey exactly when 0 < |q| < 2^-96
// (+-0 wraps to the largest key); the minimum over a chunk decides the redo
__device__ __forceinline__ uint32_t fgs_tiny_key(float q) { return __builtin_bit_cast(uint32_t, q) * 2u - 1u; }

template <bool TWO> struct FgsRhs;
template <> struct FgsRhs<true> {
    typedef float2 T;
    static __device__ __forceinline__ float x(const T& v) { return v.x; }
    static __device__ __forceinline__ float y(const T& v) { return v.y; }
    static __device__ __forceinline__ T make(float a, float b) { return make_float2(a, b); }
};
template <> struct FgsRhs<false> {
    typedef float T;
    static __device__ __forceinline__ float x(const T& v) { return v; }
    static __device__ __forceinline__ float y(const T&) { return 0.0f; }
    static __device__ __forceinline__ T make(float a, float) { return a; }
};

typedef __attribute__((address_space(3))) void* th_lds_ptr;
typedef __attribute__((address_space(1))) void* th_glb_ptr;

// s_waitcnt vmcnt(N) alone (gfx9 encoding: vmcnt [3:0] + [15:14], expcnt [6:4], lgkmcnt [11:8])
template <int N> __device__ __forceinline__ void th_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}
// s_waitcnt lgkmcnt(0) alone: the solver's LDS rows are written before the barrier
__device__ __forceinline__ void th_lgkm0() { __builtin_amdgcn_s_waitcnt(15 | (3 << 14) | (7 << 4)); }
// the workgroup barrier without the fence __syncthreads() carries (whose vmcnt(0) would drain the
// loaders' DMA in flight); the empty asm keeps the compiler from moving LDS accesses across it
__device__ __forceinline__ void th_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// A loader wave's share (lw = 0, 1) of one stream's chunk image: CH = 1024 / LPB sample rows of
// LPB lines x ES bytes, ES wave-instructions of 1 KiB, the wave taking every other one.  Slot j
// holds sample k0 + dk * j (clamped into the line: the slots past its end are never read).
template <int LPB, int ES>
__device__ __forceinline__ void th_issue(const char* g, size_t st, int l0, int k0, int dk, int last, char* img,
                                         int lw, int lane) {
    constexpr int SB = LPB * ES;  // bytes of a slot
    static_assert(ES % 2 == 0 && SB % 16 == 0, "two loader waves, whole pieces");
#pragma unroll
    for (int q = 0; q < ES / 2; q++) {
        const int ii = 2 * q + lw;  // wave-uniform
        const int off = ii * 1024 + lane * 16;
        const int j = off / SB, b = off - j * SB;
        const int k = min(max(k0 + dk * j, 0), last);
        const char* src = g + ((size_t)k * st + l0) * ES + b;
        __builtin_amdgcn_global_load_lds((th_glb_ptr)src, (th_lds_ptr)(img + ii * 1024), 16, 0, 0);
    }
}

// waits until at most m of the wave's younger chunks (IW instructions each) are in flight
template <int IW> __device__ __forceinline__ void th_wait_chunks(int m) {
    static_assert(kThNB == 5, "m <= kThNB - 3");
    if (m >= 2) th_vmcnt<2 * IW>();
    else if (m == 1) th_vmcnt<IW>();
    else th_vmcnt<0>();
}

// A loader wave over one phase of nch chunks (chunk c = samples k0 + dk * (c * CH + j)): chunks
// 0 .. kThNB-2 ahead, then per iteration c chunk c + kThNB - 1 into the buffer chunk c - 1 left,
// and chunk c + 2 landed before the barrier; 1 + extra + nch barriers, as every wave of the phase.
// (not inlined: with the loaders' DMA in the kernel body the compiler's wait analysis, merging
// paths, put a vmcnt(0) before LDS writes of the other waves' code -- every row of a job)
template <int LPB, int ES0, int ES1>
__device__ __noinline__ void th_load_phase(const char* g0, const char* g1, size_t st, int l0, int k0, int dk,
                                              int last, int nch, char* lds, int lw, int lane, int extra = 0) {
    constexpr int CH = 1024 / LPB, IW = (ES0 + ES1) / 2;
    auto issue = [&](int c) __attribute__((always_inline)) {
        char* buf = lds + (c % kThNB) * kThBuf;
        th_issue<LPB, ES0>(g0, st, l0, k0 + dk * c * CH, dk, last, buf, lw, lane);
        if constexpr (ES1 > 0) th_issue<LPB, ES1>(g1, st, l0, k0 + dk * c * CH, dk, last, buf + 1024 * ES0, lw, lane);
    };
    const int pre = min(kThNB - 1, nch);
    for (int c = 0; c < pre; c++) issue(c);
    th_wait_chunks<IW>(pre - 2);
    th_barrier();
    for (int i = 0; i < extra; i++) th_barrier();  // (a job's flag barrier)
    for (int c = 0; c < nch; c++) {
        if (c + kThNB - 1 < nch) issue(c + kThNB - 1);
        if (lw == 0) TH_STAMP(2, (dk < 0 ? 512 : 0) + c);
        th_wait_chunks<IW>(min(c + kThNB - 1, nch - 1) - (c + 2));
        if (lw == 0) TH_STAMP(3, (dk < 0 ? 512 : 0) + c);
        th_barrier();
    }
}

// The writer wave: the solver's rows of chunk c (double-buffered by chunk parity) go to memory
// during iteration c + 1, the last chunk's after the phase's final barrier.
//   fwd:  row j = sample c * CH + j of the forward values, k-major in place (a row = the block's
//         LPB lines, contiguous); all in memory (vmcnt(0)) before the barrier that ends the phase,
//         since the back substitution's loaders read them
//   back: row j = sample kb - j, kb = last - 1 - c * CH, in the padded ThRows layout: line-major
//         into O (a wave-instruction: CH consecutive samples of 64 / CH lines) or k-major split
//         into O0 / O1 (the last pass)
//   job:  row j = (a, den, 1/den, t) of sample c * CH + j -> coef and tt, k-major
template <bool TWO, int LPB>
__device__ __forceinline__ void th_write_fwd_phase(void* U, size_t st, size_t fofs, int l0, int nl, int last, int nch,
                                                   const char* orow, int lane) {
    typedef typename FgsRhs<TWO>::T V;
    constexpr int ES = TWO ? 8 : 4, CH = 1024 / LPB;
    const int line = lane % LPB;
    const bool lv = l0 + line < nl;
    V* u = (V*)U + fofs + l0 + line;
    auto put = [&](int c) __attribute__((always_inline)) {
        const char* rows = orow + (c & 1) * 1024 * ES;
#pragma unroll 4
        for (int it = 0; it < 16; it++) {
            const int jj = it * (64 / LPB) + lane / LPB;
            const int k = c * CH + jj;
            if (lv && k <= last) u[(size_t)k * st] = *(const V*)(rows + (jj * LPB + line) * ES);
        }
    };
    th_barrier();
    for (int c = 0; c < nch; c++) {
        if (c > 0) put(c - 1);
        TH_STAMP(4, c);
        th_barrier();
    }
    if (nch > 0) put(nch - 1);
    th_vmcnt<0>();
}

template <bool TWO, int LPB>
__device__ __forceinline__ void th_write_back_phase(const FgsThArgs& a, size_t fofs, int l0, int last, int nch,
                                                    const char* orow, int lane) {
    typedef typename FgsRhs<TWO>::T V;
    constexpr int ES = TWO ? 8 : 4;
    typedef ThRows<LPB, ES> RW;
    constexpr int CH = RW::CH;
    auto put = [&](int c) __attribute__((always_inline)) {
        const char* rows = orow + (c & 1) * CH * RW::S * 4;
        const int kb = last - 1 - c * CH;
        if (a.O) {
            const int cnt = min(CH, kb + 1), kmin = kb - cnt + 1;
            const int s = lane % CH;
#pragma unroll 4
            for (int it = 0; it < 16; it++) {
                const int line = it * (64 / CH) + lane / CH;
                if (s < cnt && l0 + line < a.nl) {
                    const int k = kmin + s;
                    const V v = *(const V*)(rows + (kb - k) * RW::S * 4 + line * ES);
                    ((V*)a.O)[fofs + (size_t)(l0 + line) * a.onp + k] = v;
                }
            }
        } else {
            const int line = lane % LPB;
            const size_t fo = (size_t)blockIdx.y * a.ofs + l0 + line;
#pragma unroll 4
            for (int it = 0; it < 16; it++) {
                const int jj = it * (64 / LPB) + lane / LPB;
                const int k = kb - jj;
                if (k >= 0 && l0 + line < a.nl) {
                    const V v = *(const V*)(rows + jj * RW::S * 4 + line * ES);
                    a.O0[fo + (size_t)k * a.ost] = FgsRhs<TWO>::x(v);
                    if constexpr (TWO) a.O1[fo + (size_t)k * a.ost] = FgsRhs<TWO>::y(v);
                }
            }
        }
    };
    th_barrier();
    for (int c = 0; c < nch; c++) {
        if (c > 0) put(c - 1);
        th_barrier();
    }
    if (nch > 0) put(nch - 1);
}

// A coefficient job.  Its pivots' reciprocal is fgs_rcp and t = cc / den comes from it
// (Markstein) -- exact unless cc / den can fall below ~2^-96, which happens only when cc = lam * C
// is tiny (the weights of gray-level steps of ~80 and more at sigma 1.1).  The writer flags each
// chunk holding such a weight on any of the workgroup's lines (kThFlags in LDS, one word per
// chunk parity; chunk c + 1's during iteration c, chunk 0's between two prologue barriers) and the
// solver runs a flagged chunk with IEEE divisions, a clean one with no per-sample test or branch
// (a branch a sample cost more than the divisions it saved: 63 us a 560-sample job launch on a
// noise guide, 48 on a scene).

template <int LPB>
__device__ __forceinline__ void th_write_job_phase(const FgsCoefJob& J, size_t fofs, int l0, int nch, const char* lds,
                                                   char* orow, int lane) {
    constexpr int CH = 1024 / LPB;
    const int line = lane % LPB, last = J.n - 1;
    const bool lv = l0 + line < J.nl;
    float4* co = J.coef + fofs + l0 + line;
    float* tt = J.tt + fofs + l0 + line;
    const size_t st = (size_t)J.st;
    const float lam = J.lam, tiny = 0x1p-96f * (1.0f + 2.0f * lam);
    auto put = [&](int c) __attribute__((always_inline)) {
        const char* rows = orow + (c & 1) * 1024 * 16;
#pragma unroll 4
        for (int it = 0; it < 16; it++) {
            const int jj = it * (64 / LPB) + lane / LPB;
            const int k = c * CH + jj;
            if (lv && k <= last) {
                const float4 v = *(const float4*)(rows + (jj * LPB + line) * 16);
                co[(size_t)k * st] = v;
                tt[(size_t)k * st] = v.w;
            }
        }
    };
    // chunk c's weights (1024 floats, 16 a lane): any tiny lam * C on a real line and sample
    auto flag = [&](int c) __attribute__((always_inline)) {
        const float* cw = (const float*)(lds + (c % kThNB) * kThBuf);
        bool t = false;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e0 = (q * 64 + lane) * 4;  // element j * LPB + l
            const float4 v = *(const float4*)(cw + e0);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float x = lam * (&v.x)[e];
                const int el = e0 + e, j = el / LPB, l = el % LPB;
                t = t || (fabsf(x) < tiny && x != 0.0f && c * CH + j <= last && l0 + l < J.nl);
            }
        }
        // (the vote before the branch: inside it only lane 0 would take part, and the flag would
        // see 16 of the chunk's 1024 weights)
        const bool any = __builtin_amdgcn_ballot_w64(t) != 0;
        if (lane == 0) *(int*)(orow + kThFlags + (c & 1) * 4) = any;
    };
    th_barrier();
    if (nch > 0) flag(0);
    th_lgkm0();
    th_barrier();
    for (int c = 0; c < nch; c++) {
        if (c > 0) put(c - 1);
        if (c + 1 < nch) flag(c + 1);
        th_lgkm0();
        th_barrier();
    }
    if (nch > 0) put(nch - 1);
}

// a coefficient job's LPB lines on the solver wave: the t recurrence; (a, den, 1/den, t) per
// sample into the writer's rows
template <int LPB>
__device__ __forceinline__ void th_job_solver(const FgsCoefJob& J, int l0, int lane, const char* lds, char* orow) {
    constexpr int CH = 1024 / LPB;
    const int ln = lane & (LPB - 1);
    const int last = J.n - 1, nch = (J.n + CH - 1) / CH;
    const float lam = J.lam;
    float rc[kThPF];
    th_barrier();
    th_barrier();  // (chunk 0's flag)
#pragma unroll
    for (int j = 0; j < kThPF; j++) rc[j] = *(const float*)(lds + (j * LPB + ln) * 4);
    float cprev = 0.0f, tprev = 0.0f;
    for (int c = 0; c < nch; c++) {
        const char* cur = lds + (c % kThNB) * kThBuf;
        const char* nxt = lds + ((c + 1) % kThNB) * kThBuf;
        const int kc = c * CH;
        char* w = orow + (c & 1) * 1024 * 16 + ln * 16;
        TH_STAMP(0, c);
        // a chunk with a tiny weight divides (IEEE), a clean one takes the reciprocal form
        auto body = [&](auto guard, auto exact) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < CH; j++) {
                if (j % 16 == 0) TH_STAMP(5, c * 8 + j / 16);
                const float cw = rc[j % kThPF];
                const int jn = j + kThPF;
                rc[j % kThPF] = jn < CH ? *(const float*)(cur + (jn * LPB + ln) * 4)
                                        : *(const float*)(nxt + ((jn - CH) * LPB + ln) * 4);
                if (!decltype(guard)::value || kc + j <= last) {
                    const float aa = lam * cprev;
                    const float cc = lam * cw;
                    const float den = (1.0f - cc) - aa * (1.0f + tprev);
                    const float r = fgs_rcp(den);
                    if constexpr (decltype(exact)::value) {
                        tprev = cc / den;
                    } else {
                        const float q0 = cc * r;
                        tprev = __builtin_fmaf(-__builtin_fmaf(q0, den, -cc), r, q0);  // cc / den
                    }
                    *(float4*)(w + j * LPB * 16) = make_float4(aa, den, r, tprev);
                    cprev = cw;
                }
            }
        };
        const bool full = kc + CH - 1 <= last;
        if (*(const volatile int*)(orow + kThFlags + (c & 1) * 4)) {
            if (full) body(std::false_type{}, std::true_type{});
            else body(std::true_type{}, std::true_type{});
        } else {
            if (full) body(std::false_type{}, std::false_type{});
            else body(std::true_type{}, std::false_type{});
        }
        TH_STAMP(1, c);
        th_lgkm0();
        th_barrier();
    }
}

// The solver wave of one pass: forward elimination (streams U and (a, den, 1/den, t)), then the
// back substitution (streams U -- the forward values -- and t); every result into the writer's
// LDS rows.
template <bool TWO, int LPB>
__device__ __forceinline__ void th_pass_solver(const FgsThArgs& a, size_t fofs, int l0, int lane, const char* lds,
                                               char* orow) {
    typedef FgsRhs<TWO> R;
    typedef typename R::T V;
    constexpr int ESU = TWO ? 8 : 4;
    constexpr int CH = 1024 / LPB;
    constexpr int S1 = 1024 * ESU;  // stream 1's offset in a chunk buffer
    typedef ThRows<LPB, ESU> RW;
    const int ln = lane & (LPB - 1);
    const int l = l0 + ln;
    const bool valid = lane < LPB && l < a.nl;
    const int n = a.n, last = n - 1;
    const int nch = (n + CH - 1) / CH;
    auto rdu = [&](const char* buf, int j) __attribute__((always_inline)) {
        return *(const V*)(buf + (j * LPB + ln) * ESU);
    };
    auto rdq = [&](const char* buf, int j) __attribute__((always_inline)) {
        return *(const float4*)(buf + S1 + (j * LPB + ln) * 16);
    };
    // ---- forward elimination ----
    TH_BLK(0);
    V ru[kThPF];
    float4 rq[kThPF];
    auto rd = [&](const char* buf, int j, int r) __attribute__((always_inline)) {
        ru[r] = rdu(buf, j);
        rq[r] = rdq(buf, j);
    };
    th_barrier();
#pragma unroll
    for (int j = 0; j < kThPF; j++) rd(lds, j, j);
    float p0 = 0.0f, p1 = 0.0f;
    for (int c = 0; c < nch; c++) {
        const char* cur = lds + (c % kThNB) * kThBuf;
        const char* nxt = lds + ((c + 1) % kThNB) * kThBuf;
        const int kc = c * CH;
        char* wu = orow + (c & 1) * 1024 * ESU + ln * ESU;  // this chunk's rows
        TH_STAMP(0, c);
        const float ps0 = p0, ps1 = p1;
        uint32_t key = 0xffffffffu;
        // exact: IEEE divisions (the right-hand sides decayed into the range the reciprocal form
        // does not cover: long runs of zero confidence); otherwise the reciprocal form with the
        // tiny-quotient key
        auto body = [&](auto guard, auto exact) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < CH; j++) {
                if (j % 16 == 0) TH_STAMP(5, c * 8 + j / 16);
                const int r = j % kThPF;
                const V xu = ru[r];
                const float4 xq = rq[r];  // a, den, 1/den, t
                const int jn = j + kThPF;
                if (jn < CH) rd(cur, jn, r);
                else rd(nxt, jn - CH, r);
                if (!decltype(guard)::value || kc + j <= last) {
                    const float x0 = R::x(xu) - xq.x * p0;
                    const float x1 = TWO ? R::y(xu) - xq.x * p1 : 0.0f;
                    if constexpr (decltype(exact)::value) {
                        p0 = x0 / xq.y;
                        if constexpr (TWO) p1 = x1 / xq.y;
                    } else {
                        const float q00 = x0 * xq.z;
                        p0 = __builtin_fmaf(-__builtin_fmaf(q00, xq.y, -x0), xq.z, q00);
                        key = min(key, fgs_tiny_key(q00));
                        if constexpr (TWO) {
                            const float q01 = x1 * xq.z;
                            p1 = __builtin_fmaf(-__builtin_fmaf(q01, xq.y, -x1), xq.z, q01);
                            key = min(key, fgs_tiny_key(q01));
                        }
                    }
                    *(V*)(wu + j * LPB * ESU) = R::make(p0, p1);
                }
            }
        };
        const bool full = kc + CH - 1 <= last;
        // a chunk starting from values already small (|p| < 2^-64) is likely to decay through the
        // uncovered range: it divides from the start
        const uint32_t small = 0x3EFFFFFFu;  // fgs_tiny_key(q) < small <=> 0 < |q| < 2^-64
        if (__builtin_amdgcn_ballot_w64(valid && (fgs_tiny_key(p0) < small || (TWO && fgs_tiny_key(p1) < small)))) {
            TH_COUNT(1);
            if (full) body(std::false_type{}, std::true_type{});
            else body(std::true_type{}, std::true_type{});
        } else {
            if (full) body(std::false_type{}, std::false_type{});
            else body(std::true_type{}, std::false_type{});
            // a chunk with a quotient the reciprocal form does not cover runs again from its start
            // with real divisions, its rows overwriting the first run's (the chunk's buffer is
            // intact until the barrier; the operand ring restarts at its first slots)
            TH_COUNT(0);
            if (__builtin_amdgcn_ballot_w64(valid && key < kFgsTinyKey)) {
                TH_COUNT(2);
                p0 = ps0;
                p1 = ps1;
#pragma unroll
                for (int j = 0; j < kThPF; j++) rd(cur, j, j);
                if (full) body(std::false_type{}, std::true_type{});
                else body(std::true_type{}, std::true_type{});
            }
        }
        TH_STAMP(1, c);
        th_lgkm0();
        th_barrier();
    }
    // (the writer has the forward values in memory before this barrier)
    TH_BLK(1);
    th_barrier();
    // ---- back substitution: u_k -= t[k] * u_{k+1}, k = n-2 .. 0 (the last sample keeps p) ----
    if (valid) {
        if (a.O) ((V*)a.O)[fofs + (size_t)l * a.onp + last] = R::make(p0, p1);
        else {
            a.O0[(size_t)blockIdx.y * a.ofs + (size_t)last * a.ost + l] = p0;
            if constexpr (TWO) a.O1[(size_t)blockIdx.y * a.ofs + (size_t)last * a.ost + l] = p1;
        }
    }
    const int nchb = (last + CH - 1) / CH;
    float q0 = p0, q1 = p1;
    V bu[kThPF];
    float bt[kThPF];
    auto rdb = [&](const char* buf, int j, int r) __attribute__((always_inline)) {
        bu[r] = rdu(buf, j);
        bt[r] = *(const float*)(buf + S1 + (j * LPB + ln) * 4);
    };
    th_barrier();
#pragma unroll
    for (int j = 0; j < kThPF; j++) rdb(lds, j, j);
    for (int c = 0; c < nchb; c++) {
        const char* cur = lds + (c % kThNB) * kThBuf;
        const char* nxt = lds + ((c + 1) % kThNB) * kThBuf;
        char* rows = orow + (c & 1) * CH * RW::S * 4 + ln * ESU;
        const int kb = last - 1 - c * CH;
        TH_STAMP(0, 512 + c);
        auto body = [&](auto guard) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < CH; j++) {
                const int r = j % kThPF;
                const V xu = bu[r];
                const float xt = bt[r];
                const int jn = j + kThPF;
                if (jn < CH) rdb(cur, jn, r);
                else rdb(nxt, jn - CH, r);
                if (!decltype(guard)::value || kb - j >= 0) {
                    q0 = R::x(xu) - xt * q0;
                    if constexpr (TWO) q1 = R::y(xu) - xt * q1;
                    *(V*)(rows + j * RW::S * 4) = R::make(q0, q1);
                }
            }
        };
        if (kb - CH + 1 >= 0) body(std::false_type{});
        else body(std::true_type{});
        TH_STAMP(1, 512 + c);
        th_lgkm0();
        th_barrier();
    }
    TH_BLK(2);
}

// One FGS pass (all lines of F frames) in ximgproc's order from its jobs' coefficients; blocks
// past main_blocks run coefficient jobs (a.job) instead (a launch of jobs alone: main_blocks = 0).
// 256 threads: solver, two loaders, writer.
template <bool TWO, int LPB>
__global__ __launch_bounds__(256) void k_fgs_th(FgsThArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[kThLds];
    char* orow = lds + kThNB * kThBuf;
    constexpr int CH = 1024 / LPB;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const size_t fofs = (size_t)blockIdx.y * a.fs;
    const int blk = blockIdx.x;
    if (blk >= a.main_blocks) {
        int jb = blk - a.main_blocks, j = 0;
        while (j < a.njobs && jb >= a.job[j].blocks) jb -= a.job[j++].blocks;
        if (j >= a.njobs) return;  // uniform over the workgroup
        const FgsCoefJob& J = a.job[j];
        const int l0 = jb * LPB, nch = (J.n + CH - 1) / CH;
        if (wave == 0) th_job_solver<LPB>(J, l0, lane, lds, orow);
        else if (wave <= 2)
            th_load_phase<LPB, 4, 0>((const char*)(J.Cw + fofs), nullptr, J.st, l0, 0, 1, J.n - 1, nch, lds,
                                     wave - 1, lane, 1);
        else th_write_job_phase<LPB>(J, fofs, l0, nch, lds, orow, lane);
        return;
    }
    constexpr int ESU = TWO ? 8 : 4;
    const int l0 = blk * LPB, n = a.n, last = n - 1;
    const int nch = (n + CH - 1) / CH, nchb = (last + CH - 1) / CH;
    const char* gu = (const char*)a.U + fofs * ESU;
    if (wave == 0) {
        th_pass_solver<TWO, LPB>(a, fofs, l0, lane, lds, orow);
    } else if (wave <= 2) {
        const int lw = wave - 1;
        th_load_phase<LPB, ESU, 16>(gu, (const char*)(a.coef + fofs), a.st, l0, 0, 1, last, nch, lds, lw, lane);
        th_barrier();
        th_load_phase<LPB, ESU, 4>(gu, (const char*)(a.tt + fofs), a.st, l0, last - 1, -1, last, nchb, lds, lw, lane);
    } else {
        th_write_fwd_phase<TWO, LPB>(a.U, a.st, fofs, l0, a.nl, last, nch, orow, lane);
        th_barrier();
        th_write_back_phase<TWO, LPB>(a, fofs, l0, last, nchb, orow, lane);
    }
}

// ---- k_fgs_lr: the sequential pass with its lines resident in LDS (round 6) ----------------
// The same recurrences, operations and roundings as k_fgs_th (ximgproc's order, bit-exact), for
// both right-hand sides at once, rebuilt around what bounds a one-wave chain: every instruction
// the chain's wave issues is on the critical path (a dependent f32 op takes ~4.9 cycles, the
// issue of the next about 4: nothing hides behind the chain), so the pass time is the solver
// wave's instruction count per sample times the line length (scripts/probe/fgs_rows.hip).
//  * one solver wave PER IMAGE (waves 0 and 1, on two SIMDs): scalar chains, 5 dependent ops a
//    forward sample and 2 a back sample (the packed form issues at 8 cycles an op: no gain);
//  * lane = (row, line): L <= 16 lines on the 16 lanes of each 16-lane row, and the four rows hold
//    four consecutive samples each of a 16-sample group, so ONE LDS instruction reads or writes
//    4 samples x L lines; the chain value walks the rows 0 -> 1 -> 3 -> 2 (one v_permlane16/32_swap
//    per row change, every 4 samples), every row computing every step (the issue cost is the
//    wave's whatever the rows), each row keeping its own steps' results (selected per lane at the
//    group's end: no exec masks);
//  * the whole line stays in LDS: the loader waves (2 and 3) DMA the pass's input U and its
//    coefficients (a, den, 1/den, t) once, a chunk of 1024 line-samples at a time, up to
//    kLrAhead chunks ahead; the forward values overwrite U in place and the back substitution
//    reads them from there (no global round trip between the two phases, no buffer reuse), its
//    results overwrite them again and the same two waves store them to global memory a chunk
//    behind the solvers;
//  * the reciprocal-form division with the tiny-quotient key per 16-sample group; a group whose
//    key trips runs again from its start with IEEE divisions (its operands are still in
//    registers), and a group starting from an already small value (|p| < 2^-64) divides from the
//    start (the same rule as k_fgs_th's chunks, per 16 samples instead of per chunk).
// LDS: [U: kLrChunks x 8 KiB][coef: kLrChunks x 16 KiB], sample k of line l at (k * L + l): a line
// of up to kLrChunks * 1024 / L samples (L = 16: 384, 8: 768, 4: 1536, 2: 3072).  Longer lines
// take k_fgs_th.
constexpr int kLrChunks = 6;
constexpr int kLrU = kLrChunks * 8192, kLrLds = kLrChunks * 24576;
constexpr int kLrAhead = 4;  // chunks in flight (th_wait_chunks waits for at most 2 beyond)
static_assert(kLrAhead - 2 <= kThNB - 3, "th_wait_chunks' range");

// the chain value from one lane row to the next in the walk 0 -> 1 -> 3 -> 2 -> 0: the swap of p
// with itself keeps the source row's value where it was AND copies it into the next row, so the
// result is both the step's kept value (for the source row) and the next row's chain input
__device__ __forceinline__ float lr_row(int step, float p) {
    const int b = __builtin_bit_cast(int, p);
    if (step == 0) return __builtin_bit_cast(float, (int)__builtin_amdgcn_permlane16_swap(b, b, false, false)[0]);
    if (step == 1) return __builtin_bit_cast(float, (int)__builtin_amdgcn_permlane32_swap(b, b, false, false)[0]);
    if (step == 2) return __builtin_bit_cast(float, (int)__builtin_amdgcn_permlane16_swap(b, b, false, false)[1]);
    return __builtin_bit_cast(float, (int)__builtin_amdgcn_permlane32_swap(b, b, false, false)[1]);
}

// a lane's own row's value among the walk's four steps (rows 0, 1, 3, 2 take steps 0, 1, 2, 3)
template <typename T>
__device__ __forceinline__ T lr_own(const T (&v)[4], bool s0, bool s1, bool s2) {
    return s0 ? v[0] : s1 ? v[1] : s2 ? v[2] : v[3];
}

struct LrFwdOps {
    float4 q[4];  // (a, den, 1/den, t) of the lane's 4 samples
    float x[4];   // the right-hand side
};
struct LrBackOps {
    float t[4];
    float x[4];  // the forward values
};

template <int L>
struct LrLane {
    int l, step;     // line within the workgroup, the walk step of the lane's row
    bool s0, s1, s2;  // step == 0, 1, 2
    bool valid;       // a real line (l < L and inside the pass)
    int img4;         // 4 * image (the float2 half)
};

// forward group: samples k0 .. k0 + 15 (k0 = 16 g); lane row of walk step s holds k0 + 4 s + e.
// The reciprocal form keeps per walk step the tiny-quotient key of its row's steps (kk[s]: each
// row's own is selected after the group).
template <bool EXACT, bool GUARD>
__device__ __forceinline__ void lr_fwd_body(float& p, const LrFwdOps& o, int k0, int n, float (&res)[4][4],
                                            uint32_t (&kk)[4]) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
        if constexpr (!EXACT) kk[s] = 0xffffffffu;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (!GUARD || k0 + 4 * s + e < n) {
                const float x = o.x[e] - o.q[e].x * p;
                if constexpr (EXACT) {
                    p = x / o.q[e].y;
                } else {
                    const float q0 = x * o.q[e].z;
                    p = __builtin_fmaf(-__builtin_fmaf(q0, o.q[e].y, -x), o.q[e].z, q0);
                    kk[s] = min(kk[s], fgs_tiny_key(q0));
                }
            }
            if (e < 3) res[s][e] = p;
        }
        p = lr_row(s, p);  // keeps the row's value and hands it to the next row
        res[s][3] = p;
    }
}

// The group with the reciprocal form, or with IEEE divisions when it starts from an already small
// value (0 < |p| < 2^-64: a decaying run of zero right-hand sides) or when a quotient came out
// 0 < |q0| < 2^-96 (outside what the reciprocal form covers, scripts/markstein_check.c): then
// again from the group's start value.  k_fgs_th's rules, per 16 samples.
template <int L, bool GUARD>
__device__ __forceinline__ void lr_fwd_group(float& p, const LrFwdOps& o, const LrLane<L>& ln, int k0, int n,
                                             char* uw) {
    float res[4][4];
    uint32_t kk[4];
    const float ps = p;  // (valid in row 0, where the walk starts)
    const uint32_t small = 0x3EFFFFFFu;  // fgs_tiny_key(p) < small <=> 0 < |p| < 2^-64
    bool exact = __builtin_amdgcn_ballot_w64(ln.valid & ln.s0 & (fgs_tiny_key(p) < small)) != 0;
    if (!exact) {
        lr_fwd_body<false, GUARD>(p, o, k0, n, res, kk);
        exact = __builtin_amdgcn_ballot_w64(ln.valid & (lr_own(kk, ln.s0, ln.s1, ln.s2) < kFgsTinyKey)) != 0;
        if (exact) p = ps;
    }
    if (exact) lr_fwd_body<true, GUARD>(p, o, k0, n, res, kk);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float v[4] = {res[0][e], res[1][e], res[2][e], res[3][e]};
        if (!GUARD || k0 + 4 * ln.step + e < n) *(float*)(uw + e * L * 8) = lr_own(v, ln.s0, ln.s1, ln.s2);
    }
}

// back group: samples k1 .. k1 - 15 (k1 = n - 1 - 16 gb); lane row of walk step s holds
// k1 - 4 s - e; the line's last sample keeps its forward value
template <int L, bool GUARD>
__device__ __forceinline__ void lr_back_group(float& p, const LrBackOps& o, const LrLane<L>& ln, int k1, int n,
                                              char* uw) {
    float res[4][4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int k = k1 - 4 * s - e;
            if (!GUARD || k >= 0) {
                if (GUARD && k == n - 1) p = o.x[e];
                else p = o.x[e] - o.t[e] * p;
            }
            if (e < 3) res[s][e] = p;
        }
        p = lr_row(s, p);
        res[s][3] = p;
    }
    // the lane's samples k1 - 4 s - e sit at uw - e * L * 8 (uw: its first, the highest)
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float v[4] = {res[0][e], res[1][e], res[2][e], res[3][e]};
        if (!GUARD || k1 - 4 * ln.step - e >= 0) *(float*)(uw - e * L * 8) = lr_own(v, ln.s0, ln.s1, ln.s2);
    }
}

// The solver wave of image `img` (0: A / U.x, 1: B / U.y).  The whole groups of a chunk run in
// unrolled blocks of up to 8 with the next group's operands loaded during the current one into a
// second, static register set (a loop-carried pair made the compiler copy the loads and wait for
// each right away); every load is unconditional, clamped inside the chunk images (a conditional
// load made it wait for all of them).  The partial groups -- the line's last forward group, the
// back groups holding its last and its first samples -- take the guarded form.
template <int L>
__device__ __forceinline__ void lr_solver(int n, int nch, int img, int lane, bool lv, char* lds, int dbg) {
    constexpr int CH = 1024 / L;  // samples a chunk
    constexpr int G = CH / 16;    // groups a chunk
    constexpr int UB = G < 8 ? G : 8;  // groups an unrolled block
    LrLane<L> ln;
    ln.l = lane & 15;
    const int row = lane >> 4;
    ln.step = row == 0 ? 0 : row == 1 ? 1 : row == 3 ? 2 : 3;
    ln.s0 = ln.step == 0;
    ln.s1 = ln.step == 1;
    ln.s2 = ln.step == 2;
    ln.valid = lv && ln.l < L;
    const int l = ln.l < L ? ln.l : L - 1;  // (lanes past L repeat line L - 1: the same values)
    ln.img4 = img * 4;
    char* U = lds + img * 4;
    const char* Cq = lds + kLrU;
    const int kmax = nch * CH - 1;  // the last sample slot of the chunk images
    auto uaddr = [&](int k) __attribute__((always_inline)) { return U + (k * L + l) * 8; };
    auto ld_fwd = [&](int g, LrFwdOps& o) __attribute__((always_inline)) {
        const int k = min(16 * g + 4 * ln.step, kmax - 3);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            o.q[e] = *(const float4*)(Cq + ((k + e) * L + l) * 16);
            o.x[e] = *(const float*)uaddr(k + e);
        }
    };
    const int ng = (n + 15) / 16, ngf = n / 16;  // groups of the line, whole ones
    // ---- forward elimination: barrier c = chunks <= c + 1 landed ----
    float p = 0.0f;
    th_barrier();
    LR_STAMP(img == 0, dbg, 1);
    for (int c = 0; c < nch; c++) {
        if (c > 0) th_barrier();
        for (int b0 = c * G; b0 < min(c * G + G, ngf); b0 += UB) {
            LrFwdOps ops[UB];  // (one set per unrolled group: static indices, no copies)
            ld_fwd(b0, ops[0]);
#pragma unroll
            for (int gg = 0; gg < UB; gg++) {
                const int g = b0 + gg;
                if (gg + 1 < UB) ld_fwd(g + 1, ops[gg + 1 < UB ? gg + 1 : gg]);
                if (g < ngf) lr_fwd_group<L, false>(p, ops[gg], ln, 16 * g, n, uaddr(16 * g + 4 * ln.step));
            }
        }
        if (ngf < ng && ngf >= c * G && ngf < c * G + G) {  // the partial last group is in this chunk
            LrFwdOps A;
            const int k = 16 * ngf + 4 * ln.step;  // (each sample clamped on its own: the mapping holds)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                A.q[e] = *(const float4*)(Cq + (min(k + e, kmax) * L + l) * 16);
                A.x[e] = *(const float*)uaddr(min(k + e, kmax));
            }
            lr_fwd_group<L, true>(p, A, ln, 16 * ngf, n, uaddr(min(16 * ngf + 4 * ln.step, kmax)));
        }
    }
    LR_STAMP(img == 0, dbg, 2);
    // ---- back substitution: barrier cb = chunk cb's results in LDS for the writers ----
    // back group gb: samples k1 .. k1 - 15, k1 = n - 1 - 16 gb: gb = 0 holds the last sample,
    // gb = ngf the first ones when n % 16 != 0 (guarded); the others are whole
    auto ld_back = [&](int gb, LrBackOps& o) __attribute__((always_inline)) {
        const int k = max(n - 1 - 16 * gb - 4 * ln.step, 3);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            o.t[e] = *(const float*)(Cq + ((k - e) * L + l) * 16 + 12);
            o.x[e] = *(const float*)uaddr(k - e);
        }
    };
    auto back_guarded = [&](int gb, float& q) __attribute__((always_inline)) {
        LrBackOps A;
        const int k1 = n - 1 - 16 * gb;
        const int k = k1 - 4 * ln.step;  // (each sample clamped on its own: the mapping holds)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            A.t[e] = *(const float*)(Cq + (max(k - e, 0) * L + l) * 16 + 12);
            A.x[e] = *(const float*)uaddr(max(k - e, 0));
        }
        lr_back_group<L, true>(q, A, ln, k1, n, uaddr(max(k1 - 4 * ln.step, 0)));
    };
    float q = 0.0f;
    for (int cb = 0; cb < nch; cb++) {
        const int lo = max(cb * G, 1), hi = min(cb * G + G, ngf);  // whole back groups: 1 .. ngf - 1
        if (cb == 0) back_guarded(0, q);
        for (int b0 = lo; b0 < hi; b0 += UB) {
            LrBackOps ops[UB];
            ld_back(b0, ops[0]);
#pragma unroll
            for (int gg = 0; gg < UB; gg++) {
                const int gb = b0 + gg;
                if (gg + 1 < UB) ld_back(gb + 1, ops[gg + 1 < UB ? gg + 1 : gg]);
                if (gb < hi) {
                    const int k1 = n - 1 - 16 * gb;
                    lr_back_group<L, false>(q, ops[gg], ln, k1, n, uaddr(k1 - 4 * ln.step));
                }
            }
        }
        if (ng > ngf && ngf >= cb * G && ngf < cb * G + G && ngf >= 1) back_guarded(ngf, q);
        th_lgkm0();
        th_barrier();
    }
    LR_STAMP(img == 0, dbg, 3);
}

// The loader waves (lw = 0, 1): the pass's U (float2) and coefficient chunks, up to kLrAhead in
// flight; before barrier c, chunks <= c + 1 have landed.  Then, as writers, the results of back
// chunk cb after barrier cb: line-major float2 into a.O (the next pass's input), or k-major split
// into a.O0 / a.O1 (the last pass).
template <int L>
__device__ __forceinline__ void lr_loader_writer(const FgsThArgs& a, size_t fofs, int l0, int nch, int lw, int lane,
                                                 char* lds) {
    constexpr int CH = 1024 / L, IW = (8 + 16) / 2;
    const int n = a.n, last = n - 1;
    const char* gu = (const char*)((const float2*)a.U + fofs);
    const char* gc = (const char*)(a.coef + fofs);
    auto issue = [&](int c) __attribute__((always_inline)) {
        th_issue<L, 8>(gu, a.st, l0, c * CH, 1, last, lds + c * 8192, lw, lane);
        th_issue<L, 16>(gc, a.st, l0, c * CH, 1, last, lds + kLrU + c * 16384, lw, lane);
    };
    int issued = 0;
    for (; issued < min(kLrAhead, nch); issued++) issue(issued);
    for (int c = 0; c < nch; c++) {
        th_wait_chunks<IW>(issued - min(c + 2, issued));
        th_barrier();
        if (issued < nch) issue(issued++);
    }
    // ---- writers ----
    const float2* R = (const float2*)lds;
    for (int cb = 0; cb < nch; cb++) {
        th_barrier();
        const int khi = n - cb * CH, klo = max(khi - CH, 0);  // samples [klo, khi)
        if (a.O) {
            // line-major: a wave-instruction = 64 consecutive samples of one line
            for (int l = lw; l < L; l += 2) {
                if (l0 + l >= a.nl) break;
                float2* o = (float2*)a.O + fofs + (size_t)(l0 + l) * a.onp;
                for (int k = klo + lane; k < khi; k += 64) o[k] = R[k * L + l];
            }
        } else {
            // k-major split: a wave-instruction = 64 / L samples x L lines
            const size_t fo = (size_t)blockIdx.y * a.ofs + l0;
            const int l = lane % L;
            for (int k = klo + lw * (64 / L) + lane / L; k < khi; k += 2 * (64 / L)) {
                if (l0 + l < a.nl) {
                    const float2 v = R[k * L + l];
                    a.O0[fo + (size_t)k * a.ost + l] = v.x;
                    a.O1[fo + (size_t)k * a.ost + l] = v.y;
                }
            }
        }
    }
}

// One FGS pass of two right-hand sides (a.U float2), L lines a workgroup, every line resident.
template <int L>
__global__ __launch_bounds__(256) void k_fgs_lr(FgsThArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[kLrLds];
    constexpr int CH = 1024 / L;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const size_t fofs = (size_t)blockIdx.y * a.fs;
    const int l0 = blockIdx.x * L;
    const int nch = (a.n + CH - 1) / CH;
    LR_STAMP(wave == 0, a.dbg, 0);
    if (wave < 2) lr_solver<L>(a.n, nch, wave, lane, l0 + (lane & 15) < a.nl, lds, a.dbg);
    else lr_loader_writer<L>(a, fofs, l0, nch, wave - 2, lane, lds);
    LR_STAMP(wave == 2, a.dbg, 4);
    LR_STAMP(wave == 0, a.dbg, 5);
}

// ---- k_fgs_lrjob: the coefficient jobs the k_fgs_lr way (round 6) --------------------------
// th_job_solver's recurrence, operations and roundings (bit-exact): per sample k of a line
//   aa = lam * C[k-1] (C[-1] = 0),  cc = lam * C[k],  den = (1 - cc) - aa * (1 + t),
//   r = fgs_rcp(den),  t = cc / den (from r by Markstein, or IEEE in a group holding a tiny cc)
// with t carried from sample to sample: a chain of 9 dependent operations.  On one wave every
// instruction it issues is on that chain (k_fgs_lr's finding), so the work is split so that the
// chain's wave issues little else:
//   wave 0     the solver: lane = (row, line) as in k_fgs_lr -- 4 consecutive samples x L lines
//              an LDS instruction, the chain walking the rows by permlane swaps -- reading each
//              sample's (aa, cc, 1 - cc) and writing (den, 1/den, t) with its row's stores
//              (exec-masked per walk step, no selects; the writers add aa);
//   wave 1     the prep wave: the line's weights DMA'd at the start (resident, kLrChunks chunks),
//              then per chunk (aa, cc, 1 - cc) into LDS and a flag bit per 16-sample group holding a
//              tiny cc (one word a chunk, read once by the solver) (0 < |cc| < 2^-96 (1 + 2 lam), where the reciprocal form may round apart
//              from the division), a chunk ahead of the solver;
//   waves 2, 3 the writers: chunk c's rows to coef and tt, a chunk behind the solver.
// Iteration i (a barrier each, nch + 2 of them): prep chunk i, solve chunk i - 1, write chunk i - 2.
// LDS: [weights: kLrChunks x 4 KiB][prep: kLrChunks x 16 KiB][rows: 2 x 16 KiB][chunk flags].
constexpr int kLjW = kLrChunks * 4096, kLjP = kLrChunks * 16384, kLjO = 2 * 16384;
constexpr int kLjLds = kLjW + kLjP + kLjO + kLrChunks * 4;  // + a flag word a chunk (bit: group)
static_assert(1024 / 4 / 16 <= 32, "a chunk's groups fit a flag word");
static_assert(kLjLds <= 160 * 1024, "one workgroup's LDS");

// one walk step after another: the step-s row's 4 samples are the chain's, its stores the only
// ones that land (the other rows compute from their own operands and are masked off)
template <int L, bool EXACT, bool GUARD>
__device__ __forceinline__ void lj_body(float& t, const float4 (&q)[4], int step, int k0, int n, float4* orow) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
        float3 res[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (!GUARD || k0 + 4 * s + e < n) {
                const float aa = q[e].x, cc = q[e].y;
                const float den = q[e].z - aa * (1.0f + t);
                const float r = fgs_rcp(den);
                if constexpr (EXACT) {
                    t = cc / den;
                } else {
                    const float q0 = cc * r;
                    t = __builtin_fmaf(-__builtin_fmaf(q0, den, -cc), r, q0);  // cc / den
                }
                res[e] = make_float3(den, r, t);
            }
        }
        if (step == s) {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (!GUARD || k0 + 4 * s + e < n) *(float3*)(orow + e * L) = res[e];
        }
        t = lr_row(s, t);
    }
}

template <int L>
__device__ __forceinline__ void lj_solver(int n, int nch, int lane, char* lds) {
    constexpr int CH = 1024 / L, G = CH / 16;
    constexpr int UB = G < 8 ? G : 8;  // groups an unrolled block (within a chunk)
    const int row = lane >> 4, lq = lane & 15;
    const int l = lq < L ? lq : L - 1;  // (lanes past L repeat line L - 1: the same values, the same slots)
    const int step = row == 0 ? 0 : row == 1 ? 1 : row == 3 ? 2 : 3;
    const float4* P = (const float4*)(lds + kLjW);
    float4* O = (float4*)(lds + kLjW + kLjP);
    const uint32_t* flags = (const uint32_t*)(lds + kLjW + kLjP + kLjO);
    const int ng = (n + 15) / 16, ngf = n / 16;
    struct Ops {
        float4 q[4];
    };
    // a group's operands (every slot of a chunk holds a value: the prep wave covers all)
    auto ld = [&](int g, Ops& o) __attribute__((always_inline)) {
        const int k = 16 * g + 4 * step;
#pragma unroll
        for (int e = 0; e < 4; e++) o.q[e] = P[(k + e) * L + l];
    };
    uint32_t cflags = 0;  // the chunk's group flags (bit g - c * G), wave-uniform
    auto group = [&](float& t, const Ops& o, int g, int c, auto guard) __attribute__((always_inline)) {
        constexpr bool GU = decltype(guard)::value;
        float4* orow = O + (c & 1) * 1024 + (16 * g - c * CH + 4 * step) * L + l;
        if ((cflags >> (g - c * G)) & 1u) lj_body<L, true, GU>(t, o.q, step, 16 * g, n, orow);
        else lj_body<L, false, GU>(t, o.q, step, 16 * g, n, orow);
    };
    float t = 0.0f;
    th_barrier();  // iteration 0: chunk 0 prepared
    LJ_STAMP(true, 2);
    for (int c = 0; c < nch; c++) {
        cflags = __builtin_amdgcn_readfirstlane(flags[c]);
        for (int b0 = c * G; b0 < min(c * G + G, ngf); b0 += UB) {
            Ops ops[UB];  // (one set per unrolled group: static indices, no copies)
            ld(b0, ops[0]);
#pragma unroll
            for (int gg = 0; gg < UB; gg++) {
                const int g = b0 + gg;
                if (gg + 1 < UB) ld(g + 1, ops[gg + 1 < UB ? gg + 1 : gg]);
                if (g < ngf) group(t, ops[gg], g, c, std::false_type{});
            }
        }
        if (ngf < ng && ngf >= c * G && ngf < c * G + G) {  // the line's partial last group
            Ops o;
            ld(ngf, o);
            group(t, o, ngf, c, std::true_type{});
        }
        th_lgkm0();
        th_barrier();
    }
    LJ_STAMP(true, 3);
    th_barrier();  // iteration nch + 1: the writers' last chunk
}

// s_waitcnt for the prep wave's DMA: chunk i landed when at most `younger` chunks (4
// wave-instructions each) are in flight after it
__device__ __forceinline__ void lj_wait(int younger) {
    static_assert(kLrChunks <= 6, "vmcnt cases");
    switch (younger) {
        case 0: th_vmcnt<0>(); break;
        case 1: th_vmcnt<4>(); break;
        case 2: th_vmcnt<8>(); break;
        case 3: th_vmcnt<12>(); break;
        case 4: th_vmcnt<16>(); break;
        default: th_vmcnt<20>(); break;
    }
}

template <int L>
__device__ __forceinline__ void lj_prep(const FgsCoefJob& J, size_t fofs, int l0, int nch, int lane, char* lds) {
    constexpr int CH = 1024 / L;
    const int last = J.n - 1;
    const float lam = J.lam, tiny = 0x1p-96f * (1.0f + 2.0f * lam);
    const float* W = (const float*)lds;
    float4* P = (float4*)(lds + kLjW);
    uint32_t* flags = (uint32_t*)(lds + kLjW + kLjP + kLjO);
    if (lane < kLrChunks) flags[lane] = 0;
    const char* gw = (const char*)(J.Cw + fofs);
    for (int c = 0; c < nch; c++) {
        th_issue<L, 4>(gw, J.st, l0, c * CH, 1, last, lds + c * 4096, 0, lane);
        th_issue<L, 4>(gw, J.st, l0, c * CH, 1, last, lds + c * 4096, 1, lane);
    }
    for (int i = 0; i < nch + 2; i++) {
        if (i < nch) {
            lj_wait(nch - 1 - i);
#pragma unroll 4
            for (int it = 0; it < 16; it++) {
                const int j = i * 1024 + it * 64 + lane;  // = k * L + l
                const int k = j / L, l = j % L;
                const float cw = W[j];
                const float cp = k > 0 ? W[j - L] : 0.0f;
                const float aa = lam * cp, cc = lam * cw;
                P[j] = make_float4(aa, cc, 1.0f - cc, 0.0f);
                if (fabsf(cc) < tiny && cc != 0.0f && k <= last && l0 + l < J.nl)
                    atomicOr(&flags[i], 1u << (k / 16 - i * (CH / 16)));
            }
            if (i == 0) LJ_STAMP(true, 1);
        }
        th_lgkm0();
        th_barrier();
    }
    LJ_STAMP(true, 5);
}

template <int L>
__device__ __forceinline__ void lj_writer(const FgsCoefJob& J, size_t fofs, int l0, int nch, int lw, int lane,
                                          const char* lds) {
    constexpr int CH = 1024 / L;
    const int last = J.n - 1;
    const float4* O = (const float4*)(lds + kLjW + kLjP);
    const float* W = (const float*)lds;
    for (int i = 0; i < nch + 2; i++) {
        const int c = i - 2;
        if (c >= 0) {
            const float4* Oc = O + (c & 1) * 1024;
#pragma unroll 4
            for (int it = 0; it < 8; it++) {
                const int j = (2 * it + lw) * 64 + lane;  // = (k - c * CH) * L + l
                const int k = c * CH + j / L, l = j % L;
                if (k <= last && l0 + l < J.nl) {
                    // the solver's (den, 1/den, t); aa = lam * C[k-1] again from the weights
                    const float4 v = Oc[j];
                    const float aa = J.lam * (k > 0 ? W[c * 1024 + j - L] : 0.0f);
                    const size_t o = fofs + (size_t)k * J.st + l0 + l;
                    J.coef[o] = make_float4(aa, v.x, v.y, v.z);
                    J.tt[o] = v.z;
                }
            }
        }
        th_barrier();
    }
    LJ_STAMP(lw == 0, 4);
}

template <int L>
__device__ __forceinline__ void lj_block(const FgsCoefJob& J, size_t fofs, int jb, int wave, int lane, char* lds) {
    constexpr int CH = 1024 / L;
    const int l0 = jb * L, nch = (J.n + CH - 1) / CH;
    if (wave == 0) lj_solver<L>(J.n, nch, lane, lds);
    else if (wave == 1) lj_prep<L>(J, fofs, l0, nch, lane, lds);
    else lj_writer<L>(J, fofs, l0, nch, wave - 2, lane, lds);
}

// The coefficient jobs of a launch (a.job, blocks of job.lpb lines each; blockIdx.y = frame).
__global__ __launch_bounds__(256) void k_fgs_lrjob(FgsThArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[kLjLds];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const size_t fofs = (size_t)blockIdx.y * a.fs;
    int jb = blockIdx.x, j = 0;
    while (j < a.njobs && jb >= a.job[j].blocks) jb -= a.job[j++].blocks;
    if (j >= a.njobs) return;  // uniform over the workgroup
    const FgsCoefJob& J = a.job[j];
    LJ_STAMP(wave == 0, 0);
    switch (J.lpb) {
        case 16: lj_block<16>(J, fofs, jb, wave, lane, lds); break;
        case 8: lj_block<8>(J, fofs, jb, wave, lane, lds); break;
        default: lj_block<4>(J, fofs, jb, wave, lane, lds); break;
    }
}

// ---- the dispatch plan and the launchers ----
// k_fgs_th's lines a workgroup for one launch -- a pass, or the jobs of several -- over `count`
// sets of nl[i] lines: the fewest (LPB) whose workgroups still all fit on a chip of `cus` CUs at
// once (one a CU: the LDS ring), so that every chain runs on a CU's memory pipeline shared with as
// few lines as possible.
static int fgs_th_lpb(const int* nl, int count, int F, int cus) {
    for (int c : {16, 32, 64}) {
        int blocks = 0;
        for (int i = 0; i < count; i++) blocks += (nl[i] + c - 1) / c;
        if ((long long)blocks * F <= cus) return c;
    }
    return 64;
}

// k_fgs_lr's lines a workgroup for a pass of lines of n samples: the largest L of 16, 8, 4, 2
// (at most SDR_FGS_LR_MAXL) whose lines fit in LDS, n <= 6 * 1024 / L; 0: take k_fgs_th (one
// right-hand side, longer lines, SDR_FGS_LR=0).
static int fgs_lr_lines(int n, bool two) {
    static const bool off = getenv("SDR_FGS_LR") && atoi(getenv("SDR_FGS_LR")) == 0;  // A/B knob
    if (!two || off) return 0;
    // at most 8 lines a workgroup by default (profiles/r6_fgs_lr_maxl.txt, C4): the 360-sample
    // column passes on 16 lines ran ~15 % slower a sample than the row passes on 8 (the four rows'
    // reads of 16 distinct lines conflict in LDS); capped at 8, one stream 0.4195 -> 0.413 ms with
    // 6 frames in flight unchanged within noise; at 4, one stream 0.4123 ms but 6 frames in flight
    // 4128 -> 3948 fps (a workgroup of ~147 KiB LDS per CU, 4x as many)
    static const int maxl = getenv("SDR_FGS_LR_MAXL") ? atoi(getenv("SDR_FGS_LR_MAXL")) : 8;  // A/B knob
    for (int L : {16, 8, 4, 2})
        if (L <= maxl && n <= kLrChunks * 1024 / L) return L;
    return 0;
}

// k_fgs_lrjob's lines a workgroup for a job of lines of n samples, as above from 16, 8, 4 (2 lines:
// the weights' 8-byte rows are not whole DMA pieces); 0: they do not fit, or SDR_FGS_LRJOB=0
static int fgs_lrjob_lines(int n) {
    static const bool off = getenv("SDR_FGS_LRJOB") && atoi(getenv("SDR_FGS_LRJOB")) == 0;  // A/B knob
    for (int L : {16, 8, 4})
        if (!off && n <= kLrChunks * 1024 / L) return L;
    return 0;
}

FgsPlan fgs_plan(int w, int h, int F, bool two, int iters, int cus) {
    const int npass = 2 * iters;
    FgsPlan P{std::vector<sdr_fgs_launch>(npass), std::vector<sdr_fgs_launch>(npass)};
    // a launch of coefficient jobs takes k_fgs_lrjob when every job's lines fit in LDS, k_fgs_th
    // with all of them otherwise
    for (int p0 = 0; p0 < npass; p0 += kFgsMaxJobs) {
        const int nj = std::min(kFgsMaxJobs, npass - p0);
        int nl[kFgsMaxJobs], n;
        bool lr = true;
        for (int j = 0; j < nj; j++) {
            fgs_pass_shape(p0 + j, w, h, &nl[j], &n);
            P.job[p0 + j] = {SDR_FGS_KERNEL_LRJOB, fgs_lrjob_lines(n)};
            lr = lr && P.job[p0 + j].lines;
        }
        if (!lr) std::fill_n(&P.job[p0], nj, sdr_fgs_launch{SDR_FGS_KERNEL_TH, fgs_th_lpb(nl, nj, F, cus)});
    }
    // a pass takes k_fgs_lr when its lines fit in LDS, k_fgs_th otherwise
    for (int p = 0; p < npass; p++) {
        int nl, n;
        fgs_pass_shape(p, w, h, &nl, &n);
        const int L = fgs_lr_lines(n, two);
        if (L) P.pass[p] = {SDR_FGS_KERNEL_LR, L};
        else P.pass[p] = {SDR_FGS_KERNEL_TH, fgs_th_lpb(&nl, 1, F, cus)};
    }
    return P;
}

// One k_fgs_th launch: the pass (a.nl lines; none when !pass) or its jobs, lpb lines a workgroup.
static void launch_fgs_th(FgsThArgs a, bool pass, int lpb, bool two, int F, hipStream_t st) {
    a.main_blocks = pass ? (a.nl + lpb - 1) / lpb : 0;
    int blocks = a.main_blocks;
    for (int j = 0; j < a.njobs; j++) blocks += a.job[j].blocks = (a.job[j].nl + lpb - 1) / lpb;
    th_stamps_arm(st);
    static void (*const K[2][3])(FgsThArgs) = {{k_fgs_th<false, 16>, k_fgs_th<false, 32>, k_fgs_th<false, 64>},
                                               {k_fgs_th<true, 16>, k_fgs_th<true, 32>, k_fgs_th<true, 64>}};
    hipLaunchKernelGGL(K[two][lpb == 16 ? 0 : lpb == 32 ? 1 : 2], dim3(blocks, F), dim3(256), 0, st, a);
}

void launch_fgs_jobs(FgsThArgs c, const sdr_fgs_launch* k, bool two, int F, hipStream_t st) {
    if (k[0].kernel == SDR_FGS_KERNEL_TH) return launch_fgs_th(c, false, k[0].lines, two, F, st);
    int blocks = 0;
    for (int j = 0; j < c.njobs; j++) {
        FgsCoefJob& J = c.job[j];
        J.lpb = k[j].lines;
        blocks += J.blocks = (J.nl + J.lpb - 1) / J.lpb;
    }
    hipLaunchKernelGGL(k_fgs_lrjob, dim3(blocks, F), dim3(256), 0, st, c);
}

void launch_fgs_pass(FgsThArgs a, const sdr_fgs_launch& k, bool two, int F, hipStream_t st) {
    if (k.kernel == SDR_FGS_KERNEL_TH) return launch_fgs_th(a, true, k.lines, two, F, st);
    a.dbg = lr_stamp_slot();
    const int L = k.lines;
    auto* lr = L == 16 ? k_fgs_lr<16> : L == 8 ? k_fgs_lr<8> : L == 4 ? k_fgs_lr<4> : k_fgs_lr<2>;
    hipLaunchKernelGGL(lr, dim3((a.nl + L - 1) / L, F), dim3(256), 0, st, a);
}

// sdr_fgs_rcp_selftest: fgs_rcp against the IEEE division for all 2^23 mantissas of d in
// [2^e, 2^(e+1)) (C linkage: the kernel's symbol is the plain k_fgs_rcp_check)
extern "C" __global__ __launch_bounds__(256) void k_fgs_rcp_check(int e, unsigned int* bad) {
    const uint32_t m = blockIdx.x * 256 + threadIdx.x;
    const float d = __builtin_bit_cast(float, (uint32_t)(127 + e) << 23 | m);
    const volatile float one = 1.0f;
    if (__builtin_bit_cast(uint32_t, fgs_rcp(d)) != __builtin_bit_cast(uint32_t, one / d)) atomicAdd(bad, 1u);
}

}  // namespace sdr

extern "C" int sdr_fgs_rcp_selftest(int e, unsigned int* mismatches) {
    if (!mismatches || e < 0 || e > 126) return sdr::set_error(SDR_ERR_ARG, "e must be in [0, 126]");
    unsigned int* d = nullptr;
    hipError_t err = hipMalloc((void**)&d, 4);
    if (err == hipSuccess) err = hipMemset(d, 0, 4);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(sdr::k_fgs_rcp_check, dim3((1u << 23) / 256), dim3(256), 0, 0, e, d);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpy(mismatches, d, 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (err != hipSuccess) return sdr::set_error(SDR_ERR_DEVICE, std::string("sdr_fgs_rcp_selftest: ") + hipGetErrorString(err));
    return SDR_OK;
}
