// sdr_sgbm_rules.hpp -- the SGBM rules that decide an output bit, each stated once for the kernels
// of sdr_paths.hip (scanline chains), sdr_sweep.hip (row sweeps) and sdr_post.hip: the path
// recurrence (A.4), the WTA decision after the first minimum (A.8), the left-right verdict (A.9; the
// disp2 key's format sits beside kD2None in sdr_internal.hpp), the median network (A.10) and the
// two-chain workgroup count.  Every function is inlined into its kernel; the scalar rules are
// __host__ __device__, so tests/cpp/sgbm_rules_check.hip checks them as a host program.
#pragma once
#include "sdr_device.hpp"
#include "sdr_internal.hpp"

namespace sdr {

// The per-word recurrence of one step: L = C + min(Lp, min(Lp[d-1], Lp[d+1]) + P1, delta2) -
// delta2 for the lane's K words; returns the minimum of L's pairs.  up / dn: the d-1 / d+1
// neighbour words from the adjacent lanes -- the caller's (a wave shift for the chains, a row
// shift for the sweeps).  (Issuing two words' packed ops alternately -- 4 x int16 vector ops, no
// packed op right after the one it reads, so none of gfx950's wait states -- removed ~40 % of the
// path kernels' s_nops and measured no faster: at 3-4 waves per SIMD the other waves fill those
// slots; profiles/r4_ab_variants.txt.)
// WE: also E = C - L = delta2 - t, the 12-bit record's value (0 <= E <= P2: minLp <= t <= delta2),
// one packed op beside the dependency chain.  (Returned through a reference, m moved k_sweep16's code.)
template <int K, bool PAD, bool WE = false>
__device__ __forceinline__ uint32_t step_words(const uint32_t (&c)[K], const uint32_t (&Lp)[K], uint32_t delta2,
                                               uint32_t P1x2, bool active, uint32_t up, uint32_t dn,
                                               uint32_t (&L)[K], uint32_t* E = nullptr) {
    uint32_t m = kMaxPair;
#pragma unroll
    for (int i = 0; i < K; i++) {
        const uint32_t dm1 = funnel16(Lp[i], i == 0 ? up : Lp[i == 0 ? 0 : i - 1]);
        const uint32_t dp1 = funnel16(i == K - 1 ? dn : Lp[i == K - 1 ? 0 : i + 1], Lp[i]);
        uint32_t t = pk_add_sat(pk_min(dm1, dp1), P1x2);
        t = pk_min(pk_min(t, Lp[i]), delta2);
        uint32_t l = pk_sub(pk_add(c[i], t), delta2);
        if constexpr (PAD) l = active ? l : kMaxPair;
        if constexpr (WE) E[i] = pk_sub(delta2, t);
        L[i] = l;
        m = pk_min(m, l);
    }
    return m;
}

// ---- A.8 after the first minimum (minS at disparity index best) ----
// The first-minimum key stays with each kernel: the chains order (S + 32768) << 16 | d from sign-
// extended halves, the sweeps S << 16 | d straight from the packed word (S >= 0 in both); either
// yields (minS, best), and one form for both changes the other kernel's instructions.
// OpenCV's two uniqueness rules are monotone in S[d], so only min2 = the smallest S[d] with |d -
// best| > 1 is tested.  Scalar: reject when S[d] * (100 - u) < 100 * minS.  SIMD: when S[d] <
// (short)(thresh + 1), thresh = (100 * minS) / (100 - u) truncated, as a double product: 1 / (100 - u)
// rounded up by 2^-40 gives the exact quotient for all u in [0, 99], minS in [0, 32767] (sgbm_rules_check).
struct UniqRule {
    bool check, simd;
    int lhs_scale;
    double inv100u;
};
__host__ __device__ __forceinline__ UniqRule make_uniq_rule(int uniq, int uniq_simd) {
    return {uniq > 0 || !uniq_simd, uniq_simd != 0, 100 - uniq, 1.0 / (double)(100 - uniq) * (1.0 + 0x1p-40)};
}
__host__ __device__ __forceinline__ bool uniq_rejects(const UniqRule& u, int minS, int min2) {
    const int thr16 = (int)(short)((int)((double)(100 * minS) * u.inv100u) + 1);
    return u.check && (u.simd ? (min2 < thr16) : (min2 * u.lhs_scale < minS * 100));
}

// The WTA disparity of an accepted pixel: d * 16 + ((S[d-1] - S[d+1]) * 16 + den) / (2 * den), C
// truncating division; Sm / Sp = S at best -+ 1.  (Accepted needs minS < kMaxCost: with every S saturated
// OpenCV's first-minimum scan keeps bestDisp = -1, INVALID, whose disp2 candidate never wins.)
__host__ __device__ __forceinline__ int wta_subpixel(int best, int minS, int Sm, int Sp, int D, int minD) {
    const int s = Sm + Sp - 2 * minS;
    const int den = s > 1 ? s : 1;
    const int qq = div_trunc_small((Sm - Sp) * 16 + den, 2 * den);
    return best * 16 + (((0 < best) & (best < D - 1)) ? qq : 0) + minD * 16;
}

// On a pixel's staged S row (int16 S[d], lane gl of the pixel's 16-lane row having written its WK
// words): S at best -+ 1, and min2 = the minimum of S[d] over |d - best| > 1 (0 <= S <= 32767:
// 0x7fff masks a half).  The halfword accesses alias the row's 32-bit words: may_alias keeps their order.
template <int WK>
__device__ __forceinline__ int wta_second_min(uint32_t __attribute__((may_alias))* srow, int gl, bool active,
                                              int best, int D, int& Sm, int& Sp) {
    typedef int16_t __attribute__((may_alias)) s16a;
    const int dm = max(best - 1, 0), dp = min(best + 1, D - 1);
    s16a* s16 = (s16a*)srow;
    Sm = s16[dm];
    Sp = s16[dp];
    s16[dm] = 0x7fff;
    s16[best] = 0x7fff;
    s16[dp] = 0x7fff;
    uint32_t m2 = kMaxPair;
#pragma unroll
    for (int i = 0; i < WK; i++) m2 = pk_min(m2, srow[gl * WK + i]);
    m2 = active ? m2 : kMaxPair;
    m2 = pk_min(m2, funnel16(m2, m2));
    m2 = row16_min_u32(m2);
    return (int)(m2 & 0x7fff);
}

// ---- A.9, OpenCV's disp12MaxDiff check.  d1: the pixel's WTA value (not INVALID); a2 / b2: the
// right view's disparities (d2_disparity) at the columns x - lr_lo(d1) and x - lr_hi(d1), which the
// caller has found inside [0, W) (else d1 stands).  Returns d1, or INVALID when both disagree ----
__host__ __device__ __forceinline__ int lr_lo(int d1) { return d1 >> 4; }
__host__ __device__ __forceinline__ int lr_hi(int d1) { return (d1 + 15) >> 4; }
__host__ __device__ __forceinline__ int lr_verdict(int d1, int a2, int b2, int minD, int d12) {
    const bool bad = a2 >= minD && abs(a2 - lr_lo(d1)) > d12 && b2 >= minD && abs(b2 - lr_hi(d1)) > d12;
    return bad ? (minD - 1) * 16 : d1;
}
// A.9 at pixel (x, y) of a frame: raw is its WTA map, d2 its right-view keys (both [H][W]).  Every
// consumer of the LR-checked map (the median's tiles, the debug stage) computes it on the fly.
__device__ __forceinline__ int lr_at(const Geometry& g, const int16_t* __restrict__ raw,
                                     const uint32_t* __restrict__ d2, int x, int y, int d12) {
    const int invalid = (g.minD - 1) * 16;
    if (x < g.minX1 || x >= g.minX1 + g.W1) return invalid;
    const size_t ro = (size_t)y * g.W;
    const int d1 = raw[ro + x];
    if (d1 == invalid) return d1;
    const int _x = x - lr_lo(d1), x_ = x - lr_hi(d1);
    if (_x < 0 || _x >= g.W || x_ < 0 || x_ >= g.W) return d1;
    return lr_verdict(d1, d2_disparity(d2[ro + _x], _x, g), d2_disparity(d2[ro + x_], x_, g), g.minD, d12);
}

// ---- A.10: Devillard's 19-exchange median-of-9 network; returns the median, permutes p ----
__host__ __device__ __forceinline__ int median9(int (&p)[9]) {
#define SDR_S(a, b) { const int t_ = p[a] < p[b] ? p[a] : p[b]; p[b] = p[a] < p[b] ? p[b] : p[a]; p[a] = t_; }
    SDR_S(1, 2) SDR_S(4, 5) SDR_S(7, 8) SDR_S(0, 1) SDR_S(3, 4) SDR_S(6, 7)
    SDR_S(1, 2) SDR_S(4, 5) SDR_S(7, 8) SDR_S(0, 3) SDR_S(5, 8) SDR_S(4, 7)
    SDR_S(3, 6) SDR_S(1, 4) SDR_S(2, 5) SDR_S(4, 7) SDR_S(4, 2) SDR_S(6, 4)
    SDR_S(4, 2)
#undef SDR_S
    return p[4];
}

// ---- two chains a wave (k_paths_tc) / two columns a workgroup (k_south_wta TC): a direction
// entry's chains go in pairs, numbered entry by entry; an odd entry's last pair has no chain B ----
__host__ __device__ __forceinline__ int pair_count(int nchains) { return (nchains + 1) / 2; }
inline int pair_workgroups(const PathLaunch& pl) {
    int n = 0;
    for (int i = 0; i < pl.ndirs; i++) n += pair_count(pl.d[i].nchains);
    return n;
}

}  // namespace sdr
