// sdr_voxel_plan.hpp -- the plan of one voxel-grid call (sdr_cloud.hip), derived on the host: the
// layout of the call's scratch arena for n points, and the grid a cloud's bounds and leaf sizes
// give (PCL 1.14 VoxelGrid::applyFilter, restated as oracle/pcl_oracle.c does).  Plain host
// arithmetic: no HIP call, no device code, so a host program can include it
// (tests/cpp/voxel_plan_check.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "sdr_layout.hpp"

namespace sdr {

constexpr int kMinMaxBlocks = 512;                              // k_minmax: at most this many partials
constexpr int kScanItems = 8, kScanSeg = 256 * kScanItems;      // k_scan_*: ints a workgroup
constexpr int kRsRounds = 16, kRsTile = 256 * kRsRounds;        // k_rs_*: keys a workgroup

struct VoxelParams {
    float inv[3];
    int minb[3];
    uint32_t mul1, mul2;
};

// ---- the arena ----------------------------------------------------------------------------------
// Everything a call keeps on the device, in one block: the min/max partials, the 64-bit keys
// before and after the sort, the heads and their scanned positions, the sort's ping-pong (voxel,
// point) arrays, its histograms and the scan's block totals, laid out by sdr_layout.hpp's rule.
struct VoxelArena {
    // a layout slice as (offset, bytes): the call resolves it to the element type it took
    struct Slice {
        size_t off = 0, bytes = 0;
        Slice() = default;
        template <typename T>
        Slice(const sdr::Slice<T>& s) : off(s.off), bytes(s.bytes()) {}
    };
    int nb_rs, nh, nb_scan;  // radix-sort tiles, histogram entries (256 a tile), scan segments
    Slice partial, keys, sorted, head, pos, kv[4], hist, spart;
    size_t total;
};

inline VoxelArena voxel_arena(int n) {
    VoxelArena a{};
    a.nb_rs = (n + kRsTile - 1) / kRsTile;
    a.nh = 256 * a.nb_rs;
    a.nb_scan = (std::max(n, a.nh) + kScanSeg - 1) / kScanSeg;
    ScratchLayout l;
    const size_t un = (size_t)n;
    a.partial = l.take<float>((size_t)7 * kMinMaxBlocks);
    a.keys = l.take<uint64_t>(un);
    a.sorted = l.take<uint64_t>(un);
    a.head = l.take<int>(un);
    a.pos = l.take<int>(un);
    for (auto& s : a.kv) s = l.take<uint32_t>(un);
    a.hist = l.take<int>((size_t)a.nh);
    a.spart = l.take<int>((size_t)a.nb_scan);
    a.total = l.total;
    return a;
}

// ---- the grid -----------------------------------------------------------------------------------
// PCL's "Leaf size is too small for the input dataset. Integer indices would overflow.": the
// product of the three 64-bit counts, which may wrap, compared as a signed value
inline bool voxel_overflows(const long long d[3]) {
    const long long prod = (long long)((unsigned long long)d[0] * (unsigned long long)d[1] *
                                       (unsigned long long)d[2]);
    return prod > 2147483647LL;
}

// Voxel indices are below div0 * div1 * div2 (each div at most one above PCL's d, whose product
// passed the overflow check); `past` = that bound, clamped to 32 bits, marks the non-finite points,
// which sort last
inline uint32_t voxel_past(const int div[3]) {
    const unsigned long long divprod = (unsigned long long)div[0] * (unsigned long long)div[1] * (unsigned long long)div[2];
    return divprod < 0xFFFFFFFFull ? (uint32_t)divprod : 0xFFFFFFFFu;
}

// the bits of the largest sort key, `past`: the radix sort runs ceil(bits / 8) passes
inline int voxel_sort_bits(uint32_t past) {
    int bits = 1;
    while (bits < 32 && (past >> bits) != 0) bits++;
    return bits;
}

enum VoxelKind {
    VOXEL_EMPTY,        // no finite point: the output is empty
    VOXEL_PASSTHROUGH,  // PCL's overflow refusal: the output is the input cloud unchanged
    VOXEL_GRID,
};

struct VoxelGrid {
    VoxelKind kind;
    VoxelParams v;  // the rest: VOXEL_GRID only
    int div[3];
    uint32_t past;
    int bits;
};

// mn, mx: the bounds of the nfin finite points; lx, ly, lz > 0: the leaf sizes
inline VoxelGrid voxel_grid(const float mn[3], const float mx[3], long long nfin, float lx, float ly, float lz) {
#pragma clang fp contract(off)
    VoxelGrid g{};
    g.kind = VOXEL_EMPTY;
    if (!nfin) return g;
    const float inv[3] = {1.0f / lx, 1.0f / ly, 1.0f / lz};
    long long d[3];
    for (int c = 0; c < 3; c++) d[c] = (long long)((mx[c] - mn[c]) * inv[c]) + 1;
    g.kind = VOXEL_PASSTHROUGH;
    if (voxel_overflows(d)) return g;
    g.kind = VOXEL_GRID;
    for (int c = 0; c < 3; c++) {
        g.v.inv[c] = inv[c];
        g.v.minb[c] = (int)std::floor(mn[c] * inv[c]);
        const int maxb = (int)std::floor(mx[c] * inv[c]);
        g.div[c] = maxb - g.v.minb[c] + 1;
    }
    g.v.mul1 = (uint32_t)g.div[0];
    g.v.mul2 = (uint32_t)g.div[0] * (uint32_t)g.div[1];
    g.past = voxel_past(g.div);
    g.bits = voxel_sort_bits(g.past);
    return g;
}

}  // namespace sdr
