// voxel_plan_check.hip -- the voxel grid's host plan (csrc/sdr_voxel_plan.hpp) as a stand-alone host
// program, for a sanitizer build: the grid derivation against PCL's expressions as
// oracle/pcl_oracle.c states them (restated here), and the arena layout against the sizes and the
// total the voxel-grid entry asked its bump allocator for before the layout existed.  Prints
// "voxel_plan_check: N checks, M failures"; exit status 1 on a failure.
//
//   hipcc --cuda-host-only -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -std=c++17 tests/cpp/voxel_plan_check.hip -o voxel_plan_check
#include "../../stereo_depth_ruler_amd/csrc/sdr_voxel_plan.hpp"

#include <math.h>

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

int checks = 0, failures = 0;

void check(bool ok, const char* what, int line) {
    checks++;
    if (ok) return;
    failures++;
    std::printf("FAILED line %d: %s\n", line, what);
}
#define CHECK(x) check((x), #x, __LINE__)

// ---- (a) the grid ---------------------------------------------------------------------------------
struct Ref {
    int kind;  // 0 empty, 1 pass-through, 2 grid
    int minb[3], div[3];
    uint32_t mul1, mul2;
};

// orc_voxel_grid's decisions and index arithmetic (oracle/pcl_oracle.c), from the bounds on
Ref ref_grid(const float mn[3], const float mx[3], long long nfin, const float leaf[3]) {
    Ref r{};
    if (!nfin) return r;
    const float inv[3] = {1.0f / leaf[0], 1.0f / leaf[1], 1.0f / leaf[2]};
    long long d[3];
    for (int c = 0; c < 3; c++) d[c] = (long long)((mx[c] - mn[c]) * inv[c]) + 1;
    const long long prod = (long long)((unsigned long long)d[0] * (unsigned long long)d[1] * (unsigned long long)d[2]);
    r.kind = 1;
    if (prod > 2147483647LL) return r;
    r.kind = 2;
    for (int c = 0; c < 3; c++) {
        r.minb[c] = (int)floorf(mn[c] * inv[c]);
        r.div[c] = (int)floorf(mx[c] * inv[c]) - r.minb[c] + 1;
    }
    r.mul1 = (uint32_t)r.div[0];
    r.mul2 = (uint32_t)r.div[0] * (uint32_t)r.div[1];
    return r;
}

// the sort's bound and width, stated another way: min(div0 * div1 * div2 mod 2^64, 2^32 - 1), and
// the position of its highest set bit (1 for 0 and 1)
uint32_t ref_past(const int div[3]) {
    const unsigned __int128 full = (unsigned __int128)(unsigned long long)div[0] * (unsigned long long)div[1] *
                                   (unsigned long long)div[2];
    const unsigned long long wrapped = (unsigned long long)full;
    return wrapped >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)wrapped;
}
int ref_bits(uint32_t past) { return past < 2 ? 1 : 32 - __builtin_clz(past); }

// one cloud's bounds through the derivation and the restatement; returns the plan's kind
int grid_case(const float mn[3], const float mx[3], long long nfin, float lx, float ly, float lz) {
    const float leaf[3] = {lx, ly, lz};
    const Ref r = ref_grid(mn, mx, nfin, leaf);
    const sdr::VoxelGrid g = sdr::voxel_grid(mn, mx, nfin, lx, ly, lz);
    CHECK((int)g.kind == r.kind);
    CHECK((g.kind == sdr::VOXEL_EMPTY) == (r.kind == 0) && (g.kind == sdr::VOXEL_PASSTHROUGH) == (r.kind == 1));
    if (g.kind != sdr::VOXEL_GRID || r.kind != 2) return (int)g.kind;
    for (int c = 0; c < 3; c++) {
        const float inv = 1.0f / leaf[c];
        CHECK(std::memcmp(&g.v.inv[c], &inv, 4) == 0);
        CHECK(g.v.minb[c] == r.minb[c] && g.div[c] == r.div[c]);
    }
    CHECK(g.v.mul1 == r.mul1 && g.v.mul2 == r.mul2);
    CHECK(g.past == ref_past(r.div) && g.bits == ref_bits(g.past));
    CHECK(g.bits >= 1 && g.bits <= 32 && (g.bits == 32 || (g.past >> g.bits) == 0));
    return (int)g.kind;
}

void grid_cases() {
    const int EMPTY = sdr::VOXEL_EMPTY, PASS = sdr::VOXEL_PASSTHROUGH, GRID = sdr::VOXEL_GRID;
    {  // a single point: mn == mx, one voxel
        const float p[3] = {1.5f, -2.25f, 3.0f};
        CHECK(grid_case(p, p, 1, 0.1f, 0.1f, 0.1f) == GRID);
        const sdr::VoxelGrid g = sdr::voxel_grid(p, p, 1, 0.1f, 0.1f, 0.1f);
        CHECK(g.div[0] == 1 && g.div[1] == 1 && g.div[2] == 1 && g.past == 1 && g.bits == 1);
    }
    {  // negative coordinates: floor(-10.5) = -11 where truncation gives -10
        const float mn[3] = {-1.05f, -0.31f, -7.9f}, mx[3] = {-0.2f, 0.47f, -0.01f};
        CHECK(grid_case(mn, mx, 5, 0.1f, 0.07f, 0.3f) == GRID);
        const sdr::VoxelGrid g = sdr::voxel_grid(mn, mx, 5, 0.1f, 0.07f, 0.3f);
        CHECK(g.v.minb[0] == -11 && g.v.minb[2] == -27);
        // a box that straddles 0 by less than a leaf has PCL's d = 1 and div = 2
        const float a[3] = {-0.25f, -0.25f, -0.25f}, b[3] = {0.25f, 0.25f, 0.25f};
        CHECK(grid_case(a, b, 2, 1.0f, 1.0f, 1.0f) == GRID);
        CHECK(sdr::voxel_grid(a, b, 2, 1.0f, 1.0f, 1.0f).past == 8);
    }
    {  // PCL's product at exactly INT32_MAX and one above.  2147483647 is prime, and a count d is one
        // above a float, which 2147483646 is not: no leaf sizes give that product, so the compare
        // takes the counts directly; the nearest products leaf sizes do give follow
        const long long at[3] = {1, 1, 2147483647LL}, above[3] = {1, 2147483648LL, 1}, two31[3] = {1024, 1024, 2048};
        CHECK(!sdr::voxel_overflows(at));
        CHECK(sdr::voxel_overflows(above));
        CHECK(sdr::voxel_overflows(two31));
        const float mn[3] = {0.f, 0.f, 0.f}, below[3] = {1023.f, 1023.f, 2046.f}, over[3] = {1023.f, 1023.f, 2047.f};
        CHECK(grid_case(mn, below, 2, 1.0f, 1.0f, 1.0f) == GRID);  // 1024 * 1024 * 2047
        CHECK(grid_case(mn, over, 2, 1.0f, 1.0f, 1.0f) == PASS);   // 2^31: one above INT32_MAX
        const float top[3] = {0.f, 0.f, 2147483520.f}, past31[3] = {0.f, 0.f, 2147483648.f};
        CHECK(grid_case(mn, top, 2, 1.0f, 1.0f, 1.0f) == GRID);     // 2147483521, the largest count below
        CHECK(grid_case(mn, past31, 2, 1.0f, 1.0f, 1.0f) == PASS);  // 2147483649, the smallest above
        // the same two through the leaf size: 0.5 doubles the counts of a box of (511.5, 511.5, 1023[.5])
        const float h0[3] = {511.5f, 511.5f, 1023.0f}, h1[3] = {511.5f, 511.5f, 1023.5f};
        CHECK(grid_case(mn, h0, 2, 0.5f, 0.5f, 0.5f) == GRID);
        CHECK(grid_case(mn, h1, 2, 0.5f, 0.5f, 0.5f) == PASS);
    }
    {  // a product that wraps 64 bits: 2^66 wraps to 0 and 2^63 to a negative value, which both pass
        // the signed compare (a grid, as compiled PCL would run it); 2^62 does not wrap
        const long long w66[3] = {1LL << 22, 1LL << 22, 1LL << 22}, w63[3] = {1LL << 21, 1LL << 21, 1LL << 21};
        const long long big[3] = {1LL << 21, 1LL << 21, 1LL << 20};
        CHECK(!sdr::voxel_overflows(w66) && !sdr::voxel_overflows(w63) && sdr::voxel_overflows(big));
        const float mn[3] = {0.f, 0.f, 0.f}, m22[3] = {4194303.f, 4194303.f, 4194303.f};
        const float m21[3] = {2097151.f, 2097151.f, 2097151.f}, m20[3] = {2097151.f, 2097151.f, 1048575.f};
        CHECK(grid_case(mn, m22, 9, 1.0f, 1.0f, 1.0f) == GRID);
        const sdr::VoxelGrid g = sdr::voxel_grid(mn, m22, 9, 1.0f, 1.0f, 1.0f);
        CHECK(g.v.mul1 == (1u << 22) && g.v.mul2 == 0u && g.past == 0u && g.bits == 1);  // every product wrapped
        CHECK(grid_case(mn, m21, 9, 1.0f, 1.0f, 1.0f) == GRID);
        CHECK(sdr::voxel_grid(mn, m21, 9, 1.0f, 1.0f, 1.0f).past == 0xFFFFFFFFu);
        CHECK(grid_case(mn, m20, 9, 1.0f, 1.0f, 1.0f) == PASS);
    }
    {  // the clamp of `past`: divprod at 2^32 - 2, at 2^32 - 1 and above it
        const int lo[3] = {2, 1, 2147483647}, at[3] = {255, 257, 65537}, above[3] = {256, 256, 65537};
        CHECK(sdr::voxel_past(lo) == 0xFFFFFFFEu && ref_past(lo) == 0xFFFFFFFEu);
        CHECK(sdr::voxel_past(at) == 0xFFFFFFFFu && ref_past(at) == 0xFFFFFFFFu);
        CHECK(sdr::voxel_past(above) == 0xFFFFFFFFu && ref_past(above) == 0xFFFFFFFFu);
        // above it from real bounds: d = (1, 1, 2147483521) passes PCL's check with div = (2, 2, d)
        const float mn[3] = {-0.25f, -0.25f, 0.f}, mx[3] = {0.25f, 0.25f, 2147483520.f};
        CHECK(grid_case(mn, mx, 2, 1.0f, 1.0f, 1.0f) == GRID);
        const sdr::VoxelGrid g = sdr::voxel_grid(mn, mx, 2, 1.0f, 1.0f, 1.0f);
        CHECK(g.div[0] == 2 && g.div[1] == 2 && g.div[2] == 2147483521 && g.past == 0xFFFFFFFFu && g.bits == 32);
    }
    // the sort's width
    CHECK(sdr::voxel_sort_bits(1u) == 1 && sdr::voxel_sort_bits(255u) == 8 && sdr::voxel_sort_bits(256u) == 9);
    CHECK(sdr::voxel_sort_bits(1u << 31) == 32 && sdr::voxel_sort_bits(0xFFFFFFFFu) == 32 && sdr::voxel_sort_bits(0u) == 1);
    for (uint32_t p : {0u, 1u, 2u, 255u, 256u, 65535u, 65536u, 1u << 24, 1u << 31, 0xFFFFFFFEu, 0xFFFFFFFFu})
        CHECK(sdr::voxel_sort_bits(p) == ref_bits(p));
    {  // zero finite points: the reduction's identities come back, nothing is derived from them
        const float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        CHECK(grid_case(mn, mx, 0, 0.1f, 0.1f, 0.1f) == EMPTY);
    }
}

// ---- (b) the arena ----------------------------------------------------------------------------------
void arena_case(int n) {
    const sdr::VoxelArena a = sdr::voxel_arena(n);
    // the block counts, and the total the entry used to reserve
    const size_t un = (size_t)n;
    const int nb_rs = (n + sdr::kRsTile - 1) / sdr::kRsTile, nh = 256 * nb_rs;
    const int nb_scan = ((n > nh ? n : nh) + sdr::kScanSeg - 1) / sdr::kScanSeg;
    const size_t need = sizeof(float) * 7 * sdr::kMinMaxBlocks + un * (8 + 8 + 4 + 4 + 4 * 4) +
                        sizeof(int) * ((size_t)nh + nb_scan) + 11 * 256;
    CHECK(a.nb_rs == nb_rs && a.nh == nh && a.nb_scan == nb_scan);
    CHECK(a.total <= need);
    // every slice with the size the entry asked scratch.get() for
    const struct {
        sdr::VoxelArena::Slice s;
        size_t want;
    } slices[] = {{a.partial, sizeof(float) * 7 * sdr::kMinMaxBlocks}, {a.keys, 8 * un}, {a.sorted, 8 * un},
                  {a.head, 4 * un},  {a.pos, 4 * un},   {a.kv[0], 4 * un},         {a.kv[1], 4 * un},
                  {a.kv[2], 4 * un}, {a.kv[3], 4 * un}, {a.hist, 4 * (size_t)nh}, {a.spart, 4 * (size_t)nb_scan}};
    for (const auto& x : slices) {
        CHECK(x.s.off % 256 == 0);
        CHECK(x.s.bytes >= x.want && x.s.bytes > 0);
        CHECK(x.s.off + x.s.bytes <= a.total);
        for (const auto& y : slices)
            CHECK(&x == &y || x.s.off + x.s.bytes <= y.s.off || y.s.off + y.s.bytes <= x.s.off);
    }
    // a block of `total` bytes holds every slice's last byte (the sanitizer watches the writes)
    std::vector<char> block(a.total);
    for (const auto& x : slices) block[x.s.off] = block[x.s.off + x.s.bytes - 1] = 1;
}

}  // namespace

int main() {
    grid_cases();
    for (int n : {1, 255, 256, 257, sdr::kRsTile - 1, sdr::kRsTile, sdr::kRsTile + 1, sdr::kScanSeg - 1, sdr::kScanSeg + 1,
                  (1 << 20) + 3})
        arena_case(n);
    std::printf("voxel_plan_check: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
