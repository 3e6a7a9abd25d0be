// layout_check.hip -- the scratch layout rule (csrc/sdr_layout.hpp) as a stand-alone host program,
// for a sanitizer build: the rule itself, the voxel arena against the rule as sdr_voxel_plan.hpp
// stated it before the header existed (restated here), and the slice lists of the device entries
// against the packed byte offsets those entries computed by hand.  Prints
// "layout_check: N checks, M failures"; exit status 1 on a failure.
//
//   hipcc --cuda-host-only -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -std=c++17 tests/cpp/layout_check.hip -o layout_check
#include "../../stereo_depth_ruler_amd/csrc/sdr_layout.hpp"
#include "../../stereo_depth_ruler_amd/csrc/sdr_voxel_plan.hpp"

#include <cstdio>
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

template <size_t N>
struct Bytes {
    char b[N];
};
using E48 = Bytes<48>;
using E3616 = Bytes<3616>;
struct Span {
    size_t off, bytes;
};

// a slice as (off, bytes), after the checks every slice passes alone
template <typename T>
Span span(const sdr::Slice<T>& s, size_t count) {
    CHECK(s.off % 256 == 0);
    CHECK(s.count == count && s.bytes() == count * sizeof(T) && s.end() == s.off + s.bytes());
    return {s.off, s.bytes()};
}

// slices in take order: each starts at or after the end of the one before, less than 256 bytes
// after it; `total` is the last one's end; a block of `total` bytes holds every slice's first and
// last byte (the sanitizer watches the writes)
void check_order(const std::vector<Span>& v, size_t total) {
    size_t end = 0;
    for (const Span& s : v) {
        CHECK(s.off >= end && s.off - end < 256);
        end = s.off + s.bytes;
    }
    CHECK(total == end);
    std::vector<char> block(total + 1);
    for (const Span& s : v)
        if (s.bytes) block[s.off] = block[s.off + s.bytes - 1] = 1;
}

// ---- (a) the rule ---------------------------------------------------------------------------------
void rule_cases() {
    CHECK(sdr::ScratchLayout().total == 0);
    for (size_t n : {(size_t)1, (size_t)3, (size_t)63, (size_t)64, (size_t)65, (size_t)255, (size_t)256, (size_t)257,
                     (size_t)4097}) {
        sdr::ScratchLayout L;
        std::vector<Span> v;
        v.push_back(span(L.take<unsigned char>(n), n));
        v.push_back(span(L.take<float>(n), n));
        v.push_back(span(L.take<long long>(n), n));
        v.push_back(span(L.take<E48>(n), n));
        v.push_back(span(L.take<E3616>(n), n));
        v.push_back(span(L.take<unsigned char>(1), 1));
        CHECK(v[0].off == 0);
        check_order(v, L.total);
    }
    {  // zero-count slices: first, in the middle, twice in a row and last
        sdr::ScratchLayout L;
        std::vector<Span> v;
        v.push_back(span(L.take<E3616>(0), 0));
        CHECK(v[0].off == 0 && L.total == 0);
        v.push_back(span(L.take<float>(5), 5));
        CHECK(v[1].off == 0 && L.total == 20);
        v.push_back(span(L.take<long long>(0), 0));
        v.push_back(span(L.take<E48>(0), 0));
        CHECK(v[2].off == 256 && v[3].off == 256 && L.total == 256);
        v.push_back(span(L.take<unsigned char>(257), 257));
        CHECK(v[4].off == 256 && L.total == 513);
        v.push_back(span(L.take<unsigned>(0), 0));
        CHECK(v[5].off == 768 && L.total == 768);
        check_order(v, L.total);
    }
}

// ---- (b) the voxel arena --------------------------------------------------------------------------
// the arena as sdr_voxel_plan.hpp laid it out with a rule of its own
void arena_case(int n) {
    const int nb_rs = (n + sdr::kRsTile - 1) / sdr::kRsTile, nh = 256 * nb_rs;
    const int nb_scan = ((n > nh ? n : nh) + sdr::kScanSeg - 1) / sdr::kScanSeg;
    size_t used = 0;
    auto take = [&used](size_t bytes) {
        const Span s{(used + 255) & ~(size_t)255, bytes};
        used = s.off + bytes;
        return s;
    };
    const size_t un = (size_t)n;
    std::vector<Span> want;
    want.push_back(take(sizeof(float) * 7 * sdr::kMinMaxBlocks));
    want.push_back(take(8 * un));
    want.push_back(take(8 * un));
    want.push_back(take(4 * un));
    want.push_back(take(4 * un));
    for (int q = 0; q < 4; q++) want.push_back(take(4 * un));
    want.push_back(take(4 * (size_t)nh));
    want.push_back(take(4 * (size_t)nb_scan));
    const sdr::VoxelArena a = sdr::voxel_arena(n);
    const sdr::VoxelArena::Slice got[] = {a.partial, a.keys, a.sorted, a.head, a.pos, a.kv[0],
                                          a.kv[1],   a.kv[2], a.kv[3],  a.hist, a.spart};
    CHECK(a.nb_rs == nb_rs && a.nh == nh && a.nb_scan == nb_scan);
    CHECK(want.size() == sizeof got / sizeof got[0]);
    for (size_t i = 0; i < want.size(); i++) CHECK(got[i].off == want[i].off && got[i].bytes == want[i].bytes);
    CHECK(a.total == used);
    check_order(want, a.total);
}

// ---- (c) the device entries' slice lists ----------------------------------------------------------
// A unit's slices as (element size, count) in take order, and the byte offset the entry computed by
// hand for each before the rule existed (packed; the plane search aligned two of them to 64): no
// slice starts before the one ahead of it ends, none is shorter than the old formula's, and the
// block grows by less than 256 bytes a slice.
struct Item {
    size_t elem, count, old_off;
};
void unit_case(const std::vector<Item>& items, size_t old_total) {
    sdr::ScratchLayout L;
    std::vector<Span> v;
    for (const Item& it : items) {
        Span s{};
        switch (it.elem) {
            case 1: s = span(L.take<unsigned char>(it.count), it.count); break;
            case 4: s = span(L.take<unsigned>(it.count), it.count); break;
            case 8: s = span(L.take<unsigned long long>(it.count), it.count); break;
            case 16: s = span(L.take<Bytes<16>>(it.count), it.count); break;
            case 48: s = span(L.take<E48>(it.count), it.count); break;
            case 272: s = span(L.take<Bytes<272>>(it.count), it.count); break;
            case 1568: s = span(L.take<Bytes<1568>>(it.count), it.count); break;
            case 3616: s = span(L.take<E3616>(it.count), it.count); break;
            default: CHECK(!"element size");
        }
        v.push_back(s);
    }
    check_order(v, L.total);
    for (size_t i = 0; i < items.size(); i++) {
        const size_t old_end = i + 1 < items.size() ? items[i + 1].old_off : old_total;
        CHECK(v[i].bytes == old_end - items[i].old_off);  // (these units packed their arrays)
        CHECK(v[i].off >= items[i].old_off);
    }
    CHECK(L.total >= old_total && L.total < old_total + 256 * items.size());
}

void unit_cases() {
    for (size_t px : {(size_t)1, (size_t)99, (size_t)12288, ((size_t)1 << 24)}) {
        // the objects: parents and sizes (int a pixel), candidates (u64), the tiles' and the slices'
        // counts (16 bytes each), the state (3616)
        for (size_t maxobj : {(size_t)1, (size_t)16, (size_t)64}) {
            const size_t slices = (px + 65535) / 65536 + 1, tiles = (px + 1023) / 1024;
            const size_t o_sz = px * 4, o_cand = 2 * o_sz, o_tiles = o_cand + slices * maxobj * 8;
            const size_t o_slices = o_tiles + tiles * 16, o_state = o_slices + slices * 16;
            unit_case({{4, px, 0}, {4, px, o_sz}, {8, slices * maxobj, o_cand}, {16, tiles, o_tiles},
                       {16, slices, o_slices}, {3616, 1, o_state}},
                      o_state + 3616);
        }
        // the speckle filter: labels and sizes (int a pixel) in one block of 8 bytes a pixel
        unit_case({{4, px, 0}, {4, px, 4 * px}}, 8 * px);
        // the plane search without a caller's label map: the state (40 bytes in a 64-byte slot), the
        // accumulators (i64), the scores (u32), the hypotheses (32 bytes, as four u64) at a multiple
        // of 64, the claim map (a byte a pixel)
        for (size_t NP : {(size_t)1, (size_t)8})
            for (size_t M : {(size_t)1, (size_t)63, (size_t)4096}) {
                const size_t per = 5 * 16, o_acc = 64, o_sc = o_acc + NP * per * 8;
                const size_t o_hyp = (o_sc + NP * M * 4 + 63) & ~(size_t)63, o_lab = o_hyp + M * 32;
                sdr::ScratchLayout L;
                const auto st = L.take<unsigned long long>(5);
                const auto acc = L.take<long long>(NP * per);
                const auto sc = L.take<unsigned>(NP * M);
                const auto hyp = L.take<unsigned long long>(4 * M);
                const auto lab = L.take<unsigned char>(px);
                CHECK(st.off == 0 && st.bytes() <= o_acc && acc.off >= o_acc && acc.bytes() == o_sc - o_acc);
                CHECK(sc.off >= o_sc && sc.end() <= hyp.off && hyp.off >= o_hyp && hyp.bytes() == o_lab - o_hyp);
                CHECK(lab.off >= o_lab && lab.bytes() == px && L.total >= o_lab + px && L.total < o_lab + px + 5 * 256);
                // the zeroed prefix ends where the hypotheses begin and covers state, accumulators and scores
                CHECK(hyp.off >= sc.end() && hyp.off % 256 == 0);
            }
    }
    // the relief: states (272 bytes), pass 1's histograms, pass 2's and pass 3's (u32); nq
    // may be 0, which leaves two empty slices at the end
    for (size_t KB : {(size_t)1, (size_t)7, (size_t)256})
        for (size_t nq : {(size_t)0, (size_t)3, (size_t)8}) {
            const size_t bins = 2048, last = 1024;  // only their products enter
            const size_t o_h1 = KB * 272, o_h2 = o_h1 + KB * bins * 4, o_h3 = o_h2 + KB * nq * bins * 4;
            unit_case({{272, KB, 0}, {4, KB * bins, o_h1}, {4, KB * nq * bins, o_h2}, {4, KB * nq * last, o_h3}},
                      o_h3 + KB * nq * last * 4);
        }
    // the footprint: the grids (u32 a cell), the states (1568 bytes)
    for (size_t KB : {(size_t)1, (size_t)16, (size_t)256})
        for (size_t G : {(size_t)16, (size_t)100, (size_t)512}) {
            const size_t o_st = KB * G * G * 4;
            unit_case({{4, KB * G * G, 0}, {1568, KB, o_st}}, o_st + KB * 1568);
        }
}

}  // namespace

int main() {
    rule_cases();
    for (int n : {1, 4096, 4097}) arena_case(n);
    unit_cases();
    std::printf("layout_check: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
