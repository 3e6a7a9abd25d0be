// The footprint through include/sdr/stereo.hpp: sdr::Ruler::find_planes, then sdr::Ruler::footprint
// of every plane found in plane 0 over the whole map, under its label and without a mask.
// usage: facade_footprint <W> <H> <max_planes> <hypotheses> <seed> <dir>
//   dir holds disp.bin (float HxW), conf.bin (float HxW), q.bin (double 16); writes planes.bin,
//   labels.bin and footprint.bin (2 records a plane found) there.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "sdr/stereo.hpp"

static std::vector<uint8_t> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), {});
}

static bool dump(const std::string& p, const void* d, size_t n) {
    std::ofstream f(p, std::ios::binary);
    f.write((const char*)d, (std::streamsize)n);
    return (bool)f;
}

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int W = std::stoi(argv[1]), H = std::stoi(argv[2]);
    const int max_planes = std::stoi(argv[3]), hypotheses = std::stoi(argv[4]);
    const uint32_t seed = (uint32_t)std::stoul(argv[5]);
    const std::string dir = argv[6];
    std::vector<uint8_t> disp = slurp(dir + "/disp.bin"), conf = slurp(dir + "/conf.bin"), qb = slurp(dir + "/q.bin");
    if (disp.size() != (size_t)W * H * 4 || conf.size() != disp.size() || qb.size() != 128) return 3;
    static_assert(sizeof(sdr::Footprint) == 256 && sizeof(sdr_relief_query) == 32 && sizeof(sdr_footprint_params) == 64,
                  "record layout");
    try {
        sdr::Mat D = sdr::Mat::view(H, W, sdr::CV_32FC1, disp.data());
        sdr::Mat C = sdr::Mat::view(H, W, sdr::CV_32FC1, conf.data());
        sdr::Mat Q = sdr::Mat::view(4, 4, sdr::CV_64FC1, qb.data());
        sdr::Ruler ruler(Q, 0, 1, -1.0f, 10.0f);
        const sdr::Ruler::PlaneSearch s =
            ruler.find_planes(D, {0, 0}, {W - 1, H - 1}, &C, max_planes, hypotheses, seed, 2, 1.5f, 6, true);
        std::vector<sdr_relief_query> qs;
        for (int i = 0; i < (int)s.planes.size(); i++) {
            qs.push_back(sdr_relief_query{0, W - 1, 0, 0, H - 1, 0, i, 0});
            qs.push_back(sdr_relief_query{0, 0, 0, W - 1, H - 1, i, -1, 0});
        }
        const std::vector<sdr::Footprint> r = ruler.footprint(D, s.planes, qs, &s.labels, &C, 8.0f, 128, 3, -500.0f, 500.0f);
        if (!dump(dir + "/planes.bin", s.planes.data(), s.planes.size() * 128)) return 4;
        if (!dump(dir + "/labels.bin", s.labels.data, (size_t)W * H)) return 4;
        if (!dump(dir + "/footprint.bin", r.data(), r.size() * 256)) return 4;
        std::printf("planes=%zu footprints=%zu\n", s.planes.size(), r.size());
        // the single-record form: the defaults
        if (!s.planes.empty()) {
            const sdr::Footprint one = ruler.footprint(D, s.planes[0], {0, 0}, {W - 1, H - 1}, &s.labels, 0, &C);
            const std::vector<sdr::Footprint> same =
                ruler.footprint(D, {s.planes[0]}, {sdr_relief_query{0, 0, 0, W - 1, H - 1, 0, 0, 0}}, &s.labels, &C);
            std::printf("single_equal=%d\n", std::memcmp(&one, same.data(), 256) == 0 && (one.flags & SDR_FOOTPRINT_VALID));
        }
        try {
            ruler.footprint(D, s.planes, qs, nullptr, nullptr, 4.0f, 15);
            std::printf("bad_grid_code=0\n");
        } catch (const sdr::Exception& e) {
            std::printf("bad_grid_code=%d\n", e.code);
        }
    } catch (const sdr::Exception& e) {
        std::fprintf(stderr, "exception code=%d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
