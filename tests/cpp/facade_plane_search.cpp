// The plane search through include/sdr/stereo.hpp: sdr::Ruler::find_planes on a float disparity
// map with a confidence map.
// usage: facade_plane_search <W> <H> <x0> <y0> <x1> <y1> <max_planes> <hypotheses> <seed> <dir>
//   dir holds disp.bin (float HxW), conf.bin (float HxW), q.bin (double 16); writes planes.bin (the
//   planes found), rounds.bin and labels.bin there.
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
    if (argc != 11) return 2;
    const int W = std::stoi(argv[1]), H = std::stoi(argv[2]);
    const sdr::Point a{std::stoi(argv[3]), std::stoi(argv[4])}, b{std::stoi(argv[5]), std::stoi(argv[6])};
    const int max_planes = std::stoi(argv[7]), hypotheses = std::stoi(argv[8]);
    const uint32_t seed = (uint32_t)std::stoul(argv[9]);
    const std::string dir = argv[10];
    std::vector<uint8_t> disp = slurp(dir + "/disp.bin"), conf = slurp(dir + "/conf.bin"), qb = slurp(dir + "/q.bin");
    if (disp.size() != (size_t)W * H * 4 || conf.size() != disp.size() || qb.size() != 128) return 3;
    static_assert(sizeof(sdr::Plane) == 128 && sizeof(sdr_plane_search_round) == 16 &&
                      sizeof(sdr_plane_search_params) == 64,
                  "record layout");
    try {
        sdr::Mat D = sdr::Mat::view(H, W, sdr::CV_32FC1, disp.data());
        sdr::Mat C = sdr::Mat::view(H, W, sdr::CV_32FC1, conf.data());
        sdr::Mat Q = sdr::Mat::view(4, 4, sdr::CV_64FC1, qb.data());
        sdr::Ruler ruler(Q, 0, 1, -1.0f, 10.0f);
        const sdr::Ruler::PlaneSearch s = ruler.find_planes(D, a, b, &C, max_planes, hypotheses, seed, 2, 1.5f, 6, true);
        if (!dump(dir + "/planes.bin", s.planes.data(), s.planes.size() * 128)) return 4;
        if (!dump(dir + "/rounds.bin", s.rounds.data(), s.rounds.size() * 16)) return 4;
        if (s.labels.rows != H || s.labels.cols != W || s.labels.step != (size_t)W) return 5;
        if (!dump(dir + "/labels.bin", s.labels.data, (size_t)W * H)) return 4;
        std::printf("count=%zu rounds=%zu\n", s.planes.size(), s.rounds.size());
        // without labels: the same planes, no label map
        const sdr::Ruler::PlaneSearch t = ruler.find_planes(D, a, b, &C, max_planes, hypotheses, seed, 2, 1.5f, 6);
        std::printf("no_labels_equal=%d\n", t.labels.empty() && t.planes.size() == s.planes.size() &&
                                                 (s.planes.empty() || std::memcmp(t.planes.data(), s.planes.data(),
                                                                                  s.planes.size() * 128) == 0));
        try {
            ruler.find_planes(D, a, b, nullptr, 9);
            std::printf("bad_max_planes_code=0\n");
        } catch (const sdr::Exception& e) {
            std::printf("bad_max_planes_code=%d\n", e.code);
        }
    } catch (const sdr::Exception& e) {
        std::fprintf(stderr, "exception code=%d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
