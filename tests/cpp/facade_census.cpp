// The census cost type through include/sdr/stereo.hpp: setCostType + compute against the Python
// surface's result, createRightMatcher copying the cost type.
// usage: facade_census <W> <H> <D> <P1> <P2> <dir>   (dir holds l.bin r.bin want.bin want_r.bin)
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

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int W = std::stoi(argv[1]), H = std::stoi(argv[2]), D = std::stoi(argv[3]);
    const int P1 = std::stoi(argv[4]), P2 = std::stoi(argv[5]);
    const std::string dir = argv[6];
    std::vector<uint8_t> l = slurp(dir + "/l.bin"), r = slurp(dir + "/r.bin");
    std::vector<uint8_t> want = slurp(dir + "/want.bin"), want_r = slurp(dir + "/want_r.bin");
    const size_t nd = (size_t)W * H * 2;
    if (l.size() != (size_t)W * H || r.size() != l.size() || want.size() != nd || want_r.size() != nd) return 3;
    try {
        sdr::Mat L = sdr::Mat::view(H, W, sdr::CV_8UC1, l.data()), R = sdr::Mat::view(H, W, sdr::CV_8UC1, r.data());
        auto sgbm = sdr::StereoSGBM::create(0, D, 5, P1, P2, 1, 0, 12, 0, 0, sdr::StereoSGBM::MODE_SGBM_3WAY);
        const bool was_bt = sgbm->getCostType() == sdr::StereoSGBM::COST_BT;
        sgbm->setCostType(sdr::StereoSGBM::COST_CENSUS);
        std::printf("cost_roundtrip=%d\n", was_bt && sgbm->getCostType() == sdr::StereoSGBM::COST_CENSUS);
        sdr::Mat disp;
        sgbm->compute(L, R, disp);
        std::printf("census_equal=%d\n", std::memcmp(disp.data, want.data(), nd) == 0);
        auto right = sdr::ximgproc::createRightMatcher(sgbm);
        sdr::Mat disp_r;
        right->compute(R, L, disp_r);
        std::printf("right_equal=%d\n", right->getCostType() == sdr::StereoSGBM::COST_CENSUS &&
                                           std::memcmp(disp_r.data, want_r.data(), nd) == 0);
        try {
            sgbm->setCostType(7);
            std::printf("bad_cost_code=0\n");
        } catch (const sdr::Exception& e) {
            std::printf("bad_cost_code=%d\n", e.code);
        }
    } catch (const sdr::Exception& e) {
        std::fprintf(stderr, "exception code=%d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
