// The ruler over time through include/sdr/stereo.hpp: sdr::Ruler::fuse of F frames with their
// confidence maps, in both modes, then sdr::Ruler::measure on the fused map.
// usage: facade_fuse <W> <H> <F> <dir>
//   dir holds stack.bin (float FxHxW), conf.bin (float FxHxW) and q.bin (double 16); writes
//   mean.bin, median.bin (float HxW each), support.bin (uint8 HxW), spread.bin (float HxW),
//   records.bin (two sdr_fusion: mean, median) and measure.bin (one sdr_measurement) there.
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
    if (argc != 5) return 2;
    const int W = std::stoi(argv[1]), H = std::stoi(argv[2]), F = std::stoi(argv[3]);
    const std::string dir = argv[4];
    std::vector<uint8_t> stack = slurp(dir + "/stack.bin"), conf = slurp(dir + "/conf.bin"), qb = slurp(dir + "/q.bin");
    const size_t frame = (size_t)W * H * 4;
    if (stack.size() != frame * F || conf.size() != frame * F || qb.size() != 128) return 3;
    static_assert(sizeof(sdr_fusion) == 64 && sizeof(sdr_fuse_params) == 32, "record layout");
    try {
        sdr::Mat Q = sdr::Mat::view(4, 4, sdr::CV_64FC1, qb.data());
        std::vector<sdr::Mat> frames, confs;
        for (int k = 0; k < F; k++) {
            frames.push_back(sdr::Mat::view(H, W, sdr::CV_32FC1, stack.data() + k * frame));
            confs.push_back(sdr::Mat::view(H, W, sdr::CV_32FC1, conf.data() + k * frame));
        }
        sdr::Ruler ruler(Q, 0, 1, -1.0f, 100.0f);
        const sdr::Ruler::Fused mean = ruler.fuse(frames, confs, 1.0f, 2, SDR_FUSE_MEAN, nullptr, true);
        const float nan = std::numeric_limits<float>::quiet_NaN();
        const sdr::Ruler::Fused median = ruler.fuse(frames, confs, 0.5f, 3, SDR_FUSE_MEDIAN, &nan);
        const sdr_fusion recs[2] = {mean.record, median.record};
        const sdr::Measurement m = ruler.measure(mean.map, {1, 1}, {W - 2, H - 2});
        if (!dump(dir + "/mean.bin", mean.map.data, frame) || !dump(dir + "/median.bin", median.map.data, frame) ||
            !dump(dir + "/support.bin", mean.support.data, (size_t)W * H) ||
            !dump(dir + "/spread.bin", mean.spread.data, frame) || !dump(dir + "/records.bin", recs, sizeof recs) ||
            !dump(dir + "/measure.bin", &m, sizeof m))
            return 4;
        std::printf("fused=%d median_has_maps=%d\n", mean.record.n_fused, !median.support.empty());
        // frames of two sizes, a fill that is a valid disparity, and more frames than the entry takes
        try {
            std::vector<sdr::Mat> odd = frames;
            odd.push_back(sdr::Mat::view(H - 1, W, sdr::CV_32FC1, stack.data()));
            ruler.fuse(odd);
            std::printf("odd_code=0\n");
        } catch (const sdr::Exception& e) {
            std::printf("odd_code=%d\n", e.code);
        }
        try {
            const float measured = 5.0f;
            ruler.fuse(frames, {}, 1.0f, 2, SDR_FUSE_MEAN, &measured);
            std::printf("fill_code=0\n");
        } catch (const sdr::Exception& e) {
            std::printf("fill_code=%d\n", e.code);
        }
        try {
            ruler.fuse(std::vector<sdr::Mat>(33, frames[0]));
            std::printf("many_code=0\n");
        } catch (const sdr::Exception& e) {
            std::printf("many_code=%d\n", e.code);
        }
    } catch (const sdr::Exception& e) {
        std::fprintf(stderr, "exception code=%d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
