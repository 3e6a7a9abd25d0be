// The ruler through include/sdr/stereo.hpp: sdr::Ruler on a float disparity map with a confidence
// map (records + profile), measure_xyz on the reprojected map, and the MeasurementLog's CSV.
// usage: facade_ruler <W> <H> <K> <radius> <min_count> <cap> <dir>
//   dir holds disp.bin (float HxW), conf.bin (float HxW), segs.bin (int32 Kx5), q.bin (double 16);
//   writes rec.bin, prof.bin, rec_xyz.bin, log.csv there.
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
    if (argc != 8) return 2;
    const int W = std::stoi(argv[1]), H = std::stoi(argv[2]), K = std::stoi(argv[3]);
    const int radius = std::stoi(argv[4]), min_count = std::stoi(argv[5]), cap = std::stoi(argv[6]);
    const std::string dir = argv[7];
    std::vector<uint8_t> disp = slurp(dir + "/disp.bin"), conf = slurp(dir + "/conf.bin");
    std::vector<uint8_t> segb = slurp(dir + "/segs.bin"), qb = slurp(dir + "/q.bin");
    if (disp.size() != (size_t)W * H * 4 || conf.size() != disp.size() || segb.size() != (size_t)K * 20 ||
        qb.size() != 128)
        return 3;
    static_assert(sizeof(sdr::Measurement) == 80 && sizeof(sdr_segment) == 20, "record layout");
    try {
        sdr::Mat D = sdr::Mat::view(H, W, sdr::CV_32FC1, disp.data());
        sdr::Mat C = sdr::Mat::view(H, W, sdr::CV_32FC1, conf.data());
        sdr::Mat Q = sdr::Mat::view(4, 4, sdr::CV_64FC1, qb.data());
        std::vector<sdr_segment> segs(K);
        std::memcpy(segs.data(), segb.data(), segb.size());
        sdr::Ruler ruler(Q, radius, min_count, -1.0f, 10.0f, true);
        std::vector<float> prof;
        std::vector<sdr::Measurement> rec = ruler.measure(D, segs, &C, &prof, cap);
        if (!dump(dir + "/rec.bin", rec.data(), rec.size() * 80) || !dump(dir + "/prof.bin", prof.data(), prof.size() * 4))
            return 4;
        // the single-segment form equals the batch's first record
        const sdr::Measurement one =
            ruler.measure(D, sdr::Point{segs[0].x0, segs[0].y0}, sdr::Point{segs[0].x1, segs[0].y1}, &C);
        std::printf("single_equal=%d\n", std::memcmp(&one, &rec[0], 80) == 0);
        // the reference's measurement on the reprojected map
        sdr::Mat xyz;
        sdr::reprojectImageTo3D(D, xyz, Q);
        std::vector<sdr::Measurement> rx = sdr::Ruler(Q).measure_xyz(xyz, segs);
        if (!dump(dir + "/rec_xyz.bin", rx.data(), rx.size() * 80)) return 4;
        sdr::MeasurementLog log;
        for (int k = 0; k < K; k++)
            log.add(100 + k, rec[k], sdr::Point{segs[k].x0, segs[k].y0}, sdr::Point{segs[k].x1, segs[k].y1});
        log.save_csv(dir + "/log.csv");
        std::printf("log_size=%zu\n", log.size());
        try {
            sdr::Ruler(Q, 5).measure(D, segs);
            std::printf("bad_radius_code=0\n");
        } catch (const sdr::Exception& e) {
            std::printf("bad_radius_code=%d\n", e.code);
        }
    } catch (const sdr::Exception& e) {
        std::fprintf(stderr, "exception code=%d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
