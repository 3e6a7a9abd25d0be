// The plane fit through include/sdr/stereo.hpp: sdr::Ruler::fit_plane on a float disparity map
// with a confidence map, and plane_distance of points against the fitted planes.
// usage: facade_plane <W> <H> <K> <NQ> <radius> <min_count> <dir>
//   dir holds disp.bin (float HxW), conf.bin (float HxW), regs.bin (int32 Kx5), pts.bin (int32 NQx4),
//   q.bin (double 16); writes planes.bin and dist.bin there.
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
    const int W = std::stoi(argv[1]), H = std::stoi(argv[2]), K = std::stoi(argv[3]), NQ = std::stoi(argv[4]);
    const int radius = std::stoi(argv[5]), min_count = std::stoi(argv[6]);
    const std::string dir = argv[7];
    std::vector<uint8_t> disp = slurp(dir + "/disp.bin"), conf = slurp(dir + "/conf.bin");
    std::vector<uint8_t> regb = slurp(dir + "/regs.bin"), ptb = slurp(dir + "/pts.bin"), qb = slurp(dir + "/q.bin");
    if (disp.size() != (size_t)W * H * 4 || conf.size() != disp.size() || regb.size() != (size_t)K * 20 ||
        ptb.size() != (size_t)NQ * 16 || qb.size() != 128)
        return 3;
    static_assert(sizeof(sdr::Plane) == 128 && sizeof(sdr::PlaneDistance) == 32 && sizeof(sdr_plane_query) == 16,
                  "record layout");
    try {
        sdr::Mat D = sdr::Mat::view(H, W, sdr::CV_32FC1, disp.data());
        sdr::Mat C = sdr::Mat::view(H, W, sdr::CV_32FC1, conf.data());
        sdr::Mat Q = sdr::Mat::view(4, 4, sdr::CV_64FC1, qb.data());
        std::vector<sdr_segment> regs(K);
        std::memcpy(regs.data(), regb.data(), regb.size());
        std::vector<sdr_plane_query> pts(NQ);
        std::memcpy(pts.data(), ptb.data(), ptb.size());
        sdr::Ruler ruler(Q, radius, min_count, -1.0f, 10.0f);
        std::vector<sdr::Plane> planes = ruler.fit_plane(D, regs, &C, 2, 1.5f, 6);
        if (!dump(dir + "/planes.bin", planes.data(), planes.size() * 128)) return 4;
        std::vector<sdr::PlaneDistance> dist = ruler.plane_distance(D, planes, pts, &C);
        if (!dump(dir + "/dist.bin", dist.data(), dist.size() * 32)) return 4;
        // the single-region form equals the batch's first record
        const sdr::Plane one = ruler.fit_plane(D, sdr::Point{regs[0].x0, regs[0].y0},
                                               sdr::Point{regs[0].x1, regs[0].y1}, &C, 2, 1.5f, 6);
        const sdr::PlaneDistance d1 = ruler.plane_distance(D, one, sdr::Point{W / 2, H / 2}, &C);
        const sdr::PlaneDistance d2 =
            ruler.plane_distance(D, planes, {sdr_plane_query{0, W / 2, H / 2, 0}}, &C)[0];
        std::printf("single_equal=%d\n", std::memcmp(&one, &planes[0], 128) == 0 && std::memcmp(&d1, &d2, 32) == 0);
        try {
            ruler.fit_plane(D, regs, nullptr, 9);
            std::printf("bad_iterations_code=0\n");
        } catch (const sdr::Exception& e) {
            std::printf("bad_iterations_code=%d\n", e.code);
        }
    } catch (const sdr::Exception& e) {
        std::fprintf(stderr, "exception code=%d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
