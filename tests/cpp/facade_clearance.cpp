// The clearance through include/sdr/stereo.hpp: sdr::Ruler::find_planes for the floor, then
// sdr::Ruler::find_objects of the pixels it did not claim (label 255), then sdr::Ruler::clearance
// between objects 0 and 1 in both orders under the label map find_objects returned, the ruler
// sampling with radius 2 and min_count 9.
// usage: facade_clearance <W> <H> <dir>
//   dir holds disp.bin (float HxW) and q.bin (double 16); writes clearance.bin (two records) there.
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
    if (argc != 4) return 2;
    const int W = std::stoi(argv[1]), H = std::stoi(argv[2]);
    const std::string dir = argv[3];
    std::vector<uint8_t> disp = slurp(dir + "/disp.bin"), qb = slurp(dir + "/q.bin");
    if (disp.size() != (size_t)W * H * 4 || qb.size() != 128) return 3;
    static_assert(sizeof(sdr::Clearance) == 128 && sizeof(sdr_clearance_params) == 64 &&
                      sizeof(sdr_clearance_query) == 32,
                  "record layout");
    try {
        sdr::Mat D = sdr::Mat::view(H, W, sdr::CV_32FC1, disp.data());
        sdr::Mat Q = sdr::Mat::view(4, 4, sdr::CV_64FC1, qb.data());
        sdr::Ruler ruler(Q, 2, 9);
        const sdr::Ruler::PlaneSearch s = ruler.find_planes(D, {0, 0}, {W - 1, H - 1}, nullptr, 1, 256, 0, 3, 1.0f, 1000, true);
        const sdr_relief_query whole{0, 0, 0, W - 1, H - 1, 0, 255, 0};
        const sdr::Ruler::Objects o =
            ruler.find_objects(D, s.planes, whole, &s.labels, nullptr, 10.0f, 1000.0f, 1.0f, 8, 64, 4, true);
        const std::vector<sdr::Clearance> c = ruler.clearance(
            D, s.planes, {sdr_clearance_query{0, 0, 0, W - 1, H - 1, 0, 0, 1}, sdr_clearance_query{0, 0, 0, W - 1, H - 1, 0, 1, 0}},
            o.labels);
        if (!dump(dir + "/clearance.bin", c.data(), c.size() * 128)) return 4;
        std::printf("objects=%zu valid=%d\n", o.objects.size(),
                    c[0].flags == SDR_CLEARANCE_VALID && c[1].flags == SDR_CLEARANCE_VALID);
        // the single-pair form, a refused pair, and a map that is no label map
        if (!s.planes.empty()) {
            const sdr::Clearance one = ruler.clearance(D, s.planes[0], {0, 0}, {W - 1, H - 1}, o.labels, 0, 1);
            std::printf("single_equal=%d\n", std::memcmp(&one, &c[0], 128) == 0);
            const sdr::Clearance same = ruler.clearance(D, s.planes[0], {0, 0}, {W - 1, H - 1}, o.labels, 1, 1);
            std::printf("same_label_flags=%u\n", same.flags);
        }
        try {
            ruler.clearance(D, s.planes, {sdr_clearance_query{0, 0, 0, W - 1, H - 1, 0, 0, 1}}, sdr::Mat());
            std::printf("bad_labels_code=0\n");
        } catch (const sdr::Exception& e) {
            std::printf("bad_labels_code=%d\n", e.code);
        }
    } catch (const sdr::Exception& e) {
        std::fprintf(stderr, "exception code=%d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
