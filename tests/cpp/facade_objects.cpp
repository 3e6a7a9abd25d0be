// The objects through include/sdr/stereo.hpp: sdr::Ruler::find_planes, then sdr::Ruler::find_objects
// of the pixels no plane claimed (label 255) above plane 0 over the whole map, then sdr::Ruler::relief
// of every object found under the label map find_objects returned.
// usage: facade_objects <W> <H> <max_planes> <hypotheses> <seed> <dir>
//   dir holds disp.bin (float HxW) and q.bin (double 16); writes planes.bin, objects.bin (the objects
//   found), scan.bin, labels.bin and relief.bin (a record an object) there.
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
    std::vector<uint8_t> disp = slurp(dir + "/disp.bin"), qb = slurp(dir + "/q.bin");
    if (disp.size() != (size_t)W * H * 4 || qb.size() != 128) return 3;
    static_assert(sizeof(sdr::Object) == 64 && sizeof(sdr::ObjectScan) == 64 && sizeof(sdr_object_params) == 64,
                  "record layout");
    try {
        sdr::Mat D = sdr::Mat::view(H, W, sdr::CV_32FC1, disp.data());
        sdr::Mat Q = sdr::Mat::view(4, 4, sdr::CV_64FC1, qb.data());
        sdr::Ruler ruler(Q);
        const sdr::Ruler::PlaneSearch s =
            ruler.find_planes(D, {0, 0}, {W - 1, H - 1}, nullptr, max_planes, hypotheses, seed, 3, 1.0f, 1000, true);
        const sdr_relief_query whole{0, 0, 0, W - 1, H - 1, 0, 255, 0};
        const sdr::Ruler::Objects o =
            ruler.find_objects(D, s.planes, whole, &s.labels, nullptr, 10.0f, 1000.0f, 1.0f, 8, 64, 4, true);
        std::vector<sdr_relief_query> qs;
        for (int k = 0; k < (int)o.objects.size(); k++) qs.push_back(sdr_relief_query{0, 0, 0, W - 1, H - 1, 0, k, 0});
        const std::vector<sdr::Relief> r = ruler.relief(D, s.planes, qs, &o.labels);
        if (!dump(dir + "/planes.bin", s.planes.data(), s.planes.size() * 128)) return 4;
        if (!dump(dir + "/objects.bin", o.objects.data(), o.objects.size() * 64)) return 4;
        if (!dump(dir + "/scan.bin", &o.scan, 64)) return 4;
        if (!dump(dir + "/labels.bin", o.labels.data, (size_t)W * H)) return 4;
        if (!dump(dir + "/relief.bin", r.data(), r.size() * 128)) return 4;
        std::printf("planes=%zu objects=%zu count=%d\n", s.planes.size(), o.objects.size(), o.scan.count);
        // the single-plane form (the defaults), and the call without a label map
        if (!s.planes.empty()) {
            const sdr::Ruler::Objects one = ruler.find_objects(D, s.planes[0], {0, 0}, {W - 1, H - 1}, &s.labels, 255);
            const sdr::Ruler::Objects same = ruler.find_objects(D, {s.planes[0]}, whole, &s.labels);
            std::printf("single_equal=%d\n", one.objects.size() == same.objects.size() &&
                                                 std::memcmp(&one.scan, &same.scan, 64) == 0 &&
                                                 std::memcmp(one.objects.data(), same.objects.data(),
                                                             one.objects.size() * 64) == 0 &&
                                                 std::memcmp(one.labels.data, same.labels.data, (size_t)W * H) == 0);
            const sdr::Ruler::Objects bare =
                ruler.find_objects(D, s.planes, whole, &s.labels, nullptr, 10.0f, 1000.0f, 1.0f, 8, 64, 4, false);
            std::printf("no_labels_equal=%d\n", bare.labels.data == nullptr &&
                                                    bare.objects.size() == o.objects.size() &&
                                                    std::memcmp(bare.objects.data(), o.objects.data(),
                                                                o.objects.size() * 64) == 0);
        }
        try {
            ruler.find_objects(D, s.planes, whole, &s.labels, nullptr, 10.0f, 1000.0f, 1.0f, 6);
            std::printf("bad_connectivity_code=0\n");
        } catch (const sdr::Exception& e) {
            std::printf("bad_connectivity_code=%d\n", e.code);
        }
    } catch (const sdr::Exception& e) {
        std::fprintf(stderr, "exception code=%d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
