// mirror_refine.cpp -- tscm::stereo_refine, tscm::range_weights and tscm::parse_refine_option of include/tscm/tscm_calib.hpp,
// driven by tests/test_gpu_cpp_mirror_refine.py.
//   mirror_refine in.bin out.bin [OPTION]
// in.bin: int32 width, height, min_disparity, radius, iterations, fill_invalid, wrap_x, then one double sigma (negative: no
// table, every weight 255), then width * height int16 (the map), then width * height bytes (the guide).
// OPTION: the text of a demo's --refine, parsed over radius / iterations / fill_invalid and sigma of the file.
// out.bin: width * height int16 (the refined map).
#include <cstdio>
#include <exception>
#include <vector>

#include "tscm/tscm_calib.hpp"

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin [RADIUS,SIGMA[,ITERATIONS[,FILL]]]\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    int head[7];
    double sigma = 0.0;
    if (!in || std::fread(head, sizeof(int), 7, in) != 7 || std::fread(&sigma, sizeof(double), 1, in) != 1 || head[0] < 0 || head[1] < 0) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const tscm::Size size = { head[0], head[1] };
    std::vector<short> map((size_t)size.width * size.height);
    std::vector<unsigned char> guide(map.size());
    if (std::fread(map.data(), sizeof(short), map.size(), in) != map.size() || std::fread(guide.data(), 1, guide.size(), in) != guide.size()) {
        std::fprintf(stderr, "%s is too short\n", argv[1]);
        return 2;
    }
    std::fclose(in);
    tscm_stereo_refine_params p;
    tscm_stereo_refine_default_params(&p);
    p.min_disparity = head[2]; p.radius = head[3]; p.iterations = head[4]; p.fill_invalid = head[5]; p.wrap_x = head[6];
    if (argc > 3 && !tscm::parse_refine_option(argv[3], &p, &sigma)) { std::fprintf(stderr, "bad option %s\n", argv[3]); return 2; }
    try {
        const std::vector<unsigned char> table = tscm::range_weights(sigma);
        const std::vector<short> out = tscm::stereo_refine(map, guide, size, sigma < 0.0 ? NULL : &table, &p);
        std::FILE *f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(out.data(), sizeof(short), out.size(), f) != out.size() || std::fclose(f)) {
            std::fprintf(stderr, "cannot write %s\n", argv[2]);
            return 2;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
