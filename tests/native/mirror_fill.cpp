// mirror_fill.cpp -- tscm::stereo_fill and tscm::parse_fill_option of include/tscm/tscm_calib.hpp, driven by
// tests/test_gpu_cpp_mirror_fill.py.
//   mirror_fill in.bin out.bin [OPTION]
// in.bin: int32 width, height, min_disparity, rule, paths, max_distance, min_directions, wrap_x, then width * height int16.
// OPTION: the text of a demo's --fill, parsed over rule / max_distance / min_directions of the file.
// out.bin: width * height int16 (the filled map), then width * height bytes (the mask).
#include <cstdio>
#include <exception>
#include <vector>

#include "tscm/tscm_calib.hpp"

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin [RULE[,MAX_DISTANCE[,MIN_DIRECTIONS]]]\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    int head[8];
    if (!in || std::fread(head, sizeof(int), 8, in) != 8 || head[0] < 0 || head[1] < 0) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const tscm::Size size = { head[0], head[1] };
    std::vector<short> map((size_t)size.width * size.height);
    if (std::fread(map.data(), sizeof(short), map.size(), in) != map.size()) { std::fprintf(stderr, "%s is too short\n", argv[1]); return 2; }
    std::fclose(in);
    tscm_stereo_fill_params p;
    tscm_stereo_fill_default_params(&p);
    p.min_disparity = head[2]; p.rule = head[3]; p.paths = head[4]; p.max_distance = head[5]; p.min_directions = head[6]; p.wrap_x = head[7];
    if (argc > 3 && !tscm::parse_fill_option(argv[3], &p)) { std::fprintf(stderr, "bad option %s\n", argv[3]); return 2; }
    try {
        std::vector<unsigned char> mask;
        const std::vector<short> out = tscm::stereo_fill(map, size, &p, 0, &mask);
        std::FILE *f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(out.data(), sizeof(short), out.size(), f) != out.size() || std::fwrite(mask.data(), 1, mask.size(), f) != mask.size() || std::fclose(f)) {
            std::fprintf(stderr, "cannot write %s\n", argv[2]);
            return 2;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
