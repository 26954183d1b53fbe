// mirror_visibility.cpp -- tscm::Sweep::visibility, the tscm::Sweep::compose overload under visibility and
// tscm::parse_visibility_option of include/tscm/tscm_calib.hpp, driven by tests/test_gpu_cpp_mirror_visibility.py.
//   mirror_visibility calib.yaml in.bin out.bin [OPTION]
// in.bin: int32 width, height (source images), pano_w, pano_h, hypotheses, paths, channels, mode, cell_shift, tolerance,
// dilate, near_is_high, with_map; one double near; n grey images (the depth pass); n images of `channels` bytes per pixel
// (the frame); with_map = 1: pano_w * pano_h int16, the index map both calls get; 0: they take the map that depth() left on
// the device.  n: the cameras of calib.yaml.  An empty in.bin parses OPTION and does nothing else.
// OPTION: the text of the demo's --visibility, parsed over cell_shift / tolerance / dilate of the file.
// out.bin: n * pano_w * pano_h bytes (use), pano_w * pano_h bytes (state), pano_w * pano_h * channels bytes (the frame).
#include <cstdio>
#include <exception>
#include <vector>

#include "tscm/tscm_calib.hpp"

static bool read_all(std::FILE *f, void *dst, size_t size, size_t count) { return std::fread(dst, size, count, f) == count; }

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s calib.yaml in.bin out.bin [SHIFT,TOLERANCE[,DILATE]]\n", argv[0]); return 2; }
    tscm_sweep_visibility_params vp;
    tscm_sweep_visibility_default_params(&vp);
    std::FILE *in = std::fopen(argv[2], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    int head[13];
    double near = 0.0;
    const size_t got = std::fread(head, sizeof(int), 13, in);
    if (got == 0) {                                             // nothing to compute: the option alone
        std::fclose(in);
        if (argc > 4 && !tscm::parse_visibility_option(argv[4], &vp)) { std::fprintf(stderr, "bad option %s\n", argv[4]); return 2; }
        std::printf("%d %d %d\n", vp.cell_shift, vp.tolerance, vp.dilate);
        return 0;
    }
    if (got != 13 || !read_all(in, &near, sizeof(double), 1) || head[0] < 1 || head[1] < 1 || head[2] < 1 || head[3] < 1 || head[4] < 2 || (head[6] != 1 && head[6] != 3)) {
        std::fprintf(stderr, "%s: bad header\n", argv[2]);
        return 2;
    }
    vp.cell_shift = head[8]; vp.tolerance = head[9]; vp.dilate = head[10]; vp.near_is_high = head[11];
    if (argc > 4 && !tscm::parse_visibility_option(argv[4], &vp)) { std::fprintf(stderr, "bad option %s\n", argv[4]); return 2; }
    try {
        enum { kMaxCameras = 8 };
        std::vector<double> intr(9 * kMaxCameras), Twc(12 * kMaxCameras);
        int n = 0;
        tscm::check(tscm_yaml_read(argv[1], kMaxCameras, &n, intr.data(), Twc.data()));
        const tscm::Size size = { head[0], head[1] }, pano = { head[2], head[3] };
        const int D = head[4], channels = head[6];
        const size_t px = (size_t)size.width * size.height, ppx = (size_t)pano.width * pano.height;
        std::vector<std::vector<unsigned char> > grey((size_t)n, std::vector<unsigned char>(px)), frame((size_t)n, std::vector<unsigned char>(px * channels));
        std::vector<const unsigned char *> gptr((size_t)n), fptr((size_t)n);
        for (int k = 0; k < n; ++k) {
            if (!read_all(in, grey[(size_t)k].data(), 1, px)) { std::fprintf(stderr, "%s is too short\n", argv[2]); return 2; }
            gptr[(size_t)k] = grey[(size_t)k].data();
        }
        for (int k = 0; k < n; ++k) {
            if (!read_all(in, frame[(size_t)k].data(), 1, px * channels)) { std::fprintf(stderr, "%s is too short\n", argv[2]); return 2; }
            fptr[(size_t)k] = frame[(size_t)k].data();
        }
        std::vector<short> map(head[12] ? ppx : 0);
        if (head[12] && !read_all(in, map.data(), sizeof(short), ppx)) { std::fprintf(stderr, "%s is too short\n", argv[2]); return 2; }
        std::fclose(in);
        std::vector<double> inv((size_t)D);
        for (int z = 0; z < D; ++z) inv[(size_t)z] = (double)z / ((double)(D - 1) * near);
        tscm_sweep_params sp;
        tscm_sweep_default_params(&sp);
        sp.num_hypotheses = D; sp.paths = head[5];
        tscm_sweep_compose_params cp;
        tscm_sweep_compose_default_params(&cp);
        cp.mode = head[7];
        tscm::Sweep sweep(n, intr.data(), Twc.data(), size, pano, inv, &sp);
        sweep.depth(gptr.data());
        const std::vector<short> *at = head[12] ? &map : NULL;
        std::vector<unsigned char> state;
        const std::vector<unsigned char> use = sweep.visibility(at, &vp, &state);
        const std::vector<unsigned char> out = sweep.compose(fptr.data(), channels, at, &cp, vp);
        std::FILE *f = std::fopen(argv[3], "wb");
        if (!f || std::fwrite(use.data(), 1, use.size(), f) != use.size() || std::fwrite(state.data(), 1, state.size(), f) != state.size() ||
            std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fclose(f)) {
            std::fprintf(stderr, "cannot write %s\n", argv[3]);
            return 2;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
