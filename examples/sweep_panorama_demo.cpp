// sweep_panorama_demo.cpp -- the parallax-free panorama of a calibrated rig: the sphere sweep gives the depth of every
// panorama pixel (tscm_sweep_depth, on the grey values of the frame), and the frame is blended at that depth
// (tscm_sweep_compose) instead of at infinity, so that near objects are not doubled where two cameras overlap.
// Images are binary PGM (P5, grey) or PPM (P6, read as 3 channels in file order) files of one size and kind, one per camera.
//   usage: sweep_panorama_demo calib.yaml cam0.ppm cam1.ppm ... [--size W H] [--near N] [--hypotheses D] [--paths 4|8]
//                              [--mode seam|feather|multiband] [--levels L] [--fill RULE[,MAX_DISTANCE[,MIN_DIRECTIONS]]]
//                              [--refine RADIUS,SIGMA[,ITERATIONS[,FILL]]] [--visibility SHIFT,TOLERANCE[,DILATE]]
// --fill: every pixel without depth gets the lowest | second_lowest | median of the nearest valid indices along the 8 path
// directions, over the seam too (tscm_stereo_fill with wrap_x = 1), and the frame is composed at the filled map.
// --refine: after that, the weighted median of every pixel's (2 RADIUS + 1)^2 window, over the seam too (tscm_stereo_refine
// with wrap_x = 1), a neighbour weighted by exp(-|difference of grey values| / SIGMA) in the grey frame composed by seam at
// the map as it stands, in ITERATIONS passes (1); FILL 1 gives pixels without depth a value too (0).  The frame is composed
// at the refined map.
// --visibility: the frame is composed under per-camera visibility (tscm_sweep_compose_visible): at every pixel a camera that
// looks at the point through something nearer -- by more than TOLERANCE hypotheses, in a depth buffer of 2^SHIFT x 2^SHIFT
// source pixels per cell, read over (2 DILATE + 1)^2 cells (DILATE 0) -- is left out, unless no camera would remain.
// writes sweep_panorama.pgm or .ppm into the working directory.  near: in the units of the calibration's translations.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "tscm/tscm_calib.hpp"

// P5 -> 1 channel, P6 -> 3 channels
static bool read_pnm(const char *path, std::vector<unsigned char> &pix, int &w, int &h, int &channels)
{
    std::ifstream f(path, std::ios::binary);
    std::string magic;
    int maxval = 0;
    if (!(f >> magic >> w >> h >> maxval) || (magic != "P5" && magic != "P6") || maxval != 255 || w < 1 || h < 1) return false;
    f.get();
    channels = magic == "P5" ? 1 : 3;
    pix.resize((size_t)w * h * channels);
    f.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size());
    return (size_t)f.gcount() == pix.size();
}

int main(int argc, char **argv)
{
    std::vector<const char *> files;
    tscm::Size pano = { 1024, 512 };
    double near = 500.0;
    tscm_sweep_params params;
    tscm_sweep_default_params(&params);
    tscm_sweep_compose_params blend;
    tscm_sweep_compose_default_params(&blend);
    bool bad = false, fill = false, refine = false, visible = false;
    tscm_sweep_visibility_params vis_params;
    tscm_sweep_visibility_default_params(&vis_params);
    tscm_stereo_fill_params fill_params;
    tscm_stereo_fill_default_params(&fill_params);
    fill_params.wrap_x = 1;
    tscm_stereo_refine_params refine_params;
    tscm_stereo_refine_default_params(&refine_params);
    refine_params.wrap_x = 1;
    double sigma = 0.0;
    for (int a = 2; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--size") && a + 2 < argc) { pano.width = std::atoi(argv[a + 1]); pano.height = std::atoi(argv[a + 2]); a += 2; }
        else if (!std::strcmp(argv[a], "--near") && a + 1 < argc) near = std::atof(argv[++a]);
        else if (!std::strcmp(argv[a], "--hypotheses") && a + 1 < argc) params.num_hypotheses = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--paths") && a + 1 < argc) params.paths = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--levels") && a + 1 < argc) blend.levels = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--fill") && a + 1 < argc) { fill = true; bad |= !tscm::parse_fill_option(argv[++a], &fill_params); }
        else if (!std::strcmp(argv[a], "--refine") && a + 1 < argc) { refine = true; bad |= !tscm::parse_refine_option(argv[++a], &refine_params, &sigma); }
        else if (!std::strcmp(argv[a], "--visibility") && a + 1 < argc) { visible = true; bad |= !tscm::parse_visibility_option(argv[++a], &vis_params); }
        else if (!std::strcmp(argv[a], "--mode") && a + 1 < argc) {
            const std::string m = argv[++a];
            if (m == "seam") blend.mode = TSCM_PANO_SEAM;
            else if (m == "feather") blend.mode = TSCM_PANO_FEATHER;
            else if (m == "multiband") blend.mode = TSCM_PANO_MULTIBAND;
            else bad = true;
        } else files.push_back(argv[a]);
    }
    if (bad || argc < 4 || files.size() < 2 || !(near > 0.0) || params.num_hypotheses < 2) {
        std::fprintf(stderr, "usage: %s calib.yaml cam0.ppm cam1.ppm ... [--size W H] [--near N] [--hypotheses D] [--paths 4|8] [--mode seam|feather|multiband] [--levels L] [--fill RULE[,MAX_DISTANCE[,MIN_DIRECTIONS]]] [--refine RADIUS,SIGMA[,ITERATIONS[,FILL]]] [--visibility SHIFT,TOLERANCE[,DILATE]]\n",
                     argv[0]);
        return 2;
    }
    try {
        enum { kMaxCameras = 8 };
        std::vector<double> intr(9 * kMaxCameras), Twc(12 * kMaxCameras);
        int n = 0;
        tscm::check(tscm_yaml_read(argv[1], kMaxCameras, &n, intr.data(), Twc.data()));
        if ((int)files.size() != n) { std::fprintf(stderr, "%s has %d cameras, %d images given\n", argv[1], n, (int)files.size()); return 2; }
        std::vector<std::vector<unsigned char> > img((size_t)n), grey((size_t)n);
        std::vector<const unsigned char *> ptr((size_t)n), gptr((size_t)n);
        tscm::Size size = { 0, 0 };
        int channels = 0;
        for (int k = 0; k < n; ++k) {
            int w = 0, h = 0, ch = 0;
            if (!read_pnm(files[(size_t)k], img[(size_t)k], w, h, ch)) { std::fprintf(stderr, "%s: not a binary 8-bit PGM or PPM\n", files[(size_t)k]); return 2; }
            if (k && (w != size.width || h != size.height || ch != channels)) { std::fprintf(stderr, "%s: the images differ in size or kind\n", files[(size_t)k]); return 2; }
            size.width = w; size.height = h; channels = ch;
            ptr[(size_t)k] = img[(size_t)k].data();
            // the depth pass works on grey values: the composer's BGR2GRAY integers on the three bytes in file order
            if (ch == 3) {
                grey[(size_t)k].resize((size_t)w * h);
                for (size_t t = 0; t < grey[(size_t)k].size(); ++t) {
                    const unsigned char *q = &img[(size_t)k][3 * t];
                    grey[(size_t)k][t] = (unsigned char)((q[0] * 1868 + q[1] * 9617 + q[2] * 4899 + (1 << 13)) >> 14);
                }
                gptr[(size_t)k] = grey[(size_t)k].data();
            } else gptr[(size_t)k] = ptr[(size_t)k];
        }
        // uniform in inverse distance, index 0 = infinity: a pixel without depth is composed there (fallback_index 0)
        const int D = params.num_hypotheses;
        std::vector<double> inv((size_t)D);
        for (int z = 0; z < D; ++z) inv[(size_t)z] = (double)z / ((double)(D - 1) * near);
        tscm::Sweep sweep(n, intr.data(), Twc.data(), size, pano, inv, &params);
        double sec_depth = 0.0, sec_compose = 0.0;
        std::vector<short> index16 = sweep.depth(gptr.data(), 0, &sec_depth);
        if (fill) index16 = tscm::stereo_fill(index16, pano, &fill_params);
        if (refine) {                                           // the guide: the grey frame at the map as it stands, holes at the fallback
            tscm_sweep_compose_params seam;
            tscm_sweep_compose_default_params(&seam);
            seam.mode = TSCM_PANO_SEAM;
            seam.fallback_index = blend.fallback_index;
            const std::vector<unsigned char> guide = sweep.compose(gptr.data(), 1, &index16, &seam), table = tscm::range_weights(sigma);
            index16 = tscm::stereo_refine(index16, guide, pano, &table, &refine_params);
        }
        const std::vector<short> *at = fill || refine ? &index16 : NULL;     // NULL: the map the depth pass left on the device
        const std::vector<unsigned char> out = visible ? sweep.compose(ptr.data(), channels, at, &blend, vis_params, NULL, 0, NULL, &sec_compose)
                                                       : sweep.compose(ptr.data(), channels, at, &blend, NULL, 0, NULL, &sec_compose);
        size_t n_valid = 0;
        for (size_t t = 0; t < index16.size(); ++t) n_valid += index16[t] >= 0;
        const char *name = channels == 1 ? "sweep_panorama.pgm" : "sweep_panorama.ppm";
        std::ofstream f(name, std::ios::binary);
        f << (channels == 1 ? "P5\n" : "P6\n") << pano.width << " " << pano.height << "\n255\n";
        f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
        std::printf("%s: %d x %d from %d cameras, %d hypotheses, %zu pixels with depth, kernels %.3f ms depth + %.3f ms compose\n", name, pano.width, pano.height, n, D,
                    n_valid, 1e3 * sec_depth, 1e3 * sec_compose);
        return f ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
