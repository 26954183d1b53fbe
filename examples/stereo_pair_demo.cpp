// stereo_pair_demo.cpp -- from two fisheye images of adjacent cameras of a calibrated rig to 3-D points: the long-lat
// rectification of rectify_pair_demo.cpp (tscm_build_maps_ex, tscm_remap), then census + semi-global matching along the
// rows (tscm_stereo_match), optionally the post-filter of the disparity map (tscm_stereo_filter) and the points of the
// disparities in the pair frame of camera a (tscm_stereo_points).  Images are 8-bit binary PGM files (P5).
//   usage: stereo_pair_demo [--speckle N,R] [--median M] [--fill RULE[,MAX_DISTANCE[,MIN_DIRECTIONS]]] [--refine RADIUS,SIGMA[,ITERATIONS[,FILL]]]
//                           calib.yaml cam_a cam_b a.pgm b.pgm disparity.pgm points.txt [width height [num_disparities [paths]]]
// --speckle N,R: components of at most N pixels whose neighbours differ by at most R disparities are dropped;
// --median M: masked median of M x M (3 or 5) afterwards;
// --fill RULE: after those, every invalid pixel gets the lowest | second_lowest | median of the nearest valid disparities
// along the 8 path directions (tscm_stereo_fill), no further than MAX_DISTANCE pixels (0: any) and from at least
// MIN_DIRECTIONS of them (1);
// --refine RADIUS,SIGMA: last, the weighted median of every pixel's (2 RADIUS + 1)^2 window (tscm_stereo_refine), a neighbour
// weighted by exp(-|difference of grey values in the rectified left image| / SIGMA), in ITERATIONS passes (1); FILL 1 gives
// invalid pixels a value too (0).
// disparity.pgm: disparity in pixels (saturated at 255), 0 where invalid; points.txt: one "column row X Y Z" line per
// valid pixel, X Y Z in the units of the calibration's translations, pair frame (x along the baseline from a to b).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "tscm/tscm_calib.hpp"

static bool read_pgm(const char *path, std::vector<unsigned char> &pix, int &w, int &h)
{
    std::ifstream f(path, std::ios::binary);
    std::string magic;
    int maxval = 0;
    if (!(f >> magic >> w >> h >> maxval) || magic != "P5" || maxval != 255 || w < 1 || h < 1) return false;
    f.get();
    pix.resize((size_t)w * h);
    f.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size());
    return (size_t)f.gcount() == pix.size();
}

static bool write_pgm(const char *path, const std::vector<unsigned char> &pix, int w, int h)
{
    std::ofstream f(path, std::ios::binary);
    f << "P5\n" << w << " " << h << "\n255\n";
    f.write(reinterpret_cast<const char *>(pix.data()), (std::streamsize)pix.size());
    return (bool)f;
}

int main(int argc_all, char **argv_all)
{
    // the options may stand anywhere; what is left are the positional arguments
    int speckle_window = 0, speckle_range = 0, median = 0;
    bool bad_option = false, fill = false, refine = false;
    tscm_stereo_fill_params fill_params;
    tscm_stereo_fill_default_params(&fill_params);
    tscm_stereo_refine_params refine_params;
    tscm_stereo_refine_default_params(&refine_params);
    double sigma = 0.0;
    std::vector<char *> argv(1, argv_all[0]);
    for (int k = 1; k < argc_all; ++k) {
        if (!std::strcmp(argv_all[k], "--speckle") && k + 1 < argc_all) bad_option |= std::sscanf(argv_all[++k], "%d,%d", &speckle_window, &speckle_range) != 2;
        else if (!std::strcmp(argv_all[k], "--median") && k + 1 < argc_all) median = std::atoi(argv_all[++k]);
        else if (!std::strcmp(argv_all[k], "--fill") && k + 1 < argc_all) { fill = true; bad_option |= !tscm::parse_fill_option(argv_all[++k], &fill_params); }
        else if (!std::strcmp(argv_all[k], "--refine") && k + 1 < argc_all) { refine = true; bad_option |= !tscm::parse_refine_option(argv_all[++k], &refine_params, &sigma); }
        else if (!std::strncmp(argv_all[k], "--", 2)) bad_option = true;
        else argv.push_back(argv_all[k]);
    }
    const int argc = (int)argv.size();
    if (argc < 8 || bad_option) {
        std::fprintf(stderr, "usage: %s [--speckle N,R] [--median M] [--fill RULE[,MAX_DISTANCE[,MIN_DIRECTIONS]]] [--refine RADIUS,SIGMA[,ITERATIONS[,FILL]]] calib.yaml cam_a cam_b a.pgm b.pgm disparity.pgm points.txt [width height [num_disparities [paths]]]\n",
                     argv[0]);
        return 2;
    }
    const int cam[2] = { std::atoi(argv[2]), std::atoi(argv[3]) };
    tscm::Size size = { argc > 9 ? std::atoi(argv[8]) : 640, argc > 9 ? std::atoi(argv[9]) : 320 };
    const double pi = 3.14159265358979323846;
    try {
        enum { kMaxCameras = 32 };
        std::vector<double> intr(9 * kMaxCameras), Twc(12 * kMaxCameras);
        int n_cameras = 0;
        tscm::check(tscm_yaml_read(argv[1], kMaxCameras, &n_cameras, intr.data(), Twc.data()));
        for (int k = 0; k < 2; ++k)
            if (cam[k] < 0 || cam[k] >= n_cameras) { std::fprintf(stderr, "%s has cameras 0..%d\n", argv[1], n_cameras - 1); return 2; }
        const double *Ta = &Twc[12 * cam[0]], *Tb = &Twc[12 * cam[1]];
        tscm_map_desc desc[2];
        std::vector<float> mapx[2], mapy[2];
        tscm::rectify_pair_maps(&intr[9 * cam[0]], Ta, &intr[9 * cam[1]], Tb, TSCM_PROJ_LONGLAT, size, pi, pi / 2, desc, mapx, mapy);
        std::vector<unsigned char> rect[2];
        for (int k = 0; k < 2; ++k) {
            std::vector<unsigned char> img;
            int w = 0, h = 0;
            if (!read_pgm(argv[4 + k], img, w, h)) { std::fprintf(stderr, "cannot read %s as an 8-bit binary PGM\n", argv[4 + k]); return 2; }
            rect[k].assign((size_t)size.width * size.height, 0);
            tscm::check(tscm_remap(img.data(), w, h, w, 1, mapx[k].data(), mapy[k].data(), size.width, size.height, size.width, 0, 0, rect[k].data(), size.width));
        }
        tscm_stereo_params params;
        tscm_stereo_default_params(&params);
        if (argc > 10) params.num_disparities = std::atoi(argv[10]);
        if (argc > 11) params.paths = std::atoi(argv[11]);
        std::vector<short> disparity = tscm::stereo_match(rect[0].data(), rect[1].data(), size, &params);
        if (speckle_window > 0 || median > 0) {
            tscm_stereo_filter_params post;
            tscm_stereo_filter_default_params(&post);
            post.min_disparity = params.min_disparity;
            post.speckle_window_size = speckle_window; post.speckle_range = speckle_range;
            post.median = median;
            disparity = tscm::stereo_filter(disparity, size, &post);
        }
        if (fill) {
            fill_params.min_disparity = params.min_disparity;
            disparity = tscm::stereo_fill(disparity, size, &fill_params);
        }
        if (refine) {
            refine_params.min_disparity = params.min_disparity;
            const std::vector<unsigned char> table = tscm::range_weights(sigma);
            disparity = tscm::stereo_refine(disparity, rect[0], size, &table, &refine_params);
        }
        const double dt[3] = { Tb[3] - Ta[3], Tb[7] - Ta[7], Tb[11] - Ta[11] };
        const double baseline = std::sqrt(dt[0] * dt[0] + dt[1] * dt[1] + dt[2] * dt[2]);
        std::vector<unsigned char> valid;
        const std::vector<tscm::Point3d> points = tscm::stereo_points(disparity, size, params.min_disparity, desc[0], TSCM_PROJ_LONGLAT, baseline, valid);
        std::vector<unsigned char> shown(disparity.size(), 0);
        std::ofstream list(argv[7]);
        list.precision(9);
        size_t n_valid = 0;
        for (size_t e = 0; e < disparity.size(); ++e) {
            if (!valid[e]) continue;
            ++n_valid;
            const int px = (disparity[e] + 8) / 16;
            shown[e] = (unsigned char)(px < 0 ? 0 : px > 255 ? 255 : px);
            list << e % (size_t)size.width << " " << e / (size_t)size.width << " " << points[e].x << " " << points[e].y << " " << points[e].z << "\n";
        }
        if (!list || !write_pgm(argv[6], shown, size.width, size.height)) { std::fprintf(stderr, "cannot write %s / %s\n", argv[6], argv[7]); return 2; }
        std::printf("cameras %d, %d: baseline %.3f, %d x %d, %d disparities, %d paths: %zu of %zu pixels with a point\n", cam[0], cam[1], baseline, size.width,
                    size.height, params.num_disparities, params.paths, n_valid, disparity.size());
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 3;
    }
    return 0;
}
