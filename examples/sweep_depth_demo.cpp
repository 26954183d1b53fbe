// sweep_depth_demo.cpp -- depth in the rig frame over the whole 360 x 180 degree panorama from all cameras of a calibrated
// rig at once: sweep tables (tscm_build_sweep_maps), the fused census cost volume, path aggregation and winner
// (tscm_sweep_depth) and the 3-D points of the index map (tscm_sweep_points).
// Images are binary grey PGM (P5) files of one size, one per camera of the file.
//   usage: sweep_depth_demo calib.yaml cam0.pgm cam1.pgm ... [--size W H] [--near N] [--hypotheses D] [--paths 4|8]
//                           [--fill RULE[,MAX_DISTANCE[,MIN_DIRECTIONS]]] [--refine RADIUS,SIGMA[,ITERATIONS[,FILL]]]
// --fill: every pixel without depth gets the lowest | second_lowest | median of the nearest valid indices along the 8 path
// directions, over the seam too (tscm_stereo_fill with wrap_x = 1), before the points are taken.
// --refine: after that, the weighted median of every pixel's (2 RADIUS + 1)^2 window, over the seam too (tscm_stereo_refine
// with wrap_x = 1), a neighbour weighted by exp(-|difference of grey values| / SIGMA) in the frame composed by seam at the
// map as it stands, in ITERATIONS passes (1); FILL 1 gives pixels without depth a value too (0).
// writes sweep_index.pgm (16-bit, big-endian as PGM has it: 16 x hypothesis index + 16, so 0 = invalid) and sweep_points.ply
// (ASCII, the valid points in the rig frame) into the working directory.  near: in the units of the calibration's translations.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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

int main(int argc, char **argv)
{
    std::vector<const char *> files;
    tscm::Size pano = { 1024, 512 };
    double near = 500.0;
    tscm_sweep_params params;
    tscm_sweep_default_params(&params);
    bool fill = false, refine = false, bad = false;
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
        else if (!std::strcmp(argv[a], "--fill") && a + 1 < argc) { fill = true; bad |= !tscm::parse_fill_option(argv[++a], &fill_params); }
        else if (!std::strcmp(argv[a], "--refine") && a + 1 < argc) { refine = true; bad |= !tscm::parse_refine_option(argv[++a], &refine_params, &sigma); }
        else files.push_back(argv[a]);
    }
    if (bad || argc < 4 || files.size() < 2 || !(near > 0.0) || params.num_hypotheses < 2) {
        std::fprintf(stderr, "usage: %s calib.yaml cam0.pgm cam1.pgm ... [--size W H] [--near N] [--hypotheses D] [--paths 4|8] [--fill RULE[,MAX_DISTANCE[,MIN_DIRECTIONS]]] [--refine RADIUS,SIGMA[,ITERATIONS[,FILL]]]\n",
                     argv[0]);
        return 2;
    }
    try {
        enum { kMaxCameras = 8 };
        std::vector<double> intr(9 * kMaxCameras), Twc(12 * kMaxCameras);
        int n = 0;
        tscm::check(tscm_yaml_read(argv[1], kMaxCameras, &n, intr.data(), Twc.data()));
        if ((int)files.size() != n) { std::fprintf(stderr, "%s has %d cameras, %d images given\n", argv[1], n, (int)files.size()); return 2; }
        std::vector<std::vector<unsigned char> > img((size_t)n);
        std::vector<const unsigned char *> ptr((size_t)n);
        tscm::Size size = { 0, 0 };
        for (int k = 0; k < n; ++k) {
            int w = 0, h = 0;
            if (!read_pgm(files[(size_t)k], img[(size_t)k], w, h)) { std::fprintf(stderr, "%s: not a binary 8-bit PGM\n", files[(size_t)k]); return 2; }
            if (k && (w != size.width || h != size.height)) { std::fprintf(stderr, "%s: the images differ in size\n", files[(size_t)k]); return 2; }
            size.width = w; size.height = h;
            ptr[(size_t)k] = img[(size_t)k].data();
        }
        // uniform in inverse distance, index 0 = infinity
        const int D = params.num_hypotheses;
        std::vector<double> inv((size_t)D);
        for (int z = 0; z < D; ++z) inv[(size_t)z] = (double)z / ((double)(D - 1) * near);
        tscm::Sweep sweep(n, intr.data(), Twc.data(), size, pano, inv, &params);
        double seconds = 0.0;
        std::vector<short> index16 = sweep.depth(ptr.data(), 0, &seconds);
        if (fill) index16 = tscm::stereo_fill(index16, pano, &fill_params);
        if (refine) {                                           // the guide: the grey frame at the map as it stands, holes at infinity
            tscm_sweep_compose_params seam;
            tscm_sweep_compose_default_params(&seam);
            seam.mode = TSCM_PANO_SEAM;
            const std::vector<unsigned char> guide = sweep.compose(ptr.data(), 1, &index16, &seam), table = tscm::range_weights(sigma);
            index16 = tscm::stereo_refine(index16, guide, pano, &table, &refine_params);
        }
        std::vector<unsigned char> valid;
        const std::vector<tscm::Point3d> pts = sweep.points(index16, valid);
        std::ofstream f("sweep_index.pgm", std::ios::binary);
        f << "P5\n" << pano.width << " " << pano.height << "\n65535\n";
        for (size_t t = 0; t < index16.size(); ++t) {
            const unsigned v = (unsigned)(index16[t] + 16);
            f.put((char)(v >> 8)); f.put((char)(v & 0xffu));
        }
        size_t n_valid = 0;
        for (size_t t = 0; t < valid.size(); ++t) n_valid += valid[t];
        std::ofstream ply("sweep_points.ply");
        ply << "ply\nformat ascii 1.0\nelement vertex " << n_valid << "\nproperty float x\nproperty float y\nproperty float z\nend_header\n";
        for (size_t t = 0; t < pts.size(); ++t)
            if (valid[t]) ply << pts[t].x << " " << pts[t].y << " " << pts[t].z << "\n";
        std::printf("sweep_index.pgm, sweep_points.ply: %d x %d from %d cameras, %d hypotheses, %zu points, kernels %.3f ms\n", pano.width, pano.height, n, D,
                    n_valid, 1e3 * seconds);
        return f && ply ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
