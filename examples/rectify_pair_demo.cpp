// rectify_pair_demo.cpp -- epipolar rectification of two adjacent fisheye cameras of a calibrated rig over the whole
// hemisphere: what EpipolarRectify/rectify.cpp:86-199 does with 90-degree pinhole tables, here with longitude-latitude
// tables (TSCM_PROJ_LONGLAT, 180 x 90 degrees), in which a scene point lies on the same row of both outputs.
// Tables by tscm_build_maps_ex, applied by tscm_remap; images are 8-bit binary PGM files (P5).
//   usage: rectify_pair_demo calib.yaml cam_a cam_b a.pgm b.pgm out_a.pgm out_b.pgm [width height [kind]]
//   kind: 0 perspective (90 x 90 degrees), 1 longlat (default), 2 cylindrical, 3 stereographic, 4 equirect
#include <cstdio>
#include <cstdlib>
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

int main(int argc, char **argv)
{
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s calib.yaml cam_a cam_b a.pgm b.pgm out_a.pgm out_b.pgm [width height [kind]]\n", argv[0]);
        return 2;
    }
    const int cam[2] = { std::atoi(argv[2]), std::atoi(argv[3]) };
    tscm::Size size = { argc > 9 ? std::atoi(argv[8]) : 640, argc > 9 ? std::atoi(argv[9]) : 320 };
    const int kind = argc > 10 ? std::atoi(argv[10]) : TSCM_PROJ_LONGLAT;
    const double pi = 3.14159265358979323846;
    const double fov_x = kind == TSCM_PROJ_PERSPECTIVE ? pi / 2 : pi, fov_y = pi / 2;
    try {
        enum { kMaxCameras = 32 };
        std::vector<double> intr(9 * kMaxCameras), Twc(12 * kMaxCameras);
        int n_cameras = 0;
        tscm::check(tscm_yaml_read(argv[1], kMaxCameras, &n_cameras, intr.data(), Twc.data()));
        for (int k = 0; k < 2; ++k)
            if (cam[k] < 0 || cam[k] >= n_cameras) { std::fprintf(stderr, "%s has cameras 0..%d\n", argv[1], n_cameras - 1); return 2; }
        tscm_map_desc desc[2];
        std::vector<float> mapx[2], mapy[2];
        tscm::rectify_pair_maps(&intr[9 * cam[0]], &Twc[12 * cam[0]], &intr[9 * cam[1]], &Twc[12 * cam[1]], kind, size, fov_x, fov_y, desc, mapx, mapy);
        for (int k = 0; k < 2; ++k) {
            std::vector<unsigned char> img, out((size_t)size.width * size.height);
            int w = 0, h = 0;
            if (!read_pgm(argv[4 + k], img, w, h)) { std::fprintf(stderr, "cannot read %s as an 8-bit binary PGM\n", argv[4 + k]); return 2; }
            tscm::check(tscm_remap(img.data(), w, h, w, 1, mapx[k].data(), mapy[k].data(), size.width, size.height, size.width, 0, 0, out.data(), size.width));
            if (!write_pgm(argv[6 + k], out, size.width, size.height)) { std::fprintf(stderr, "cannot write %s\n", argv[6 + k]); return 2; }
            size_t seen = 0;
            for (size_t e = 0; e < mapx[k].size(); ++e)
                if (mapx[k][e] >= 0.f && mapy[k][e] >= 0.f && mapx[k][e] <= w - 1.f && mapy[k][e] <= h - 1.f) ++seen;
            std::printf("camera %d -> %s: %d x %d, %.1f %% of the table inside the image\n", cam[k], argv[6 + k], size.width, size.height,
                        100.0 * (double)seen / (double)mapx[k].size());
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 3;
    }
    return 0;
}
