// panorama_demo.cpp -- the stitched 360 x 180 degree panorama of a calibrated rig: one equirect table per camera in the rig
// frame (tscm_build_maps_ex), kept on the device by a tscm_panorama handle, gain compensation from the overlap sums
// (tscm_panorama_overlap, tscm::exposure_gains) and a multi-band blend (tscm_panorama_compose).
// Images are binary PGM (P5, grey) or PPM (P6, three channels) files, all of one kind and size, one per camera of the file.
//   usage: panorama_demo calib.yaml cam0.ppm cam1.ppm ... [--size W H] [--mode seam|feather|multiband] [--levels L] [--no-gains]
// writes panorama.ppm (or panorama.pgm for grey input) into the working directory.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "tscm/tscm_calib.hpp"

static bool read_pnm(const char *path, std::vector<unsigned char> &pix, int &w, int &h, int &channels)
{
    std::ifstream f(path, std::ios::binary);
    std::string magic;
    int maxval = 0;
    if (!(f >> magic >> w >> h >> maxval) || (magic != "P5" && magic != "P6") || maxval != 255 || w < 1 || h < 1) return false;
    channels = magic == "P6" ? 3 : 1;
    f.get();
    pix.resize((size_t)w * h * channels);
    f.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size());
    return (size_t)f.gcount() == pix.size();
}

int main(int argc, char **argv)
{
    std::vector<const char *> files;
    tscm::Size pano = { 2048, 1024 };
    tscm_panorama_params params;
    tscm_panorama_default_params(&params);
    bool gains = true, bad = false;
    for (int a = 2; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--size") && a + 2 < argc) { pano.width = std::atoi(argv[a + 1]); pano.height = std::atoi(argv[a + 2]); a += 2; }
        else if (!std::strcmp(argv[a], "--mode") && a + 1 < argc) {
            const std::string m = argv[++a];
            if (m == "seam") params.mode = TSCM_PANO_SEAM;
            else if (m == "feather") params.mode = TSCM_PANO_FEATHER;
            else if (m == "multiband") params.mode = TSCM_PANO_MULTIBAND;
            else bad = true;
        }
        else if (!std::strcmp(argv[a], "--levels") && a + 1 < argc) params.levels = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--no-gains")) gains = false;
        else files.push_back(argv[a]);
    }
    if (bad || argc < 3 || files.empty()) {
        std::fprintf(stderr, "usage: %s calib.yaml cam0.ppm cam1.ppm ... [--size W H] [--mode seam|feather|multiband] [--levels L] [--no-gains]\n", argv[0]);
        return 2;
    }
    try {
        enum { kMaxCameras = 16 };
        std::vector<double> intr(9 * kMaxCameras), Twc(12 * kMaxCameras);
        int n = 0;
        tscm::check(tscm_yaml_read(argv[1], kMaxCameras, &n, intr.data(), Twc.data()));
        if ((int)files.size() != n) { std::fprintf(stderr, "%s has %d cameras, %d images given\n", argv[1], n, (int)files.size()); return 2; }
        std::vector<std::vector<unsigned char> > img((size_t)n);
        std::vector<const unsigned char *> ptr((size_t)n);
        tscm::Size size = { 0, 0 };
        int channels = 0;
        for (int k = 0; k < n; ++k) {
            int w = 0, h = 0, c = 0;
            if (!read_pnm(files[(size_t)k], img[(size_t)k], w, h, c)) { std::fprintf(stderr, "%s: not a binary 8-bit PGM / PPM\n", files[(size_t)k]); return 2; }
            if (k && (w != size.width || h != size.height || c != channels)) { std::fprintf(stderr, "%s: the images differ in size or kind\n", files[(size_t)k]); return 2; }
            size.width = w; size.height = h; channels = c;
            ptr[(size_t)k] = img[(size_t)k].data();
        }
        tscm::Panorama p(n, intr.data(), Twc.data(), size, channels, pano, &params);
        std::vector<unsigned short> g((size_t)n, 256);
        if (gains) {
            std::vector<long long> count, sum;
            p.overlap(ptr.data(), 0, count, sum);
            g = tscm::exposure_gains(n, count, sum);
        }
        double seconds = 0.0;
        const std::vector<unsigned char> out = p.compose(ptr.data(), 0, g.data(), &seconds);
        const char *name = channels == 3 ? "panorama.ppm" : "panorama.pgm";
        std::ofstream f(name, std::ios::binary);
        f << (channels == 3 ? "P6\n" : "P5\n") << pano.width << " " << pano.height << "\n255\n";
        f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
        std::printf("%s: %d x %d from %d cameras, gains", name, pano.width, pano.height, n);
        for (int k = 0; k < n; ++k) std::printf(" %.3f", g[(size_t)k] / 256.0);
        std::printf(", kernels %.3f ms\n", 1e3 * seconds);
        return f ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
