// mirror_ransac.cpp -- TripleSphereCamera::estimate_extrinsic_ransac and tscm::parse_ransac_option of
// include/tscm/tscm_calib.hpp, driven by tests/test_gpu_cpp_mirror_ransac.py.
//   mirror_ransac in.bin out.bin [OPTION]
// in.bin: int32 views, corners, board_w, n_hypotheses, min_inliers, seed, then doubles: threshold_px, intr[9],
// worlds[corners * 3], then int32 has[views], then doubles u[views * corners], v[views * corners].
// OPTION: the text of a demo's --ransac, parsed over threshold_px / n_hypotheses / min_inliers of the file.
// out.bin: int32 poses written, int32 code[views], double Rt[views * 9], bytes inlier[views * corners].
#include <cstdio>
#include <exception>
#include <vector>

#include "tscm/tscm_calib.hpp"

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin [THRESHOLD[,HYPOTHESES[,MIN_INLIERS]]]\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    int head[6];
    double thr = 0.0;
    if (!in || std::fread(head, sizeof(int), 6, in) != 6 || std::fread(&thr, sizeof(double), 1, in) != 1 || head[0] < 0 || head[1] < 0) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const size_t V = (size_t)head[0], n = (size_t)head[1];
    std::vector<double> intr(9), W(3 * n), u(V * n), v(V * n);
    std::vector<int> has(V);
    if (std::fread(intr.data(), sizeof(double), 9, in) != 9 || std::fread(W.data(), sizeof(double), W.size(), in) != W.size() ||
        std::fread(has.data(), sizeof(int), V, in) != V || std::fread(u.data(), sizeof(double), u.size(), in) != u.size() ||
        std::fread(v.data(), sizeof(double), v.size(), in) != v.size()) {
        std::fprintf(stderr, "%s is too short\n", argv[1]);
        return 2;
    }
    std::fclose(in);
    tscm_ransac_params p;
    tscm_ransac_default_params(&p);
    p.threshold_px = thr; p.n_hypotheses = head[3]; p.min_inliers = head[4]; p.seed = (unsigned)head[5];
    if (argc > 3 && !tscm::parse_ransac_option(argv[3], &p)) { std::fprintf(stderr, "bad option %s\n", argv[3]); return 2; }
    try {
        tscm::TripleSphereCamera cam;
        cam.intrinsic_ = intr;
        std::vector<tscm::Point3d> worlds(n);
        for (size_t j = 0; j < n; ++j) worlds[j] = tscm::Point3d{ W[3 * j], W[3 * j + 1], W[3 * j + 2] };
        std::vector<std::vector<tscm::Point2d> > pixels(V);
        cam.has_chessboard_.assign(V, false);
        for (size_t k = 0; k < V; ++k) {
            cam.has_chessboard_[k] = has[k] != 0;
            if (!has[k]) continue;
            pixels[k].resize(n);
            for (size_t j = 0; j < n; ++j) pixels[k][j] = tscm::Point2d{ u[k * n + j], v[k * n + j] };
        }
        std::vector<std::vector<unsigned char> > inliers;
        const tscm::Size board = { head[2], head[2] ? (int)n / head[2] : 0 };
        const int done = cam.estimate_extrinsic_ransac(pixels, worlds, board, &p, &inliers);
        std::FILE *f = std::fopen(argv[2], "wb");
        bool ok = f && std::fwrite(&done, sizeof(int), 1, f) == 1 && std::fwrite(cam.ransac_code_.data(), sizeof(int), V, f) == V;
        for (size_t k = 0; ok && k < V; ++k) ok = std::fwrite(cam.Rt_[k].a, sizeof(double), 9, f) == 9;
        for (size_t k = 0; ok && k < V; ++k) ok = std::fwrite(inliers[k].data(), 1, n, f) == n;
        if (!ok || std::fclose(f)) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
