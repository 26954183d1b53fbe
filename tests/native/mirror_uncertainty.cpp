// mirror_uncertainty.cpp -- MultiCalib::projection_uncertainty of include/tscm/tscm_calib.hpp, driven by
// tests/test_gpu_cpp_mirror_uncertainty.py: the flow of examples/calibrate_from_corners.cpp (per-camera calibration, MultiCalib,
// calibrate), covariance() with the masks the solve had, then projection_uncertainty() on the image grid with the requests of
// uncertainty_requests().
//   mirror_uncertainty corners.txt out.bin MASK STEP INV_DISTANCE      MASK: one TSCM_FIX_* word for every camera (decimal)
// out.bin: int32 C, B, n_requests, nx, ny, pad; doubles cam rt [C*6], intrinsics [C*9], board rt [B*6]; int32 board is_initial [B];
// per request int32 camera_a, camera_b and double inv_distance; doubles planes [n_requests*7*ny*nx], max_sd [n_requests];
// int64 n_valid [n_requests]; bytes flags [n_requests*ny*nx].
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "tscm/tscm_calib.hpp"

static bool put(std::FILE *f, const std::vector<double> &v) { return v.empty() || std::fwrite(v.data(), sizeof(double), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: %s corners.txt out.bin MASK STEP INV_DISTANCE\n", argv[0]); return 2; }
    const unsigned short fixed = (unsigned short)std::atoi(argv[3]);
    const double step = std::strtod(argv[4], nullptr), inv_distance = std::strtod(argv[5], nullptr);
    tscm_corner_set cs;
    if (tscm_corners_read(argv[1], &cs) != 0) { std::fprintf(stderr, "%s\n", tscm_last_error()); return 2; }
    int rc = 0;
    try {
        const int C = cs.n_cameras, B = cs.n_boards, n = cs.board_cols * cs.board_rows;
        const tscm::Size board = { cs.board_cols, cs.board_rows }, image = { cs.image_width, cs.image_height };
        std::vector<tscm::Point3d> worlds;
        for (int u = 0; u < board.height; ++u)
            for (int v = 0; v < board.width; ++v) worlds.push_back(tscm::Point3d{ v * cs.pitch, u * cs.pitch, 0.0 });
        std::vector<tscm::TripleSphereCamera> cameras(C);
        for (int m = 0; m < C; ++m) {
            std::vector<std::vector<tscm::Point2d> > pixels(B);
            std::vector<bool> has(B);
            for (int b = 0; b < B; ++b) {
                has[b] = cs.has[(size_t)m * B + b] != 0;
                if (!has[b]) continue;
                pixels[b].resize(n);
                for (int j = 0; j < n; ++j) pixels[b][j] = tscm::Point2d{ cs.pix_u[((size_t)m * B + b) * n + j], cs.pix_v[((size_t)m * B + b) * n + j] };
            }
            cameras[m].set_fixed_intrinsics(fixed);
            if (!cameras[m].calibrate(pixels, has, worlds, image, board)) std::fprintf(stderr, "camera %d: no CONVERGENCE (the rig solve follows all the same)\n", m);
        }
        tscm::MultiCalib mul(cameras, worlds);
        for (int m = 0; m < C; ++m) mul.set_fixed_intrinsics(m, fixed);
        mul.calibrate();
        const tscm::MultiCalib::Covariance cov = mul.covariance();
        const std::vector<tscm_uncertainty_request> req = mul.uncertainty_requests(std::vector<double>(1, inv_distance));
        const tscm::MultiCalib::Uncertainty unc = mul.projection_uncertainty(cov, tscm::MultiCalib::image_grid(image.width, image.height, step), req);
        std::vector<double> crt, I, brt;
        std::vector<int> init;
        for (int m = 0; m < C; ++m) { crt.insert(crt.end(), mul.cameras_[m].rt_.begin(), mul.cameras_[m].rt_.end()); I.insert(I.end(), mul.cameras_[m].intrinsic_.begin(), mul.cameras_[m].intrinsic_.end()); }
        for (int b = 0; b < B; ++b) {
            init.push_back(mul.chessboards_[b].is_initial() ? 1 : 0);
            for (int a = 0; a < 6; ++a) brt.push_back(init.back() ? mul.chessboards_[b].rt_[a] : 0.0);
        }
        std::FILE *f = std::fopen(argv[2], "wb");
        const int head[6] = { C, B, unc.n_requests, unc.nx, unc.ny, 0 };
        bool ok = f && std::fwrite(head, sizeof(int), 6, f) == 6 && put(f, crt) && put(f, I) && put(f, brt) && std::fwrite(init.data(), sizeof(int), init.size(), f) == init.size();
        for (size_t r = 0; ok && r < req.size(); ++r) {
            const int ab[2] = { req[r].camera_a, req[r].camera_b };
            ok = std::fwrite(ab, sizeof(int), 2, f) == 2 && std::fwrite(&req[r].inv_distance, sizeof(double), 1, f) == 1;
        }
        ok = ok && put(f, unc.planes) && put(f, unc.max_sd) && std::fwrite(unc.n_valid.data(), sizeof(long long), unc.n_valid.size(), f) == unc.n_valid.size() &&
             std::fwrite(unc.flags.data(), 1, unc.flags.size(), f) == unc.flags.size();
        if (!ok || std::fclose(f)) { std::fprintf(stderr, "cannot write %s\n", argv[2]); rc = 2; }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 3;
    }
    tscm_corners_free(&cs);
    return rc;
}
