// mirror_covariance.cpp -- MultiCalib::covariance of include/tscm/tscm_calib.hpp, driven by
// tests/test_gpu_cpp_mirror_covariance.py: the flow of examples/calibrate_from_corners.cpp (per-camera calibration, MultiCalib,
// calibrate), then covariance() with the masks the solve had.
//   mirror_covariance corners.txt out.bin MASK          MASK: one TSCM_FIX_* word for every camera (decimal)
// out.bin: int32 C, B, status, n_free; double sigma2, min_pivot_ratio; doubles cam rt [C*6], intrinsics [C*9], board rt [B*6];
// int32 board is_initial [B]; doubles cam_rt_std [C*6], intr_std [C*9], board_rt_std [B*6], cam_cov [(15 C)^2], board_cov [B*36].
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "tscm/tscm_calib.hpp"

static bool put(std::FILE *f, const std::vector<double> &v) { return v.empty() || std::fwrite(v.data(), sizeof(double), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s corners.txt out.bin MASK\n", argv[0]); return 2; }
    const unsigned short fixed = (unsigned short)std::atoi(argv[3]);
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
        std::vector<double> crt, I, brt;
        std::vector<int> init;
        for (int m = 0; m < C; ++m) { crt.insert(crt.end(), mul.cameras_[m].rt_.begin(), mul.cameras_[m].rt_.end()); I.insert(I.end(), mul.cameras_[m].intrinsic_.begin(), mul.cameras_[m].intrinsic_.end()); }
        for (int b = 0; b < B; ++b) {
            init.push_back(mul.chessboards_[b].is_initial() ? 1 : 0);
            for (int a = 0; a < 6; ++a) brt.push_back(init.back() ? mul.chessboards_[b].rt_[a] : 0.0);
        }
        std::FILE *f = std::fopen(argv[2], "wb");
        const int head[4] = { C, B, cov.info.status, cov.info.n_free };
        const double scal[2] = { cov.sigma2, cov.info.min_pivot_ratio };
        bool ok = f && std::fwrite(head, sizeof(int), 4, f) == 4 && std::fwrite(scal, sizeof(double), 2, f) == 2 && put(f, crt) && put(f, I) && put(f, brt) &&
                  std::fwrite(init.data(), sizeof(int), init.size(), f) == init.size() && put(f, cov.cam_rt_std) && put(f, cov.intr_std) && put(f, cov.board_rt_std) &&
                  put(f, cov.cam_cov) && put(f, cov.board_cov);
        if (!ok || std::fclose(f)) { std::fprintf(stderr, "cannot write %s\n", argv[2]); rc = 2; }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 3;
    }
    tscm_corners_free(&cs);
    return rc;
}
