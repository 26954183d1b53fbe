// mirror_priors.cpp -- Gaussian priors through include/tscm/tscm_calib.hpp, driven by tests/test_gpu_cpp_mirror_priors.py: the flow of
// examples/calibrate_from_corners.cpp without priors (per-camera calibration), then
//   mono: a copy of camera 0 with set_camera_priors -- the intrinsics named in PRIORS about its values moved by OFFSET sigmas --
//         and refinement();
//   rig:  MultiCalib with set_camera_priors -- the same on every camera's intrinsics, and every camera's pose about its start
//         value with sigma ROT on the rotation and TRANS on the translation -- then calibrate() and covariance().
//   mirror_priors corners.txt out.bin PRIORS OFFSET ROT TRANS          PRIORS: name:sigma[,name:sigma...] (parse_prior_option)
// out.bin, all doubles: C, B, n;
//   mono: has [B], start intrinsic [9], start rt [B*6], mean [9], weight [9], intrinsic [9], rt [B*6], num_iterations, final_cost, rmse;
//   rig:  board is_initial [B], start cam rt [C*6], intrinsics [C*9], board rt [B*6], cam_rt_mean [C*6], cam_rt_weight [C*6],
//         intr_mean [C*9], intr_weight [C*9], cam rt [C*6], intrinsics [C*9], board rt [B*6], num_iterations, final_cost, rmse,
//         n_residuals, n_free, sigma2, status, cam_rt_std [C*6], intr_std [C*9].
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "tscm/tscm_calib.hpp"

typedef std::vector<double> Vec;
static void add(Vec &out, const Vec &v) { out.insert(out.end(), v.begin(), v.end()); }

int main(int argc, char **argv)
{
    double sigma[7];
    if (argc < 7 || !tscm::parse_prior_option(argv[3], sigma)) { std::fprintf(stderr, "usage: %s corners.txt out.bin PRIORS OFFSET ROT TRANS\n", argv[0]); return 2; }
    const double offset = std::atof(argv[4]), rot = std::atof(argv[5]), trans = std::atof(argv[6]);
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
            if (!cameras[m].calibrate(pixels, has, worlds, image, board)) std::fprintf(stderr, "camera %d: no CONVERGENCE (the flow goes on all the same)\n", m);
        }
        // priors on intrinsics: about `intr` moved by `offset` sigmas
        auto shifted = [&](const Vec &intr) {
            tscm::CameraPriors p = tscm::intrinsic_priors_about(intr, sigma);
            for (size_t i = 0; i < intr.size(); ++i) if (p.intr_weight[i] > 0.0) p.intr_mean[i] += offset * sigma[i % 9];
            return p;
        };
        auto poses = [&](const std::vector<std::vector<double> > &rt, const std::vector<bool> &has) {
            Vec out;
            for (size_t i = 0; i < rt.size(); ++i) for (int a = 0; a < 6; ++a) out.push_back(has[i] ? rt[i][a] : 0.0);
            return out;
        };
        Vec out = { (double)C, (double)B, (double)n };
        {   // ---- mono
            tscm::TripleSphereCamera cam = cameras[0];
            for (int b = 0; b < B; ++b) out.push_back(cam.has_chessboard_[b] ? 1.0 : 0.0);
            add(out, cam.intrinsic_);
            add(out, poses(cam.rt_, cam.has_chessboard_));
            const tscm::CameraPriors pr = shifted(cam.intrinsic_);
            add(out, pr.intr_mean); add(out, pr.intr_weight);
            cam.set_camera_priors(&pr);
            cam.refinement(cam.pixels_, worlds);
            add(out, cam.intrinsic_);
            add(out, poses(cam.rt_, cam.has_chessboard_));
            out.push_back(cam.summary.num_iterations); out.push_back(cam.summary.final_cost); out.push_back(cam.summary.rmse);
        }
        {   // ---- rig
            tscm::MultiCalib mul(cameras, worlds);
            Vec crt, I, brt, init;
            auto state = [&]() {
                crt.clear(); I.clear(); brt.clear(); init.clear();
                for (int m = 0; m < C; ++m) { add(crt, mul.cameras_[m].rt_); add(I, mul.cameras_[m].intrinsic_); }
                for (int b = 0; b < B; ++b) {
                    init.push_back(mul.chessboards_[b].is_initial() ? 1.0 : 0.0);
                    for (int a = 0; a < 6; ++a) brt.push_back(init.back() != 0.0 ? mul.chessboards_[b].rt_[a] : 0.0);
                }
            };
            state();
            add(out, init); add(out, crt); add(out, I); add(out, brt);
            tscm::CameraPriors pr = shifted(I);
            pr.cam_rt_mean = crt;
            for (int m = 0; m < C; ++m) for (int a = 0; a < 6; ++a) pr.cam_rt_weight.push_back(1.0 / ((a < 3 ? rot : trans) * (a < 3 ? rot : trans)));
            add(out, pr.cam_rt_mean); add(out, pr.cam_rt_weight); add(out, pr.intr_mean); add(out, pr.intr_weight);
            mul.set_camera_priors(&pr);
            mul.calibrate();
            state();
            add(out, crt); add(out, I); add(out, brt);
            out.push_back(mul.summary.num_iterations); out.push_back(mul.summary.final_cost); out.push_back(mul.summary.rmse);
            const tscm::MultiCalib::Covariance cov = mul.covariance();
            out.push_back((double)cov.info.n_residuals); out.push_back(cov.info.n_free); out.push_back(cov.sigma2); out.push_back(cov.info.status);
            add(out, cov.cam_rt_std); add(out, cov.intr_std);
        }
        std::FILE *f = std::fopen(argv[2], "wb");
        const bool ok = f && std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
        if (!ok || std::fclose(f)) { std::fprintf(stderr, "cannot write %s\n", argv[2]); rc = 2; }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 3;
    }
    tscm_corners_free(&cs);
    return rc;
}
