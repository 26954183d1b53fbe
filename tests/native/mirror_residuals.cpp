// mirror_residuals.cpp -- MultiCalib::residual_report, tscm::view_outliers and MultiCalib::prune_views of
// include/tscm/tscm_calib.hpp, driven by tests/test_gpu_cpp_mirror_residuals.py: the flow of examples/calibrate_from_corners.cpp
// (per-camera calibration, MultiCalib, calibrate), then the report with a 4 x 3 grid and 8 angle bins, the flags at K, and
// prune_views(K) followed by a second calibrate().
//   mirror_residuals corners.txt out.bin K MAX_FRACTION
// out.bin: int32 C, B, V, N; doubles cam rt [C*6], intrinsics [C*9], board rt [B*6]; int32 board is_initial [B], view_camera [V],
// view_board [V], view_worst [V], flags [V]; doubles corner [N*6], view [V*8], camera [C*8], cost, rmse; int64 grid_count [C*12*2],
// angle_count [C*8*2], grid_outside [C], angle_outside [C]; doubles grid [C*12*3], angle [C*8*4]; int32 pruned pairs count, then
// (camera, board) pairs; doubles rmse of the first and of the second calibrate().
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "tscm/tscm_calib.hpp"

template <typename T>
static bool put(std::FILE *f, const std::vector<T> &v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 5) { std::fprintf(stderr, "usage: %s corners.txt out.bin K MAX_FRACTION\n", argv[0]); return 2; }
    const double k = std::atof(argv[3]), max_fraction = std::atof(argv[4]);
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
            if (!cameras[m].calibrate(pixels, has, worlds, image, board)) std::fprintf(stderr, "camera %d: no CONVERGENCE (the rig solve follows all the same)\n", m);
        }
        tscm::MultiCalib mul(cameras, worlds);
        mul.calibrate();
        const double rmse_first = mul.summary.rmse;
        tscm_residual_params prm;
        tscm_residual_default_params(&prm);
        prm.grid_w = 4; prm.grid_h = 3; prm.image_width = image.width; prm.image_height = image.height;
        prm.n_angle_bins = 8; prm.max_angle = 2.4;
        const tscm::ResidualReport rep = mul.residual_report(&prm);
        const std::vector<bool> flags = tscm::view_outliers(rep, k, 0.0, max_fraction);
        std::vector<double> crt, I, brt;
        std::vector<int> init, fl(flags.size());
        for (size_t v = 0; v < flags.size(); ++v) fl[v] = flags[v] ? 1 : 0;
        for (int m = 0; m < C; ++m) { crt.insert(crt.end(), mul.cameras_[m].rt_.begin(), mul.cameras_[m].rt_.end()); I.insert(I.end(), mul.cameras_[m].intrinsic_.begin(), mul.cameras_[m].intrinsic_.end()); }
        for (int b = 0; b < B; ++b) {
            init.push_back(mul.chessboards_[b].is_initial() ? 1 : 0);
            for (int a = 0; a < 6; ++a) brt.push_back(init.back() ? mul.chessboards_[b].rt_[a] : 0.0);
        }
        // the pruning step on the object, then the solve without the flagged views
        const std::vector<std::pair<int, int> > pruned = mul.prune_views(k, 0.0, max_fraction);
        mul.calibrate();
        std::vector<int> pairs;
        for (const std::pair<int, int> &mb : pruned) { pairs.push_back(mb.first); pairs.push_back(mb.second); }
        const std::vector<long long> g_out(rep.info.grid_outside, rep.info.grid_outside + C), a_out(rep.info.angle_outside, rep.info.angle_outside + C);
        std::FILE *f = std::fopen(argv[2], "wb");
        const int head[4] = { C, B, (int)rep.view_camera.size(), (int)(rep.corner.size() / 6) }, n_pairs = (int)pruned.size();
        const double scal[2] = { rep.info.cost, rep.info.rmse }, rmse[2] = { rmse_first, mul.summary.rmse };
        bool ok = f && std::fwrite(head, sizeof(int), 4, f) == 4 && put(f, crt) && put(f, I) && put(f, brt) && put(f, init) && put(f, rep.view_camera) &&
                  put(f, rep.view_board) && put(f, rep.view_worst) && put(f, fl) && put(f, rep.corner) && put(f, rep.view) && put(f, rep.camera) &&
                  std::fwrite(scal, sizeof(double), 2, f) == 2 && put(f, rep.grid_count) && put(f, rep.angle_count) && put(f, g_out) && put(f, a_out) &&
                  put(f, rep.grid) && put(f, rep.angle) && std::fwrite(&n_pairs, sizeof(int), 1, f) == 1 && put(f, pairs) &&
                  std::fwrite(rmse, sizeof(double), 2, f) == 2;
        if (!ok || std::fclose(f)) { std::fprintf(stderr, "cannot write %s\n", argv[2]); rc = 2; }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 3;
    }
    tscm_corners_free(&cs);
    return rc;
}
