// mirror_view_gain.cpp -- MultiCalib::view_gain and view_gain_apply of include/tscm/tscm_calib.hpp, driven by
// tests/test_gpu_cpp_mirror_view_gain.py: the flow of examples/calibrate_from_corners.cpp (per-camera calibration, MultiCalib,
// calibrate), covariance() with the masks the solve had, then view_gain() on the candidates of a file and view_gain_apply()
// of the first of them.
//   mirror_view_gain corners.txt candidates.bin out.bin MASK BORDER MIN_CORNERS      MASK: one TSCM_FIX_* word for every camera
// candidates.bin: int32 n, pad; per candidate int32 camera_a, camera_b and doubles board_rt [6] (tscm_view_candidate).
// out.bin: int32 C, B, n, pad; doubles cam rt [C*6], intrinsics [C*9], board rt [B*6]; int32 board is_initial [B]; doubles
// gain_logdet [n], gain_trace [n]; int32 n_visible [n*2], flags [n]; of the apply: doubles gain_logdet, gain_trace; int32
// n_visible [2], flags, pad; doubles cam_cov [C*15*C*15].
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "tscm/tscm_calib.hpp"

static bool put(std::FILE *f, const std::vector<double> &v) { return v.empty() || std::fwrite(v.data(), sizeof(double), v.size(), f) == v.size(); }
static bool put(std::FILE *f, const std::vector<int> &v) { return v.empty() || std::fwrite(v.data(), sizeof(int), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 7) { std::fprintf(stderr, "usage: %s corners.txt candidates.bin out.bin MASK BORDER MIN_CORNERS\n", argv[0]); return 2; }
    const unsigned short fixed = (unsigned short)std::atoi(argv[4]);
    const double border = std::strtod(argv[5], nullptr);
    const int min_corners = std::atoi(argv[6]);
    std::vector<tscm_view_candidate> cands;
    {
        std::FILE *f = std::fopen(argv[2], "rb");
        int head[2] = { 0, 0 };
        if (!f || std::fread(head, sizeof(int), 2, f) != 2 || head[0] < 1 || head[0] > (1 << 20)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        cands.resize((size_t)head[0]);
        const bool ok = std::fread(cands.data(), sizeof(tscm_view_candidate), cands.size(), f) == cands.size();
        std::fclose(f);
        if (!ok) { std::fprintf(stderr, "%s is short\n", argv[2]); return 2; }
    }
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
        const tscm::MultiCalib::ViewGain all = mul.view_gain(cov, cands, image, border, min_corners);
        const tscm::MultiCalib::ViewGain one = mul.view_gain_apply(cov.cam_cov, cands[0], image, border, min_corners);
        std::vector<double> crt, I, brt;
        std::vector<int> init;
        for (int m = 0; m < C; ++m) { crt.insert(crt.end(), mul.cameras_[m].rt_.begin(), mul.cameras_[m].rt_.end()); I.insert(I.end(), mul.cameras_[m].intrinsic_.begin(), mul.cameras_[m].intrinsic_.end()); }
        for (int b = 0; b < B; ++b) {
            init.push_back(mul.chessboards_[b].is_initial() ? 1 : 0);
            for (int a = 0; a < 6; ++a) brt.push_back(init.back() ? mul.chessboards_[b].rt_[a] : 0.0);
        }
        std::FILE *f = std::fopen(argv[3], "wb");
        const int head[4] = { C, B, (int)cands.size(), 0 };
        std::vector<int> tail(one.n_visible);
        tail.push_back(one.flags[0]);
        tail.push_back(0);
        const bool ok = f && std::fwrite(head, sizeof(int), 4, f) == 4 && put(f, crt) && put(f, I) && put(f, brt) && put(f, init) && put(f, all.gain_logdet) &&
                        put(f, all.gain_trace) && put(f, all.n_visible) && put(f, all.flags) && put(f, one.gain_logdet) && put(f, one.gain_trace) && put(f, tail) &&
                        put(f, one.cam_cov);
        if (!ok || std::fclose(f)) { std::fprintf(stderr, "cannot write %s\n", argv[3]); rc = 2; }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 3;
    }
    tscm_corners_free(&cs);
    return rc;
}
