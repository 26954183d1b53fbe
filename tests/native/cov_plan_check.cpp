// CPU check of the covariance stage's host plan (tscm_calib_amd/csrc/tscm_cov_plan.h).  Host logic only (no GPU).
//   usage: cov_plan_check plan < problems     one JSON line: the masks (cov_masks) and every table of plan_covariance for each
//          problem on standard input, for tests/test_cov_plan.py to compare with a Python statement of the same rules.
//          Input, integers separated by white space: the number of problems, then per problem
//            C B V mono has_cam_const has_board_const has_fixed, V x (camera board corners), [C cam_const] [B board_const] [C fixed]
//          cov_plan_check refuse          one JSON line: plan_covariance's refusals, checked here
#include "../../tscm_calib_amd/csrc/tscm_cov_plan.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace tscm;

template <typename T>
static void put(const char *name, const std::vector<T> &v, bool last = false)
{
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? ", " : "", (int)v[i]);
    std::printf("]%s", last ? "" : ", ");
}

static int plan_mode()
{
    int n = 0;
    if (!(std::cin >> n)) return 2;
    std::printf("[");
    for (int k = 0; k < n; ++k) {
        int C, B, V, mono, hc, hb, hf;
        if (!(std::cin >> C >> B >> V >> mono >> hc >> hb >> hf)) return 2;
        std::vector<int> cam(V), board(V), count(V), offset(V, 0);
        for (int v = 0; v < V; ++v) { std::cin >> cam[v] >> board[v] >> count[v]; offset[v] = v ? offset[v - 1] + count[v - 1] : 0; }
        std::vector<unsigned char> cc(hc ? C : 0), bc(hb ? B : 0);
        std::vector<unsigned short> fixed(hf ? C : 0);
        for (auto &x : cc) { int t; std::cin >> t; x = (unsigned char)t; }
        for (auto &x : bc) { int t; std::cin >> t; x = (unsigned char)t; }
        for (auto &x : fixed) { int t; std::cin >> t; x = (unsigned short)t; }
        if (!std::cin) return 2;
        tscm_problem p{};
        p.n_cameras = C; p.n_boards = B; p.n_points = 1 << 20; p.n_views = V; p.mono = mono;
        p.view_camera = cam.data(); p.view_board = board.data(); p.view_count = count.data(); p.view_offset = offset.data();
        p.cam_pose_constant = hc ? cc.data() : nullptr; p.board_pose_constant = hb ? bc.data() : nullptr;
        std::vector<unsigned char> cam_free, board_free;
        cov_masks(&p, hf ? fixed.data() : nullptr, cam_free, board_free);
        CovPlan c;
        std::string err;
        const int rc = plan_covariance(C, B, V, cam.data(), board.data(), cam_free.data(), board_free.data(), c, err);
        std::printf("%s{\"rc\": %d, \"n_cam_free\": %d, \"n_free\": %d, ", k ? ", " : "", rc, c.n_cam_free, c.n_free);
        put("cam_free", cam_free); put("board_free", board_free); put("compact_of", c.compact_of); put("wide_of", c.wide_of);
        put("free_boards", c.free_boards); put("board_start", c.board_start); put("board_views", c.board_views); put("view_slot", c.view_slot);
        put("tile_a", c.tile_a); put("tile_b", c.tile_b); put("tile_of", c.tile_of); put("tile_start", c.tile_start);
        put("pair_v", c.pair_v); put("pair_w", c.pair_w); put("tile_chunk", c.tile_chunk); put("chunk_begin", c.chunk_begin);
        put("chunk_end", c.chunk_end, true);
        std::printf("}");
    }
    std::printf("]\n");
    return 0;
}

static int refuse_mode()
{
    std::string fail;
    auto expect = [&](int C, int B, int V, const int *vc, const int *vb, const unsigned char *cf, const unsigned char *bf, const char *word) {
        CovPlan c;
        c.n_free = -7;
        std::string err;
        const int rc = plan_covariance(C, B, V, vc, vb, cf, bf, c, err);
        if ((rc != TSCM_E_INVALID || err.find(word) == std::string::npos || c.n_free != -7) && fail.empty()) fail = std::string(word) + ": " + err;
    };
    const int vc[2] = { 0, 1 }, vb[2] = { 0, 0 }, vc_bad[2] = { 0, 2 }, vb_bad[2] = { 0, -1 };
    std::vector<unsigned char> cf(33 * 15, 0), bf(1, 1), cf_b(30, 0);
    cf_b[15 + 13] = 1;
    expect(0, 1, 2, vc, vb, cf.data(), bf.data(), "n_cameras");
    expect(33, 1, 2, vc, vb, cf.data(), bf.data(), "n_cameras");
    expect(2, -1, 0, vc, vb, cf.data(), bf.data(), "n_boards");
    expect(2, 1, -1, vc, vb, cf.data(), bf.data(), "n_views");
    expect(2, 1, 2, nullptr, vb, cf.data(), bf.data(), "view_camera");
    expect(2, 1, 2, vc, nullptr, cf.data(), bf.data(), "view_board");
    expect(2, 1, 2, vc, vb, nullptr, bf.data(), "cam_free");
    expect(2, 1, 2, vc, vb, cf.data(), nullptr, "board_free");
    expect(2, 1, 2, vc_bad, vb, cf.data(), bf.data(), "view_camera[1]");
    expect(2, 1, 2, vc, vb_bad, cf.data(), bf.data(), "view_board[1]");
    expect(2, 1, 2, vc, vb, cf_b.data(), bf.data(), "cam_free");
    std::printf("{\"ok\": %s, \"fail\": \"%s\"}\n", fail.empty() ? "true" : "false", fail.c_str());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "plan")) return plan_mode();
    if (argc >= 2 && !std::strcmp(argv[1], "refuse")) return refuse_mode();
    std::fprintf(stderr, "usage: cov_plan_check plan < problems | cov_plan_check refuse\n");
    return 2;
}
