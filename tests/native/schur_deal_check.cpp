// CPU check of k_schur_gram's deal of board groups (tscm_calib_amd/csrc/tscm_layout.h: schur_group_of,
// schur_virtual_wave): for every chunk size and every rot, each group of four boards is taken exactly once, the waves' counts
// differ by at most one, and what a VIRTUAL wave takes does not depend on rot.  Host logic only (no GPU).
//   usage: schur_deal_check deal                         one JSON line: ok / the first failed condition, the deals of 40 and 64 boards
//          schur_deal_check chunks < problem             one JSON line: the board chunks plan_layout makes of a problem, as [views per
//                                                        board, boards] pairs in launch order.  stdin: n_cameras n_boards n_points
//                                                        n_views, (camera board corners) per view, n_cu waves_per_cu
#include "../../tscm_calib_amd/csrc/tscm_layout.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace tscm;

static std::string g_fail;
static int g_nbd = 0, g_rot = 0;      // the case a failed condition is reported with
#define CHECK(cond) do { if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ", nbd " + std::to_string(g_nbd) + ", rot " + std::to_string(g_rot) + ")"; } while (0)

static void print_counts(const char *name, int nbd, const char *end)
{
    std::printf("\"%s\": [", name);
    for (int v = 0; v < 4; ++v) {
        int n = 0;
        for (int k = 0; k < 4; ++k) n += schur_group_of(nbd, v, k) >= 0;
        std::printf("%d%s", n, v < 3 ? ", " : "");
    }
    std::printf("]%s", end);
}

static int deal()
{
    long cases = 0;
    for (int nbd = 1; nbd <= kChunkBoards; ++nbd)
        for (int rot = 0; rot < 4; ++rot) {
            g_nbd = nbd; g_rot = rot;
            int rot0[4][4];      // what virtual wave v takes as its k-th group when physical wave v plays it (rot 0)
            for (int v = 0; v < 4; ++v) for (int k = 0; k < 4; ++k) rot0[v][k] = schur_group_of(nbd, schur_virtual_wave(v, 0), k);
            const int n_groups = (nbd + 3) / 4;
            std::vector<int> taken(n_groups, 0);
            int lo = 4, hi = 0;
            bool virtual_seen[4] = { false, false, false, false };
            for (int wave = 0; wave < 4; ++wave) {
                const int v = schur_virtual_wave(wave, rot);
                CHECK(v >= 0 && v < 4 && ((v + rot) & 3) == wave && !virtual_seen[v]);      // physical wave = (v + rot) & 3, one to one
                virtual_seen[v] = true;
                int n = 0, last = -1;
                for (int k = 0; k < 4; ++k) {
                    const int g = schur_group_of(nbd, v, k);
                    CHECK(g >= -1 && g < n_groups);
                    CHECK(g == rot0[v][k]);                                                  // the (virtual wave, k) -> group map of rot 0
                    if (g < 0) { last = n_groups; continue; }                                // (none: none for any later k either)
                    CHECK(last < n_groups && g > last);                                      // ascending in k
                    CHECK(4 * g < nbd);                                                      // the group has a board
                    last = g;
                    ++taken[g];
                    ++n;
                }
                lo = std::min(lo, n); hi = std::max(hi, n);
            }
            for (int g = 0; g < n_groups; ++g) CHECK(taken[g] == 1);
            CHECK(hi - lo <= 1);
            if (nbd == kChunkBoards) CHECK(lo == 4 && hi == 4);
            ++cases;
        }
    std::printf("{\"ok\": %s, \"failed\": \"%s\", \"cases\": %ld, ", g_fail.empty() ? "true" : "false", g_fail.c_str(), cases);
    print_counts("boards16", 16, ", ");
    print_counts("boards17", 17, ", ");
    print_counts("boards40", 40, ", ");
    print_counts("boards64", 64, "}\n");
    return g_fail.empty() ? 0 : 1;
}

static int next_int()
{
    int v = 0;
    if (std::scanf("%d", &v) != 1) { std::fprintf(stderr, "chunks: input ends early\n"); std::exit(2); }
    return v;
}

static int chunks()
{
    tscm_problem p{};
    p.n_cameras = next_int(); p.n_boards = next_int(); p.n_points = next_int(); p.n_views = next_int();
    if (p.n_views < 0 || p.n_views > (1 << 24)) { std::fprintf(stderr, "chunks: n_views out of range\n"); return 2; }
    std::vector<int> cam(p.n_views), board(p.n_views), offset(p.n_views), count(p.n_views);
    for (int v = 0, o = 0; v < p.n_views; ++v) { cam[v] = next_int(); board[v] = next_int(); count[v] = next_int(); offset[v] = o; o += count[v]; }
    LayoutDevice dev;
    dev.n_cu = next_int(); dev.waves_per_cu = next_int();
    double dummy[2] = { 0.0, 0.0 };      // (the plan never reads the parameters or the observations)
    p.board_xy = dummy; p.intr = dummy; p.board_rt = dummy; p.cam_rt = dummy; p.obs_u = dummy; p.obs_v = dummy;
    p.view_camera = cam.data(); p.view_board = board.data(); p.view_offset = offset.data(); p.view_count = count.data();
    std::string err;
    if (int rc = validate(&p, err)) { std::fprintf(stderr, "chunks: %d %s\n", rc, err.c_str()); return 2; }
    Layout L;
    if (int rc = plan_layout(&p, 0, 1, dev, L, err)) { std::fprintf(stderr, "chunks: %d %s\n", rc, err.c_str()); return 2; }
    std::printf("{\"slow_boards\": %d, \"chunks\": [", (int)L.slow_boards.size());
    for (size_t c = 0; c < L.bc_desc.size(); ++c) std::printf("[%d, %d]%s", L.bc_desc[c].w, L.bc_desc[c].y - L.bc_desc[c].x, c + 1 < L.bc_desc.size() ? ", " : "");
    std::printf("]}\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "deal")) return deal();
    if (argc >= 2 && !std::strcmp(argv[1], "chunks")) return chunks();
    std::fprintf(stderr, "usage: schur_deal_check deal | chunks < problem\n");
    return 2;
}
