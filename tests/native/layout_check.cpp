// CPU check of solver creation's layout plan (tscm_calib_amd/csrc/tscm_layout.h): random problems -- 1 to 32 cameras and
// mono, boards seen by 0, 1, 2, 3 and more cameras, views without corners, boards without views, held board and camera
// poses -- are planned for every rank of 1 to 8 and a range of CU counts and waves per CU, and every invariant the kernels'
// addressing rests on is re-derived here from the problem and the stated rules, not from the planner's code.  The
// refusals at the problem-size limits are planned on view tables only (the plan never reads the observations).
// Host logic only (no GPU).
//   usage: layout_check random <seed> <problems>     one JSON line: counts of what the problems exercised
//          layout_check refusals                      one JSON line: code and message of every refusal case
#include "../../tscm_calib_amd/csrc/tscm_layout.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

using namespace tscm;

// a problem's view tables and masks (the parameter arrays only need to be non-NULL: the plan does not read them)
struct Prob {
    int C = 1, B = 0, n_points = 1, mono = 0;
    std::vector<int> cam, board, offset, count;
    std::vector<unsigned char> bconst, cconst;
    bool with_bconst = false, with_cconst = false;
    double dummy[2] = { 0.0, 0.0 };
    tscm_problem p{};
    const tscm_problem *get()
    {
        p = tscm_problem{};
        p.n_cameras = C; p.n_boards = B; p.n_points = n_points; p.n_views = (int)cam.size(); p.mono = mono;
        p.board_xy = dummy; p.intr = dummy; p.board_rt = dummy; p.cam_rt = dummy;
        p.view_camera = cam.data(); p.view_board = board.data(); p.view_offset = offset.data(); p.view_count = count.data();
        p.obs_u = dummy; p.obs_v = dummy;
        p.board_pose_constant = with_bconst ? bconst.data() : nullptr;
        p.cam_pose_constant = with_cconst ? cconst.data() : nullptr;
        return &p;
    }
    void add(int c, int b, int n) { offset.push_back(offset.empty() ? 0 : offset.back() + count.back()); cam.push_back(c); board.push_back(b); count.push_back(n); }
};

static std::string g_fail;
#define CHECK(cond) do { if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; } while (0)

static Prob random_problem(std::mt19937_64 &rng)
{
    auto uni = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
    Prob q;
    q.mono = uni(0, 5) == 0;
    q.C = q.mono ? 1 : (uni(0, 2) == 0 ? uni(1, 32) : uni(1, 9));
    q.n_points = uni(1, 90);
    const int shape = uni(0, 3);        // 0: small, 1: many boards (full Schur chunks), 2: many cameras per board (fallback pairs), 3: mixed
    q.B = shape == 0 ? uni(0, 12) : shape == 1 ? uni(300, 2000) : uni(10, 120);
    const int empty_pct = uni(0, 3) * 10;
    for (int b = 0; b < q.B; ++b) {
        int k;      // cameras that see the board
        const int r = uni(0, 9);
        if (shape == 2) k = uni(0, 1) ? uni(4, std::max(4, q.C)) : uni(0, 3);
        else if (shape == 1) k = r < 1 ? 0 : r < 5 ? 1 : r < 8 ? 2 : 3;
        else k = r < 1 ? 0 : r < 3 ? 1 : r < 5 ? 2 : r < 7 ? 3 : uni(4, 8);
        k = std::min(k, q.C);
        std::vector<int> cams(q.C);
        for (int m = 0; m < q.C; ++m) cams[m] = m;
        std::shuffle(cams.begin(), cams.end(), rng);
        for (int i = 0; i < k; ++i) q.add(cams[i], b, uni(0, 99) < empty_pct ? 0 : uni(1, q.n_points));
    }
    // views in a random problem order (with a view without corners now and then that repeats a (camera, board))
    std::vector<int> idx(q.cam.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int)i;
    std::shuffle(idx.begin(), idx.end(), rng);
    Prob s = q;
    s.cam.clear(); s.board.clear(); s.offset.clear(); s.count.clear();
    for (int i : idx) s.add(q.cam[i], q.board[i], q.count[i]);
    if (!s.cam.empty() && uni(0, 4) == 0) s.add(s.cam[0], s.board[0], 0);
    s.with_bconst = uni(0, 1); s.with_cconst = uni(0, 1);
    s.bconst.resize(s.B); s.cconst.resize(s.C);
    for (auto &x : s.bconst) x = uni(0, 3) == 0;
    for (auto &x : s.cconst) x = uni(0, 2) == 0;
    return s;
}

// every invariant of one rank's layout, derived from the problem and the stated rules
static void check_rank(const tscm_problem *p, int world, const LayoutDevice &dev, const Layout &L)
{
    const int C = p->n_cameras, B = L.B, V = L.V, nvw = p->n_views;
    CHECK(L.B_total == p->n_boards && 0 <= L.b0 && L.b0 <= L.b1 && L.b1 <= p->n_boards && B == L.b1 - L.b0);
    // whole-problem facts
    std::vector<std::vector<int>> board_cams(p->n_boards);
    long N_total = 0;
    for (int v = 0; v < nvw; ++v) if (p->view_count[v] > 0) { board_cams[p->view_board[v]].push_back(p->view_camera[v]); N_total += p->view_count[v]; }
    CHECK(L.N_total == N_total);
    std::vector<unsigned char> act(C, 0), pair((size_t)C * C, 0);
    for (auto &cs : board_cams) for (int a : cs) { act[a] = 1; for (int b : cs) pair[(size_t)std::min(a, b) * C + std::max(a, b)] = 1; }
    CHECK(L.cam_active == act && L.pair_present == pair);
    for (int m = 0; m < C; ++m) CHECK(L.cam_const[m] == ((p->mono || (p->cam_pose_constant && p->cam_pose_constant[m])) ? 1 : 0));

    // board_perm: a permutation of the owned boards; boards with views first, by (view count, camera list), ties in
    // caller order; boards without views last
    CHECK((int)L.board_perm.size() == B);
    std::vector<int> dev_board(B, -1);
    for (int i = 0; i < B; ++i) { const int b = L.board_perm[i]; CHECK(b >= 0 && b < B); if (b >= 0 && b < B) { CHECK(dev_board[b] < 0); dev_board[b] = i; } }
    if (!g_fail.empty()) return;
    auto sig = [&](int b) { std::vector<int> cs = board_cams[L.b0 + b]; std::sort(cs.begin(), cs.end()); return cs; };
    for (int i = 1; i < B; ++i) {
        const std::vector<int> x = sig(L.board_perm[i - 1]), y = sig(L.board_perm[i]);
        if (y.empty()) { if (x.empty()) CHECK(L.board_perm[i - 1] < L.board_perm[i]); continue; }
        CHECK(!x.empty());
        CHECK(x.size() < y.size() || (x.size() == y.size() && x <= y));
        if (x == y) CHECK(L.board_perm[i - 1] < L.board_perm[i]);
    }

    // dev2orig: the owned views with corners, camera-major, then by device board; per-view tables follow
    std::vector<int> want;
    for (int v = 0; v < nvw; ++v) if (p->view_count[v] > 0 && p->view_board[v] >= L.b0 && p->view_board[v] < L.b1) want.push_back(v);
    std::vector<int> got = L.dev2orig;
    std::sort(got.begin(), got.end());
    CHECK(got == want && V == (int)want.size());
    if (!g_fail.empty()) return;
    CHECK((int)L.view_cam.size() == V && (int)L.view_board.size() == V && (int)L.view_obs.size() == V && (int)L.view_count.size() == V);
    long N = 0;
    for (int i = 0; i < V; ++i) {
        const int v = L.dev2orig[i];
        CHECK(L.view_cam[i] == p->view_camera[v] && L.view_board[i] == dev_board[p->view_board[v] - L.b0] && L.view_count[i] == p->view_count[v]);
        CHECK(L.view_obs[i] == N);
        N += p->view_count[v];
        if (i) CHECK(L.view_cam[i - 1] < L.view_cam[i] || (L.view_cam[i - 1] == L.view_cam[i] && L.view_board[i - 1] < L.view_board[i]));
    }
    CHECK(L.N == N);
    if (!g_fail.empty()) return;

    // Gram chunks: per camera a run of whole workgroups that covers its views once, in order, and nothing else
    const int n_chunks = (int)L.chunk_vb.size();
    CHECK(n_chunks % 4 == 0 && (int)L.chunk_ve.size() == n_chunks && (int)L.chunk_cam.size() == n_chunks && (int)L.chunk_desc.size() == n_chunks);
    CHECK((int)L.cam_chunk_ptr.size() == C + 1 && L.cam_chunk_ptr[0] == 0 && 4 * L.cam_chunk_ptr[C] == n_chunks);
    if (!g_fail.empty()) return;
    const int target = std::max(64, dev.n_cu * dev.waves_per_cu - 4 * C), per_chunk = std::max(1, (V + target - 1) / target);
    for (int m = 0, vi = 0; m < C; ++m) {
        int ve = vi;
        while (ve < V && L.view_cam[ve] == m) ++ve;
        CHECK(L.cam_chunk_ptr[m] <= L.cam_chunk_ptr[m + 1]);
        int next = vi;
        bool padding = false;
        for (int q = 4 * L.cam_chunk_ptr[m]; q < 4 * L.cam_chunk_ptr[m + 1]; ++q) {
            CHECK(L.chunk_cam[q] == m);
            if (L.chunk_vb[q] == L.chunk_ve[q]) { padding = true; CHECK(L.chunk_vb[q] == ve); continue; }
            CHECK(!padding && L.chunk_vb[q] == next && L.chunk_vb[q] < L.chunk_ve[q] && L.chunk_ve[q] <= ve && L.chunk_ve[q] - L.chunk_vb[q] <= per_chunk);
            next = L.chunk_ve[q];
        }
        CHECK(next == ve);
        CHECK(L.cam_chunk_ptr[m + 1] - L.cam_chunk_ptr[m] == (ve - vi + 4 * per_chunk - 1) / (4 * per_chunk));   // no workgroup that is all padding
        vi = ve;
    }
    for (int q = 0; q < n_chunks; ++q) {
        const Int4 d = L.chunk_desc[q];
        CHECK(d.x == L.chunk_cam[q] && d.y == L.chunk_vb[q] && d.z == L.chunk_ve[q] && d.w == (L.chunk_vb[q] < V ? L.view_obs[L.chunk_vb[q]] : 0));
    }
    for (int q = 0; q <= kMaxCamLds; ++q) CHECK(L.cam_wg[q] == L.cam_chunk_ptr[std::min(q, C)]);

    // slots: board-major, the views of a board in device (= camera) order
    CHECK((int)L.bv_ptr.size() == B + 1 && L.bv_ptr[0] == 0 && L.bv_ptr[B] == V);
    CHECK((int)L.view_slot.size() == V && (int)L.slot_view.size() == V && (int)L.slot_cam.size() == V && (int)L.slot_board.size() == V);
    if (!g_fail.empty()) return;
    for (int q = 0; q < V; ++q) {
        const int v = L.slot_view[q];
        CHECK(v >= 0 && v < V);
        if (v < 0 || v >= V) return;
        CHECK(L.view_slot[v] == q && L.slot_cam[q] == L.view_cam[v] && L.slot_board[q] == L.view_board[v]);
        CHECK(L.bv_ptr[L.slot_board[q]] <= q && q < L.bv_ptr[L.slot_board[q] + 1]);
        if (q && L.slot_board[q - 1] == L.slot_board[q]) CHECK(L.slot_view[q - 1] < v && L.slot_cam[q - 1] < L.slot_cam[q]);
        if (q) CHECK(L.slot_board[q - 1] <= L.slot_board[q]);
    }
    auto nv_of = [&](int b) { return L.bv_ptr[b + 1] - L.bv_ptr[b]; };
    for (int b = 0; b < B; ++b) CHECK(nv_of(b) == (int)board_cams[L.b0 + L.board_perm[b]].size());

    // blocks: every camera pair mi <= mj that shares a board anywhere, in lexicographic order
    std::vector<int> bid((size_t)C * C, -1);
    int n_bids = 0;
    unsigned long long mask = 0;
    for (int mi = 0; mi < C; ++mi)
        for (int mj = mi; mj < C; ++mj)
            if (pair[(size_t)mi * C + mj]) { bid[(size_t)mi * C + mj] = n_bids++; if (C <= kMaxCamLds) mask |= 1ull << (mi * 8 + mj); }
    CHECK(L.n_bids == n_bids && L.bid_of == bid && L.pair_mask == mask);

    // device boards: [0, n_fast) 1-3 views, [n_fast, n_fast + n_slow) more, the rest none
    int n_fast = 0, n_slow = 0;
    while (n_fast < B && nv_of(n_fast) >= 1 && nv_of(n_fast) <= 3) ++n_fast;
    while (n_fast + n_slow < B && nv_of(n_fast + n_slow) > 3) ++n_slow;
    for (int b = n_fast + n_slow; b < B; ++b) CHECK(nv_of(b) == 0);
    // board chunks: contiguous boards (and slots) of one signature, at most kChunkBoards, together exactly the fast boards
    const int n_bc = (int)L.bc_desc.size();
    CHECK((int)L.bc_tile.size() == 6 * n_bc && L.nv_chunks[0] == 0);
    if (!g_fail.empty()) return;
    std::vector<int> tile_use(L.n_tiles > 0 ? L.n_tiles : 0, 0);
    CHECK((int)L.bid_part_ptr.size() == n_bids + 1 && L.bid_part_ptr[0] == 0 && L.bid_part_ptr[n_bids] == L.n_tiles);
    if (!g_fail.empty()) return;
    for (int b = 0; b < n_bids; ++b) CHECK(L.bid_part_ptr[b] <= L.bid_part_ptr[b + 1]);
    for (int b = 0; b <= kSmallBids; ++b) CHECK(L.bid_part_small[b] == L.bid_part_ptr[std::min(b, n_bids)]);
    auto use_tile = [&](int t, int block) {
        CHECK(t >= 0 && t < L.n_tiles && block >= 0);
        if (t < 0 || t >= L.n_tiles || block < 0) return;
        tile_use[t]++;
        CHECK(L.bid_part_ptr[block] <= t && t < L.bid_part_ptr[block + 1]);
    };
    int at = 0, seen[4] = { 0, 0, 0, 0 };
    for (int c = 0; c < n_bc; ++c) {
        const Int4 d = L.bc_desc[c];
        CHECK(d.x == at && d.x < d.y && d.y - d.x <= kChunkBoards && d.y <= n_fast && d.w >= 1 && d.w <= 3);
        if (!g_fail.empty()) return;
        CHECK(d.z == L.bv_ptr[d.x] && L.bv_ptr[d.y] - L.bv_ptr[d.x] == d.w * (d.y - d.x));
        for (int b = d.x; b < d.y; ++b) CHECK(nv_of(b) == d.w && sig(L.board_perm[b]) == sig(L.board_perm[d.x]));
        if (c) CHECK(L.bc_desc[c - 1].w <= d.w);
        CHECK(c >= L.nv_chunk0[d.w] && c < L.nv_chunk0[d.w] + L.nv_chunks[d.w]);
        seen[d.w]++;
        int t = 0;
        for (int p1 = 0; p1 < d.w; ++p1)
            for (int p2 = p1; p2 < d.w; ++p2, ++t) use_tile(L.bc_tile[6 * c + t], bid[(size_t)L.slot_cam[d.z + p1] * C + L.slot_cam[d.z + p2]]);
        for (; t < 6; ++t) CHECK(L.bc_tile[6 * c + t] == -1);
        at = d.y;
    }
    CHECK(at == n_fast);
    for (int nv = 1; nv <= 3; ++nv) CHECK(seen[nv] == L.nv_chunks[nv] && (L.nv_chunks[nv] || L.nv_chunk0[nv] == 0));

    // fallback pairs: every slot pair q1 <= q2 of every board of more than three views once, in chunks of one block
    std::vector<int> slow;
    for (int b = n_fast; b < n_fast + n_slow; ++b) slow.push_back(b);
    CHECK(L.slow_boards == slow);
    const int n_pairs = (int)L.pair_i.size();
    CHECK((int)L.pair_j.size() == n_pairs && (int)L.pair_board.size() == n_pairs);
    CHECK(L.pc_end.size() == L.pc_begin.size() && L.pc_tile.size() == L.pc_begin.size());
    if (!g_fail.empty()) return;
    std::map<std::pair<int, int>, int> pairs;
    for (int k = 0; k < n_pairs; ++k) {
        CHECK(L.pair_board[k] >= n_fast && L.pair_board[k] < n_fast + n_slow);
        if (!g_fail.empty()) return;
        const int b = L.pair_board[k];
        CHECK(L.bv_ptr[b] <= L.pair_i[k] && L.pair_i[k] <= L.pair_j[k] && L.pair_j[k] < L.bv_ptr[b + 1]);
        pairs[{ L.pair_i[k], L.pair_j[k] }]++;
    }
    size_t want_pairs = 0;
    for (int b : slow) {
        want_pairs += (size_t)nv_of(b) * (nv_of(b) + 1) / 2;
        for (int q1 = L.bv_ptr[b]; q1 < L.bv_ptr[b + 1]; ++q1) for (int q2 = q1; q2 < L.bv_ptr[b + 1]; ++q2) CHECK(pairs[std::make_pair(q1, q2)] == 1);
    }
    CHECK((size_t)n_pairs == want_pairs);
    for (size_t c = 0, next = 0; c < L.pc_begin.size(); ++c) {
        CHECK(L.pc_begin[c] == (int)next && L.pc_begin[c] < L.pc_end[c] && L.pc_end[c] <= n_pairs);
        if (!g_fail.empty()) return;
        const int blk = bid[(size_t)L.slot_cam[L.pair_i[L.pc_begin[c]]] * C + L.slot_cam[L.pair_j[L.pc_begin[c]]]];
        for (int k = L.pc_begin[c]; k < L.pc_end[c]; ++k) CHECK(bid[(size_t)L.slot_cam[L.pair_i[k]] * C + L.slot_cam[L.pair_j[k]]] == blk);
        use_tile(L.pc_tile[c], blk);
        next = L.pc_end[c];
        if (c + 1 == L.pc_begin.size()) CHECK((int)next == n_pairs);
    }
    if (L.pc_begin.empty()) CHECK(n_pairs == 0);
    // tiles: each used exactly once
    for (int t = 0; t < L.n_tiles; ++t) CHECK(tile_use[t] == 1);

    // back-substitution geometry, held board poses
    CHECK(L.bs_threads == 128 || L.bs_threads == 256);
    if (C <= kMaxCamLds && n_bids > 0) CHECK(L.bs_threads == 256);
    CHECK(L.n_bs_blocks == (B + L.bs_threads / 8 - 1) / (L.bs_threads / 8));
    CHECK((int)L.board_const.size() == B);
    for (int i = 0; i < B && g_fail.empty(); ++i) CHECK(L.board_const[i] == (p->board_pose_constant && p->board_pose_constant[L.b0 + L.board_perm[i]] ? 1 : 0));
    (void)world;
}

static int run_random(unsigned long long seed, int n)
{
    std::mt19937_64 rng(seed);
    const int cus[] = { 1, 4, 32, 80, 256 }, waves[] = { 4, 8, 12, 16 };
    long layouts = 0, fallback_pairs = 0, slow_boards = 0, chunks_full = 0, multi_view_chunks = 0, empty_views = 0, mono = 0, big_rigs = 0, cams_max = 0;
    std::set<int> worlds;
    for (int it = 0; it < n; ++it) {
        Prob q = random_problem(rng);
        const tscm_problem *p = q.get();
        std::string err;
        if (int rc = validate(p, err)) { std::printf("{\"ok\": false, \"problem\": %d, \"error\": \"validate %d %s\"}\n", it, rc, err.c_str()); return 1; }
        LayoutDevice dev;
        dev.n_cu = cus[rng() % 5]; dev.waves_per_cu = waves[rng() % 4];
        const int world = 1 + (int)(rng() % 8);
        worlds.insert(world);
        mono += q.mono; big_rigs += q.C > kMaxCamLds; cams_max = std::max<long>(cams_max, q.C);
        for (int v = 0; v < p->n_views; ++v) empty_views += p->view_count[v] == 0;
        int next_b0 = 0;
        std::vector<unsigned char> views_seen(p->n_views, 0);
        long N_total = -1;
        for (int rank = 0; rank < world; ++rank) {
            Layout L;
            if (int rc = plan_layout(p, rank, world, dev, L, err)) {
                std::printf("{\"ok\": false, \"problem\": %d, \"rank\": %d, \"error\": \"plan %d %s\"}\n", it, rank, rc, err.c_str());
                return 1;
            }
            check_rank(p, world, dev, L);
            // over the ranks: the owned board ranges partition the boards, the views with corners once, one N_total
            CHECK(L.b0 == next_b0);
            next_b0 = L.b1;
            for (int v : L.dev2orig) { CHECK(!views_seen[v]); views_seen[v] = 1; }
            CHECK(N_total < 0 || L.N_total == N_total);
            N_total = L.N_total;
            if (!g_fail.empty()) {
                std::printf("{\"ok\": false, \"problem\": %d, \"rank\": %d, \"world\": %d, \"C\": %d, \"B\": %d, \"failed\": \"%s\"}\n", it, rank, world, q.C, q.B, g_fail.c_str());
                return 1;
            }
            ++layouts;
            fallback_pairs += (long)L.pair_i.size(); slow_boards += (long)L.slow_boards.size();
            for (auto &d : L.bc_desc) { chunks_full += d.y - d.x == kChunkBoards; }
            for (size_t k = 0; k < L.chunk_vb.size(); ++k) multi_view_chunks += L.chunk_ve[k] - L.chunk_vb[k] > 1;
        }
        CHECK(next_b0 == p->n_boards);
        for (int v = 0; v < p->n_views; ++v) CHECK(views_seen[v] == (p->view_count[v] > 0));
        if (!g_fail.empty()) { std::printf("{\"ok\": false, \"problem\": %d, \"failed\": \"%s\"}\n", it, g_fail.c_str()); return 1; }
    }
    std::printf("{\"ok\": true, \"problems\": %d, \"layouts\": %ld, \"worlds\": %zu, \"mono\": %ld, \"big_rigs\": %ld, \"cams_max\": %ld, "
                "\"empty_views\": %ld, \"slow_boards\": %ld, \"fallback_pairs\": %ld, \"full_board_chunks\": %ld, \"multi_view_chunks\": %ld}\n",
                n, layouts, worlds.size(), mono, big_rigs, cams_max, empty_views, slow_boards, fallback_pairs, chunks_full, multi_view_chunks);
    return 0;
}

// one refusal case: "name": [code, "message"] (0, "" when the problem is accepted)
static void report(const char *name, int rc, const std::string &err, bool last = false)
{
    std::printf("\"%s\": [%d, \"%s\"]%s", name, rc, rc ? err.c_str() : "", last ? "" : ", ");
}

static int plan_one(Prob &q, std::string &err)
{
    const tscm_problem *p = q.get();
    if (int rc = validate(p, err)) return rc;
    Layout L;
    return plan_layout(p, 0, 1, LayoutDevice{}, L, err);
}

static int run_refusals()
{
    std::string err;
    std::printf("{");
    // a (camera, board) seen twice; twice with one of them empty is not a duplicate (views without corners are dropped)
    { Prob q; q.C = 2; q.B = 2; q.n_points = 4; q.add(0, 0, 4); q.add(1, 1, 4); q.add(0, 0, 3); report("duplicate_view", plan_one(q, err), err); }
    { Prob q; q.C = 2; q.B = 2; q.n_points = 4; q.add(0, 0, 4); q.add(1, 1, 4); q.add(0, 0, 0); report("duplicate_empty_view", plan_one(q, err), err); }
    // corners: 32-bit observation offsets (N * 8 < 0xffffe000) and more than 2^31 -- one camera, one full board per view
    const int np = 1 << 20;
    const long n_lim = (long)((0xffffe000ull - 1) / sizeof(double));      // the largest N whose byte offsets fit
    for (long n : { n_lim, n_lim + 1, 0x80000000L }) {
        Prob q; q.C = 1; q.n_points = np;
        const int full = (int)(n / np), rest = (int)(n % np);
        q.B = full + (rest ? 1 : 0);
        for (int b = 0; b < full; ++b) q.add(0, b, np);
        if (rest) q.add(0, full, rest);
        report(n == n_lim ? "corners_at_limit" : n == n_lim + 1 ? "corners_above_limit" : "corners_2_31", plan_one(q, err), err);
    }
    // views: 32-bit record offsets (V * kRec * 8 < 0xffffe000) -- boards of three views of one corner
    const long v_lim = (long)((0xffffe000ull - 1) / (sizeof(double) * kRec));
    for (long V : { v_lim, v_lim + 1 }) {
        Prob q; q.C = 3; q.n_points = 1; q.B = (int)((V + 2) / 3);
        q.cam.reserve(V); q.board.reserve(V); q.offset.reserve(V); q.count.reserve(V);
        for (long v = 0; v < V; ++v) q.add((int)(v % 3), (int)(v / 3), 1);
        report(V == v_lim ? "views_at_limit" : "views_above_limit", plan_one(q, err), err);
    }
    // validate()
    auto base = []() { Prob q; q.C = 2; q.B = 2; q.n_points = 4; q.add(0, 0, 4); q.add(1, 0, 4); q.add(1, 1, 2); return q; };
    report("null_problem", validate(nullptr, err), err);
    { Prob q = base(); q.n_points = 0; report("zero_points", plan_one(q, err), err); }
    { Prob q = base(); q.B = -1; report("negative_boards", plan_one(q, err), err); }
    { Prob q = base(); q.mono = 1; report("mono_two_cameras", plan_one(q, err), err); }
    { Prob q = base(); const tscm_problem *p = q.get(); tscm_problem r = *p; r.board_xy = nullptr; report("null_board_xy", validate(&r, err), err); }
    { Prob q = base(); const tscm_problem *p = q.get(); tscm_problem r = *p; r.cam_rt = nullptr; report("null_cam_rt", validate(&r, err), err); }
    { Prob q = base(); const tscm_problem *p = q.get(); tscm_problem r = *p; r.obs_v = nullptr; report("null_obs", validate(&r, err), err); }
    { Prob q = base(); q.C = 33; report("too_many_cameras", plan_one(q, err), err); }
    { Prob q = base(); q.cam[1] = 2; report("camera_out_of_range", plan_one(q, err), err); }
    { Prob q = base(); q.board[2] = 2; report("board_out_of_range", plan_one(q, err), err); }
    { Prob q = base(); q.count[0] = 5; report("count_above_points", plan_one(q, err), err); }
    { Prob q = base(); q.offset[1] = -1; report("negative_offset", plan_one(q, err), err); }
    { Prob q = base(); report("valid", plan_one(q, err), err, true); }
    std::printf("}\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return run_random(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3]));
    if (argc >= 2 && !std::strcmp(argv[1], "refusals")) return run_refusals();
    std::fprintf(stderr, "usage: layout_check random <seed> <problems> | refusals\n");
    return 2;
}
