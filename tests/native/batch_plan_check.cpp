// CPU check of the batched mono refinement's host plan (tscm_calib_amd/csrc/tscm_batch_plan.h): random batches are planned
// and every invariant the batched kernels rely on is re-derived from the problems; a problem's plan must be the same
// wherever it sits in the batch; the refusals come back with their codes.  Prints one JSON line; exit code 1 on a failure.
//   batch_plan_check random <seed> <batches>
//   batch_plan_check refusals
//   batch_plan_check plan <n_points> <problem>...     plans the batch described on the command line and prints its shape:
//       <problem> = <n_boards>/<corner count of view 0>,<of view 1>,.../<constant board>,<constant board>,...
//       (view v sees board v; the list of constant boards may be empty): per problem its chunks (slots of each) and the
//       active flag of every slot, in slot order
#include "../../tscm_calib_amd/csrc/tscm_batch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace tscm;

namespace {

struct Owned {                      // the arrays behind one tscm_problem (views only: observations are never read by the plan)
    std::vector<int> cam, board, off, cnt;
    std::vector<double> u, v, intr, board_rt;
    std::vector<unsigned char> bconst;
    tscm_problem p{};
};

std::vector<double> board_xy(int cols, int rows)
{
    std::vector<double> xy;
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) { xy.push_back(45.0 * c); xy.push_back(45.0 * r); }
    return xy;
}

void make(Owned &o, std::mt19937 &rng, const std::vector<double> &xy, int max_views)
{
    const int n_points = (int)xy.size() / 2;
    std::uniform_int_distribution<int> nv(0, max_views);
    const int B = nv(rng), V = B;
    o.cam.assign(V, 0); o.board.resize(V); o.off.resize(V); o.cnt.resize(V);
    std::vector<int> perm(B);
    for (int b = 0; b < B; ++b) perm[b] = b;
    std::shuffle(perm.begin(), perm.end(), rng);           // views in any board order
    int n = 0;
    for (int v = 0; v < V; ++v) {
        o.board[v] = perm[v];
        o.off[v] = n;
        o.cnt[v] = rng() % 8 == 0 ? 0 : (int)(rng() % n_points) + 1;
        n += o.cnt[v];
    }
    o.u.assign(std::max(n, 1), 0.0); o.v.assign(std::max(n, 1), 0.0);
    o.intr.assign(9, 1.0); o.board_rt.assign(6 * (size_t)std::max(B, 1), 0.0);
    o.bconst.assign(std::max(B, 1), 0);
    const bool some_const = rng() % 4 == 0;
    if (some_const) for (int b = 0; b < B; ++b) o.bconst[b] = rng() % 3 == 0;
    tscm_problem &p = o.p;
    p = tscm_problem{};
    p.n_cameras = 1; p.n_boards = B; p.n_points = n_points; p.n_views = V;
    p.board_xy = xy.data(); p.view_camera = o.cam.data(); p.view_board = o.board.data(); p.view_offset = o.off.data();
    p.view_count = o.cnt.data(); p.obs_u = o.u.data(); p.obs_v = o.v.data(); p.intr = o.intr.data(); p.board_rt = o.board_rt.data();
    p.mono = 1;
    p.board_pose_constant = some_const ? o.bconst.data() : nullptr;
}

tscm_options defaults()
{
    tscm_options o{};
    o.struct_size = sizeof(o); o.max_num_iterations = 100; o.check_every = 4; o.jacobi_scaling = 1;
    return o;
}

// the shape of one problem's plan, relative to its own first slot and chunk
std::vector<long> shape(const BatchPlan &b, int k)
{
    std::vector<long> s;
    const int s0 = b.slot_ptr[k];
    for (int c = b.chunk_ptr[k]; c < b.chunk_ptr[k + 1]; ++c) { s.push_back(b.chunk[c].y - s0); s.push_back(b.chunk[c].z - s0); }
    for (int q = s0; q < b.slot_ptr[k + 1]; ++q) {
        s.push_back(b.slot_view[q]); s.push_back(b.slot_board[q] - b.board_ptr[k]); s.push_back(b.slot_count[q]);
        s.push_back(b.slot_obs[q] - b.obs_ptr[k]); s.push_back(b.slot_active[q]);
    }
    return s;
}

int g_fail = 0;
std::string g_why;
void check(bool c, const std::string &why) { if (!c && !g_fail) { g_fail = 1; g_why = why; } }

int random_mode(unsigned seed, int batches)
{
    std::mt19937 rng(seed);
    const std::vector<double> xy[2] = { board_xy(9, 6), board_xy(11, 8) };
    long problems = 0, empty = 0, big = 0, masked = 0, multi_chunk = 0, max_chunks = 0, repeated = 0;
    for (int it = 0; it < batches && !g_fail; ++it) {
        const std::vector<double> &bxy = xy[rng() % 2];
        const int n = 1 + (int)(rng() % (it % 10 == 0 ? 300 : 24));
        std::vector<Owned> own(n);
        for (int i = 0; i < n; ++i) make(own[i], rng, bxy, rng() % 16 == 0 ? 2000 : 200);
        std::vector<tscm_problem> ps(n);
        std::vector<unsigned short> fixed(n);
        for (int i = 0; i < n; ++i) { ps[i] = own[i].p; fixed[i] = (unsigned short)(rng() % 3 == 0 ? rng() % 512 : 0); masked += fixed[i] != 0; }
        BatchPlan b;
        std::string err;
        if (it % 5 == 4) {
            // one problem of the batch gets a board seen by two views with corners: the whole batch is refused
            Owned &d = own[rng() % n];
            if (d.p.n_views >= 2) {
                const int v0 = (int)(rng() % d.p.n_views), v1 = (v0 + 1 + (int)(rng() % (d.p.n_views - 1))) % d.p.n_views;
                const int keep_b = d.board[v1], keep_c0 = d.cnt[v0], keep_c1 = d.cnt[v1];
                d.board[v1] = d.board[v0];
                d.cnt[v0] = std::max(d.cnt[v0], 1); d.cnt[v1] = std::max(d.cnt[v1], 1);     // (offsets overlap: never read by the plan)
                BatchPlan r;
                const int rrc = plan_batch(ps.data(), n, defaults(), fixed.data(), TSCM_LOSS_NONE, 0.0, r, err);
                check(rrc == TSCM_E_INVALID && err.find("two views with the same (camera, board)") != std::string::npos,
                      "a repeated board is not refused");
                ++repeated;
                d.board[v1] = keep_b; d.cnt[v0] = keep_c0; d.cnt[v1] = keep_c1;
            }
        }
        const int rc = plan_batch(ps.data(), n, defaults(), fixed.data(), TSCM_LOSS_NONE, 0.0, b, err);
        check(rc == 0, "random batch refused: " + err);
        if (rc) break;
        problems += n;
        // problems -> device problems
        int k_seen = 0;
        for (int i = 0; i < n; ++i) {
            long corners = 0;
            for (int v = 0; v < ps[i].n_views; ++v) corners += ps[i].view_count[v];
            check((b.dev_of[i] < 0) == (corners == 0), "a problem without corners goes to the device, or one with corners does not");
            if (b.dev_of[i] < 0) { ++empty; continue; }
            check(b.dev_of[i] == k_seen && b.dev_prob[k_seen] == i, "device problems are not in problem order");
            check(b.mask[k_seen] == fixed[i], "mask of a device problem");
            ++k_seen;
        }
        check(b.K == k_seen && (int)b.slot_ptr.size() == b.K + 1 && (int)b.chunk_ptr.size() == b.K + 1, "range arrays");
        // every view with corners is exactly one slot of its own problem; corners contiguous in slot order
        long corner = 0;
        for (int k = 0; k < b.K; ++k) {
            const tscm_problem &p = ps[b.dev_prob[k]];
            std::vector<int> hit(p.n_views, 0);
            int prev_board = -1;
            for (int q = b.slot_ptr[k]; q < b.slot_ptr[k + 1]; ++q) {
                const int v = b.slot_view[q];
                check(b.slot_prob[q] == k, "slot of another problem inside a problem's range");
                check(v >= 0 && v < p.n_views && p.view_count[v] > 0, "slot of a view without corners");
                if (v < 0 || v >= p.n_views) continue;
                ++hit[v];
                check(b.slot_board[q] == b.board_ptr[k] + p.view_board[v], "slot board");
                check(p.view_board[v] > prev_board, "slots not in board order");
                prev_board = p.view_board[v];
                check(b.slot_count[q] == p.view_count[v] && b.slot_obs[q] == corner, "slot corners not contiguous");
                check(b.slot_active[q] == (p.board_pose_constant && p.board_pose_constant[p.view_board[v]] ? 0 : 1), "slot active flag");
                corner += b.slot_count[q];
            }
            for (int v = 0; v < p.n_views; ++v) check(hit[v] == (p.view_count[v] > 0 ? 1 : 0), "a view is not exactly one slot");
            check(b.obs_ptr[k + 1] == corner, "problem corner range");
            check(b.board_ptr[k + 1] - b.board_ptr[k] == p.n_boards, "problem board range");
            // chunks: the problem's slots exactly once, in order, never another problem's, within the size limits
            const int nslots = b.slot_ptr[k + 1] - b.slot_ptr[k];
            int at = b.slot_ptr[k];
            for (int c = b.chunk_ptr[k]; c < b.chunk_ptr[k + 1]; ++c) {
                check(b.chunk[c].x == k, "chunk of another problem");
                check(b.chunk[c].y == at && b.chunk[c].z > b.chunk[c].y, "chunks do not tile the problem's slots");
                check(b.chunk[c].z - b.chunk[c].y <= kMbMaxChunkSlots, "chunk larger than the kernels' LDS");
                for (int q = b.chunk[c].y; q < b.chunk[c].z; ++q) check(b.slot_prob[q] == k, "chunk spans two problems");
                at = b.chunk[c].z;
            }
            check(at == b.slot_ptr[k + 1], "chunks end before the problem's last slot");
            const int nch = b.chunk_ptr[k + 1] - b.chunk_ptr[k];
            check(nslots <= kMbMaxChunks * kMbMaxChunkSlots ? nch <= kMbMaxChunks : true, "more chunks than the solve kernel reduces");
            max_chunks = std::max<long>(max_chunks, nch);
            multi_chunk += nch > 1;
            big += nslots > 1000;
        }
        check(corner == b.N && (int)b.chunk.size() == b.chunk_ptr[b.K], "batch totals");
        // position independence: every device problem planned alone, and in the reversed batch, has the same shape
        std::vector<tscm_problem> rev(ps.rbegin(), ps.rend());
        std::vector<unsigned short> rfix(fixed.rbegin(), fixed.rend());
        BatchPlan r;
        check(plan_batch(rev.data(), n, defaults(), rfix.data(), TSCM_LOSS_NONE, 0.0, r, err) == 0, "reversed batch refused");
        for (int k = 0; k < b.K && !g_fail; ++k) {
            const int i = b.dev_prob[k];
            BatchPlan one;
            check(plan_batch(&ps[i], 1, defaults(), &fixed[i], TSCM_LOSS_NONE, 0.0, one, err) == 0 && one.K == 1, "problem alone refused");
            check(shape(one, 0) == shape(b, k), "a problem's plan depends on where it sits (alone)");
            check(shape(r, r.dev_of[n - 1 - i]) == shape(b, k), "a problem's plan depends on where it sits (reversed)");
        }
    }
    std::printf("{\"ok\": %s, \"problems\": %ld, \"empty\": %ld, \"big\": %ld, \"masked\": %ld, \"multi_chunk\": %ld, \"max_chunks\": %ld, \"repeated\": %ld, \"why\": \"%s\"}\n",
                g_fail ? "false" : "true", problems, empty, big, masked, multi_chunk, max_chunks, repeated, g_why.c_str());
    return g_fail;
}

int refusals_mode()
{
    std::mt19937 rng(7);
    const std::vector<double> xy = board_xy(9, 6), xy2 = board_xy(11, 8);
    std::vector<double> xy3 = xy;
    xy3[5] += 1.0;
    Owned a, b, c, d;
    make(a, rng, xy, 30); make(b, rng, xy, 30); make(c, rng, xy2, 30); make(d, rng, xy3, 30);
    std::vector<std::pair<std::string, int>> out;
    auto run = [&](const char *name, std::vector<tscm_problem> ps, int n, tscm_options o, const unsigned short *f, int kind, double scale) {
        BatchPlan bp;
        std::string err;
        out.emplace_back(name, plan_batch(ps.empty() ? nullptr : ps.data(), n, o, f, kind, scale, bp, err));
    };
    const tscm_options o = defaults();
    run("ok", { a.p, b.p }, 2, o, nullptr, TSCM_LOSS_NONE, 0.0);
    run("zero_problems", { a.p }, 0, o, nullptr, TSCM_LOSS_NONE, 0.0);
    run("null_problems", {}, 2, o, nullptr, TSCM_LOSS_NONE, 0.0);
    { tscm_problem q = b.p; q.mono = 0; std::vector<double> cam(6, 0.0); q.cam_rt = cam.data();
      run("not_mono", { a.p, q }, 2, o, nullptr, TSCM_LOSS_NONE, 0.0); }
    { tscm_problem q = b.p; q.n_cameras = 2; run("mono_two_cameras", { a.p, q }, 2, o, nullptr, TSCM_LOSS_NONE, 0.0); }
    { tscm_problem q = b.p; q.mono = 0; q.n_cameras = 2; std::vector<double> cam(12, 0.0); q.cam_rt = cam.data();
      run("rig", { a.p, q }, 2, o, nullptr, TSCM_LOSS_NONE, 0.0); }
    run("board_points_differ", { a.p, c.p }, 2, o, nullptr, TSCM_LOSS_NONE, 0.0);
    run("board_xy_differ", { a.p, d.p }, 2, o, nullptr, TSCM_LOSS_NONE, 0.0);
    { const unsigned short f[2] = { 0, 1u << 9 }; run("mask_bits", { a.p, b.p }, 2, o, f, TSCM_LOSS_NONE, 0.0); }
    { const unsigned short f[2] = { TSCM_FIX_ALL, TSCM_MODEL_UCM }; run("masks_ok", { a.p, b.p }, 2, o, f, TSCM_LOSS_NONE, 0.0); }
    run("loss_kind", { a.p, b.p }, 2, o, nullptr, 7, 1.0);
    run("loss_scale", { a.p, b.p }, 2, o, nullptr, TSCM_LOSS_HUBER, 0.0);
    run("loss_ok", { a.p, b.p }, 2, o, nullptr, TSCM_LOSS_CAUCHY, 2.0);
    { tscm_options q = o; q.max_num_iterations = 256; run("iterations", { a.p, b.p }, 2, q, nullptr, TSCM_LOSS_NONE, 0.0); }
    { tscm_options q = o; q.jacobian_fp32 = 1; run("fp32", { a.p, b.p }, 2, q, nullptr, TSCM_LOSS_NONE, 0.0); }
    { tscm_options q = o; q.exec_flags = TSCM_EXEC_SEPARATE_BACKSUB; run("exec_flags", { a.p, b.p }, 2, q, nullptr, TSCM_LOSS_NONE, 0.0); }
    { tscm_options q = o; q.exec_flags = 1 << 20; run("exec_flags_unknown", { a.p, b.p }, 2, q, nullptr, TSCM_LOSS_NONE, 0.0); }
    {   // a board seen by two views with corners: refused as build_layout refuses it; two views of a board of which one is
        // empty: accepted (the empty one is no slot)
        Owned e;
        make(e, rng, xy, 30);
        while (e.p.n_views < 2) make(e, rng, xy, 30);
        e.board[1] = e.board[0];
        e.cnt[0] = e.cnt[1] = 3;
        run("repeated_board", { a.p, e.p }, 2, o, nullptr, TSCM_LOSS_NONE, 0.0);
        e.cnt[1] = 0;
        run("repeated_board_empty", { a.p, e.p }, 2, o, nullptr, TSCM_LOSS_NONE, 0.0);
    }
    std::printf("{");
    for (size_t i = 0; i < out.size(); ++i) std::printf("%s\"%s\": %d", i ? ", " : "", out[i].first.c_str(), out[i].second);
    std::printf("}\n");
    return 0;
}

// a comma-separated list of non-negative integers; false on anything else
bool int_list(const std::string &s, std::vector<int> &out)
{
    out.clear();
    size_t at = 0;
    while (at < s.size()) {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        if (end == at || end - at > 9) return false;
        int v = 0;
        for (size_t i = at; i < end; ++i) {
            if (s[i] < '0' || s[i] > '9') return false;
            v = 10 * v + (s[i] - '0');
        }
        out.push_back(v);
        at = end + 1;
    }
    return s.empty() || s.back() != ',';
}

int plan_mode(int argc, char **argv)
{
    std::vector<int> one;
    if (!int_list(argv[2], one) || one.size() != 1 || one[0] < 1 || one[0] > 4096) { std::fprintf(stderr, "plan: bad n_points\n"); return 2; }
    const int n_points = one[0], n = argc - 3;
    std::vector<double> xy;
    for (int j = 0; j < n_points; ++j) { xy.push_back(45.0 * (j % 16)); xy.push_back(45.0 * (j / 16)); }
    std::vector<Owned> own(n);
    std::vector<tscm_problem> ps(n);
    for (int i = 0; i < n; ++i) {
        const std::string a = argv[3 + i];
        const size_t s1 = a.find('/'), s2 = s1 == std::string::npos ? s1 : a.find('/', s1 + 1);
        std::vector<int> nb, cnt, cst;
        if (s2 == std::string::npos || !int_list(a.substr(0, s1), nb) || nb.size() != 1 || !int_list(a.substr(s1 + 1, s2 - s1 - 1), cnt) ||
            !int_list(a.substr(s2 + 1), cst) || (int)cnt.size() > nb[0]) { std::fprintf(stderr, "plan: bad problem '%s'\n", a.c_str()); return 2; }
        Owned &o = own[i];
        const int B = nb[0], V = (int)cnt.size();
        o.cam.assign(V, 0); o.board.resize(V); o.off.resize(V); o.cnt = cnt;
        int total = 0;
        for (int v = 0; v < V; ++v) { o.board[v] = v; o.off[v] = total; total += cnt[v]; }
        o.u.assign(std::max(total, 1), 0.0); o.v.assign(std::max(total, 1), 0.0);
        o.intr.assign(9, 1.0); o.board_rt.assign(6 * (size_t)std::max(B, 1), 0.0);
        o.bconst.assign(std::max(B, 1), 0);
        for (int b : cst) { if (b >= B) { std::fprintf(stderr, "plan: constant board %d of %d\n", b, B); return 2; } o.bconst[b] = 1; }
        tscm_problem &p = o.p;
        p = tscm_problem{};
        p.n_cameras = 1; p.n_boards = B; p.n_points = n_points; p.n_views = V;
        p.board_xy = xy.data(); p.view_camera = o.cam.data(); p.view_board = o.board.data(); p.view_offset = o.off.data();
        p.view_count = o.cnt.data(); p.obs_u = o.u.data(); p.obs_v = o.v.data(); p.intr = o.intr.data(); p.board_rt = o.board_rt.data();
        p.mono = 1;
        p.board_pose_constant = cst.empty() ? nullptr : o.bconst.data();
        ps[i] = p;
    }
    BatchPlan b;
    std::string err;
    const int rc = plan_batch(ps.data(), n, defaults(), nullptr, TSCM_LOSS_NONE, 0.0, b, err);
    if (rc) { std::printf("{\"ok\": false, \"rc\": %d, \"why\": \"%s\"}\n", rc, err.c_str()); return 0; }
    std::printf("{\"ok\": true, \"n_chunks\": %d, \"n_slots\": %d, \"n_boards\": %d, \"min_chunk\": %d, \"max_chunks\": %d, \"max_chunk_slots\": %d, \"max_points\": %d, \"problems\": [",
                (int)b.chunk.size(), (int)b.slot_prob.size(), b.B, kMbMinChunk, kMbMaxChunks, kMbMaxChunkSlots, kMbMaxPoints);
    for (int i = 0; i < n; ++i) {
        const int k = b.dev_of[i];
        std::printf("%s{\"device\": %s, \"chunks\": [", i ? ", " : "", k >= 0 ? "true" : "false");
        if (k >= 0) for (int c = b.chunk_ptr[k]; c < b.chunk_ptr[k + 1]; ++c) std::printf("%s%d", c > b.chunk_ptr[k] ? ", " : "", b.chunk[c].z - b.chunk[c].y);
        std::printf("], \"active\": [");
        if (k >= 0) for (int q = b.slot_ptr[k]; q < b.slot_ptr[k + 1]; ++q) std::printf("%s%d", q > b.slot_ptr[k] ? ", " : "", (int)b.slot_active[q]);
        std::printf("], \"counts\": [");
        if (k >= 0) for (int q = b.slot_ptr[k]; q < b.slot_ptr[k + 1]; ++q) std::printf("%s%d", q > b.slot_ptr[k] ? ", " : "", b.slot_count[q]);
        std::printf("], \"boards\": %d}", k >= 0 ? b.board_ptr[k + 1] - b.board_ptr[k] : 0);
    }
    std::printf("]}\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return random_mode((unsigned)std::atoi(argv[2]), std::atoi(argv[3]));
    if (argc >= 2 && !std::strcmp(argv[1], "refusals")) return refusals_mode();
    if (argc >= 4 && !std::strcmp(argv[1], "plan")) return plan_mode(argc, argv);
    std::fprintf(stderr, "usage: batch_plan_check random <seed> <batches> | refusals | plan <n_points> <problem>...\n");
    return 2;
}
