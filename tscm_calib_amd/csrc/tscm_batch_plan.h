// tscm_batch_plan.h -- host side of the batched mono refinement (tscm_solve_mono_batch): n independent
// TripleSphereCamera::refinement problems (TS.cpp:247-282) concatenated into one device batch.
//
// Pure integer work on the view tables of the problems (never the observations or parameters): the refusals, which
// problems go to the device and which are solved alone, the record slots of every device problem (one per view with
// corners, in board order), the chunks of slots the batched kernels take one workgroup each -- never straddling two
// problems -- and the ranges of every problem.  Every per-problem reduction of the batched kernels runs over the problem's
// own chunks in order and over a chunk's slots in order, so a problem's arithmetic is fixed by its own plan: the chunk
// shapes depend on nothing but the problem itself (checked on the CPU by tests/native/batch_plan_check.cpp).
// Plain C++17 like tscm_layout.h.
#ifndef TSCM_BATCH_PLAN_H
#define TSCM_BATCH_PLAN_H

#include "tscm_layout.h"
#include "tscm_exec_plan.h"
#include "tscm_spec.h"

#include <algorithm>
#include <string>
#include <vector>

namespace tscm {

constexpr int kMbMinChunk = 8;          // slots (views with corners) of one chunk at least ...
constexpr int kMbMaxChunks = 64;        // ... and at most this many chunks per problem: a big problem gets bigger chunks
constexpr int kMbMaxChunkSlots = 32;    // the batched kernels' per-chunk LDS holds this many slots (more than 2,048 views: see below)
constexpr int kMbMaxPoints = 256;       // board corners the evaluation kernel's LDS holds

// Slots per chunk of a problem with n slots: at least kMbMinChunk, enough that the problem has at most kMbMaxChunks chunks
// (the solve kernel's workgroups each reduce all of their problem's chunk partials) -- a function of n alone.  Problems of more
// than kMbMaxChunks * kMbMaxChunkSlots = 2,048 views take more chunks of the largest size.
inline int mb_chunk_slots(int n)
{
    const int per = (n + kMbMaxChunks - 1) / kMbMaxChunks;
    return std::min(kMbMaxChunkSlots, std::max(kMbMinChunk, per));
}

struct BatchPlan {
    int n_problems = 0, n_points = 0;
    // problem -> its index among the device problems, or -1: solved alone (no corner at all: what tscm_solve_fixed does with it)
    std::vector<int> dev_of;
    std::vector<int> dev_prob;                  // device problem -> problem
    int K = 0;                                  // device problems
    // per device problem k: slots [slot_ptr[k], slot_ptr[k + 1]), chunks [chunk_ptr[k], chunk_ptr[k + 1]), boards
    // [board_ptr[k], board_ptr[k + 1]) of the concatenated board array, corners [obs_ptr[k], obs_ptr[k + 1])
    std::vector<int> slot_ptr, chunk_ptr, board_ptr;
    std::vector<long> obs_ptr;
    std::vector<unsigned short> mask;           // [K] held intrinsics (TSCM_FIX_*)
    // per slot: its problem, its view in the problem, the concatenated board, the pose block is free (seen, not held),
    // its first corner in the concatenated observations, its corners
    std::vector<int> slot_prob, slot_view, slot_board, slot_obs, slot_count;
    std::vector<unsigned char> slot_active;
    // per chunk: device problem, first slot, end slot (x, y, z; w = 0)
    std::vector<Int4> chunk;
    long N = 0;                                 // corners of the device batch
    int B = 0;                                  // concatenated boards
    LossArg loss{};                             // the shared loss as the kernels take it (make_spec)
};

// 0, or a TSCM_E_* code and its message in err (out is then untouched).  opt: the caller's options as the library read them
// (read_options); loss_kind / loss_scale: the shared loss; fixed: [n] masks or NULL.  Refusals in order: the arguments,
// every problem's own validation (tscm_layout.h: validate), the batch's shape (mono, one camera, one board), the loss, the
// masks (tscm_spec.h: make_spec), the options (the same codes as tscm_solve_fixed), what this route does not take (fp32
// Jacobians, exec_flags), then a board seen by two views with corners (TSCM_E_INVALID, as the single-problem solver).
inline int plan_batch(const tscm_problem *problems, int n, const tscm_options &opt, const unsigned short *fixed, int loss_kind,
                      double loss_scale, BatchPlan &out, std::string &err)
{
    if (!problems || n <= 0) return layout_fail(err, TSCM_E_INVALID, "tscm_solve_mono_batch needs n_problems > 0 problems");
    for (int i = 0; i < n; ++i) {
        if (int rc = validate(&problems[i], err)) { err = "problem " + std::to_string(i) + ": " + err; return rc; }
    }
    const tscm_problem &p0 = problems[0];
    for (int i = 0; i < n; ++i) {
        const tscm_problem &p = problems[i];
        if (!p.mono || p.n_cameras != 1)
            return layout_fail(err, TSCM_E_UNSUPPORTED, "tscm_solve_mono_batch takes mono problems of one camera only");
        if (p.n_points != p0.n_points)
            return layout_fail(err, TSCM_E_UNSUPPORTED, "the problems of a batch share one board (n_points differ)");
        for (int j = 0; j < 2 * p.n_points; ++j)
            if (p.board_xy[j] != p0.board_xy[j]) return layout_fail(err, TSCM_E_UNSUPPORTED, "the problems of a batch share one board (board_xy differ)");
    }
    if (p0.n_points > kMbMaxPoints) return layout_fail(err, TSCM_E_UNSUPPORTED, "boards of more than 256 corners are not batched");
    SolveSpec spec;                             // (one camera per problem: fixed is the [n] masks of make_spec)
    if (int rc = make_spec(loss_kind, loss_scale, fixed, n, spec, err)) return rc;
    if (int rc = check_exec_options(opt, loss_kind, err)) return rc;
    if (opt.jacobian_fp32) return layout_fail(err, TSCM_E_UNSUPPORTED, "tscm_solve_mono_batch has no fp32-Jacobian tier");
    if (opt.exec_flags) return layout_fail(err, TSCM_E_UNSUPPORTED, "tscm_solve_mono_batch takes no exec_flags");

    BatchPlan b;
    b.n_problems = n; b.n_points = p0.n_points; b.loss = spec.loss;
    b.dev_of.assign(n, -1);
    b.slot_ptr.push_back(0); b.chunk_ptr.push_back(0); b.board_ptr.push_back(0); b.obs_ptr.push_back(0);
    for (int i = 0; i < n; ++i) {
        const tscm_problem &p = problems[i];
        // the views with corners in board order.  A board seen by two such views is refused as the single-problem solver
        // refuses it (tscm_layout.h: build_layout): every slot is one board's 6x6 block in the batched kernels
        std::vector<int> order;
        for (int v = 0; v < p.n_views; ++v) if (p.view_count[v] > 0) order.push_back(v);
        std::sort(order.begin(), order.end(), [&](int x, int y) { return p.view_board[x] < p.view_board[y]; });
        for (size_t q = 1; q < order.size(); ++q)
            if (p.view_board[order[q]] == p.view_board[order[q - 1]]) {
                err = "problem " + std::to_string(i) + ": two views with the same (camera, board)";
                return TSCM_E_INVALID;
            }
        if (order.empty()) continue;
        const int k = b.K++;
        b.dev_of[i] = k; b.dev_prob.push_back(i);
        b.mask.push_back(fixed ? fixed[i] : (unsigned short)0);
        const int ns = (int)order.size(), per = mb_chunk_slots(ns), s0 = b.slot_ptr.back();
        for (int q = 0; q < ns; ++q) {
            const int v = order[q];
            b.slot_prob.push_back(k); b.slot_view.push_back(v);
            b.slot_board.push_back(b.B + p.view_board[v]);
            b.slot_active.push_back(p.board_pose_constant && p.board_pose_constant[p.view_board[v]] ? 0 : 1);
            b.slot_obs.push_back((int)b.N);
            b.slot_count.push_back(p.view_count[v]);
            b.N += p.view_count[v];
        }
        for (int q = 0; q < ns; q += per) b.chunk.push_back(Int4{ k, s0 + q, s0 + std::min(ns, q + per), 0 });
        b.B += p.n_boards;
        b.slot_ptr.push_back(s0 + ns);
        b.chunk_ptr.push_back((int)b.chunk.size());
        b.board_ptr.push_back(b.B);
        b.obs_ptr.push_back(b.N);
    }
    if (b.N > 0x7fffffffL) return layout_fail(err, TSCM_E_UNSUPPORTED, "more than 2^31 corners in one batch");
    out = std::move(b);
    return 0;
}

}  // namespace tscm

#endif
