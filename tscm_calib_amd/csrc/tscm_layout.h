// tscm_layout.h -- host side of solver creation: the layout of one rank's share of a problem on the device.
//
// Pure integer work on the view tables of a tscm_problem (never the observations): which boards this rank owns, the
// whole-problem facts every rank derives identically, the device order of views and boards, the Gram kernels' view
// chunks, the board-major record slots, the camera-pair blocks of T, the Schur kernels' board chunks and fallback pairs
// and the numbering of their partial tiles.  tscm_solver_create_sharded uploads what plan_layout returns; every kernel's
// addressing rests on the invariants stated here (checked on the CPU by tests/native/layout_check.cpp).
#ifndef TSCM_LAYOUT_H
#define TSCM_LAYOUT_H

#include "../../include/tscm/tscm.h"

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

namespace tscm {

constexpr int kRecW = 84;          // doubles per view in the W region: E^T [F | r], 14 columns x 6 rows, column-major
constexpr int kRecE = 18;          // doubles per view in the E region: E^T E_wb, 3 columns x 6 rows, column-major
constexpr int kRecG = 6;           // doubles per view in the G region: E^T r once more, compact (round 5): the board statistics read 48
                                   // contiguous bytes per view instead of the last 48 of every 672-byte W record
constexpr int kRec = kRecW + kRecE + kRecG;  // doubles per view over the regions (allocation size, offset limits)
constexpr int kSmallBids = 36;     // camera-pair blocks of a rig of <= 8 cameras (8 + 28): their partial-tile ranges travel as kernel arguments
constexpr int kMaxCamLds = 8;      // n_pad = 16*C <= 128: reduced system solved in registers/LDS (k_solve_reduced)
constexpr int kMaxCam = 32;        // larger rigs: k_solve_reduced_big factors the system in global memory (n_pad <= 512)
constexpr int kChunkBoards = 64;   // boards of one chunk of k_schur_gram at most (its LDS holds their factors)
static_assert(kSmallBids >= kMaxCamLds * (kMaxCamLds + 1) / 2, "every camera pair of a rig the register/LDS solver takes");

// shared with device code (k_schur_gram): unmarked under a plain C++ compiler
#ifdef __HIPCC__
#define TSCM_LAYOUT_FN __host__ __device__ inline
#else
#define TSCM_LAYOUT_FN inline
#endif

// Phase 1 of k_schur_gram contracts a chunk of nbd <= kChunkBoards boards in groups of four (the last one ragged), and the
// four waves of the workgroup share the n = ceil(nbd / 4) groups evenly, each a run of adjacent groups: VIRTUAL wave v takes
// floor(n / 4) groups, the first n mod 4 waves one more; its k-th group is returned, or -1 when it has no such group (then it
// has none for any later k either).  40 boards: 3, 3, 2, 2 groups (0-2, 3-5, 6-7, 8-9), not the 4, 4, 2, 0 of "wave w takes
// boards 16 w .. 16 w + 15"; 64 boards: 4, 4, 4, 4, which IS that assignment -- a full chunk keeps its bits and its access
// pattern.  (Dealing the groups round-robin, v, v + 4, .., balances the same and measured the same at config 4, but a wave's
// requests then stride over the chunk and config 5's launch was 0.45 us slower: DESIGN 13.)
// Sums are ordered by the virtual wave -- a wave adds its groups in ascending k, the four waves' tiles are added as
// (v0 + v1) + (v2 + v3) -- and physical wave (v + rot) & 3 plays virtual wave v: the result does not depend on rot, which only
// decides which wave (and with it which SIMD of the CU) does the work.  Every launch runs at rot 0: giving the second
// workgroup of a CU rot 2 (3, 3, 2, 2 groups against 2, 2, 3, 3 on the four SIMDs) was measured and bought nothing
// (DESIGN 13); the argument stays for the tests, which ask for the same bits at rot 0 and 2.
TSCM_LAYOUT_FN int schur_group_of(int nbd, int v, int k)
{
    const int n = (nbd + 3) >> 2, base = n >> 2, rem = n & 3;
    return k < base + (v < rem ? 1 : 0) ? v * base + (v < rem ? v : rem) + k : -1;
}
// ... and the virtual wave that physical wave `wave` plays under rot
TSCM_LAYOUT_FN int schur_virtual_wave(int wave, int rot) { return (wave - rot) & 3; }

struct Int4 { int x, y, z, w; };   // what the device reads as int4 (the upload converts)

// the device facts the layout depends on: compute units, and resident waves per CU of the Gram kernel (k_eval_gram4)
struct LayoutDevice { int n_cu = 1, waves_per_cu = 4; };

struct Layout {
    // frame ownership: this rank owns boards [b0, b1) of the caller's B_total
    int b0 = 0, b1 = 0, B = 0, B_total = 0;
    // whole-problem facts (identical on every rank): per camera, its pose is held / it has views; per camera pair
    // (mi <= mj, [mi * C + mj]), they share a board; corners of the whole job
    std::vector<unsigned char> cam_const, cam_active, pair_present;
    long N_total = 0;
    // this rank's views with corners in device order (camera-major, then device board) and its corners
    int V = 0, N = 0;
    std::vector<int> dev2orig;                  // device view -> problem view
    std::vector<int> board_perm;                // device board -> board of the caller, relative to b0
    std::vector<int> view_cam, view_board, view_obs, view_count;   // per device view; view_board: the DEVICE board
    // Gram kernels: chunks of views (one wave each), whole workgroups of 4 per camera, never straddling a camera
    std::vector<int> chunk_vb, chunk_ve, chunk_cam;
    std::vector<int> cam_chunk_ptr;             // [C + 1] first workgroup of each camera
    std::vector<Int4> chunk_desc;               // per chunk: camera, first view, end view, observation offset of the first view
    int cam_wg[kMaxCamLds + 1] = {};            // cam_chunk_ptr by value (rigs of <= kMaxCamLds cameras)
    // records are stored board-major: slot q of board b lies in [bv_ptr[b], bv_ptr[b + 1])
    std::vector<int> bv_ptr, view_slot, slot_cam, slot_view, slot_board;
    // camera-pair blocks ("bids") of T: every pair that shares a board on ANY rank, in lexicographic order
    int n_bids = 0;
    std::vector<int> bid_of;                    // [C * C] block of (mi, mj), mi <= mj; -1: none (the device's bid_lut)
    unsigned long long pair_mask = 0;           // bit mi * 8 + mj: the pair has a block (rigs of <= kMaxCamLds cameras)
    // Schur kernels: chunks of boards of one signature (<= 3 views per board), in signature order
    std::vector<Int4> bc_desc;                  // first board, end board, first slot, views per board
    std::vector<int> bc_tile;                   // [chunk * 6 + t] partial tile of the chunk's t-th view pair, -1 past nv (nv + 1) / 2
    int nv_chunk0[4] = {}, nv_chunks[4] = {};   // chunks of NV views per board: [nv_chunk0[NV], + nv_chunks[NV])
    // boards of more than three views: factored one by one, their view pairs (q1 <= q2, slots) in chunks per block
    std::vector<int> slow_boards, pair_i, pair_j, pair_board;
    std::vector<int> pc_begin, pc_end, pc_tile;
    // partial tiles: those of block b are [bid_part_ptr[b], bid_part_ptr[b + 1])
    int n_tiles = 0;
    std::vector<int> bid_part_ptr;
    int bid_part_small[kSmallBids + 1] = {};    // bid_part_ptr by value (rigs of <= kMaxCamLds cameras)
    // back-substitution geometry: 128 threads / 16 boards or 256 / 32 per workgroup
    int bs_threads = 128, n_bs_blocks = 0;
    std::vector<unsigned char> board_const;     // [B] device board: pose block held constant
};

inline int layout_fail(std::string &err, int code, const char *msg) { err = msg; return code; }

inline int validate(const tscm_problem *p, std::string &err)
{
    if (!p) return layout_fail(err, TSCM_E_INVALID, "problem is NULL");
    if (p->n_cameras < 1 || p->n_boards < 0 || p->n_points < 1 || p->n_views < 0) return layout_fail(err, TSCM_E_INVALID, "negative or zero problem dimensions");
    if (p->mono && p->n_cameras != 1) return layout_fail(err, TSCM_E_INVALID, "mono problem needs exactly one camera");
    if (!p->board_xy || !p->intr || (!p->board_rt && p->n_boards) || (!p->mono && !p->cam_rt)) return layout_fail(err, TSCM_E_INVALID, "NULL parameter/board array");
    if (p->n_views && (!p->view_camera || !p->view_board || !p->view_offset || !p->view_count || !p->obs_u || !p->obs_v)) return layout_fail(err, TSCM_E_INVALID, "NULL view/observation array");
    if (p->n_cameras > kMaxCam) return layout_fail(err, TSCM_E_UNSUPPORTED, "more than 32 cameras");
    for (int v = 0; v < p->n_views; ++v) {
        if (p->view_camera[v] < 0 || p->view_camera[v] >= p->n_cameras) return layout_fail(err, TSCM_E_INVALID, "view_camera out of range");
        if (p->view_board[v] < 0 || p->view_board[v] >= p->n_boards) return layout_fail(err, TSCM_E_INVALID, "view_board out of range");
        if (p->view_count[v] < 0 || p->view_count[v] > p->n_points) return layout_fail(err, TSCM_E_INVALID, "view_count outside [0, n_points]");
        if (p->view_offset[v] < 0) return layout_fail(err, TSCM_E_INVALID, "negative view_offset");
    }
    return 0;
}

// owner[b] = rank of board b: contiguous ranges balanced by corner count (shared by tscm_shard_frames and the solver)
inline void shard_owner(const tscm_problem *p, int world, std::vector<int> &owner)
{
    std::vector<double> per_board(p->n_boards, 0.0);
    for (int v = 0; v < p->n_views; ++v) per_board[p->view_board[v]] += p->view_count[v];
    double total = 0.0;
    for (double x : per_board) total += x;
    owner.assign(p->n_boards, 0);
    double before = 0.0;
    for (int b = 0; b < p->n_boards; ++b) {
        const int r = total > 0.0 ? (int)(before * world / total) : 0;
        owner[b] = std::min(r, world - 1);
        before += per_board[b];
    }
}

// The layout of rank `rank` of `world` for a validated problem: 0, or the TSCM_E_* code of a problem the kernels cannot
// address (and its message in err).  Every rank is handed the WHOLE problem description and keeps the views of the boards
// it owns; what the ranks must agree on is derived from the whole problem, identically on every rank: which cameras have
// views at all (free columns of the reduced system), which camera pairs share a board (tiles of T) and the total corner
// count.
inline int plan_layout(const tscm_problem *p, int rank, int world, const LayoutDevice &dev, Layout &L, std::string &err)
{
    L = Layout{};
    const int C = p->n_cameras;
    // ---- frame ownership ------------------------------------------------------------------------
    std::vector<int> owner;
    shard_owner(p, world, owner);
    int b0 = 0;
    while (b0 < p->n_boards && owner[b0] < rank) ++b0;
    int b1 = b0;
    while (b1 < p->n_boards && owner[b1] == rank) ++b1;
    L.b0 = b0; L.b1 = b1; L.B_total = p->n_boards;
    const int B = L.B = b1 - b0;

    // ---- whole-problem facts (identical on every rank) -------------------------------------------
    L.cam_const.assign(C, 0); L.cam_active.assign(C, 0); L.pair_present.assign((size_t)C * C, 0);
    for (int m = 0; m < C; ++m) L.cam_const[m] = (p->mono || (p->cam_pose_constant && p->cam_pose_constant[m])) ? 1 : 0;
    {
        // cameras per board, then every camera pair (mi <= mj) that shares a board
        std::vector<int> ptr(p->n_boards + 1, 0), cams;
        for (int v = 0; v < p->n_views; ++v) if (p->view_count[v] > 0) ptr[p->view_board[v] + 1]++;
        for (int b = 0; b < p->n_boards; ++b) ptr[b + 1] += ptr[b];
        cams.resize(ptr[p->n_boards]);
        std::vector<int> fill(p->n_boards, 0);
        for (int v = 0; v < p->n_views; ++v) {
            if (p->view_count[v] <= 0) continue;
            const int b = p->view_board[v];
            cams[ptr[b] + fill[b]++] = p->view_camera[v];
            L.cam_active[p->view_camera[v]] = 1;
            L.N_total += p->view_count[v];
        }
        for (int b = 0; b < p->n_boards; ++b)
            for (int i = ptr[b]; i < ptr[b + 1]; ++i)
                for (int j = ptr[b]; j < ptr[b + 1]; ++j) {
                    const int mi = std::min(cams[i], cams[j]), mj = std::max(cams[i], cams[j]);
                    L.pair_present[(size_t)mi * C + mj] = 1;
                }
    }

    // ---- device view order: this rank's views with corners, sorted by (camera, board) -----------
    std::vector<int> &order = L.dev2orig;
    for (int v = 0; v < p->n_views; ++v) if (p->view_count[v] > 0 && p->view_board[v] >= b0 && p->view_board[v] < b1) order.push_back(v);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        if (p->view_camera[a] != p->view_camera[b]) return p->view_camera[a] < p->view_camera[b];
        return p->view_board[a] < p->view_board[b];
    });
    for (size_t i = 1; i < order.size(); ++i)
        if (p->view_camera[order[i]] == p->view_camera[order[i - 1]] && p->view_board[order[i]] == p->view_board[order[i - 1]])
            return layout_fail(err, TSCM_E_INVALID, "two views with the same (camera, board)");
    const int V = L.V = (int)order.size();
    // ---- device board order: boards grouped by camera-set signature (number of views, then the cameras), unseen boards
    // last.  The Schur kernels work on chunks of boards of ONE signature; with this numbering a chunk is a contiguous
    // range of boards AND of record slots, so its kernels derive every address from one small descriptor instead of
    // chasing per-board index tables (each dependent global load costs about a microsecond at the head of a kernel).
    std::vector<int> dev_board(B, -1);          // caller's board (relative to b0) -> device board
    {
        std::vector<int> ptr(B + 1, 0), cams(V);
        for (int i = 0; i < V; ++i) ptr[p->view_board[order[i]] - b0 + 1]++;
        for (int b = 0; b < B; ++b) ptr[b + 1] += ptr[b];
        std::vector<int> fill(B, 0);
        for (int i = 0; i < V; ++i) { const int b = p->view_board[order[i]] - b0; cams[ptr[b] + fill[b]++] = p->view_camera[order[i]]; }   // `order` is camera-major: sorted
        std::vector<int> &perm = L.board_perm;
        perm.resize(B);
        std::iota(perm.begin(), perm.end(), 0);
        std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) {
            const int nx = ptr[x + 1] - ptr[x], ny = ptr[y + 1] - ptr[y];
            if ((nx == 0) != (ny == 0)) return ny == 0;           // boards without views go last
            if (nx != ny) return nx < ny;
            for (int k = 0; k < nx; ++k) if (cams[ptr[x] + k] != cams[ptr[y] + k]) return cams[ptr[x] + k] < cams[ptr[y] + k];
            return false;
        });
        for (int i = 0; i < B; ++i) dev_board[perm[i]] = i;
    }
    // views of one camera sorted by device board
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        if (p->view_camera[a] != p->view_camera[b]) return p->view_camera[a] < p->view_camera[b];
        return dev_board[p->view_board[a] - b0] < dev_board[p->view_board[b] - b0];
    });
    std::vector<int> &view_cam = L.view_cam, &view_board = L.view_board, &view_obs = L.view_obs;
    view_cam.resize(V); view_board.resize(V); view_obs.resize(V); L.view_count.resize(V);
    long N = 0;
    for (int i = 0; i < V; ++i) {
        const int v = order[i];
        view_cam[i] = p->view_camera[v]; view_board[i] = dev_board[p->view_board[v] - b0]; L.view_count[i] = p->view_count[v];
        view_obs[i] = (int)N; N += p->view_count[v];
    }
    if (N > 0x7fffffffL) return layout_fail(err, TSCM_E_UNSUPPORTED, "more than 2^31 corners");
    // the Gram kernels address observations, per-view constants and records with 32-bit buffer offsets and
    // park the stores of idle lanes at offset 0xffffe000, which must lie beyond the end of every buffer
    if ((unsigned long long)N * sizeof(double) >= 0xffffe000ull || (unsigned long long)V * kRec * sizeof(double) >= 0xffffe000ull)
        return layout_fail(err, TSCM_E_UNSUPPORTED, "problem too large for 32-bit buffer offsets (more than 3.7 M views or 536 M corners on one GPU)");
    L.N = (int)N;

    // ---- chunks of views (one wave each), never straddling a camera ----------------------------
    // about one round of resident waves, less the reduction workgroups of the cameras
    const int target_chunks = std::max(64, dev.n_cu * dev.waves_per_cu - 4 * C);
    const int per_chunk = std::max(1, (V + target_chunks - 1) / target_chunks);
    L.cam_chunk_ptr.assign(C + 1, 0);
    for (int m = 0, i = 0; m < C; ++m) {
        L.cam_chunk_ptr[m] = (int)L.chunk_vb.size() / 4;     // in workgroups
        int e = i;
        while (e < V && view_cam[e] == m) ++e;
        for (int c0 = i; c0 < e; c0 += per_chunk) { L.chunk_vb.push_back(c0); L.chunk_ve.push_back(std::min(e, c0 + per_chunk)); L.chunk_cam.push_back(m); }
        while (L.chunk_vb.size() % 4) { L.chunk_vb.push_back(e); L.chunk_ve.push_back(e); L.chunk_cam.push_back(m); }   // empty chunks: whole workgroups per camera
        i = e;
    }
    L.cam_chunk_ptr[C] = (int)L.chunk_vb.size() / 4;
    // the same per chunk in ONE 16-byte record (+ the observation offset of its first view): the head of k_eval_gram4 is
    // control block + descriptor, then the data
    for (size_t q = 0; q < L.chunk_vb.size(); ++q)
        L.chunk_desc.push_back({ L.chunk_cam[q], L.chunk_vb[q], L.chunk_ve[q], L.chunk_vb[q] < V ? view_obs[L.chunk_vb[q]] : 0 });
    for (int q = 0; q <= kMaxCamLds; ++q) L.cam_wg[q] = L.cam_chunk_ptr[std::min(q, C)];

    // ---- board -> views (device order => increasing camera) --------------------------------------
    std::vector<int> &bv_ptr = L.bv_ptr, bv_idx(V);
    bv_ptr.assign(B + 1, 0);
    for (int i = 0; i < V; ++i) bv_ptr[view_board[i] + 1]++;
    for (int b = 0; b < B; ++b) bv_ptr[b + 1] += bv_ptr[b];
    {
        std::vector<int> fill(B, 0);
        for (int i = 0; i < V; ++i) { const int b = view_board[i]; bv_idx[bv_ptr[b] + fill[b]++] = i; }
    }
    // records are stored board-major: slot q of bv order <-> device view bv_idx[q]
    std::vector<int> &slot_cam = L.slot_cam;
    L.view_slot.resize(V); slot_cam.resize(V); L.slot_view.resize(V); L.slot_board.resize(V);
    for (int q = 0; q < V; ++q) { L.view_slot[bv_idx[q]] = q; slot_cam[q] = view_cam[bv_idx[q]]; L.slot_view[q] = bv_idx[q]; L.slot_board[q] = view_board[bv_idx[q]]; }

    // ---- Schur-complement work lists ------------------------------------------------------------
    // camera-pair blocks ("bids") of T: every pair that shares a board on ANY rank, in lexicographic order
    L.bid_of.assign((size_t)C * C, -1);
    for (int mi = 0; mi < C; ++mi)
        for (int mj = mi; mj < C; ++mj)
            if (L.pair_present[(size_t)mi * C + mj]) L.bid_of[mi * C + mj] = L.n_bids++;
    const int n_bids = L.n_bids;
    auto get_bid = [&](int mi, int mj) { return L.bid_of[mi * C + mj]; };      // views of a board are sorted by camera: mi <= mj
    if (C <= kMaxCamLds)
        for (int mi = 0; mi < C; ++mi) for (int mj = mi; mj < C; ++mj) if (get_bid(mi, mj) >= 0) L.pair_mask |= 1ull << (mi * 8 + mj);
    // boards grouped by camera-set signature (views of a board are already sorted by camera)
    std::vector<int> order_b;
    for (int b = 0; b < B; ++b) if (bv_ptr[b + 1] > bv_ptr[b]) order_b.push_back(b);
    auto sig_less = [&](int x, int y) {
        const int nx = bv_ptr[x + 1] - bv_ptr[x], ny = bv_ptr[y + 1] - bv_ptr[y];
        if (nx != ny) return nx < ny;
        for (int k = 0; k < nx; ++k) {
            const int cx = slot_cam[bv_ptr[x] + k], cy = slot_cam[bv_ptr[y] + k];
            if (cx != cy) return cx < cy;
        }
        return false;
    };
    std::stable_sort(order_b.begin(), order_b.end(), sig_less);
    // Every partial tile belongs to one camera-pair block; tiles of a block are numbered contiguously
    // (two passes: count, then assign) so that k_T_reduce streams them without indirection.
    struct ChunkT { int begin, end, nv, bid[6]; };   // begin / end: positions in order_b
    std::vector<ChunkT> bchunks;
    struct PChunk { int begin, end, bid; };
    std::vector<PChunk> pchunks;
    struct FbPair { int q1, q2, board; };
    std::vector<std::vector<FbPair>> fb_pairs;      // fallback pairs per bid (boards with > 3 views)
    int chunked_boards = 0;
    {
        size_t fast_boards = 0;
        for (int b : order_b) if (bv_ptr[b + 1] - bv_ptr[b] <= 3) ++fast_boards;
        // chunks of 16 .. kChunkBoards boards (k_schur_gram: 4 waves x groups of 4 boards), about 512 of them on big problems
        // The Schur kernels stream the records and a CU sustains only its share of the memory system, so the CUs must
        // get equal numbers of workgroups: two per CU on big problems (a multiple of the CU count), never more than
        // kChunkBoards boards each, at least 16 (four waves of one group of four).
        const int target_bchunks = 2 * std::max(1, dev.n_cu);
        const int per_bchunk = std::min<int>(kChunkBoards, std::max<int>(16, (int)((fast_boards + target_bchunks - 1) / target_bchunks)));
        size_t i = 0;
        while (i < order_b.size()) {
            size_t e = i + 1;
            while (e < order_b.size() && !sig_less(order_b[i], order_b[e]) && !sig_less(order_b[e], order_b[i])) ++e;
            const int bf = order_b[i];
            const int nv = bv_ptr[bf + 1] - bv_ptr[bf];
            if (nv <= 3) {
                for (size_t c0 = i; c0 < e; c0 += per_bchunk) {
                    const size_t c1 = std::min(e, c0 + per_bchunk);
                    ChunkT ch{};
                    ch.begin = chunked_boards;
                    chunked_boards += (int)(c1 - c0);
                    ch.end = chunked_boards;
                    ch.nv = nv;
                    int t = 0;
                    for (int p1 = 0; p1 < nv; ++p1)
                        for (int p2 = p1; p2 < nv; ++p2) ch.bid[t++] = get_bid(slot_cam[bv_ptr[bf] + p1], slot_cam[bv_ptr[bf] + p2]);
                    bchunks.push_back(ch);
                }
            } else {
                for (size_t k = i; k < e; ++k) {
                    const int b = order_b[k];
                    L.slow_boards.push_back(b);
                    for (int q1 = bv_ptr[b]; q1 < bv_ptr[b + 1]; ++q1)
                        for (int q2 = q1; q2 < bv_ptr[b + 1]; ++q2) {
                            const int bid = get_bid(slot_cam[q1], slot_cam[q2]);
                            if ((int)fb_pairs.size() <= bid) fb_pairs.resize(bid + 1);
                            fb_pairs[bid].push_back({ q1, q2, b });
                        }
                }
            }
            i = e;
        }
        size_t n_fb = 0;
        for (auto &v : fb_pairs) n_fb += v.size();
        const int per_pchunk = std::max<int>(1, (int)((n_fb + 511) / 512));
        for (size_t bid = 0; bid < fb_pairs.size(); ++bid) {
            const int base = (int)L.pair_i.size();
            for (auto &pr : fb_pairs[bid]) { L.pair_i.push_back(pr.q1); L.pair_j.push_back(pr.q2); L.pair_board.push_back(pr.board); }
            const int end = (int)L.pair_i.size();
            for (int c0 = base; c0 < end; c0 += per_pchunk) pchunks.push_back({ c0, std::min(end, c0 + per_pchunk), (int)bid });
        }
    }
    std::vector<int> &bid_part_ptr = L.bid_part_ptr;
    bid_part_ptr.assign(n_bids + 1, 0);
    for (auto &ch : bchunks) for (int t = 0; t < ch.nv * (ch.nv + 1) / 2; ++t) bid_part_ptr[ch.bid[t] + 1]++;
    for (auto &pc : pchunks) bid_part_ptr[pc.bid + 1]++;
    for (int b = 0; b < n_bids; ++b) bid_part_ptr[b + 1] += bid_part_ptr[b];
    L.n_tiles = bid_part_ptr[n_bids];
    for (int b = 0; b <= kSmallBids; ++b) L.bid_part_small[b] = bid_part_ptr[std::min(b, n_bids)];
    std::vector<int> next_tile(bid_part_ptr.begin(), bid_part_ptr.end() - 1);
    for (auto &ch : bchunks)
        for (int t = 0; t < 6; ++t) L.bc_tile.push_back(t < ch.nv * (ch.nv + 1) / 2 ? next_tile[ch.bid[t]]++ : -1);
    for (auto &pc : pchunks) { L.pc_begin.push_back(pc.begin); L.pc_end.push_back(pc.end); L.pc_tile.push_back(next_tile[pc.bid]++); }
    // chunks are in signature order, i.e. sorted by views per board: one launch of k_schur_gram<NV> per NV present
    int max_boards = 1;
    for (size_t c = 0; c < bchunks.size(); ++c) {
        const int nv = bchunks[c].nv;
        if (L.nv_chunks[nv]++ == 0) L.nv_chunk0[nv] = (int)c;
        max_boards = std::max(max_boards, bchunks[c].end - bchunks[c].begin);
    }
    if (max_boards > kChunkBoards) return layout_fail(err, TSCM_E_UNSUPPORTED, "internal error: board chunk larger than kChunkBoards");
    // device boards are numbered in signature order, so entry k of the chunked boards IS board k
    for (int k = 0; k < chunked_boards; ++k) if (order_b[k] != k) return layout_fail(err, TSCM_E_UNSUPPORTED, "internal error: device board order is not the signature order");
    for (auto &ch : bchunks) L.bc_desc.push_back({ ch.begin, ch.end, bv_ptr[ch.begin], ch.nv });

    // ---- back-substitution geometry and held board poses ------------------------------------------
    // groups of 16 boards while they all fit the chip at once (5 workgroups per CU), groups of 32 beyond that
    L.bs_threads = (B + 15) / 16 > 5 * std::max(1, dev.n_cu) * 3 / 2 ? 256 : 128;
    // ... and groups of 32 (256 threads, the reduced solve's workgroup shape) wherever the back-substitution can ride
    // in the reduced solve's launch (up to 8 cameras: k_solve_nd<.., true>)
    if (C <= kMaxCamLds && n_bids > 0) L.bs_threads = 256;
    L.n_bs_blocks = (B + L.bs_threads / 8 - 1) / (L.bs_threads / 8);
    L.board_const.assign(B, 0);
    if (p->board_pose_constant) for (int i = 0; i < B; ++i) L.board_const[i] = p->board_pose_constant[b0 + L.board_perm[i]] ? 1 : 0;
    return 0;
}

}  // namespace tscm

#endif  // TSCM_LAYOUT_H
