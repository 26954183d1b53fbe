// tscm_mono_batch.h -- the batched mono refinement on the device (tscm_solve_mono_batch): K independent mono
// LM solves advanced together, one launch per stage for the whole batch.
//
// A separate route: none of the single-problem kernels is touched.  Per iteration four plain launches, nothing handed over
// inside a launch:
//   k_mb_schur    one workgroup per chunk of slots (tscm_batch_plan.h): each active board's E^T E + D^2 factored, its
//                 Schur-complement term W^T (E^T E + D^2)^-1 [W | g] summed over the chunk's slots in order
//   k_mb_solve    one workgroup per chunk: the problem's reduced system (<= 7 free intrinsic columns) from its chunks'
//                 partials in chunk order -- every workgroup of a problem forms and solves the same system, the same bits
//                 -- then the back-substitution of the chunk's boards and the candidate
//   k_mb_eval     one workgroup per chunk: residuals and Jacobians of the candidate's corners, the view records and the
//                 chunk's camera-side partials
//   k_mb_control  one workgroup per problem: the partials in chunk order, then the trust-region step (lm_step,
//                 tscm_ctrl.h) on the problem's own control block
// Every kernel of a problem whose control block says done returns at once: a terminated problem is frozen.  All problem
// state is double-buffered like the single-problem route's (cur / cur ^ 1 per problem: a candidate goes into buffer
// cur ^ 1 and becomes current on acceptance).
#ifndef TSCM_MONO_BATCH_H
#define TSCM_MONO_BATCH_H

#include "tscm_batch_plan.h"

namespace tscm {

constexpr int kMbThreads = 128;     // k_mb_schur / k_mb_solve / k_mb_eval
constexpr int kMbRec = 84;          // per slot: E^T E (6x6), E^T F (6x7 row-major), E^T r (6) -- unscaled
constexpr int kMbPart = 64;         // per chunk: F^T F (7x7), F^T r (7), sum rho, board |d|_inf, |d|^2, |x|^2
constexpr int kMbTot = 56;          // per problem: F^T F (7x7), F^T r (7) at a point
constexpr int kMbSp = 64;           // per chunk: Schur terms (7x7), rhs terms (7), failure
constexpr int kMbOuts = 105;        // outputs of one view's Gram: 21 E^T E, 42 E^T F, 6 E^T r, 28 F^T F, 7 F^T r, 1 sum rho
constexpr int kMbJw = 14;           // LDS columns of a Jacobian row: E (6), F (7), r

struct MbDev {
    int K, n_points, n_chunks, n_slots;
    const double *board_xy, *obs_u, *obs_v;
    const double *obs_w;                    // corner weights in the order of obs_u / obs_v, NULL = none
    const int4 *chunk;                     // [n_chunks] problem, first slot, end slot
    const int *chunk_ptr, *board_ptr;       // [K + 1]
    const int *slot_board, *slot_obs, *slot_count;
    const unsigned char *slot_active;
    const unsigned short *mask;             // [K]
    double *intr[2], *board[2];             // parameters: [K * 9], [B * 6]
    double *rec[2], *part[2], *tot[2];      // [n_slots * kMbRec], [n_chunks * kMbPart], [K * kMbTot]
    double *schur, *solvep, *cam_mp;        // [n_chunks * kMbSp], [n_chunks * 4], [K * 4]
    double *s_b, *s_f;                      // Jacobi scaling: [n_slots * 6], [K * 7]
    CtrlHead *head;                         // [K]
    IterLog *log;                           // [K * kMaxLog]
    int *n_done;
    double *out;                            // [K * 9 + B * 6]: the accepted point (k_mb_finish)
    LossArg loss;
};

// packed lower index p of an n x n symmetric matrix -> (i, j), j <= i
__device__ __forceinline__ void mb_unpack(int p, int &i, int &j) { i = 0; while ((i + 1) * (i + 2) / 2 <= p) ++i; j = p - i * (i + 1) / 2; }
// output t of a view's Gram -> its two Jacobian columns (E 0-5, F 6-12, r 13); t = 104 is the sum of rho
__device__ __forceinline__ void mb_out_cols(int t, int &a, int &b)
{
    if (t < 21) { mb_unpack(t, a, b); return; }
    if (t < 63) { a = (t - 21) / 7; b = 6 + (t - 21) % 7; return; }
    if (t < 69) { a = t - 63; b = 13; return; }
    if (t < 97) { mb_unpack(t - 69, a, b); a += 6; b += 6; return; }
    a = 6 + (t - 97); b = 13;
}

// in-place Cholesky of a packed lower n x n matrix (n <= 7); false if it is not positive definite
template <int N>
__device__ __forceinline__ bool mb_chol(double (&a)[N * (N + 1) / 2])
{
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = a[j * (j + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= a[j * (j + 1) / 2 + k] * a[j * (j + 1) / 2 + k];
        if (!(d > 0.0)) return false;
        const double l = sqrt(d);
        a[j * (j + 1) / 2 + j] = l;
        const double il = 1.0 / l;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double s = a[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= a[i * (i + 1) / 2 + k] * a[j * (j + 1) / 2 + k];
            a[i * (i + 1) / 2 + j] = s * il;
        }
    }
    return true;
}
// L L^T x = b in place
template <int N>
__device__ __forceinline__ void mb_chol_solve(const double (&a)[N * (N + 1) / 2], double (&x)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= a[i * (i + 1) / 2 + k] * x[k];
        x[i] = s / a[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) s -= a[k * (k + 1) / 2 + i] * x[k];
        x[i] = s / a[i * (i + 1) / 2 + i];
    }
}

// E^T E + D^2 of an active slot, scaled, factored: D^2 = clamp(diag, dmin, dmax) / radius as Ceres' LM strategy forms it
__device__ __forceinline__ bool mb_board_factor(const double *rec, const double *sb, double radius, double dmin, double dmax, double (&a)[21])
{
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) a[i * (i + 1) / 2 + j] = sb[i] * rec[6 * i + j] * sb[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double D = sqrt(fmin(fmax(a[i * (i + 1) / 2 + i], dmin), dmax) / radius);
        a[i * (i + 1) / 2 + i] += D * D;
    }
    return mb_chol<6>(a);
}

__device__ __forceinline__ bool mb_frozen(const MbDev &D, int k) { return D.head[k].done != 0; }

// ---------------------------------------------------------------------------------------------
// the control blocks of a batch solve and the arrival count of terminated problems
__global__ __launch_bounds__(256) void k_mb_begin(MbDev D, CtrlHead head)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < D.K) { head.inert_cols = inert_free(D.mask[k]) ? 1 : 0; D.head[k] = head; }      // (every problem here has views)
    if (k == 0) *D.n_done = 0;
}

// Evaluation of the point in buffer cur (init) or of the candidate in cur ^ 1: per slot the Jacobian rows of its corners
// into LDS (one thread per corner), then one thread per Gram output summing over the rows in order.  Robust loss: rows and
// residuals scaled by sqrt(rho') (Ceres' Corrector, alpha = 0 for all three losses: robust_rho).
__global__ __launch_bounds__(kMbThreads) void k_mb_eval(MbDev D, int init)
{
    extern __shared__ double mb_lds[];
    double *J = mb_lds;                                 // [n_points][2][kMbJw]
    double *rho = mb_lds + 2 * kMbJw * D.n_points;      // [n_points]
    __shared__ double outv[kMbOuts];
    __shared__ double gst[3][6];                        // per board parameter of the slot: |d|, d^2, x^2
    const int4 ch = D.chunk[blockIdx.x];
    const int k = ch.x;
    if (mb_frozen(D, k)) return;
    const int t = threadIdx.x;
    const int buf = init ? D.head[k].cur : D.head[k].cur ^ 1;
    const double *I = D.intr[buf] + 9 * k;
    ViewConst vc;
    mono_view_const(I, vc);
    const bool robust = D.loss.kind != kLossNone;
    int oa = 0, ob = 0;
    if (t < kMbOuts - 1) mb_out_cols(t, oa, ob);
    double acc = 0.0;                                   // outputs 69..104: summed over the chunk's slots in order
    double gmax = 0.0, gsq = 0.0, xsq = 0.0;            // thread 0: the chunk's board-side norms
    for (int s = ch.y; s < ch.z; ++s) {
        const double *rt = D.board[buf] + 6 * (size_t)D.slot_board[s];
        double bc[kBoardConst];                         // (in line, not a helper shared with the host: behind a call the
        board_constants(rt, bc);                        // compiler pairs the Jacobian's products differently and bits move)
        for (int q = 0; q < 3; ++q) { vc.r1[q] = bc[q]; vc.r2[q] = bc[3 + q]; vc.tb[q] = rt[3 + q]; }
        for (int kk = 0; kk < 3; ++kk) for (int q = 0; q < 6; ++q) vc.db[kk][q] = bc[6 + 6 * kk + q];
        const int n = D.slot_count[s], o0 = D.slot_obs[s];
        for (int j = t; j < n; j += kMbThreads) {
            double r[2], JE[2][kE], JF[2][kFA];
            corner_residual_jacobian(vc, D.board_xy[2 * j], D.board_xy[2 * j + 1], D.obs_u[o0 + j], D.obs_v[o0 + j], r, JE, JF);
            const double sq = r[0] * r[0] + r[1] * r[1];
            double w = 1.0, rh = sq;
            // (corner weights: rho = omega rho(s), w = sqrt(omega rho'); a problem of the batch without weights has omega = 1)
            if (D.obs_w) robust_rho<true>(D.loss, sq, rh, w, D.obs_w[o0 + j]);
            else if (robust) robust_rho(D.loss, sq, rh, w);
            rho[j] = rh;
            for (int row = 0; row < 2; ++row) {
                double *Jr = J + (2 * j + row) * kMbJw;
                for (int q = 0; q < 6; ++q) Jr[q] = w * JE[row][q];
                for (int q = 0; q < 7; ++q) Jr[6 + q] = w * JF[row][6 + q];
                Jr[13] = w * r[row];
            }
        }
        __syncthreads();
        if (t < kMbOuts) {
            double v = 0.0;
            if (t == kMbOuts - 1) { for (int j = 0; j < n; ++j) v += rho[j]; }
            else { for (int i = 0; i < 2 * n; ++i) v += J[i * kMbJw + oa] * J[i * kMbJw + ob]; }
            outv[t] = v;
            if (t >= 69) acc += v;
        }
        __syncthreads();
        double *rec = D.rec[buf] + (size_t)kMbRec * s;
        if (t < 21) { rec[6 * oa + ob] = outv[t]; rec[6 * ob + oa] = outv[t]; }
        else if (t < 63) rec[36 + 7 * oa + (ob - 6)] = outv[t];
        else if (t < 69) rec[78 + oa] = outv[t];
        if (t < 6) {
            const double uii = outv[t * (t + 1) / 2 + t];
            if (init) D.s_b[6 * (size_t)s + t] = D.head[k].opt.jacobi_scaling ? 1.0 / (1.0 + sqrt(uii)) : 1.0;
            const bool act = D.slot_active[s] != 0;
            const double x = rt[t], g = outv[63 + t];
            const double d = x - (x + (-g));
            gst[0][t] = act ? fabs(d) : 0.0; gst[1][t] = act ? d * d : 0.0; gst[2][t] = act ? x * x : 0.0;
        }
        __syncthreads();
        if (t == 0) for (int q = 0; q < 6; ++q) { gmax = fmax(gmax, gst[0][q]); gsq += gst[1][q]; xsq += gst[2][q]; }
    }
    double *part = D.part[buf] + (size_t)kMbPart * blockIdx.x;
    if (t >= 69 && t < 97) { part[7 * (oa - 6) + (ob - 6)] = acc; part[7 * (ob - 6) + (oa - 6)] = acc; }
    else if (t >= 97 && t < 104) part[49 + (oa - 6)] = acc;
    else if (t == 104) part[56] = acc;
    if (t == 0) { part[57] = gmax; part[58] = gsq; part[59] = xsq; }
}

// the chunk's Schur-complement terms at the current point and radius
__global__ __launch_bounds__(kMbThreads) void k_mb_schur(MbDev D)
{
    __shared__ double Ws[kMbMaxChunkSlots][6][8];       // scaled [E^T F | E^T r]
    __shared__ double Y[kMbMaxChunkSlots][6][8];        // (E^T E + D^2)^-1 Ws
    __shared__ int bad;
    const int4 ch = D.chunk[blockIdx.x];
    const int k = ch.x;
    if (mb_frozen(D, k)) return;
    const int t = threadIdx.x, ns = ch.z - ch.y;
    const CtrlHead &h = D.head[k];
    const int cur = h.cur;
    if (t == 0) bad = 0;
    __syncthreads();
    if (t < ns) {
        const int s = ch.y + t;
        const double *rec = D.rec[cur] + (size_t)kMbRec * s;
        const double *sb = D.s_b + 6 * (size_t)s, *sf = D.s_f + 7 * k;
        const unsigned fm = ~(unsigned)D.mask[k];
        double a[21];
        const bool act = D.slot_active[s] != 0;
        const bool ok = !act || mb_board_factor(rec, sb, h.radius, h.opt.min_lm_diagonal, h.opt.max_lm_diagonal, a);
        if (!ok) atomicOr(&bad, 1);
        for (int i = 0; i < 6; ++i) {
            for (int l = 0; l < 7; ++l) Ws[t][i][l] = (act && ((fm >> l) & 1u)) ? sb[i] * rec[36 + 7 * i + l] * sf[l] : 0.0;
            Ws[t][i][7] = act ? sb[i] * rec[78 + i] : 0.0;
        }
        for (int c = 0; c < 8; ++c) {
            double y[6];
            for (int i = 0; i < 6; ++i) y[i] = Ws[t][i][c];
            if (act && ok) mb_chol_solve<6>(a, y);
            for (int i = 0; i < 6; ++i) Y[t][i][c] = (act && ok) ? y[i] : 0.0;
        }
    }
    __syncthreads();
    double *sp = D.schur + (size_t)kMbSp * blockIdx.x;
    if (t < 56) {
        const int l = t < 49 ? t / 7 : t - 49, m = t < 49 ? t % 7 : 7;
        double v = 0.0;
        for (int q = 0; q < ns; ++q)
            for (int i = 0; i < 6; ++i) v += Ws[q][i][l] * Y[q][i][m];
        sp[t] = v;
    }
    if (t == 56) sp[56] = bad ? 1.0 : 0.0;
}

// the problem's reduced system and camera step (every workgroup of the problem the same), the back-substitution of the
// chunk's boards and the candidate in buffer cur ^ 1; the first chunk of a problem writes the candidate intrinsics
__global__ __launch_bounds__(kMbThreads) void k_mb_solve(MbDev D)
{
    __shared__ double red[57];
    __shared__ double hf[7];
    __shared__ int fail;
    __shared__ double mb[kMbMaxChunkSlots][2];
    const int4 ch = D.chunk[blockIdx.x];
    const int k = ch.x;
    if (mb_frozen(D, k)) return;
    const int t = threadIdx.x, ns = ch.z - ch.y;
    const CtrlHead &h = D.head[k];
    const int cur = h.cur, nxt = cur ^ 1;
    const double radius = h.radius, dmin = h.opt.min_lm_diagonal, dmax = h.opt.max_lm_diagonal;
    const int c0 = D.chunk_ptr[k], c1 = D.chunk_ptr[k + 1];
    if (t < 57) {
        double v = 0.0;
        for (int c = c0; c < c1; ++c) { const double x = D.schur[(size_t)kMbSp * c + t]; v = t < 56 ? v + x : fmax(v, x); }
        red[t] = v;
    }
    __syncthreads();
    const double *tot = D.tot[cur] + kMbTot * k, *sf = D.s_f + 7 * k;
    const unsigned fm = ~(unsigned)D.mask[k];
    if (t == 0) {
        double a[28], z[7];
        for (int l = 0; l < 7; ++l) {
            const bool fl = (fm >> l) & 1u;
            for (int m = 0; m <= l; ++m) {
                const bool fr = (fm >> m) & 1u;
                a[l * (l + 1) / 2 + m] = (fl && fr) ? sf[l] * tot[7 * l + m] * sf[m] : 0.0;
            }
            if (fl) {
                double &d = a[l * (l + 1) / 2 + l];
                const double Dl = sqrt(fmin(fmax(d, dmin), dmax) / radius);
                d += Dl * Dl;
            } else {
                a[l * (l + 1) / 2 + l] = 1.0;       // a held intrinsic: an identity row, no right-hand side
            }
            z[l] = fl ? sf[l] * tot[49 + l] - red[49 + l] : 0.0;
        }
        for (int l = 0; l < 7; ++l)
            for (int m = 0; m <= l; ++m)
                if (((fm >> l) & 1u) && ((fm >> m) & 1u)) a[l * (l + 1) / 2 + m] -= red[7 * l + m];
        const bool ok = red[56] == 0.0 && mb_chol<7>(a);
        if (ok) mb_chol_solve<7>(a, z);
        for (int l = 0; l < 7; ++l) hf[l] = (ok && ((fm >> l) & 1u)) ? -z[l] : 0.0;
        fail = ok ? 0 : 1;
    }
    __syncthreads();
    if (t < ns) {
        const int s = ch.y + t;
        double m_b = 0.0, sq_b = 0.0;
        if (D.slot_active[s] && !fail) {
            const double *rec = D.rec[cur] + (size_t)kMbRec * s;
            const double *sb = D.s_b + 6 * (size_t)s;
            double a[21], y[6], ws[6][7], g[6];
            const bool ok = mb_board_factor(rec, sb, radius, dmin, dmax, a);
            for (int i = 0; i < 6; ++i) {
                for (int l = 0; l < 7; ++l) ws[i][l] = ((fm >> l) & 1u) ? sb[i] * rec[36 + 7 * i + l] * sf[l] : 0.0;
                g[i] = sb[i] * rec[78 + i];
                double r = g[i];
                for (int l = 0; l < 7; ++l) r -= ws[i][l] * (-hf[l]);
                y[i] = r;
            }
            if (ok) mb_chol_solve<6>(a, y);
            double *xb = D.board[cur] + 6 * (size_t)D.slot_board[s], *cb = D.board[nxt] + 6 * (size_t)D.slot_board[s];
            double hb[6];
            for (int i = 0; i < 6; ++i) hb[i] = -y[i];
            // model: h_b . g_b + 1/2 h_b^T U h_b + h_b^T W h_f  (scaled), the board part of -(J h)^T (r + J h / 2)
            for (int i = 0; i < 6; ++i) {
                double uh = 0.0, wh = 0.0;
                for (int j = 0; j < 6; ++j) uh += sb[i] * rec[6 * i + j] * sb[j] * hb[j];
                for (int l = 0; l < 7; ++l) wh += ws[i][l] * hf[l];
                m_b += hb[i] * g[i] + 0.5 * hb[i] * uh + hb[i] * wh;
                const double dlt = hb[i] * sb[i];
                cb[i] = xb[i] + dlt;
                sq_b += dlt * dlt;
            }
            if (!ok) m_b = __builtin_nan("");
        }
        mb[t][0] = m_b; mb[t][1] = sq_b;
    }
    __syncthreads();
    if (t == 0) {
        double m = 0.0, q = 0.0;
        for (int i = 0; i < ns; ++i) { m += mb[i][0]; q += mb[i][1]; }
        double *sp = D.solvep + 4 * (size_t)blockIdx.x;
        sp[0] = m; sp[1] = q;
        if (blockIdx.x == (unsigned)c0) {
            const double *xi = D.intr[cur] + 9 * k;
            double *ci = D.intr[nxt] + 9 * k;
            double m_f = 0.0, sq_f = 0.0;
            for (int l = 0; l < 7; ++l) {
                double ah = 0.0;
                for (int j = 0; j < 7; ++j) ah += (((fm >> l) & (fm >> j) & 1u) ? sf[l] * tot[7 * l + j] * sf[j] : 0.0) * hf[j];
                m_f += hf[l] * (((fm >> l) & 1u) ? sf[l] * tot[49 + l] : 0.0) + 0.5 * hf[l] * ah;
                const double dlt = hf[l] * sf[l];
                ci[l] = ((fm >> l) & 1u) ? xi[l] + dlt : xi[l];
                sq_f += ((fm >> l) & 1u) ? dlt * dlt : 0.0;
            }
            ci[7] = xi[7]; ci[8] = xi[8];
            double *cm = D.cam_mp + 4 * k;
            cm[0] = m_f; cm[1] = sq_f; cm[2] = fail ? 1.0 : 0.0;
        }
    }
}

// The problem's evaluation partials in chunk order, then the trust-region step (lm_step, tscm_ctrl.h) on this problem's
// control block, its log and its camera-side norms.
__global__ __launch_bounds__(64) void k_mb_control(MbDev D, int init)
{
    __shared__ double sv[64];
    const int k = blockIdx.x, t = threadIdx.x;
    if (mb_frozen(D, k)) return;
    const int c0 = D.chunk_ptr[k], c1 = D.chunk_ptr[k + 1];
    const int cur0 = D.head[k].cur, buf = init ? cur0 : cur0 ^ 1;
    if (t < 60) {
        double v = 0.0;
        for (int c = c0; c < c1; ++c) { const double x = D.part[buf][(size_t)kMbPart * c + t]; v = t == 57 ? fmax(v, x) : v + x; }
        sv[t] = v;
    }
    if (t == 60 || t == 61) {
        double v = 0.0;
        if (!init) for (int c = c0; c < c1; ++c) v += D.solvep[4 * (size_t)c + (t - 60)];
        sv[t] = v;
    }
    __syncthreads();
    if (t < kMbTot) D.tot[buf][kMbTot * k + t] = sv[t];
    if (t != 0) return;

    CtrlHead c = D.head[k];
    const Options &o = c.opt;
    const unsigned mask = D.mask[k], fm = ~mask;
    const bool block_const = (mask & TSCM_FIX_INTRINSICS) == TSCM_FIX_INTRINSICS;
    const double *I = D.intr[buf] + 9 * k;
    double gmax_c = 0.0, gsq_c = 0.0, xsq_c = 0.0;
    for (int l = 0; l < 7; ++l) {
        if ((fm >> l) & 1u) {
            const double x = I[l], g = sv[49 + l];
            const double d = x - (x + (-g));
            gmax_c = fmax(gmax_c, fabs(d)); gsq_c += d * d;
        }
        if (init) D.s_f[7 * k + l] = ((fm >> l) & 1u) && o.jacobi_scaling ? 1.0 / (1.0 + sqrt(sv[8 * l])) : 1.0;
    }
    if (!block_const) for (int l = 0; l < 9; ++l) xsq_c += I[l] * I[l];
    const double cost = 0.5 * sv[56];
    const double gmax_t = fmax(gmax_c, sv[57]);
    const double gnorm_t = sqrt(gsq_c + sv[58]);
    const double xnorm_t = sqrt(xsq_c + sv[59]);
    const double *cm = D.cam_mp + 4 * k;
    StepInput in = { cost, gmax_t, gnorm_t, xnorm_t, 0.0, 0.0 };
    IterLog it;
    bool logged;
    if (init) logged = lm_step(c, 1, buf, in, it);      // no step yet: cam_mp and solvep are not written
    else {
        c.lin_fail = cm[2] != 0.0 ? 1 : 0;
        // the model cost change of Ceres is -(J h)^T (r + J h / 2); the partials hold its negation
        in.model_cost_change = -(sv[60] + cm[0]);
        in.step_norm = sqrt(sv[61] + cm[1]);
        logged = lm_step(c, 0, buf, in, it);
    }
    if (logged && c.n_log <= kMaxLog) D.log[(size_t)kMaxLog * k + c.n_log - 1] = it;
    D.head[k] = c;
    if (c.done) atomicAdd(D.n_done, 1);
}

// the accepted point of every problem into one output buffer (intrinsics, then the concatenated boards)
__global__ __launch_bounds__(256) void k_mb_finish(MbDev D)
{
    const int k = blockIdx.x, t = threadIdx.x;
    const int cur = D.head[k].cur;
    if (t < 9) D.out[9 * k + t] = D.intr[cur][9 * k + t];
    const size_t b0 = 6 * (size_t)D.board_ptr[k], b1 = 6 * (size_t)D.board_ptr[k + 1];
    double *ob = D.out + 9 * (size_t)D.K;
    for (size_t i = b0 + t; i < b1; i += 256) ob[i] = D.board[cur][i];
}

}  // namespace tscm

#endif
