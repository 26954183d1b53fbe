// tscm_ops.h -- operator-level kernels, not part of an LM iteration: Ceres-layout residual / Jacobian, reprojection error,
// project and unproject.
#pragma once
// (included from tscm_kernels.h inside namespace tscm)

// ---------------------------------------------------------------------------------------------
// operator-level kernels (not on the LM hot path)
// ---------------------------------------------------------------------------------------------
// one thread per corner: residual + Jacobian in Ceres' block layout. corner order = device order.
__global__ void k_eval_functor(DevProblem P, DevState S, const int *corner_view, double *res,
                               double *Jc, double *Jb, double *Ji)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P.N) return;
    const int view = corner_view[k];
    const int j = k - P.view_obs[view];
    ViewConst vc;
    load_view_const(P, S, 0, P.view_cam[view], P.view_board[view], vc);
    double r[2], JE[2][kE], JF[2][kFA];
    corner_residual_jacobian(vc, P.board_xy[2 * j], P.board_xy[2 * j + 1], P.obs_u[k], P.obs_v[k], r, JE, JF);
    res[2 * k] = r[0]; res[2 * k + 1] = r[1];
    for (int row = 0; row < 2; ++row) {
        if (Jc) for (int i = 0; i < 6; ++i) Jc[12 * (size_t)k + 6 * row + i] = JF[row][i];
        if (Jb) for (int i = 0; i < 6; ++i) Jb[12 * (size_t)k + 6 * row + i] = JE[row][i];
        if (Ji) { for (int i = 0; i < 7; ++i) Ji[18 * (size_t)k + 9 * row + i] = JF[row][6 + i]; Ji[18 * (size_t)k + 9 * row + 7] = 0.0; Ji[18 * (size_t)k + 9 * row + 8] = 0.0; }
    }
}

// multi_calib.cpp:233-283: per-view sums of Euclidean pixel error and squared error, with
// cv::Rodrigues matrices and the skew projection.  one wave per view.
// WEIGHTED (a solve with corner weights and a loss: summary.rmse): both sums carry the corner's weight P.obs_w.
template <bool WEIGHTED = false>
__global__ __launch_bounds__(64) void k_reproj_error(DevProblem P, const double *cam_rt, const double *intr,
                                                    const double *board_rt, double *view_err, double *view_sq)
{
    const int view = blockIdx.x, lane = threadIdx.x;
    const int cam = P.view_cam[view], board = P.view_board[view];
    double Rb[9], Rc[9], dummy[27], I[9];
    // cv::Rodrigues == exact Rodrigues; below DBL_EPSILON the I + [w]x branch differs by O(theta^2) ~ 1e-32
    rotation_and_derivatives(board_rt + 6 * board, Rb, dummy);
    rotation_and_derivatives(cam_rt + 6 * cam, Rc, dummy);
    for (int i = 0; i < 9; ++i) I[i] = intr[9 * cam + i];
    const double *tb = board_rt + 6 * board + 3, *tc = cam_rt + 6 * cam + 3;
    double e = 0.0, sq = 0.0;
    for (int j = lane; j < P.view_count[view]; j += 64) {
        const double x = P.board_xy[2 * j], y = P.board_xy[2 * j + 1];
        double q[3], Pc[3];
        for (int i = 0; i < 3; ++i) q[i] = Rb[3 * i] * x + Rb[3 * i + 1] * y + tb[i];
        for (int i = 0; i < 3; ++i) Pc[i] = Rc[3 * i] * q[0] + Rc[3 * i + 1] * q[1] + Rc[3 * i + 2] * q[2] + tc[i];
        double u, v;
        project_point(I, Pc[0], Pc[1], Pc[2], u, v);
        const double du = P.obs_u[P.view_obs[view] + j] - u, dv = P.obs_v[P.view_obs[view] + j] - v;
        if constexpr (WEIGHTED) { const double om = P.obs_w[P.view_obs[view] + j]; e += om * sqrt(du * du + dv * dv); sq += om * (du * du + dv * dv); }
        else { e += sqrt(du * du + dv * dv); sq += du * du + dv * dv; }
    }
    for (int s = 32; s > 0; s >>= 1) { e += __shfl_xor(e, s); sq += __shfl_xor(sq, s); }
    if (lane == 0) { view_err[view] = e; view_sq[view] = sq; }
}

__global__ void k_project(const double *intr, const double *pts, int n, double *uv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double I[9];
    for (int k = 0; k < 9; ++k) I[k] = intr[k];
    project_point(I, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], uv[2 * i], uv[2 * i + 1]);
}

__global__ void k_unproject(const double *intr, const double *uv, int n, double *rays)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double I[9], r[3];
    for (int k = 0; k < 9; ++k) I[k] = intr[k];
    unproject_pixel(I, uv[2 * i], uv[2 * i + 1], r);
    rays[3 * i] = r[0]; rays[3 * i + 1] = r[1]; rays[3 * i + 2] = r[2];
}
