// tscm_kernels.h -- device-side data layout and HIP kernels of the TSCM LM solver (gfx950).
//
// HBM layout (all fp64, device-resident for the whole solve):
//   obs_u/obs_v      SoA corner observations, re-packed so the views of one camera are
//                    contiguous and sorted by board: a wave streams them with unit stride.
//   rec[2]           per-view Schur pieces written by the Gram kernel, two regions in one allocation:
//                      W region [V][84]  E^T [F | r]   COLUMN-major: 14 columns (F order, column 13 = E^T r) x 6 rows
//                      E region [V][18]  E^T E_wb      3 columns (the w_b columns) x 6 rows: rows 0-2 w_b x w_b,
//                                                      rows 3-5 t_b x w_b
//                      G region [V][6]   E^T r         column 13 of W once more, compact (board statistics)
//                    The t_b x t_b block of E^T E is not stored: it is (E_tb^T F_tc) R_c, three FMAs per entry from
//                    the t_c columns of W and the camera rotation the view was evaluated with (tb_tb; cconst is
//                    double-buffered like the records for that reason).
//                    views in board-major slot order; the Schur-complement and back-substitution kernels stream
//                    the W region, the e-block factorisation and the board statistics read the E region and two
//                    pieces of W.  double buffered: index ctrl->cur = system at x, cur^1 = candidate.
//   H_stage          per camera a 16x16 tile [F | r]^T [F | r]  (13x13 Gram, col 13 =
//                    F^T r, [13][13] = r^T r) + 8 scalars + one gradient-max slot per rank; fixed address so that the
//                    exchange back-end can all-reduce it without knowing the device-side buffer index.
//   fac[B][56]       per-board e-block factor (k_schur_gram; k_schur_factor for boards seen by > 3 cameras): multipliers L_ik / L_ii and
//                    s_i / L_ii, L itself for the back-substitution, 1 / L_ii, z = L^-1 S_b E^T r, the damping D^2.
//                    Y = L^-1 S_b W is never stored: k_schur_gram / k_backsub_prep re-derive it from W (21 FMAs a column).
//   T[n_bids][256]   Schur complement sum_b Y_b^T Y_b, one 16x16 tile per camera pair that shares a board.
// The LM control state (trust-region radius, accept/reject, termination, iteration log)
// lives in `Ctrl` in device memory; every kernel starts with `if (ctrl->done) return`.
#pragma once

#include "tscm_math.h"
#include "tscm_fastmath.h"
#include "tscm_nd_plan.h"
#include "tscm_layout.h"
#include "tscm_exec_plan.h"
#include "tscm_columns.h"
#include "tscm_ctrl.h"
#include "tscm_spec.h"

namespace tscm {
// one header per stage of an LM iteration, in the order the non-template kernels are defined (= their order in the code object)
#include "tscm_dev.h"
#include "tscm_probe.h"
#include "tscm_prep.h"
#include "tscm_geometry.h"
#include "tscm_eval_gram16.h"
#include "tscm_eval_f32.h"
#include "tscm_eval_gram4.h"
#include "tscm_reduce.h"
#include "tscm_schur.h"
#include "tscm_backsub.h"
// the reduced camera system (DenseSchurComplementSolver): k_solve_nd up to kMaxCamLds cameras, k_solve_reduced up to
// four (one dense block), k_solve_reduced_big for larger rigs
#include "tscm_solve_nd.h"
#include "tscm_solve_dense4.h"
#include "tscm_solve_big.h"
#include "tscm_begin_end.h"
#include "tscm_ops.h"

}  // namespace tscm
