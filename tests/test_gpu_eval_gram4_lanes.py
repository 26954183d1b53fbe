"""Lane roles of k_eval_gram4's epilogue, view loop and prefetch, bit for bit.

The epilogue picks every stored value by the lane's block and row with masked DPP moves and takes ONE t_b row evaluation for
the three sums T0 / T1 / T2; the view loop prefetches the next view's observations with all 64 lanes, skips the zeroing of lost
corners on a scalar compare and counts its priority level up.  None of this may change a bit of a record or of the camera tile.
The partner is k_eval_gram<..> on the 16x16 tile (TSCM_EXEC_GRAM_16X16), which shares none of that code: a few forced iterations
on both must give the same cost trace, parameters and per-camera errors.

A rig of up to one view per resident wave (every small rig) puts ONE view into each chunk; the chunked cases need more views
than that, so they use tiny boards or few iterations.  The host plans one chunk per resident wave, at most 16 waves per compute
unit (plan_layout), so V views make chunks of at least V / (16 CUs) views: the chunked cases assert their size against the
device's own CU count.

The ROBUST instantiation has no such partner (a loss with TSCM_EXEC_GRAM_16X16 is refused: tests/test_gpu_robust.py::test_refusals).
Its bit-level case runs the SAME kernel fused and on separate launches: it guards the hand-over to the riding reductions and
cannot see an error inside the ROBUST epilogue.  What checks that epilogue's values is the comparison with tests/robust_ref.py at the tolerance
of tests/test_gpu_robust.py::test_normal_equations (1e-11 of a block, 1e-12 of the cost).
"""
import functools

import numpy as np
import pytest

from tscm_calib_amd import api, lib, synth
from tests import helpers as H
from tests import robust_ref as R
from tests.test_gpu_gram_kernels import g4_plan, n_cus, ragged  # noqa: F401  (n_cus: fixture)

pytestmark = pytest.mark.gpu

FORCED = dict(function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0, min_trust_region_radius=0.0)
ALL_SEPARATE = lib.EXEC_SEPARATE_T_REDUCE | lib.EXEC_SEPARATE_BACKSUB | lib.EXEC_SEPARATE_CONTROL | lib.EXEC_SEPARATE_STATS

# corners -> board, and the pass plan (passes, KS) the case is there for
BOARDS = {4: (2, 2), 30: (6, 5), 49: (7, 7), 54: (9, 6), 56: (8, 7), 57: (19, 3), 88: (11, 8)}
PLANS = {4: (1, 1), 30: (1, 8), 49: (1, 13), 54: (1, 14), 56: (1, 14), 57: (2, 8), 88: (2, 11)}


def _trace(s):
    return [(it["cost"], it["trust_region_radius"], it["step_is_successful"]) for it in s["iterations"]]


def _same_bits(p, iters, flags_b=lib.EXEC_GRAM_16X16, loss=None):
    """Solves p with exec_flags = 0 and with flags_b; everything the solve returns must be the same bits."""
    a, b = p.copy().normalised(), p.copy().normalised()
    out = []
    for q, flags in ((a, 0), (b, flags_b)):
        with api.Solver(q) as s:
            if loss is not None:
                s.set_loss(*loss)
            out.append(s.solve(max_num_iterations=iters, exec_flags=flags, **FORCED))
    sa, sb = out
    # every forced iteration ran (the summary counts the initial evaluation as iteration 0, as ceres::Solver::Summary does)
    assert sa["num_iterations"] == sb["num_iterations"] == iters + 1, (sa["message"], sb["message"])
    assert len(sa["iterations"]) == len(sb["iterations"]) == iters + 1
    assert _trace(sa) == _trace(sb)
    assert np.array_equal(a.intr, b.intr) and np.array_equal(a.cam_rt, b.cam_rt) and np.array_equal(a.board_rt, b.board_rt)
    ea, eb = api.reprojection_error(a), api.reprojection_error(b)
    assert np.array_equal(np.asarray(ea[0]), np.asarray(eb[0])) and ea[1:] == eb[1:]
    # the iterations moved: the comparison is not one of two untouched starting points
    assert not np.array_equal(a.intr, p.copy().normalised().intr)
    return sa


@functools.lru_cache(maxsize=None)
def _ragged_rig(n, views_per_cam, seed):
    """Built once per shape and shared (every user works on a copy)."""
    cols, rows = BOARDS[n]
    return ragged(synth.make_problem(4, views_per_cam, seed, cols=cols, rows=rows, pitch=360.0 / max(cols, rows)), n, g4_plan(n)[1])


def test_boards_are_the_plans_they_stand_for():
    for n, (cols, rows) in BOARDS.items():
        assert cols * rows == n
        passes, per, ks = g4_plan(n)
        assert (passes, ks) == PLANS[n], (n, passes, per, ks)


@pytest.mark.parametrize("cams,frames", [(2, 6), (4, 8)])
@pytest.mark.parametrize("n", sorted(BOARDS))
def test_small_rigs_on_every_pass_plan(hip_device, n, cams, frames):
    """One view per chunk: the head, one trip through the view loop, the epilogue, the camera tile."""
    cols, rows = BOARDS[n]
    p = synth.make_problem(cams, frames, 900 + n + cams, cols=cols, rows=rows, pitch=360.0 / max(cols, rows))
    _same_bits(p, 4)


@pytest.mark.parametrize("n,views_per_cam", [(54, 2200), (88, 1100)])
def test_corner_counts_that_change_inside_a_chunk(hip_device, n_cus, n, views_per_cam):
    """More views than the chip holds waves, so a chunk holds at least two, and corner counts that step through short, full,
    empty and pass-boundary views (tests/test_gpu_gram_kernels.py: ragged): lanes lose and regain their corner from view to
    view, the zeroing runs behind every longer view and is skipped behind every shorter one, and the 64-lane prefetch reads
    into the view behind a short one."""
    q = _ragged_rig(n, views_per_cam, 940 + n)
    assert q.n_views > 16 * n_cus, (q.n_views, n_cus)           # ceil(V / chunks) >= 2 with at most 16 n_cus chunks
    assert len(set(q.view_count.tolist())) > 5
    _same_bits(q, 2)


def test_more_than_64_views_in_a_wave(hip_device, n_cus):
    """280 k views of a 2 x 2 board: more than 64 views per chunk, so the metadata of a chunk comes in several blocks (the
    vbase loop), the priority counter runs over the whole chunk and the last view of a block prefetches across the block."""
    p = synth.make_problem(4, 70000, 977, cols=2, rows=2, pitch=120.0)
    assert p.n_views == 280000 and p.n_views > 64 * 16 * n_cus, (p.n_views, n_cus)
    _same_bits(p, 2)


def test_robust_instantiation_fused_and_on_separate_launches(hip_device, n_cus):
    """k_eval_gram4<14, false, true> with ragged views in multi-view chunks: same bits whether the reductions ride in the
    neighbouring launches or not (the riding reductions read this kernel's camera tiles and records).  The same kernel on both
    sides: not a check of its epilogue's values (that is the next test)."""
    assert 4 * 2200 > 16 * n_cus
    _same_bits(_ragged_rig(54, 2200, 940 + 54), 2, flags_b=ALL_SEPARATE, loss=("huber", 1.0))


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_robust_instantiation_against_the_reference(hip_device, kind):
    """... and its corrected normal equations against tests/robust_ref.py, at the tolerance of test_gpu_robust.py."""
    p = _ragged_rig(54, 1100, 992)
    a = R.median_scale(p)
    o = R.robust_normal_equations(p, kind, a)
    g = api.normal_equations(p, hip_device, loss=(kind, a))
    assert abs(g["cost"] - o["cost"]) <= 1e-12 * o["cost"], (g["cost"], o["cost"])
    e = H.block_errors(g, o, bool(p.mono))
    assert max(e.values()) <= 1e-11, e
