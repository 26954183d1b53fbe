"""What tests/test_gpu_mono_batch_step.py rests on, without a GPU (oracle, numpy and the host plan header only).

1. Shapes: every case is planned by tscm_batch_plan.h itself (tests/native/batch_plan_check.cpp `plan`, built plain and
   under AddressSanitizer + UBSan), and the chunk shapes its table row claims are read from that plan: more than
   kMbMaxChunks chunks of kMbMaxChunkSlots slots, a chunk below kMbMinChunk, exactly one chunk, a last chunk of one slot,
   ragged slot counts, inactive slots next to active ones and alone, boards outside every slot, kMbMaxPoints corners.
2. References: every case's extended-precision step is `ok`, its relative decrease is on the intended side of
   min_relative_decrease by RD_MARGIN, both LM clamps bind in every problem of the clamp cases, the radius cases are
   damping-dominated and nearly undamped, both branches of Huber's rho occur, and the oracle's trajectories reject and
   mix their decisions as part 2 of the GPU module needs them to.
3. Sensitivity: a candidate from a deliberately wrong reference step must exceed TAU_B by MARGIN (20x, the margin of
   tests/test_step_tolerance.py), measured against the true reference with helpers.step_errors:
     corners >= 128 of each view dropped (the corner loop's second pass), two-pass:          backward error 5.6e-4
     one slot's E^T F left out (Schur term and back-substitution), 19 views:                  0.16
     a constant board eliminated as if it were free, const-boards:                            1.5e-2
     sqrt(rho') applied to the Jacobian but not to the residual, soft_l1 / cauchy / huber:    0.38 / 0.36 / 0.29
   The clean reference candidate measures 2.2e-15 at most on the same problems.
"""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import helpers as H
from tests import native_check as N
from tests import robust_ref as R
from tests import test_gpu_mono_batch_step as M
from tests.test_step_tolerance import MARGIN

pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("batch_plan_check.cpp", "batch_plan_check")


# ----------------------------------------------------------------------------- 1. shapes, from the plan header
def plan_of(ps, checker):
    """tscm_batch_plan.h's plan of a batch: per problem the slots of each chunk and the active flag and corners of each slot."""
    args = []
    for p in ps:
        assert np.array_equal(p.view_board, np.arange(p.n_views))            # the check's view v sees board v
        const = [] if p.board_pose_constant is None else np.nonzero(p.board_pose_constant)[0].tolist()
        args.append(f"{p.n_boards}/{','.join(map(str, p.view_count.tolist()))}/{','.join(map(str, const))}")
    out = N.run(checker, "plan", ps[0].n_points, *args)
    assert out["ok"], out
    return out


def test_every_batch_is_planned(checker):
    for case_id in M.CASES:
        ps = M.problems(case_id)
        out = plan_of(ps, checker)
        assert 2 <= len(ps) <= 5 and all(x["device"] for x in out["problems"]), case_id
        assert ps[0].n_points <= out["max_points"]
    for batch in M.trajectory_batches():
        assert all(x["device"] for x in plan_of(batch, checker)["problems"])


def test_chunk_shapes_of_the_table(checker):
    out = plan_of(M.problems("past-64-chunks"), checker)
    big, small = out["problems"]
    assert len(big["chunks"]) > out["max_chunks"] and set(big["chunks"][:-1]) == {out["max_chunk_slots"]}
    assert sum(big["chunks"]) == 2100 and set(big["counts"]) == {12} and small["chunks"] == [8, 8, 4]

    out = plan_of(M.problems("chunk-edges"), checker)
    k = out["min_chunk"]
    assert [x["chunks"] for x in out["problems"]] == [[1], [3], [k], [k, 1], [k, k, 1]] and k == 8

    out = plan_of(M.problems("partial-views"), checker)
    ragged, full = out["problems"]
    assert len(ragged["counts"]) == 18 and set(ragged["counts"]) == {31, 54}                 # the view without corners is no slot
    assert ragged["counts"][:4] == [31, 54, 31, 54] and set(full["counts"]) == {54}           # (views 0, 2, 3, 4)
    assert ragged["chunks"] == [8, 8, 2]

    out = plan_of(M.problems("const-boards"), checker)
    some, none = out["problems"]
    assert some["active"] == [0 if b % 3 == 0 else 1 for b in range(19)] and some["chunks"] == [8, 8, 3]
    assert none["active"] == [0] * 20

    out = plan_of(M.problems("unseen-boards"), checker)
    appended, dropped = out["problems"]
    assert (appended["boards"], sum(appended["chunks"])) == (22, 20) and (dropped["boards"], sum(dropped["chunks"])) == (20, 18)

    # the corner loop's second pass (more corners than the 128 threads of k_mb_eval) and the largest board the route takes
    assert M.problems("two-pass")[0].n_points == 160
    out = plan_of(M.problems("full-lds"), checker)
    assert M.problems("full-lds")[0].n_points == out["max_points"] == 256


def test_plan_mode_refuses_what_the_header_refuses(checker):
    out = N.run(checker, "plan", 54, "2/54,54/", "2/54,55/")
    assert not out["ok"] and out["rc"] == -1, out                                             # view_count outside [0, n_points]
    out = N.run(checker, "plan", 257, "1/257/")
    assert not out["ok"] and out["rc"] == -5, out                                             # boards of more than 256 corners


# ----------------------------------------------------------------------------- 2. the references
@pytest.mark.parametrize("case_id", list(M.CASES))
def test_reference_of_every_case(case_id):
    for i, want in enumerate(M.expected(case_id)):
        ref = M.reference(case_id, i)
        assert ref["ok"], (case_id, i)
        rd = ref["relative_decrease"]
        assert rd > M.MIN_RELATIVE_DECREASE + M.RD_MARGIN if want == "A" else rd < M.MIN_RELATIVE_DECREASE - M.RD_MARGIN, (case_id, i, rd)
    assert "A" in M.expected(case_id)                       # a rejected problem never stands alone


def test_rejected_case_rejects():
    assert M.expected("rejected")[0] == "r" and M.reference("rejected", 0)["relative_decrease"] < -10.0


def test_radius_cases_are_damped_and_nearly_undamped():
    for i in range(2):
        assert M.reference("radius-1e-2", i)["kappa"] < 2.0
        assert M.reference("radius-1e8", i)["kappa"] > 1e6


@pytest.mark.parametrize("case_id", ["clamps", "noscale-clamps", "clamps-intrinsics"])
def test_both_clamps_bind_in_every_problem(case_id):
    """On the board columns (mb_board_factor, in k_mb_schur and k_mb_solve) in every clamp case; on the intrinsic columns
    (k_mb_solve's 7x7 diagonal) in clamps-intrinsics."""
    o = M.options(case_id)
    lo, hi = o["min_lm_diagonal"], o["max_lm_diagonal"]
    for i in range(len(M.problems(case_id))):
        nrm = M.column_norms(case_id, i, o.get("jacobi_scaling", 1))
        intr, board = nrm[:M.N_INTR], nrm[M.N_INTR:]
        x = intr if case_id == "clamps-intrinsics" else board
        assert (x < lo).any() and (x > hi).any() and ((lo < x) & (x < hi)).any(), (case_id, i, lo, hi)


def test_masks_hold_columns_inside_and_at_both_ends():
    held = [[k for k in range(7) if (m >> k) & 1] for m in M.MASKS5]
    assert held == [[], [5], [4, 5], [2, 3], [0, 1, 6]]
    for i in range(5):
        assert (~M.columns("masks", i)["cam_free"][0, 6:]).nonzero()[0].tolist() == held[i]


@pytest.mark.parametrize("case_id", ["soft_l1", "cauchy", "huber-masked"])
def test_robust_cases_have_corners_on_both_sides_of_the_scale(case_id):
    kind, a = M.CASES[case_id]["loss"]
    far, moved, near = M.problems(case_id)
    assert R.fraction_beyond(far, a) == 1.0
    res = orc.evaluate(near, jets=False)[1]
    beyond = np.sum(res * res, axis=1) > a * a
    assert 10 <= beyond.sum() <= 0.1 * beyond.size, beyond.sum()                               # the moved corners, and few others
    clean = M.mono(41, 802, noise=0.3)
    d = np.hypot(moved.obs_u - clean.obs_u, moved.obs_v - clean.obs_v)
    assert np.count_nonzero(d) == 10 and np.allclose(d[d > 0], 5.0)


def test_oracle_trajectories_reject_and_mix():
    runs = M.oracle_trajectories()                          # (asserts >= 2 rejections before `settled`, both decisions at iteration 2)
    assert [len(r) for r in runs] == [4, 1, 1]
    assert [M._pattern(os_)[:4] for os_, _ in runs[0]] == ["AArr", "Arrr", "AArr", "ArAr"]
    for batch in runs:
        for os_, n in batch:
            assert os_["num_iterations"] == 31 and 4 <= n <= 31


# ----------------------------------------------------------------------------- 3. sensitivity
def _backward(case_id, i, *, terms=None, cols=None):
    """Backward error, against the true reference, of the candidate of a reference step taken with other terms / columns."""
    p, ref = M.problems(case_id)[i], M.reference(case_id, i)
    bad = H.reference_step(p, terms=M.terms(case_id, i) if terms is None else terms, cols=M.columns(case_id, i) if cols is None else cols)
    assert bad["ok"]
    return H.step_errors(p, ref, H.reference_candidate(p, bad))["backward"]


def _second_pass_dropped():
    p = M.problems("two-pass")[0]
    cost, res, Jc, Jb, Ji = orc.evaluate(p, jets=True)
    keep = (np.arange(p.n_corners) % p.n_points < 128).astype(np.float64)
    assert np.all(p.view_count == p.n_points) and keep.sum() == 128 * p.n_views
    jets = (cost, res * keep[:, None], Jc * keep[:, None, None], Jb * keep[:, None, None], Ji * keep[:, None, None])
    return _backward("two-pass", 0, terms=H.step_terms(p, jets=jets))


def _slot_cross_term_dropped():
    t = dict(M.terms("partial-views", 1))
    t["EF"] = t["EF"].copy()
    t["EF"][5] = 0
    return _backward("partial-views", 1, terms=t)


def _constant_board_eliminated():
    cols = dict(M.columns("const-boards", 0))
    assert not cols["board_free"].all()
    cols["board_free"] = cols["board_seen"].copy()
    return _backward("const-boards", 0, cols=cols)


def _residual_not_corrected(case_id):
    kind, a = M.CASES[case_id]["loss"]
    p = M.problems(case_id)[1]
    plain = orc.evaluate(p, jets=True)
    cost, _, Jc, Jb, Ji = R.robust_jets(p, kind, a, jets=plain)
    return _backward(case_id, 1, terms=H.step_terms(p, jets=(cost, plain[1], Jc, Jb, Ji)))


def test_backward_error_sees_every_mistake():
    signal = {"second pass dropped": _second_pass_dropped(), "slot cross term dropped": _slot_cross_term_dropped(),
              "constant board eliminated": _constant_board_eliminated()}
    signal.update({f"residual not corrected, {c}": _residual_not_corrected(c) for c in ("soft_l1", "cauchy", "huber-masked")})
    print("\n[mono batch step] backward error of each mistake: " + ", ".join(f"{k} {v:.2e}" for k, v in signal.items()))
    for k, v in signal.items():
        assert v >= MARGIN * M.TAU_B, (k, v)
    # the values recorded in the module docstring
    assert signal["second pass dropped"] >= 4e-4 and signal["slot cross term dropped"] >= 0.1
    assert signal["constant board eliminated"] >= 1e-2 and min(v for k, v in signal.items() if k.startswith("residual")) >= 0.2


def test_backward_error_of_the_clean_candidate_is_rounding_only():
    worst = max(_backward(c, i) for c, i in (("two-pass", 0), ("partial-views", 1), ("const-boards", 0), ("soft_l1", 1),
                                             ("cauchy", 1), ("huber-masked", 1)))
    print(f"\n[mono batch step] backward error of the clean reference candidate {worst:.2e}")
    assert worst <= 1e-14
