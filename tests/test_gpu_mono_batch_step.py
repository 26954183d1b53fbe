"""The batched mono route (tscm_solve_mono_batch, tscm_mono_batch.h) one trust-region step at a time, and over forced
trajectories with rejected steps.

1. One step.  A batch solve stopped after one iteration leaves an accepted candidate x + delta in the caller's parameters.
   It is compared with helpers.reference_step (np.longdouble Schur solve) at the same point and options, per problem, with
   the rule and the tolerances of tests/test_gpu_step.py (TAU_B, TAU_F, C_KAPPA, EPS64, tolerances()): blockwise backward
   error, forward error of intrinsics and boards, the summary's step norm and relative decrease, the cost of iteration 0
   to 1e-12, and held columns, b / c, constant boards and unseen boards bit-equal to the input.  CASES are the smallest
   shapes at which each path of k_mb_eval / k_mb_schur / k_mb_solve / k_mb_control / k_mb_finish exists (the chunk shapes
   are asked of tscm_batch_plan.h by tests/test_mono_batch_step_cases.py, which also shows without a GPU that TAU_B sees
   four kernel-shaped mistakes by at least 20x).  Every case is one batch call, so a neighbour is always present.
   A rejected step ("rejected": radius 1e12) leaves the parameters bit-unchanged; its step norm and relative decrease
   are compared with the reference's.
2. Forced trajectories (test_gpu_trajectory.FORCED, 30 iterations from radius 1e8) of six problems against orc.solve:
   accept / reject pattern, cost, radius and step norm of every iteration while the oracle's own cost changes are above
   1e-7 of the cost (test_gpu_trajectory._compare and its tolerances), the cost to 1e-6 afterwards.  Every problem
   rejects at least two steps before that point, and at iteration 2 some problems accept and some reject, so one launch
   reads buffer 0 for some problems and buffer 1 for others.  Each problem alone, and the batch reversed, give the bits
   of the mixed batch.

Measured on an MI355X (largest over the cases; printed per case by the tests):
  backward error 1.1e-13 (huber-masked, the problem that starts at the ground truth; 1.0e-13 at radius 1e-2, where the
  rounding of x + delta is all there is), <= 6.8e-14 under soft-L1 / Cauchy, <= 2.6e-15 in every other case;
  forward error <= 1.3e-11 where kappa < 1e6 (full-lds: 480 kappa eps, inside TAU_F), 3.9e-8 at radius 1e8 and 6.7e-6 at
  radius 1e12 (both 29 kappa eps); step norm within 1.1e-5 and relative decrease within 6.5e-5 relative at radius 1e12
  (kappa 8e9), to the printed digits elsewhere.  All six trajectories follow the oracle's decisions up to `settled`
  (and the two that never settle, to the end).  No kernel bug was found.
"""
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import api, synth
from tscm_calib_amd.problem import Problem
from tests import helpers as H
from tests import robust_ref as R
from tests.test_fixed_reference import masked_columns
from tests.test_gpu_mono_batch import assert_bits
from tests.test_gpu_step import C_KAPPA, EPS64, TAU_B, TAU_F, tolerances
from tests.test_gpu_trajectory import FORCED, _compare, _pattern

ONE_STEP = dict(max_num_iterations=1, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
MIN_RELATIVE_DECREASE = 1e-3            # Ceres' default, the solver's and the oracle's
# "well away" from the acceptance threshold: the reference's relative decrease is on its side of it by this much
RD_MARGIN = 0.05
N_INTR = H.N_INTR_FREE
REF_KEYS = ("initial_trust_region_radius", "min_lm_diagonal", "max_lm_diagonal", "jacobi_scaling")


# ----------------------------------------------------------------------------- problems
def mono(views, seed, *, noise=0.1, cols=9, rows=6, pitch=45.0):
    return synth.make_problem(1, views, seed, noise_px=noise, cols=cols, rows=rows, pitch=pitch)


def _partial_views():
    p = mono(19, 721)
    p.view_count[::3] = 31
    p.view_count[1] = 0
    return [p, mono(19, 722)]


def _const_boards():
    p = mono(19, 731)
    p.board_pose_constant = (np.arange(p.n_boards) % 3 == 0).astype(np.uint8)
    return [p.normalised(), synth.make_config(1, poses_fixed=True).normalised()]


def _unseen_boards():
    """Boards outside every slot: two appended behind the last view's (with poses of their own, not zeros), and two
    views without corners (one in the middle, one the last board)."""
    p = mono(20, 741)
    extra = np.array([[0.1, -0.2, 0.3, 10.0, -20.0, 500.0], [-0.3, 0.05, 0.2, -35.0, 15.0, 640.0]])
    a = Problem(1, p.n_boards + 2, p.board_xy, p.view_camera, p.view_board, p.view_offset, p.view_count, p.obs_u, p.obs_v,
                p.cam_rt, p.intr, np.concatenate([p.board_rt, extra]), p.cam_pose_constant, True, meta=dict(p.meta))
    b = mono(20, 742)
    b.view_count[[4, 19]] = 0
    return [a.normalised(), b]


def _with_outliers(p, n=10, px=5.0):
    """n corners, spread over the views, moved by px pixels."""
    q = p.copy().normalised()
    idx = (np.arange(n) * (q.obs_u.size // n) + 7) % q.obs_u.size
    ang = 0.7 * np.arange(n)
    q.obs_u[idx] += px * np.cos(ang)
    q.obs_v[idx] += px * np.sin(ang)
    return q


def _robust_pair():
    """From the perturbed start every corner lies beyond a scale of 1 px; the third problem starts at the ground truth, so
    its corners lie within the scale (noise 0.3 px) except the moved ones: both sides of every rho in one launch."""
    near = synth.make_problem(1, 20, 803, noise_px=0.3, perturb=False)
    return [mono(20, 801, noise=0.3), _with_outliers(mono(41, 802, noise=0.3)), _with_outliers(near)]


MASKS5 = [0, 32, 16 | 32, 4 | 8, 1 | 2 | 64]

# case id -> dict(build, opt, fixed, loss, clamps, expect); expect: per problem "A" (the reference step is accepted) or
# "r" (rejected), asserted of the reference by tests/test_mono_batch_step_cases.py and of the device here
CASES = {}


def _case(name, build, expect=None, *, fixed=None, loss=None, clamps=False, **opt):
    CASES[name] = dict(build=build, opt=opt, fixed=fixed, loss=loss, clamps=clamps, expect=expect)


_case("two-pass", lambda: [mono(9, 701, cols=16, rows=10, pitch=25.0), mono(9, 702, cols=16, rows=10, pitch=25.0)])
_case("full-lds", lambda: [mono(9, 711, cols=16, rows=16, pitch=20.0), mono(3, 712, cols=16, rows=16, pitch=20.0)])
_case("partial-views", _partial_views)
_case("const-boards", _const_boards)
_case("unseen-boards", _unseen_boards)
_case("chunk-edges", lambda: [mono(v, 751 + i) for i, v in enumerate((1, 3, 8, 9, 17))])
_case("past-64-chunks", lambda: [mono(2100, 761, cols=4, rows=3), mono(20, 762, cols=4, rows=3)])
_case("radius-1e-2", lambda: [mono(20, 771), mono(41, 772)], initial_trust_region_radius=1e-2)
_case("radius-1e8", lambda: [mono(20, 771), mono(41, 772)], initial_trust_region_radius=1e8)
_case("noscale", lambda: [mono(20, 781), mono(41, 782)], jacobi_scaling=0)
_case("clamps", lambda: [mono(20, 781), mono(41, 782)], clamps=True)
_case("noscale-clamps", lambda: [mono(20, 781), mono(41, 782)], jacobi_scaling=0, clamps=True)
_case("clamps-intrinsics", lambda: [mono(20, 781), mono(41, 782)], clamps="intrinsics")
_case("masks", lambda: [mono(20, 791 + i) for i in range(5)], fixed=MASKS5)
_case("soft_l1", _robust_pair, loss=("soft_l1", 1.0))
_case("cauchy", _robust_pair, loss=("cauchy", 1.0))
_case("huber-masked", _robust_pair, loss=("huber", 1.0), fixed=[32, 4 | 8, 1 | 64])
_case("rejected", lambda: [mono(20, 20241), mono(41, 812)], expect="rA", initial_trust_region_radius=1e12)


@functools.lru_cache(maxsize=None)
def problems(case_id):
    return tuple(p.normalised() for p in CASES[case_id]["build"]())


def expected(case_id):
    return CASES[case_id]["expect"] or "A" * len(problems(case_id))


def masks(case_id):
    f = CASES[case_id]["fixed"]
    return [0] * len(problems(case_id)) if f is None else list(f)


@functools.lru_cache(maxsize=None)
def terms(case_id, i):
    p, loss = problems(case_id)[i], CASES[case_id]["loss"]
    return H.step_terms(p) if loss is None else H.step_terms(p, jets=R.robust_jets(p, *loss))


def columns(case_id, i):
    return masked_columns(problems(case_id)[i], [masks(case_id)[i]])


def column_norms(case_id, i, scaled):
    """The (scaled) squared column norms of problem i's free columns, as the LM diagonal clamps see them."""
    ref = H.reference_step(problems(case_id)[i], terms=terms(case_id, i), cols=columns(case_id, i))
    assert ref["ok"]
    sc2, sb2 = (ref["sc"] ** 2, ref["sb"] ** 2) if scaled else (1, 1)
    return np.concatenate([np.asarray((sc2 * ref["nc"])[ref["cam_free"]], dtype=np.float64),
                           np.asarray((sb2 * ref["nb"])[ref["board_free"]], dtype=np.float64).ravel()])


@functools.lru_cache(maxsize=None)
def _options_items(case_id):
    c = CASES[case_id]
    opt = dict(c["opt"])
    if c["clamps"]:
        # one pair of options for the batch, as test_gpu_step.clamp_options: between the quartiles of the norms of all its
        # problems (both clamps bind in each of them: tests/test_mono_batch_step_cases.py).  Those quartiles are the board
        # columns' and leave no intrinsic column below the lower clamp; clamps="intrinsics" takes the quartiles of the
        # intrinsic columns alone, so that both clamps bind on k_mb_solve's 7x7 diagonal too
        nrm = [column_norms(case_id, i, opt.get("jacobi_scaling", 1)) for i in range(len(problems(case_id)))]
        nrm = np.concatenate([x[:N_INTR] for x in nrm] if c["clamps"] == "intrinsics" else nrm)
        lo, hi = np.quantile(nrm, [0.25, 0.75])
        opt.update(min_lm_diagonal=float(lo), max_lm_diagonal=float(hi))
    return tuple(sorted(opt.items()))


def options(case_id):
    return dict(_options_items(case_id))


def candidate_cost(case_id, q):
    loss = CASES[case_id]["loss"]
    res = orc.evaluate(q, jets=False)
    return res[0] if loss is None else R.robust_cost(res[1], *loss)


@functools.lru_cache(maxsize=None)
def reference(case_id, i):
    """The extended-precision step of problem i of a case, its norm and its relative decrease (the candidate's cost: the
    oracle's at x + delta_ref)."""
    p = problems(case_id)[i]
    opt = {k: v for k, v in options(case_id).items() if k in REF_KEYS}
    ref = H.reference_step(p, terms=terms(case_id, i), cols=columns(case_id, i), **opt)
    if not ref["ok"]:
        return ref
    rc = H.reference_candidate(p, ref)
    q = p.copy().normalised()
    q.intr[:], q.board_rt[:] = rc["intr"], rc["board_rt"]
    free = np.concatenate([np.asarray(ref["cam"], dtype=np.float64)[ref["cam_free"]],
                           np.asarray(ref["board"], dtype=np.float64)[ref["board_free"]].ravel()])
    ref["step_norm"] = float(np.linalg.norm(free))
    ref["relative_decrease"] = (ref["cost"] - candidate_cost(case_id, q)) / ref["model_cost_change"]
    return ref


def run_batch(case_id, device=0):
    c = CASES[case_id]
    qs = [p.copy().normalised() for p in problems(case_id)]
    out = api.refinement_batch(qs, device, loss=c["loss"], fixed=c["fixed"], **ONE_STEP, **options(case_id))
    return qs, [s for _, s in out]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ----------------------------------------------------------------------------- 1. one step
@pytest.mark.gpu
@pytest.mark.parametrize("case_id", list(CASES))
def test_step_against_extended_precision(hip_device, case_id):
    ps = problems(case_id)
    qs, sums = run_batch(case_id, hip_device)
    worst_b = worst_f = worst_fk = 0.0
    fails = []
    for i, (p, q, s, want) in enumerate(zip(ps, qs, sums, expected(case_id))):
        ref = reference(case_id, i)
        assert ref["ok"]
        it = s["iterations"]
        assert len(it) == 2 and it[1]["step_is_valid"], it
        tau_b, tau_f, tau_rd = tolerances((case_id, None, {}), ref["kappa"], ref["cost"], ref["model_cost_change"])
        assert (tau_b, tau_f) == (TAU_B, max(TAU_F, C_KAPPA * ref["kappa"] * EPS64))
        rd, rd_ref = it[1]["relative_decrease"], ref["relative_decrease"]
        line = (f"[mono batch step] {case_id}[{i}] views {p.n_views} kappa {ref['kappa']:.2e} rd {rd:.6g} (ref {rd_ref:.6g}) "
                f"step_norm {it[1]['step_norm']:.9g} (ref {ref['step_norm']:.9g})")
        cf, bf = ref["cam_free"][0, 6:], ref["board_free"]
        if want == "A":
            assert it[1]["step_is_successful"], it
            e = H.step_errors(p, ref, dict(cam_rt=p.cam_rt, intr=q.intr, board_rt=q.board_rt))
            fwd = max(e["forward_intr"], e["forward_board"])
            worst_b, worst_f, worst_fk = max(worst_b, e["backward"]), max(worst_f, fwd), max(worst_fk, fwd / (ref["kappa"] * EPS64))
            print(line + f" backward {e['backward']:.2e} forward intr {e['forward_intr']:.2e} board {e['forward_board']:.2e}")
            if not e["backward"] <= tau_b:
                fails.append((i, "backward", e["backward"], tau_b))
            for k in ("forward_intr", "forward_board"):
                if e[k] > tau_f:
                    fails.append((i, k, e[k], tau_f))
            # every free entry moved; what is not free carries the input's bits
            assert np.all(q.intr[0, :7][cf] != p.intr[0, :7][cf])
        else:
            print(line + " rejected")
            assert not it[1]["step_is_successful"], it
            assert np.array_equal(_bits(q.intr), _bits(p.intr)) and np.array_equal(_bits(q.board_rt), _bits(p.board_rt))
        assert np.array_equal(_bits(q.intr[0, :7][~cf]), _bits(p.intr[0, :7][~cf]))
        assert np.array_equal(_bits(q.intr[0, 7:]), _bits(p.intr[0, 7:]))
        assert np.array_equal(_bits(q.board_rt[~bf]), _bits(p.board_rt[~bf]))
        if abs(it[0]["cost"] - ref["cost"]) > 1e-12 * ref["cost"]:
            fails.append((i, "cost", it[0]["cost"], ref["cost"]))
        if abs(it[1]["step_norm"] - ref["step_norm"]) > tau_f * ref["step_norm"]:
            fails.append((i, "step_norm", it[1]["step_norm"], ref["step_norm"], tau_f))
        if abs(rd - rd_ref) > tau_rd * max(1.0, abs(rd_ref)):
            fails.append((i, "relative_decrease", rd, rd_ref, tau_rd))
    print(f"[mono batch step] {case_id}: largest backward {worst_b:.2e} forward {worst_f:.2e} ({worst_fk:.2g} kappa eps)")
    assert not fails, fails


# ----------------------------------------------------------------------------- 2. forced trajectories
TRAJECTORY = dict(FORCED, max_num_iterations=30, initial_trust_region_radius=1e8)


@functools.lru_cache(maxsize=None)
def trajectory_batches():
    """Six problems; the problems of a batch share a board, so the 160-corner and the 4x3 problem are batches of their own."""
    return ((mono(20, 601, noise=0.3), mono(41, 602, noise=0.3), mono(9, 603, noise=0.3), mono(70, 604, noise=0.3)),
            (mono(12, 605, noise=0.3, cols=16, rows=10, pitch=25.0),),
            (mono(300, 606, noise=0.3, cols=4, rows=3),))


def settled_index(os_):
    """The first iteration whose cost change is below 1e-7 of the cost in the oracle's own run (test_gpu_trajectory)."""
    rel = [abs(it["cost_change"]) / it["cost"] for it in os_["iterations"]]
    return next((i for i in range(2, len(rel)) if rel[i] < 1e-7), len(rel))


@functools.lru_cache(maxsize=None)
def oracle_trajectories():
    """orc.solve of every problem -> per batch a tuple of (summary, settled).  Asserts what the comparison rests on: at
    least two rejections before `settled`, and both decisions among the six problems at iteration 2."""
    out = []
    for batch in trajectory_batches():
        runs = []
        for p in batch:
            os_ = orc.solve(p.copy().normalised(), **TRAJECTORY)
            n = settled_index(os_)
            assert _pattern(os_)[:n - 1].count("r") >= 2, (_pattern(os_), n)
            runs.append((os_, n))
        out.append(tuple(runs))
    second = {_pattern(os_)[1] for runs in out for os_, _ in runs}
    assert second == {"A", "r"}, second
    assert {_pattern(os_)[1] for os_, _ in out[0]} == {"A", "r"}          # ... and within the one mixed launch
    return tuple(out)


def _solve_batch(ps, device):
    qs = [p.copy().normalised() for p in ps]
    out = api.refinement_batch(qs, device, **TRAJECTORY)
    return qs, [s for _, s in out]


@pytest.mark.gpu
@pytest.mark.parametrize("b", [0, 1, 2], ids=["9x6", "16x10", "4x3"])
def test_forced_trajectories_with_rejected_steps(hip_device, b):
    ps, runs = trajectory_batches()[b], oracle_trajectories()[b]
    qs, sums = _solve_batch(ps, hip_device)
    for i, (gs, (os_, n)) in enumerate(zip(sums, runs)):
        print(f"[mono batch trajectory] {b}[{i}] settled {n} oracle {_pattern(os_)} device {_pattern(gs)}")
        _compare(gs, os_, upto=n, lm_iterations=30)
        for x, y in list(zip(gs["iterations"], os_["iterations"]))[n:]:
            assert abs(x["cost"] - y["cost"]) <= 1e-6 * y["cost"], (i, x["iteration"], x["cost"], y["cost"])
    # the same bits alone and in the reversed batch: parameters, every logged cost, the counts
    qr, sr = _solve_batch(ps[::-1], hip_device)
    for i in range(len(ps)):
        assert_bits(qs[i], sums[i], qr[len(ps) - 1 - i], sr[len(ps) - 1 - i])
        if len(ps) > 1:
            q1, s1 = _solve_batch([ps[i]], hip_device)
            assert_bits(qs[i], sums[i], q1[0], s1[0])
