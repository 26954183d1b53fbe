"""The rows of tests/lm_exit_cases.py on the oracle alone (CPU): every row gives the outcome the table states, every exit
of construction 3 has its 3x margin, and the table reaches what it claims -- every TermReason of tscm_ctrl.h, both ends of
max_num_iterations, and an exit and a failure on every route (the routes asked of the library's own host plan headers, as
tests/test_step_tolerance.py does for the cases of tests/test_gpu_step.py)."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import lm_exit_cases as X
from tests import native_check as N
from tests import test_gpu_step as S
from tests import test_step_tolerance as T


@pytest.mark.parametrize("case_id", [c.id for c in X.CASES])
def test_oracle_gives_the_rows_outcome(case_id):
    case = X.BY_ID[case_id]
    s, q = X.oracle(case_id)
    assert X.outcome(s) == X.expected(case)
    p = S.problem(case.problem)
    if case.termination_type == 2 or case.pattern.count("x") == len(case.pattern):
        # no step was taken: the parameters are the input's (a NaN observation is not a parameter)
        assert np.array_equal(q.cam_rt, p.cam_rt) and np.array_equal(q.intr, p.intr) and np.array_equal(q.board_rt, p.board_rt)
    if isinstance(case.spoil, tuple):
        assert np.isnan(s["initial_cost"]) and np.isnan(s["final_cost"])
        name, k = X.nan_corner(p, case.spoil[1])
        assert int(np.isnan(getattr(X.build(case), name)).sum()) == 1 and np.isfinite(getattr(p, name)[k])
    elif case.spoil is not None:
        assert np.isfinite(s["initial_cost"]) and s["final_cost"] == s["initial_cost"]        # construction 2: finite data


def test_nan_rows_halve_the_radius_exactly():
    s, _ = X.oracle("ring4-nan")
    assert [it["trust_region_radius"] for it in s["iterations"]] == [1e4, 5e3, 1250.0, 156.25, 9.765625]
    s, _ = X.oracle("ring4-nan-255")
    r = [it["trust_region_radius"] for it in s["iterations"]]
    assert len(r) == 256 and r[-1] == 0.0 and 40 <= r.index(0.0) <= 50                 # through the denormals to 0 near entry 47
    assert all(r[k + 1] == r[k] / 2.0 ** (k + 1) for k in range(30))
    s, _ = X.oracle("ring4-nan-minradius200")
    assert s["iterations"][-1]["trust_region_radius"] == 156.25


@pytest.mark.parametrize("case_id", [c.id for c in X.EXIT_CASES])
def test_exit_rows_have_their_margin(case_id):
    case = X.BY_ID[case_id]
    opt = X.options(case)
    tol = opt[X.KIND_OPTION[case.kind]]
    # no other exit test can bind: the other three compare positive quantities with 0, and the iteration cap is 3x away
    assert all(opt[o] == 0.0 for k, o in X.KIND_OPTION.items() if k != case.kind)
    assert opt["max_num_iterations"] >= X.MARGIN * (case.at + 1)
    its = X.base_log(case.problem, case.given, case.at)["iterations"]
    assert X.pattern({"iterations": its})[:len(case.pattern)] == case.pattern
    for it in its:
        assert it["trust_region_radius"] > 0.0 and (it["iteration"] == 0 or (it["step_norm"] > 0.0 and it["cost_change"] != 0.0))
        assert it["gradient_max_norm"] > 0.0
    q = X.deciding_quantities(case)
    made = [k for k in range(case.at) if q[k] is not None]
    if case.kind != "param":
        assert q[case.at] * X.MARGIN <= tol and all(q[k] >= X.MARGIN * tol for k in made), (tol, q)
    else:
        xn = X.x_norm(S.problem(case.problem))          # within a few per cent of |x| at every iterate of these rows
        assert q[case.at] * X.MARGIN <= 0.9 * tol * xn and all(q[k] >= X.MARGIN * 1.1 * tol * (xn + tol) for k in made), (tol, xn, q)
    # ... and by the oracle itself, whatever the quantity: the tolerance times 3 and over 3 ends the solve at the same place
    for scale in (X.MARGIN, 1.0 / X.MARGIN):
        s = orc.solve(X.build(case), **X.options(case, scale))
        assert X.outcome(s) == X.expected(case), scale


@pytest.mark.parametrize("case_id", [c.id for c in X.EXIT_CASES if "r" in c.pattern])
def test_rows_with_rejected_steps_are_reproducible_by_the_oracle(case_id):
    """The logged cost of a rejected iteration is the candidate's, after a nearly undamped step: the oracle with its sums
    re-associated over four threads gives the row's decisions and its costs to a third of the GPU test's 1e-5."""
    case = X.BY_ID[case_id]
    s1, _ = X.oracle(case_id)
    orc.lib().orc_set_num_threads(4)
    try:
        s4 = orc.solve(X.build(case), **X.options(case))
    finally:
        orc.lib().orc_set_num_threads(1)
    assert X.outcome(s4) == X.outcome(s1)
    for a, b in zip(s4["iterations"], s1["iterations"]):
        assert abs(a["cost"] - b["cost"]) <= 1e-5 / X.MARGIN * b["cost"], (a["iteration"], a["cost"], b["cost"])
        assert a["trust_region_radius"] == b["trust_region_radius"]


def test_table_reaches_every_reason_and_both_iteration_caps():
    messages = {c.message for c in X.CASES}
    assert messages == set(X.TERM_REASONS.values()) and len(X.TERM_REASONS) == 6
    caps = {dict(c.given).get("max_num_iterations") for c in X.CASES}
    assert {0, 255} <= caps
    for route in X.ROUTES:
        assert any(c.problem == route for c in X.EXIT_CASES), route
        assert any(c.problem == route and c.termination_type == 2 for c in X.FAILURE_CASES), route
    # the four kinds of construction 3, and an exit iteration that is no multiple of 4 on every route (part D of the GPU tests)
    assert {c.kind for c in X.EXIT_CASES} == set(X.KIND_OPTION)
    for route in X.ROUTES:
        assert any(c.problem == route and c.at % 4 for c in X.EXIT_CASES), route


@pytest.fixture(scope="module")
def planner():
    return N.built("launch_seq_check.cpp", "launch_seq_check")


# problem -> what the library's host plan of it must show (labels of tests/test_step_tolerance.py: route)
ROUTE_CLAIMS = {
    "ring2": {"k_solve_reduced<4,16,64>", "k_backsub_prep fused", "k_T_reduce fused"},
    "ring4": {"k_solve_reduced<4,16,64>", "k_backsub_prep fused", "k_T_reduce fused"},
    "ring6": {"k_solve_nd<1> graph plan"},
    "big12": {"k_solve_reduced_big"},
    "mono": {"mono"},
    "mixed6": {"k_schur_factor + k_pair_gram", "k_schur_gram<1>", "k_schur_gram<2>", "k_schur_gram<3>"},
    "idle_cam4": {"camera without views", "k_solve_reduced<4,16,64>"},
    "idle_cam6": {"camera without views", "k_solve_nd<1> graph plan"},
    "many_boards4": {"fused back-substitution does not fit resident"},
}


def test_rows_take_the_routes_the_table_names(planner):
    assert set(X.ROUTES) <= set(ROUTE_CLAIMS) and {c.problem for c in X.CASES} == set(ROUTE_CLAIMS)
    for prob, claims in ROUTE_CLAIMS.items():
        reached = T.route((prob, prob, {}), planner)
        assert claims <= reached, (prob, claims - reached)
    plan = T.plan_of(S.problem("many_boards4"), {}, planner)
    assert sum(plan["nv_chunks"]) > 1                                  # several chunks
    # mixed6: boards of one to four and more cameras; the two NaN corners sit in a board of each kind
    p = S.problem("mixed6")
    plan = T.plan_of(p, {}, planner)
    cams = np.bincount(p.view_board[p.view_count > 0], minlength=p.n_boards)
    assert plan["slow_boards"] == int((cams > 3).sum()) > 0 and set(range(1, 5)) <= set(cams.tolist())
    for where, ok in (("slow_board", lambda n: n > 3), ("fast_board", lambda n: 2 <= n <= 3)):
        case = X.BY_ID[f"mixed6-nan-{where.replace('_', '-')}"]
        assert ok(cams[p.view_board[X.spoiled_view(case, p)]])
    # many_boards4: the NaN is the last corner of the view that the device orders last (the end of its last evaluation chunk)
    p = S.problem("many_boards4")
    plan = T.plan_of(p, {}, planner)
    case = X.BY_ID["many_boards4-nan-last-view"]
    v = X.spoiled_view(case, p)
    assert v == plan["last_dev_view"] != p.n_views - 1 and plan["eval_chunks"] > 1
    assert X.nan_corner(p, case.spoil[1])[1] == p.view_offset[v] + p.view_count[v] - 1


def test_batch_options_straddle_by_3x():
    """Part F of the GPU tests: the shared parameter tolerance ends slot 3 at its first step and no other slot, at 3 t and t / 3
    as well; the NaN slot fails after two logged invalid steps."""
    ps, opt = X.batch_problems(), X.batch_options()
    for scale in (X.MARGIN, 1.0, 1.0 / X.MARGIN):
        o = dict(opt, parameter_tolerance=scale * opt["parameter_tolerance"])
        for i, p in enumerate(ps):
            s = orc.solve(p.copy().normalised(), **o)
            want = (X.MSG_PARAM, 1) if i == 3 else (X.MSG_MAX_ITER, 4)
            assert (s["message"], s["num_iterations"]) == want, (scale, i, s["message"])
    s = orc.solve(X.batch_with_nan(ps)[1], **opt)
    assert (s["message"], s["termination_type"], s["num_iterations"], X.pattern(s)) == (X.MSG_INVALID, 2, 3, "xx")
