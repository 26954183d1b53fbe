"""How a device solve ends, and what an invalid step leaves behind, on every route: the rows of tests/lm_exit_cases.py
against the oracle (tests/test_lm_exit_cases.py shows, without a GPU, that the oracle gives each row's outcome with its margin).

A. every exit row (gradient, parameter and function tolerance, minimum radius; the iteration cap on healthy data): message,
   termination type, counts, pattern, the log and the final parameters against the oracle.
B. every row with a NaN observation or an exactly zero pivot: the oracle's outcome, the radii bit for bit, zeros in every
   invalid entry, NaN costs where the oracle has them, the parameters back bit for bit.
C. a handle after a failed solve: the next solve has the bits of a fresh handle.
D. exits and failures under every fusion flag and check_every in {1, 4, 255}: the same summary and parameter bits; and an exit
   leaves what the same solve leaves when it is capped at its last successful iteration.
E. shards (api.Group, world 2 and 3): every rank the same summary, rank 0 the unsharded decisions.
F. the batched mono route: a NaN slot and a slot that ends on a parameter tolerance next to healthy ones.
G. the fp32-Jacobian tier, a Huber loss, corner weights and camera priors.

Two places where the tests differ from a literal reading of their specification, both on the side of the library's documented
interface: tscm_solver_solve_resident(reset = 0) starts from the device's accepted point, not from the uploaded parameters, so
the upload_params half of C uploads and solves with reset = 1 and then continues with reset = 0; and the loss, weight and prior
rows of G have a different objective from the plain row, so their gradient tolerance is taken by the same 9x rule from the
device's own tolerance-free run of that objective, and what is asserted is the exit at that iteration and the invariants of D.

Measured on an MI355X:
  A: against the oracle's log, rows whose steps are all accepted: cost within 2.6e-12, radius within 1.9e-9, step norm within
     5.0e-12 (relative); the two radius rows (four rejected candidates each, from radius 1e12 and 1e10): cost within 3.8e-6, step
     norm within 3.7e-6, radius equal.  Parameters of every row within 1e-6; rows without an accepted step: the input's bits.
  B: every NaN row has the oracle's outcome, radii and zeros, and the input's parameter bits; the denormal tail of the 255-step
     radius sequence (ring4 and ring6) is the oracle's bit for bit, down to 0.0.
  G: a failed solve with a loss or with priors returns rc 0 and rmse NaN (robust_rmse sums the NaN observation); so does the
     plain rmse of the fp32 tier and of corner weights.
  No bug was found in the flag hand-offs.
  One difference from the oracle was found and fixed.  With min_lm_diagonal = 0 (idle_cam4-zero-pivot, idle_cam6-zero-pivot) the
  oracle fails on the zero pivots of the skew intrinsics b and c, which have no Jacobian column; the device keeps b and c out of
  its systems, had no such pivot and took 50 accepted steps to "Maximum number of iterations reached.".  lm_step now declares
  the step invalid where the program has such a column (CtrlHead::inert_cols, set per solve and per batch slot from the held
  intrinsics) and its pivot clamp(0, min_lm_diagonal, max_lm_diagonal) / radius is not > 0; before the fix the two cases of B
  failed, afterwards they pass, and no bit of a solve with a positive min_lm_diagonal moves.  The idle camera has no columns in
  either program, so the reduced solvers' own failure flag on finite data is still not reached by any row here.
"""
import functools
import math
import struct

import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import api, lib, synth
from tests import helpers as H
from tests import lm_exit_cases as X
from tests import test_gpu_mono_batch as MB
from tests import test_gpu_sharded as SH
from tests import test_gpu_step as S
from tests import weights_ref as W
from tests.test_gpu_priors import scattered_priors

pytestmark = pytest.mark.gpu

DBL_MIN = 2.2250738585072014e-308
TIMINGS = ("seconds_solve", "seconds_total")
# the bounds of tests/test_gpu_trajectory.py: _compare -- all-accepted runs, and its defaults where steps were rejected
TIGHT = dict(cost_rtol=1e-9, radius_rtol=1e-3)
LOOSE = dict(cost_rtol=1e-5, radius_rtol=2e-2)
PARAM_RTOL = 1e-6                     # natural solves of tests/test_gpu_parity.py, every problem size
MEASURED = dict(cost=0.0, radius=0.0, step_norm=0.0)          # part A's largest differences so far (printed by every case)


def bits(x):
    """A summary (or any nest of dicts, lists and numbers) with every float as its bit pattern: NaN equals NaN."""
    if isinstance(x, dict):
        return {k: bits(v) for k, v in x.items() if k not in TIMINGS}
    if isinstance(x, (list, tuple)):
        return [bits(v) for v in x]
    if isinstance(x, float):
        return "nan" if math.isnan(x) else struct.pack("<d", x).hex()
    return x


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))


def params_of(q):
    return q.cam_rt.copy(), q.intr.copy(), q.board_rt.copy()


def run(s, start, **opt):
    """One solve of the handle from `start` (cam_rt, intr, board_rt) -> summary, parameters."""
    s.upload_params(*start)
    r = s.solve_resident(reset=True, **opt)
    cam, intr, board = s.download_params()
    if s.problem.mono:
        cam = start[0].copy()
    return r, (cam, intr, board)


@functools.lru_cache(maxsize=None)
def device(case_id, device_index):
    """(summary, parameters, input parameters) of a row on a fresh handle; computed once, not to be changed."""
    case = X.BY_ID[case_id]
    q = X.build(case)
    start = params_of(q)
    with api.Solver(q, device_index) as s:
        r = s.solve(**X.options(case))
    return r, params_of(q), start


def assert_outcome(gs, os_):
    for k in ("message", "termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps"):
        assert gs[k] == os_[k], (k, gs[k], os_[k])
    assert X.pattern(gs) == X.pattern(os_)


# ----------------------------------------------------------------------------- A. exits against the oracle
@pytest.mark.parametrize("case_id", [c.id for c in X.HEALTHY_EXIT_CASES])
def test_exit_against_oracle(hip_device, case_id):
    case = X.BY_ID[case_id]
    gs, gp, start = device(case_id, hip_device)
    os_, po = X.oracle(case_id)
    assert X.outcome(os_) == X.expected(case)
    assert_outcome(gs, os_)
    tol = TIGHT if set(case.pattern) <= {"A"} else LOOSE
    for a, b in zip(gs["iterations"], os_["iterations"]):
        assert a["iteration"] == b["iteration"] and a["step_is_valid"] == b["step_is_valid"] == 1
        d = (abs(a["cost"] - b["cost"]) / abs(b["cost"]), abs(a["trust_region_radius"] - b["trust_region_radius"]) / b["trust_region_radius"],
             abs(a["step_norm"] - b["step_norm"]) / max(b["step_norm"], 1e-9))
        for k, v in zip(("cost", "radius", "step_norm"), d):
            MEASURED[k] = max(MEASURED[k], v)
        assert d[0] <= tol["cost_rtol"] and d[1] <= tol["radius_rtol"] and d[2] <= tol["radius_rtol"], (a["iteration"], d)
    assert abs(gs["final_cost"] - os_["final_cost"]) <= tol["cost_rtol"] * os_["final_cost"]
    if case.kind in ("param", "func"):
        # the step that triggered the exit was taken (lm_iterations) and is not in the log
        assert gs["num_iterations"] == case.at and gs["iterations"][-1]["iteration"] == case.at - 1 and gs["lm_iterations"] == case.at
    elif case.is_margin_exit:
        assert gs["num_iterations"] == case.at + 1 and gs["lm_iterations"] == case.at
    q = X.build(case)
    q.cam_rt[:], q.intr[:], q.board_rt[:] = gp
    e = H.param_rel_err(q, po)
    assert max(e.values()) < PARAM_RTOL, e
    if "A" not in case.pattern:
        assert same_bits(gp, start)                          # no step was accepted: nothing may have moved
    print("largest differences so far (cost, radius, step norm):", MEASURED)


# ----------------------------------------------------------------------------- B. invalid steps against the oracle
@pytest.mark.parametrize("case_id", [c.id for c in X.FAILURE_CASES])
def test_invalid_steps_against_oracle(hip_device, case_id):
    """The two rows of construction 2 (min_lm_diagonal = 0) are finite: their candidates are computed and evaluated, and the
    control step discards them for the zero pivot of the columns b and c that the kernels leave out."""
    case = X.BY_ID[case_id]
    gs, gp, start = device(case_id, hip_device)
    os_, _ = X.oracle(case_id)
    assert X.outcome(os_) == X.expected(case)
    assert_outcome(gs, os_)
    assert len(gs["iterations"]) == len(os_["iterations"]) == case.num_iterations
    tail_matches = True
    for k, (a, b) in enumerate(zip(gs["iterations"], os_["iterations"])):
        ra, rb = a["trust_region_radius"], b["trust_region_radius"]
        if rb >= DBL_MIN:
            assert ra == rb, (k, ra, rb)                     # divisions by powers of two: exact
        else:
            assert 0.0 <= ra <= gs["iterations"][k - 1]["trust_region_radius"], (k, ra)
            tail_matches = tail_matches and ra == rb
        assert a["iteration"] == b["iteration"] == k and a["step_is_valid"] == b["step_is_valid"]
        if k > 0:
            assert a["step_is_valid"] == 0 and a["step_is_successful"] == 0
            assert a["step_norm"] == 0.0 and a["cost_change"] == 0.0 and a["relative_decrease"] == 0.0
        assert math.isnan(a["cost"]) == math.isnan(b["cost"]), k
        if not math.isnan(b["cost"]):
            assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
    for k in ("initial_cost", "final_cost"):
        assert math.isnan(gs[k]) == math.isnan(os_[k]), k
    assert same_bits(gp, start)
    if case.num_iterations == 256:
        assert gs["lm_iterations"] == 255 and gs["iterations"][-1]["trust_region_radius"] == 0.0
        print("denormal tail of the radius sequence equal to the oracle's bit for bit:", tail_matches)


def test_zero_pivot_needs_a_free_column_without_a_jacobian(hip_device):
    """min_lm_diagonal = 0 fails through b and c alone, and only where they are columns of the program (tscm.h, held
    intrinsics): a camera with views takes them out by holding both (SubsetManifold) or by holding all of fx .. alpha
    (SetParameterBlockConstant: the block leaves the program, a pose-only refinement).  With every such camera doing so the solve
    proceeds; with one that does not, it fails, and the idle camera's word counts for nothing.  The batched mono route decides per
    slot."""
    case = X.BY_ID["idle_cam4-zero-pivot"]
    q = X.build(case)
    start, opt = params_of(q), X.options(case)
    Cn = q.n_cameras
    idle = int(np.nonzero(~H.step_columns(q)["cam_free"][:, 6])[0][0])
    other = (idle + 1) % Cn
    held, block = lib.FIX["b"] | lib.FIX["c"], lib.FIX_INTRINSICS

    def words(default, **at):
        w = np.full(Cn, default, dtype=np.int64)
        for m, v in at.items():
            w[int(m[1:])] = v
        return w

    solves = {"b c held": words(held), "b c held where there are views": words(held, **{f"m{idle}": 0}), "blocks constant": words(block),
              "blocks constant or b c held": words(block, **{f"m{other}": held | lib.FIX["fx"]})}
    fails = {"one holds b only": words(held, **{f"m{other}": lib.FIX["b"]}), "held on the idle camera only": words(0, **{f"m{idle}": held}),
             "one block not constant": words(block, **{f"m{other}": block & ~lib.FIX["alpha"]}),
             "constant on the idle camera only": words(0, **{f"m{idle}": block})}
    with api.Solver(q, hip_device) as s:
        for name, m in solves.items():
            s.set_fixed_intrinsics(m)
            r, rp = run(s, start, **opt)
            assert r["termination_type"] != 2 and "x" not in X.pattern(r) and r["num_successful_steps"] > 2 and not same_bits(rp, start), name
        for name, m in fails.items():
            s.set_fixed_intrinsics(m)
            r, rp = run(s, start, **opt)
            assert X.outcome(r) == X.expected(case) and same_bits(rp, start), name
    ps = [synth.make_problem(1, 20, seed, noise_px=0.1).normalised() for seed in (601, 602)]
    for fixed, failed in (([0, held], [True, False]), ([held, 0], [False, True]), ([block, block & ~lib.FIX["cx"]], [False, True])):
        qb, sb = MB.batch(ps, fixed=fixed, min_lm_diagonal=0.0)
        for p, qq, s, f in zip(ps, qb, sb, failed):
            assert (s["termination_type"] == 2 and X.pattern(s) == "xxxx") == f, fixed
            assert ("x" in X.pattern(s)) == f and (np.array_equal(qq.intr, p.intr) and np.array_equal(qq.board_rt, p.board_rt)) == f, fixed
    os_ = orc.solve(ps[0].copy().normalised(), min_lm_diagonal=0.0)
    assert_outcome(MB.batch(ps, min_lm_diagonal=0.0)[1][0], os_)


# ----------------------------------------------------------------------------- C. the handle after a failure
def _mask_without(q, name_k):
    """Corner weights (corner order) that take the observation `name_k` = (array, index) out."""
    _, k = name_k
    cnt, off = np.asarray(q.view_count), np.asarray(q.view_offset)
    v = int(np.nonzero((off <= k) & (k < off + cnt))[0][0])
    w = np.ones(q.n_corners)
    w[int((np.cumsum(cnt) - cnt)[v]) + k - int(off[v])] = 0.0
    return w


@pytest.mark.parametrize("name", ["ring4", "ring6", "big12"])
def test_handle_recovers_when_the_nan_corner_is_masked(hip_device, name):
    case = X.BY_ID[f"{name}-nan"]
    q = X.build(case)
    start = params_of(q)
    w = _mask_without(q, X.nan_corner(q, case.spoil[1]))
    with api.Solver(q, hip_device) as s:
        r = s.solve()
        assert r["termination_type"] == 2 and r["message"] == X.MSG_INVALID and same_bits(params_of(q), start)
        s.set_corner_weights(w)
        again = s.solve()
        got = params_of(q)
    f = X.build(case)
    with api.Solver(f, hip_device, weights=w) as s:
        fresh = s.solve()
    assert fresh["termination_type"] in (0, 1) and fresh["num_iterations"] > 3 and fresh["num_successful_steps"] > 3
    assert bits(again) == bits(fresh)
    assert same_bits(got, params_of(f))


@pytest.mark.parametrize("name", ["ring4", "ring6", "big12"])
def test_handle_recovers_after_nan_parameters(hip_device, name):
    """A NaN in camera 1's fx: failure, the NaN parameters left as they are; then the good parameters: a natural solve and a
    continuation from the device's point (reset = 0), both with the bits of a handle that never saw the NaN."""
    p = S.problem(name).copy().normalised()
    good = params_of(p)
    bad = tuple(a.copy() for a in good)
    bad[1][1, 0] = np.nan
    cont = dict(max_num_iterations=3, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)

    def good_solves(s):
        s.upload_params(*good)
        a = s.solve_resident(reset=True)
        b = s.solve_resident(reset=False, **cont)
        return a, b, s.download_params()

    with api.Solver(p, hip_device) as s:
        s.upload_params(*bad)
        r = s.solve_resident(reset=True)
        assert r["termination_type"] == 2 and r["message"] == X.MSG_INVALID and X.pattern(r) == "xxxx"
        assert same_bits(s.download_params(), bad)
        r = s.solve_resident(reset=False)                    # ... and from the device's own (NaN) point
        assert r["termination_type"] == 2 and X.pattern(r) == "xxxx" and same_bits(s.download_params(), bad)
        a, b, got = good_solves(s)
    with api.Solver(p.copy().normalised(), hip_device) as s:
        fa, fb, fresh = good_solves(s)
    assert fa["termination_type"] in (0, 1) and fa["num_successful_steps"] > 3 and fb["num_iterations"] == 4
    assert bits(a) == bits(fa) and bits(b) == bits(fb) and same_bits(got, fresh)


# ----------------------------------------------------------------------------- D. how the launches are cut
# per route: an exit whose iteration is no multiple of 4 (a poll every 4 iterations falls behind it) and a failure
CUT_ROWS = {"ring2": ("ring2-grad@2", "ring2-nan"), "ring4": ("ring4-func@3", "ring4-nan"), "ring6": ("ring6-grad@3", "ring6-nan"),
            "big12": ("big12-func@3", "big12-nan"), "mono": ("mono-grad@1", "mono-nan"), "mixed6": ("mixed6-func@6", "mixed6-nan-slow-board"),
            "idle_cam4": ("idle_cam4-func@5", "idle_cam4-nan"), "many_boards4": ("many_boards4-grad@1", "many_boards4-nan-last-view")}


@pytest.mark.parametrize("route", list(CUT_ROWS))
def test_launch_cuts_do_not_change_an_exit_or_a_failure(hip_device, route):
    assert set(CUT_ROWS) == set(X.ROUTES)
    for case_id in CUT_ROWS[route]:
        case = X.BY_ID[case_id]
        assert case.problem == route and (case.at % 4 if case.is_margin_exit else case.termination_type == 2)
        q = X.build(case)
        start, opt = params_of(q), X.options(case)
        with api.Solver(q, hip_device) as s:
            base, bp = run(s, start, **opt)
            assert X.outcome(base) == X.expected(case)
            for f in S.FUSION_FLAGS:
                r, rp = run(s, start, **dict(opt, exec_flags=f))
                assert bits(r) == bits(base) and same_bits(rp, bp), f
            for n in (1, 4, 255):
                r, rp = run(s, start, **dict(opt, check_every=n))
                assert bits(r) == bits(base) and same_bits(rp, bp), n
            again, ap = run(s, start, **opt)
            assert bits(again) == bits(base) and same_bits(ap, bp)


@pytest.mark.parametrize("case_id", [c.id for c in X.EXIT_CASES])
def test_exit_leaves_the_last_accepted_point(hip_device, case_id):
    """Exact on the device: parameters and final cost of an exit are those of the same solve with the tolerances off and the
    iteration cap at the last successful iteration -- nothing behind the exit, and nothing of a discarded step, is in them."""
    case = X.BY_ID[case_id]
    gs, gp, start = device(case_id, hip_device)
    last = max(it["iteration"] for it in gs["iterations"] if it["step_is_successful"])
    q = X.build(case)
    with api.Solver(q, hip_device) as s:
        r = s.solve(**dict(X.OFF, max_num_iterations=last, **dict(case.given)))
    assert r["message"] == X.MSG_MAX_ITER and r["num_iterations"] == last + 1
    assert bits(r["final_cost"]) == bits(gs["final_cost"]) and same_bits(params_of(q), gp)
    assert bits(r["iterations"]) == bits(gs["iterations"][:last + 1])


# ----------------------------------------------------------------------------- E. shards
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case_id", ["ring4-nan", "ring4-nan-last-view", "ring4-grad@3"])
def test_shards_agree_on_exits_and_failures(hip_device, world, case_id):
    case = X.BY_ID[case_id]
    q = X.build(case)
    start = params_of(q)
    owner = api.shard_owner(q, world)
    assert set(owner.tolist()) == set(range(world))
    if case.spoil is not None:
        # the NaN is in one rank's views only (a board's views all go to its owner); the other ranks learn of it by the
        # all-reduced scalars alone
        rank = int(owner[q.view_board[X.spoiled_view(case, q)]])
        assert rank == (0 if case.spoil[1] == "view1" else world - 1)
    with api.Group(q, world, hip_device) as g:
        sums = g.solve(**X.options(case))
    for s in sums[1:]:
        assert bits(s) == bits(sums[0])
    us, up, _ = device(case_id, hip_device)
    assert_outcome(sums[0], us)
    if case.spoil is not None:
        assert [it["trust_region_radius"] for it in sums[0]["iterations"]] == [it["trust_region_radius"] for it in us["iterations"]]
        assert same_bits(params_of(q), start)
    else:
        SH._same_run(sums[0], us)
        f = X.build(case)
        f.cam_rt[:], f.intr[:], f.board_rt[:] = up
        assert max(H.param_rel_err(q, f).values()) < 1e-8                     # (tests/test_gpu_sharded.py)


# ----------------------------------------------------------------------------- F. the batched mono route
def test_batch_with_a_nan_slot_and_an_early_exit(hip_device):
    ps, opt = X.batch_problems(), X.batch_options()      # (their 3x margin: tests/test_lm_exit_cases.py)
    bad = X.batch_with_nan(ps)
    qb, sb = MB.batch(bad, **opt)
    qh, sh = MB.batch(ps, **opt)                         # the same five with the finite value back in slot 1
    for i, p in enumerate(bad):
        q = p.copy().normalised()
        converged, ss = api.refinement(q, **opt)
        assert (sb[i]["termination_type"] == 0) == converged == (i == 3)
        if i == 1:
            os_ = orc.solve(p.copy().normalised(), **opt)
            for s in (sb[i], ss):
                assert_outcome(s, os_)
                assert s["termination_type"] == 2 and X.pattern(s) == "xx"
                assert [it["trust_region_radius"] for it in s["iterations"]] == [it["trust_region_radius"] for it in os_["iterations"]]
                assert all(math.isnan(it["cost"]) for it in s["iterations"]) and math.isnan(s["final_cost"])
                assert all(it["step_norm"] == 0.0 and it["cost_change"] == 0.0 for it in s["iterations"][1:])
            assert np.array_equal(qb[i].intr, p.intr) and np.array_equal(qb[i].board_rt, p.board_rt)
            assert np.array_equal(q.intr, p.intr) and np.array_equal(q.board_rt, p.board_rt)
            continue
        MB.assert_solo_tier(qb[i], sb[i], q, ss)
        assert sb[i]["message"] == ss["message"] == (X.MSG_PARAM if i == 3 else X.MSG_MAX_ITER)
        MB.assert_bits(qb[i], sb[i], qh[i], sh[i])       # the NaN next door changes no bit
    assert sb[3]["num_iterations"] == 1 and sb[3]["lm_iterations"] == 1
    assert np.array_equal(qb[3].intr, bad[3].intr) and np.array_equal(qb[3].board_rt, bad[3].board_rt)
    assert sh[1]["message"] == X.MSG_MAX_ITER and sh[1]["num_iterations"] == 4


# ----------------------------------------------------------------------------- G. tiers and specs
def _spec(name, q, nan_at=None):
    """Solver arguments, solve options and loss of a tier or spec on problem q."""
    if name == "fp32":
        return {}, dict(jacobian_fp32=1), None
    if name == "huber":
        return {}, {}, ("huber", 1.0)
    if name == "weights":
        w = W.scattered_weights(q, 5)
        if nan_at is not None:
            w[nan_at] = 1.5                              # the NaN corner stays in
        return dict(weights=w), {}, None
    return dict(priors=scattered_priors(q, 9)), {}, None


SPECS = ("fp32", "huber", "weights", "priors")


@pytest.mark.parametrize("spec", SPECS)
def test_nan_row_under_tiers_and_specs(hip_device, spec):
    """Decisions and radii of the plain fp64 run of the row; the parameters untouched.  With a loss or priors the summary's rmse
    comes from a launch of its own at the accepted point (robust_rmse): rc 0 and NaN -- the NaN observation is in the sum -- and
    NaN is the convention asserted here, for the plain rmse of the other two as well."""
    case = X.BY_ID["ring4-nan"]
    plain, _, _ = device(case.id, hip_device)
    q = X.build(case)
    start = params_of(q)
    nan_at = int(np.nonzero(_mask_without(q, X.nan_corner(q, case.spoil[1])) == 0.0)[0][0])
    kw, opt, loss = _spec(spec, q, nan_at)
    with api.Solver(q, hip_device, **kw) as s:
        if loss:
            s.set_loss(*loss)
        r = s.solve(**dict(X.options(case), **opt))      # (an rc other than 0 raises)
    assert_outcome(r, plain)
    assert [it["trust_region_radius"] for it in r["iterations"]] == [it["trust_region_radius"] for it in plain["iterations"]]
    assert all(it["step_norm"] == 0.0 and it["cost_change"] == 0.0 for it in r["iterations"][1:])
    assert math.isnan(r["final_cost"]) and same_bits(params_of(q), start)
    print("rmse of the failed solve:", spec, r["rmse"])
    assert math.isnan(r["rmse"])


@pytest.mark.parametrize("spec", SPECS)
def test_gradient_exit_under_tiers_and_specs(hip_device, spec):
    case = X.BY_ID["ring4-grad@3"]
    plain, _, _ = device(case.id, hip_device)
    q = X.build(case)
    start = params_of(q)
    kw, opt, loss = _spec(spec, q)
    with api.Solver(q, hip_device, **kw) as s:
        if loss:
            s.set_loss(*loss)
        if spec == "fp32":
            # the row's own problem and tolerance: the decisions of the fp64 run and its radii
            gtol = X.options(case)["gradient_tolerance"]
            r, rp = run(s, start, **dict(X.options(case), **opt))
            assert_outcome(r, plain)
            for a, b in zip(r["iterations"], plain["iterations"]):
                assert abs(a["trust_region_radius"] - b["trust_region_radius"]) <= 1e-3 * b["trust_region_radius"]
            at = case.at
        else:
            # another objective: the tolerance by the 9x rule from this objective's own tolerance-free run
            free, _ = run(s, start, **dict(X.OFF, max_num_iterations=8, **opt))
            g = [it["gradient_max_norm"] for it in free["iterations"]]
            ok = [it["step_is_successful"] for it in free["iterations"]]
            at = next(k for k in range(1, 9) if ok[k] and 9.0 * g[k] <= min(g[:k]))
            gtol = math.sqrt(g[at] * g[at - 1])
            assert gtol * X.MARGIN <= min(g[:at]) and g[at] * X.MARGIN <= gtol
            r, rp = run(s, start, **dict(X.OFF, max_num_iterations=50, gradient_tolerance=gtol, **opt))
            assert r["message"] == X.MSG_GRAD and r["termination_type"] == 0 and r["num_iterations"] == at + 1
            assert bits(r["iterations"]) == bits(free["iterations"][:at + 1])
        last = max(it["iteration"] for it in r["iterations"] if it["step_is_successful"])
        capped, cp = run(s, start, **dict(X.OFF, max_num_iterations=last, **opt))
        assert bits(capped["final_cost"]) == bits(r["final_cost"]) and same_bits(cp, rp)
        for n in (1, 4):
            again, ap = run(s, start, **dict(X.OFF, max_num_iterations=50, gradient_tolerance=gtol, check_every=n, **opt))
            assert bits(again) == bits(r) and same_bits(ap, rp), n
    assert math.isfinite(r["rmse"]) and r["rmse"] > 0.0
