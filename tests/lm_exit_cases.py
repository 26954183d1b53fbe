"""How an LM solve ends and what an invalid step leaves behind: the case table of tests/test_gpu_lm_exits.py (GPU) and
tests/test_lm_exit_cases.py (the same rows on the oracle alone).  Importable without a GPU.

A row names a problem of tests/test_gpu_step.py (one per route of the reduced-camera solver), how its input is spoiled,
its options and the outcome the oracle gives: message, termination type, num_iterations and the pattern of accepted (A),
rejected (r) and invalid (x) steps.  Three constructions:

1. NAN: one observation is NaN.  Cost, gradient and model cost change are NaN, every step is invalid, the radius is divided
   by 2, 4, 8, ... (exact in binary) and the parameters must come back untouched.
2. ZERO_PIVOT: min_lm_diagonal = 0 on a rig with a camera that has no views, finite data.  The oracle's reduced system has an
   exactly zero pivot, 0 + 0, and its factorisation fails.  The zero columns are not the idle camera's, which has no columns in
   the oracle's program either: they are the skew intrinsics b and c of every camera with views, which have no Jacobian column
   (the oracle fails in the same way on ring4, ring6 and mono).  The device leaves b and c out of its systems; its control
   step (tscm_ctrl.h: lm_step, CtrlHead::inert_cols) declares the step invalid in their place.  So these rows reach the
   invalid-step bookkeeping on finite data, with a candidate that was computed and must be discarded, but not the reduced
   solvers' own failure flag.  That flag needs a pivot of the device's own system that is not > 0 on finite data: an exactly
   zero column of a camera with views.  Corner weights of 0 on all of a camera's corners would give one, but the library
   refuses a view whose weights are all 0 (tscm_spec.h: check_corner_weights; such a view goes in with view_count 0 and the
   camera then has no columns), and a tiny weight instead is the denormal pivot that is no test of flags.  No row builds it.
3. Exits with a margin (kind grad | param | func | radius, at iteration `at`).  The oracle is run once with every tolerance
   off (base_log); the tolerance under test is the geometric mean of the deciding quantity at iteration `at` and at the
   iteration before (tolerance()).  Only pairs that differ by 9x or more are used -- 3x on each side, where the device and the
   oracle agree on these quantities to 1e-6 -- and the rows' own test shows the margin by solving again with the tolerance
   times 3 and over 3: the outcome must not move.
   The deciding quantities (tscm_ctrl.h: lm_step): gradient_max_norm of an accepted iteration against gradient_tolerance;
   step_norm against parameter_tolerance * (x_norm + parameter_tolerance); |cost_change| against function_tolerance * cost
   of the point the step starts from; the radius against min_trust_region_radius.
   Radius rows start from an initial radius of 1e10 or 1e12, not the 1e8 of tests/test_gpu_trajectory.py: from 1e8 no
   problem here rejects four steps in a row, and only the fourth division in a row (by 16) drops the radius 9x below every
   earlier one.  The rows end before any step is accepted: their rejected steps have a relative decrease of -0.9 and below,
   far from min_relative_decrease = 1e-3, and the parameters must come back bit for bit.  A candidate at such a radius is a
   nearly undamped Gauss-Newton step with a forward error of kappa eps (5e-5 at radius 1e12 by tests/test_gpu_step.py), and
   the logged cost of a rejected iteration is the candidate's: a row is used only where the oracle reproduces its own log to
   a third of the 1e-5 the GPU test asks for when its sums are re-associated over four threads
   (tests/test_lm_exit_cases.py).  That keeps ring4 from 1e12 (2.8e-6) and idle_cam4 from 1e10 (1.9e-6) and leaves out
   ring2 and ring6 from 1e12 (7e-6, 6e-5), mono from 1e16 (2e-4), mixed6 from 1e10 and big12 from 1e12 (7e-2, 4e-2).
"""
import dataclasses
import functools
import math

import numpy as np

from oracle import pyoracle as orc
from tests import helpers as H
from tests import test_gpu_step as S

OFF = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0, min_trust_region_radius=0.0)
MARGIN = 3.0

MSG_MAX_ITER = "Maximum number of iterations reached."
MSG_GRAD = "Gradient tolerance reached."
MSG_RADIUS = "Minimum trust region radius reached."
MSG_PARAM = "Parameter tolerance reached."
MSG_FUNC = "Function tolerance reached."
MSG_INVALID = "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps."
# TermReason of tscm_ctrl.h by its message (the summary carries the message, not the enum)
TERM_REASONS = {"kMaxIter": MSG_MAX_ITER, "kGradTol": MSG_GRAD, "kMinRadius": MSG_RADIUS, "kParamTol": MSG_PARAM, "kFuncTol": MSG_FUNC,
                "kInvalidSteps": MSG_INVALID}
KIND_MESSAGE = {"grad": MSG_GRAD, "param": MSG_PARAM, "func": MSG_FUNC, "radius": MSG_RADIUS}
KIND_OPTION = {"grad": "gradient_tolerance", "param": "parameter_tolerance", "func": "function_tolerance", "radius": "min_trust_region_radius"}

# the routes of the issue: problem -> what its host plan must show (tests/test_lm_exit_cases.py asks the plan headers)
ROUTES = ("ring2", "ring4", "ring6", "big12", "mono", "mixed6", "idle_cam4", "many_boards4")


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    problem: str
    spoil: object            # None | ("nan", corner name) | "min_lm_diagonal=0"
    kind: str                # grad | param | func | radius (exits with a margin) | maxiter | invalid | nan-radius (options as given)
    at: int                  # exits with a margin: the iteration whose quantity decides
    given: tuple             # options as written in the table (sorted items)
    message: str
    termination_type: int
    num_iterations: int
    pattern: str

    @property
    def is_margin_exit(self):
        return self.kind in KIND_OPTION


CASES = []


def _exit(problem, kind, at, pattern, **given):
    """An exit with a margin.  grad and radius exits log the iteration that triggers them; param and func exits do not."""
    logged = at if kind in ("grad", "radius") else at - 1
    assert len(pattern) == logged
    CASES.append(Case(f"{problem}-{kind}@{at}", problem, None, kind, at, tuple(sorted(given.items())), KIND_MESSAGE[kind], 0, logged + 1, pattern))


def _row(id_, problem, spoil, kind, message, termination_type, num_iterations, pattern, **given):
    CASES.append(Case(id_, problem, spoil, kind, -1, tuple(sorted(given.items())), message, termination_type, num_iterations, pattern))


# ---- construction 3: exits with a margin, every route
_exit("ring2", "grad", 2, "AA")
_exit("ring4", "grad", 3, "AAA")
_exit("ring4", "func", 3, "AA")
_exit("ring4", "radius", 4, "rrrr", initial_trust_region_radius=1e12)
_exit("ring6", "grad", 3, "AAA")
_exit("ring6", "func", 6, "AAAAA")
_exit("big12", "grad", 2, "AA")
_exit("big12", "func", 3, "AA")
_exit("mono", "grad", 1, "A")
_exit("mono", "param", 8, "AAAAAAA")
_exit("mixed6", "grad", 1, "A")
_exit("mixed6", "func", 6, "AAAAA")
_exit("idle_cam4", "grad", 2, "AA")
_exit("idle_cam4", "param", 4, "AAA")
_exit("idle_cam4", "func", 5, "AAAA")
_exit("idle_cam4", "radius", 4, "rrrr", initial_trust_region_radius=1e10)
_exit("many_boards4", "grad", 1, "A")
# the iteration cap on healthy data, tolerances off
_row("ring4-maxiter5", "ring4", None, "maxiter", MSG_MAX_ITER, 1, 6, "AAAAA", max_num_iterations=5, **OFF)
_row("ring4-maxiter0", "ring4", None, "maxiter", MSG_MAX_ITER, 1, 1, "", max_num_iterations=0, **OFF)

# ---- construction 1: a NaN observation, default options, every route
NAN = ("nan", "view1")
for _p in ("ring2", "ring4", "ring6", "big12", "mono", "idle_cam4"):
    _row(f"{_p}-nan", _p, NAN, "invalid", MSG_INVALID, 2, 5, "xxxx")
# mixed6: once in a board of up to three cameras (k_schur_gram factors it), once in one of more than three (k_schur_factor)
_row("mixed6-nan-fast-board", "mixed6", ("nan", "fast_board"), "invalid", MSG_INVALID, 2, 5, "xxxx")
_row("mixed6-nan-slow-board", "mixed6", ("nan", "slow_board"), "invalid", MSG_INVALID, 2, 5, "xxxx")
# many_boards4: the last corner of view 79997, which the device orders last (camera-major, then by board): the last view of the
# last evaluation chunk, as the host plan says (tests/test_lm_exit_cases.py)
_row("many_boards4-nan-last-view", "many_boards4", ("nan", "view79997"), "invalid", MSG_INVALID, 2, 5, "xxxx")
# ring4 again with the NaN in the last view: on shards, a rank other than rank 0 holds it
_row("ring4-nan-last-view", "ring4", ("nan", "last_view"), "invalid", MSG_INVALID, 2, 5, "xxxx")
# ... and how the NaN problem ends under other options
_row("ring4-nan-maxiter3", "ring4", NAN, "maxiter", MSG_MAX_ITER, 1, 4, "xxx", max_num_iterations=3)
_row("ring4-nan-maxiter0", "ring4", NAN, "maxiter", MSG_MAX_ITER, 1, 1, "", max_num_iterations=0)
_row("ring4-nan-invalid2", "ring4", NAN, "invalid", MSG_INVALID, 2, 2, "x", max_num_iterations=3, max_num_consecutive_invalid_steps=2)
_row("ring4-nan-invalid1", "ring4", NAN, "invalid", MSG_INVALID, 2, 1, "", max_num_iterations=3, max_num_consecutive_invalid_steps=1)
ALL_255 = dict(max_num_iterations=255, max_num_consecutive_invalid_steps=300, function_tolerance=0.0, gradient_tolerance=0.0,
               parameter_tolerance=0.0)
_row("ring4-nan-255", "ring4", NAN, "maxiter", MSG_MAX_ITER, 1, 256, "x" * 255, min_trust_region_radius=-1.0, **ALL_255)
_row("ring6-nan-255", "ring6", NAN, "maxiter", MSG_MAX_ITER, 1, 256, "x" * 255, min_trust_region_radius=-1.0, **ALL_255)
_row("ring4-nan-minradius200", "ring4", NAN, "nan-radius", MSG_RADIUS, 0, 4, "xxx", min_trust_region_radius=200.0, **ALL_255)

# ---- construction 2: an exactly zero pivot of the reduced system, nothing non-finite
_row("idle_cam4-zero-pivot", "idle_cam4", "min_lm_diagonal=0", "invalid", MSG_INVALID, 2, 5, "xxxx", min_lm_diagonal=0.0)
_row("idle_cam6-zero-pivot", "idle_cam6", "min_lm_diagonal=0", "invalid", MSG_INVALID, 2, 5, "xxxx", min_lm_diagonal=0.0)

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
EXIT_CASES = [c for c in CASES if c.is_margin_exit]                    # part A
HEALTHY_EXIT_CASES = [c for c in CASES if c.spoil is None]             # ... with the two iteration caps on healthy data
FAILURE_CASES = [c for c in CASES if c.spoil is not None]              # part B: constructions 1 and 2


# ----------------------------------------------------------------------------- inputs
def nan_corner(p, where):
    """(array name, corner index) of the observation a NaN row spoils."""
    cnt, off = np.asarray(p.view_count), np.asarray(p.view_offset)
    if where == "view1":
        return "obs_v", int(off[1])
    if where == "last_view" or where.startswith("view"):          # the last corner of the last view, or of view <n>
        v = p.n_views - 1 if where == "last_view" else int(where[4:])
        return "obs_u", int(off[v] + cnt[v] - 1)
    cams = np.bincount(np.asarray(p.view_board)[cnt > 0], minlength=p.n_boards)
    if where == "slow_board":                   # a board seen by more than three cameras
        b = int(np.nonzero(cams > 3)[0][0])
    elif where == "fast_board":                 # ... by two or three
        b = int(np.nonzero((cams >= 2) & (cams <= 3))[0][0])
    else:
        raise KeyError(where)
    v = int(np.nonzero((np.asarray(p.view_board) == b) & (cnt > 0))[0][-1])
    return "obs_v", int(off[v] + cnt[v] // 2)


def spoiled_view(case, p):
    """The view that holds the row's NaN corner."""
    _, k = nan_corner(p, case.spoil[1])
    off = np.asarray(p.view_offset)
    return int(np.nonzero((off <= k) & (k < off + np.asarray(p.view_count)))[0][0])


def build(case):
    """A fresh, normalised copy of the row's problem with its input spoiled."""
    q = S.problem(case.problem).copy().normalised()
    if isinstance(case.spoil, tuple):
        name, k = nan_corner(q, case.spoil[1])
        getattr(q, name)[k] = np.nan
    return q


# ----------------------------------------------------------------------------- tolerances of construction 3
def pattern(s):
    return "".join("A" if it["step_is_successful"] else ("r" if it["step_is_valid"] else "x") for it in s["iterations"][1:])


@functools.lru_cache(maxsize=None)
def base_log(problem, given, n):
    """The oracle's log of n iterations with every tolerance off."""
    q = S.problem(problem).copy().normalised()
    s = orc.solve(q, **dict(dict(given), max_num_iterations=n, **OFF))
    assert s["num_iterations"] == n + 1, s["message"]
    return s


def x_norm(p):
    """|x| over the free blocks (the oracle's prog_norm_diff: a camera's pose and its nine intrinsics, a board's pose)."""
    cols = H.step_columns(p)
    pose, intr, board = cols["cam_free"][:, 0], cols["cam_free"][:, 6], cols["board_free"]
    return math.sqrt(float((p.cam_rt[pose] ** 2).sum() + (p.intr[intr] ** 2).sum() + (p.board_rt[board] ** 2).sum()))


def deciding_quantities(case):
    """The quantity the row's exit test compares with its tolerance, per iteration 0 .. at of the tolerance-free run (None where
    the test is not made): the test reads `quantity <= tolerance`, for param `<= tolerance * (x_norm + tolerance)`."""
    its = base_log(case.problem, case.given, case.at)["iterations"]
    if case.kind == "grad":
        return [it["gradient_max_norm"] if it["step_is_successful"] else None for it in its]
    if case.kind == "radius":
        return [it["trust_region_radius"] for it in its]
    if case.kind == "param":
        return [None] + [it["step_norm"] for it in its[1:]]
    q, x_cost = [None], its[0]["cost"]
    for it in its[1:]:
        q.append(abs(it["cost_change"]) / x_cost)
        if it["step_is_successful"]:
            x_cost = it["cost"]
    return q


def tolerance(case):
    """The geometric mean of the deciding quantity at the exit iteration and at the iteration before; for a parameter
    tolerance t, that mean is t * (x_norm + t) at the point the deciding step starts from."""
    q = deciding_quantities(case)
    at = case.at
    before = next(q[k] for k in range(at - 1, -1, -1) if q[k] is not None)
    target = math.sqrt(q[at] * before)
    if case.kind != "param":
        return target
    p = S.problem(case.problem).copy().normalised()
    orc.solve(p, **dict(dict(case.given), max_num_iterations=at - 1, **OFF))
    xn = x_norm(p)
    return 2.0 * target / (xn + math.sqrt(xn * xn + 4.0 * target))          # the positive root of t^2 + xn t - target


def options(case, scale=1.0):
    """The options of a row's solve.  scale: the tolerance under test times this (the margin check of construction 3)."""
    if not case.is_margin_exit:
        return dict(case.given)
    return dict(dict(OFF, max_num_iterations=50, **dict(case.given)), **{KIND_OPTION[case.kind]: scale * tolerance(case)})


@functools.lru_cache(maxsize=None)
def oracle(case_id):
    """(summary, the problem as the oracle left it) of a row; computed once, not to be changed."""
    case = BY_ID[case_id]
    q = build(case)
    return orc.solve(q, **options(case)), q


def outcome(s):
    return dict(message=s["message"], termination_type=s["termination_type"], num_iterations=s["num_iterations"], pattern=pattern(s))


def expected(case):
    return dict(message=case.message, termination_type=case.termination_type, num_iterations=case.num_iterations, pattern=case.pattern)


# ----------------------------------------------------------------------------- the batched mono route (part F of the GPU tests)
def batch_problems():
    """Slots 0, 2, 4: mono problems far from their solution; slot 1: another one, which batch_with_nan spoils; slot 3: one that
    starts at its solution, whose first step is already below the shared parameter tolerance."""
    from tscm_calib_amd import synth
    far = [synth.make_problem(1, 20, seed, noise_px=0.1) for seed in (601, 603, 602, 604)]
    quick = synth.make_problem(1, 20, 431, noise_px=0.01, perturb=False)
    return [far[0], far[1], far[2], quick, far[3]]


def batch_options():
    """max_num_iterations 3 and a parameter tolerance t with t (|x| + t) = 1: the first step of slot 3 is 0.23, the steps of
    the other slots are 4.6 and more in their three iterations (tests/test_lm_exit_cases.py shows both on the oracle, at 3 t and
    t / 3).  Three invalid steps in a row are a failure, so the NaN slot fails after two logged ones, inside the iteration cap."""
    xn = x_norm(batch_problems()[3].copy().normalised())
    t = 2.0 / (xn + math.sqrt(xn * xn + 4.0))
    return dict(max_num_iterations=3, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=t, max_num_consecutive_invalid_steps=3)


def batch_with_nan(ps):
    bad = [p.copy().normalised() for p in ps]
    bad[1].obs_v[bad[1].view_offset[1]] = np.nan
    return bad
