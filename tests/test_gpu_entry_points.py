"""Every spelling of an entry-point family is the family's most general export (tscm.h, "Refusal order"): called with
TSCM_LOSS_NONE and NULLs where a legacy export has no argument, tscm_solve_weighted, tscm_eval_step_weighted,
tscm_eval_normal_equations_weighted, tscm_solve_mono_batch_weighted and tscm_covariance_weighted give, byte for byte, the
parameters, the iteration log and the outputs of their siblings -- and a single fault is refused with the same code and text
through every sibling.  The Python API calls the general exports only; this is what keeps the others covered."""
import ctypes as C

import numpy as np
import pytest

from tscm_calib_amd import lib, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

HUBER = (lib.LOSS_HUBER, 1.0)
NONE = (lib.LOSS_NONE, 0.0)
LOG_FIELDS = ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost",
              "n_residual_blocks", "lm_iterations", "iterations", "message", "rmse")


def _rig():
    return H.small_rig(2, 3).normalised()


def _mono():
    return synth.make_problem(1, 3, 7).normalised()


def _masks(p):
    m = np.zeros(p.n_cameras, np.uint16)
    m[0] = lib.FIX["cx"] | lib.FIX["cy"]
    return m


def _solved(p, call):
    """call(P, O, S) on a copy of p -> (rc, text, parameters as bytes, the summary but for its times)"""
    q = p.copy().normalised()
    cp, o, s = lib.c_problem(q), lib.default_options(bool(p.mono)), lib.CSummary()
    rc = call(C.byref(cp), C.byref(o), C.byref(s))
    d = lib.summary_dict(s)
    return rc, lib.lib().tscm_last_error().decode() if rc else "", (q.cam_rt.tobytes(), q.intr.tobytes(), q.board_rt.tobytes()), {k: d[k] for k in LOG_FIELDS}


def _same(a, b):
    assert a[0] == 0 and b[0] == 0, (a[:2], b[:2])
    assert a[2] == b[2], "parameters differ"
    assert a[3] == b[3], "summaries differ"
    assert a[3]["num_iterations"] > 1


def test_solves(hip_device):
    L = lib.lib()
    rig, mono = _rig(), _mono()
    for p, plain in ((rig, L.tscm_solve_multi), (mono, L.tscm_solve_mono)):
        m = lib.ushort_ptr(_masks(p))
        _same(_solved(p, lambda P, O, S: plain(P, O, S)), _solved(p, lambda P, O, S: L.tscm_solve_weighted(P, O, None, None, *NONE, S)))
        _same(_solved(p, lambda P, O, S: L.tscm_solve_robust(P, O, *HUBER, S)), _solved(p, lambda P, O, S: L.tscm_solve_weighted(P, O, None, None, *HUBER, S)))
        for loss in (NONE, HUBER):
            _same(_solved(p, lambda P, O, S: L.tscm_solve_fixed(P, O, m, *loss, S)), _solved(p, lambda P, O, S: L.tscm_solve_weighted(P, O, None, m, *loss, S)))


def _stepped(p, call):
    cam, intr, board = np.zeros_like(p.cam_rt), np.zeros_like(p.intr), np.zeros_like(p.board_rt)
    valid, s = C.c_int(-1), lib.CSummary()
    cp, o = lib.c_problem(p), lib.default_options(bool(p.mono))
    rc = call(C.byref(cp), C.byref(o), lib.dptr(cam), lib.dptr(intr), lib.dptr(board), C.byref(valid), C.byref(s))
    d = lib.summary_dict(s)
    return rc, lib.lib().tscm_last_error().decode() if rc else "", (cam.tobytes(), intr.tobytes(), board.tobytes(), valid.value), {k: d[k] for k in LOG_FIELDS}


def test_steps(hip_device):
    L, dv = lib.lib(), hip_device
    for p in (_rig(), _mono()):
        m = lib.ushort_ptr(_masks(p))
        _same(_stepped(p, lambda P, O, *out: L.tscm_eval_step_ex(P, dv, O, *out)), _stepped(p, lambda P, O, *out: L.tscm_eval_step_weighted(P, dv, O, None, None, *NONE, *out)))
        _same(_stepped(p, lambda P, O, *out: L.tscm_eval_step_robust(P, dv, O, *HUBER, *out)), _stepped(p, lambda P, O, *out: L.tscm_eval_step_weighted(P, dv, O, None, None, *HUBER, *out)))
        _same(_stepped(p, lambda P, O, *out: L.tscm_eval_step_fixed(P, dv, O, m, *HUBER, *out)), _stepped(p, lambda P, O, *out: L.tscm_eval_step_weighted(P, dv, O, None, m, *HUBER, *out)))


def _blocks(p, call):
    Cn, B, V = p.n_cameras, p.n_boards, p.n_views
    out = [np.full(n, np.nan) for n in (B * 36, B * 6, V * 90, Cn * 225, Cn * 15)]
    cost = C.c_double(np.nan)
    cp, o = lib.c_problem(p), lib.default_options(bool(p.mono))
    rc = call(C.byref(cp), C.byref(o), *[lib.dptr(x) for x in out], C.byref(cost))
    return rc, lib.lib().tscm_last_error().decode() if rc else "", tuple(x.tobytes() for x in out) + (cost.value,)


def test_normal_equations(hip_device):
    L, dv = lib.lib(), hip_device
    for p in (_rig(), _mono()):
        general = _blocks(p, lambda P, O, *out: L.tscm_eval_normal_equations_weighted(P, dv, O, None, *NONE, *out))
        assert general[0] == 0 and np.isfinite(general[2][-1]) and general[2][-1] > 0.0
        for call in (lambda P, O, *out: L.tscm_eval_normal_equations(P, dv, *out), lambda P, O, *out: L.tscm_eval_normal_equations_ex(P, dv, O, *out),
                     lambda P, O, *out: L.tscm_eval_normal_equations_robust(P, dv, O, *NONE, *out)):
            assert _blocks(p, call) == general
        assert _blocks(p, lambda P, O, *out: L.tscm_eval_normal_equations_robust(P, dv, O, *HUBER, *out)) == \
            _blocks(p, lambda P, O, *out: L.tscm_eval_normal_equations_weighted(P, dv, O, None, *HUBER, *out))


def _batch(ps, call):
    qs = [p.copy().normalised() for p in ps]
    n = len(qs)
    cps, sums, o = (lib.CProblem * n)(*[lib.c_problem(q) for q in qs]), (lib.CSummary * n)(), lib.default_options(True)
    m = np.array([0, lib.FIX["cx"], 0][:n], np.uint16)
    rc = call(cps, n, C.byref(o), lib.ushort_ptr(m), sums)
    ds = [lib.summary_dict(s) for s in sums]
    return rc, lib.lib().tscm_last_error().decode() if rc else "", tuple((q.intr.tobytes(), q.board_rt.tobytes()) for q in qs), [{k: d[k] for k in LOG_FIELDS} for d in ds]


def test_mono_batch(hip_device):
    L, dv = lib.lib(), hip_device
    ps = [synth.make_problem(1, 3, 7 + i).normalised() for i in range(3)]
    dp = C.POINTER(C.c_double)
    nulls = (dp * 3)(dp(), dp(), dp())
    for loss in (NONE, HUBER):
        legacy = _batch(ps, lambda cps, n, O, m, sums: L.tscm_solve_mono_batch(cps, n, dv, O, m, *loss, sums))
        assert legacy[0] == 0 and all(s["num_iterations"] > 1 for s in legacy[3])
        assert _batch(ps, lambda cps, n, O, m, sums: L.tscm_solve_mono_batch_weighted(cps, n, dv, O, m, None, *loss, sums)) == legacy
        assert _batch(ps, lambda cps, n, O, m, sums: L.tscm_solve_mono_batch_weighted(cps, n, dv, O, m, nulls, *loss, sums)) == legacy


def _cov(p, call):
    Cn, B = p.n_cameras, p.n_boards
    out = [np.full(n, np.nan) for n in ((Cn * 15) ** 2, B * 36, Cn * 6, Cn * 9, B * 6)]
    info = lib.CCovarianceInfo(struct_size=C.sizeof(lib.CCovarianceInfo))
    cp = lib.c_problem(p)
    rc = call(C.byref(cp), lib.ushort_ptr(_masks(p)), *[lib.dptr(x) for x in out], C.byref(info))
    return rc, lib.lib().tscm_last_error().decode() if rc else "", tuple(x.tobytes() for x in out), (info.status, info.where, info.n_free, info.n_residuals, info.cost, info.sigma2, info.min_pivot_ratio)


def test_covariance(hip_device):
    L, dv = lib.lib(), hip_device
    p = _rig()
    p.cam_pose_constant[0] = 1          # (no gauge freedom: the reduced system is regular)
    for loss in (NONE, HUBER):
        legacy = _cov(p, lambda P, m, *out: L.tscm_covariance(P, dv, m, *loss, *out))
        assert legacy[0] == 0 and legacy[3][0] == 0 and legacy[3][5] > 0.0
        assert _cov(p, lambda P, m, *out: L.tscm_covariance_weighted(P, dv, m, None, *loss, *out)) == legacy


def test_a_single_fault_reads_the_same_through_every_sibling(hip_device):
    L, dv = lib.lib(), hip_device
    rig, mono = _rig(), _mono()
    bad_flags = 1 << 20
    text = "unknown bits in tscm_options.exec_flags (an options struct of an older ABI?)"

    def with_bad_flags(f):
        def call(P, O, *rest):
            O._obj.exec_flags = bad_flags
            return f(P, O, *rest)
        return call

    for p, plain in ((rig, L.tscm_solve_multi), (mono, L.tscm_solve_mono)):
        m = lib.ushort_ptr(_masks(p))
        answers = [_solved(p, with_bad_flags(f))[:2] for f in (
            lambda P, O, S: plain(P, O, S), lambda P, O, S: L.tscm_solve_robust(P, O, *HUBER, S), lambda P, O, S: L.tscm_solve_fixed(P, O, m, *NONE, S),
            lambda P, O, S: L.tscm_solve_weighted(P, O, None, None, *NONE, S))]
        assert answers == [(-1, text)] * 4, answers
        answers = [_stepped(p, with_bad_flags(f))[:2] for f in (
            lambda P, O, *out: L.tscm_eval_step_ex(P, dv, O, *out), lambda P, O, *out: L.tscm_eval_step_robust(P, dv, O, *HUBER, *out),
            lambda P, O, *out: L.tscm_eval_step_fixed(P, dv, O, m, *NONE, *out), lambda P, O, *out: L.tscm_eval_step_weighted(P, dv, O, None, None, *NONE, *out))]
        assert answers == [(-1, text)] * 4, answers
        answers = [_blocks(p, with_bad_flags(f))[:2] for f in (
            lambda P, O, *out: L.tscm_eval_normal_equations_ex(P, dv, O, *out), lambda P, O, *out: L.tscm_eval_normal_equations_robust(P, dv, O, *HUBER, *out),
            lambda P, O, *out: L.tscm_eval_normal_equations_weighted(P, dv, O, None, *NONE, *out))]
        assert answers == [(-1, text)] * 3, answers
    # a loss of an unknown kind, through the batch's and the covariance's pair
    ps = [mono]
    answers = [_batch(ps, f)[:2] for f in (lambda cps, n, O, m, sums: L.tscm_solve_mono_batch(cps, n, dv, O, m, 7, 1.0, sums),
                                           lambda cps, n, O, m, sums: L.tscm_solve_mono_batch_weighted(cps, n, dv, O, m, None, 7, 1.0, sums))]
    assert answers == [(-1, "unknown loss kind")] * 2, answers
    answers = [_cov(rig, f)[:2] for f in (lambda P, m, *out: L.tscm_covariance(P, dv, m, 7, 1.0, *out),
                                          lambda P, m, *out: L.tscm_covariance_weighted(P, dv, m, None, 7, 1.0, *out))]
    assert answers == [(-1, "loss_kind 7 is not a TSCM_LOSS_* kind")] * 2, answers
