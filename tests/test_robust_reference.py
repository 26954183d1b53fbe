"""The robust-loss reference (tests/robust_ref.py) and the argument checks of the loss entry points (CPU only).

1. rho, rho', rho'' of the three losses against mpmath at 50 digits (derivatives by mpmath.diff of rho), and rho'' <= 0
   everywhere: the premise under which Ceres' Corrector -- and the kernels -- drop the alpha (rank-one) term.
2. The corrected gradient sum w^2 J^T r against a central difference of sum rho / 2 over the oracle's residuals.
3. Negative control, in the style of test_gram_tolerance.py / test_step_tolerance.py: the tolerances test_gpu_robust.py
   holds the kernels to see each kernel-shaped mistake by at least MARGIN x.
4. The loss arguments are checked before any device is touched.
"""
import ctypes as C

import mpmath
import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import api, lib, synth
from tests import helpers as H
from tests import robust_ref as R
from tests.test_gpu_gram_kernels import f32_excess
from tests.test_gpu_step import TAU_B32

MARGIN = 20.0
mpmath.mp.dps = 50


def mp_rho(kind, a, s):
    a, s = mpmath.mpf(a), mpmath.mpf(s)
    b = a * a
    if kind == "huber":
        return s if s <= b else 2 * a * mpmath.sqrt(s) - b
    if kind == "soft_l1":
        return 2 * b * (mpmath.sqrt(1 + s / b) - 1)
    return b * mpmath.log(1 + s / b)


@pytest.mark.parametrize("kind", ["huber", "soft_l1", "cauchy"])
@pytest.mark.parametrize("a", [0.5, 1.0, 3.0])
def test_rho_and_derivatives_against_50_digits(kind, a):
    b = a * a
    s = np.concatenate([np.linspace(0.0, 4 * b, 41), b * np.logspace(-6, 4, 60), [b * (1 - 1e-9), b * (1 + 1e-9)]])
    r0, r1, r2 = R.rho(kind, a, s)
    assert np.all(r2 <= 0.0), kind                 # Ceres' Corrector: alpha = 0, no rank-one term
    for k, sk in enumerate(s):
        # one-sided derivatives at Huber's kink and at s = 0 (the loss is defined for s >= 0)
        # (Huber at b: the s <= b branch, as Ceres takes it, i.e. the derivatives from the left)
        if sk == 0:
            side = 1
        elif kind == "huber" and abs(sk - b) < 1e-6 * b:
            side = -1 if sk <= b else 1
        else:
            side = 0
        e0 = mp_rho(kind, a, sk)
        e1 = mpmath.diff(lambda x: mp_rho(kind, a, x), sk, 1, direction=side)
        e2 = mpmath.diff(lambda x: mp_rho(kind, a, x), sk, 2, direction=side)
        assert abs(r0[k] - float(e0)) <= 1e-14 * max(1.0, abs(float(e0))), (kind, sk)
        assert abs(r1[k] - float(e1)) <= 1e-14 * max(1.0, abs(float(e1))), (kind, sk)
        assert abs(r2[k] - float(e2)) <= 1e-12 * max(c_of(a), abs(float(e2))), (kind, sk, r2[k], float(e2))


def c_of(a):
    return 1.0 / (a * a)


@pytest.mark.parametrize("kind", ["huber", "cauchy", "soft_l1"])
def test_corrected_gradient_is_the_gradient_of_the_robust_cost(kind):
    """g = sum w^2 J^T r (the normal equations' gradient column; the oracle's J = d(residual)/dx) against d/dx of
    sum rho(|r(x)|^2) / 2 by central differences, for a few intrinsics (their jets: J_intr)."""
    p = synth.make_problem(2, 6, 31).normalised()
    a = R.median_scale(p)
    cost, res, Jc, Jb, Ji = R.robust_jets(p, kind, a)
    g = np.einsum("nki,nk->i", Ji, res)             # summed over the views of both cameras, per intrinsic
    for m in range(2):
        sel = np.repeat(p.view_camera, p.view_count) == m
        g_m = np.einsum("nki,nk->i", Ji[sel], res[sel])
        for i in (0, 2, 4, 6):
            h = 1e-6 * max(1.0, abs(p.intr[m, i]))
            cost_at = []
            for sgn in (1, -1):
                q = p.copy().normalised()
                q.intr[m, i] += sgn * h
                cost_at.append(R.robust_cost(orc.evaluate(q, jets=False)[1], kind, a))
            fd = (cost_at[0] - cost_at[1]) / (2 * h)
            assert abs(g_m[i] - fd) <= 1e-5 * max(abs(fd), 1e-3 * np.abs(g_m).max()), (kind, m, i, g_m[i], fd)
    assert np.isfinite(g).all()


def _mistakes(p, kind, a):
    """Kernel-shaped mistakes -> the jets they would produce."""
    jets = orc.evaluate(p, jets=True)
    good = R.robust_jets(p, kind, a, jets)
    out = {}
    out["rho' instead of sqrt(rho')"] = R.robust_jets(p, kind, a, jets, weight_of=lambda w, r1: r1)
    c, res, Jc, Jb, Ji = good
    s = np.sum(jets[1].reshape(-1, 2) ** 2, axis=1)
    out["cost sum rho' s / 2"] = (0.5 * float(np.sum(R.rho(kind, a, s)[1] * s)), res, Jc, Jb, Ji)
    out["unweighted r column"] = (c, jets[1], Jc, Jb, Ji)
    out["weight of the neighbouring corner"] = R.robust_jets(p, kind, a, jets, weight_of=lambda w, r1: np.roll(w, 1))
    return good, out


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_gram_tolerances_see_every_mistake(kind):
    """fp64 kernel: cost to 1e-12, blocks to 1e-11 of their largest entry; fp32 tier: TOL_F32 of the Cauchy-Schwarz bound.
    Each mistake must stand out from those by MARGIN x (the fp32 measure, the loosest, is the one checked here; the cost
    mistake shows in the cost alone)."""
    p = synth.make_problem(4, 8, 41).normalised()
    a = R.median_scale(p)
    good, bad = _mistakes(p, kind, a)
    ref = H.normal_equations_from(p, *good[1:])
    ref["cost"] = good[0]
    for name, jets in bad.items():
        o = H.normal_equations_from(p, *jets[1:])
        o["cost"] = jets[0]
        cost_err = abs(o["cost"] - ref["cost"]) / ref["cost"]
        ex = f32_excess(H.gram_errors(o, ref, p))
        assert cost_err >= MARGIN * 1e-12 or ex >= MARGIN, (name, cost_err, ex)
        print(f"[robust gram] {kind} {name}: cost {cost_err:.1e}, fp32 measure {ex:.1e} x TOL_F32")


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_step_tolerance_sees_every_mistake(kind):
    """The step of a reference built with each mistake has a backward error of >= MARGIN x TAU_B32 (the fp32 tier's, the
    loosest) in the correct system; the cost mistake shows in the relative decrease instead (checked to TAU_F there)."""
    p = synth.make_problem(3, 6, 43).normalised()
    a = R.median_scale(p)
    good, bad = _mistakes(p, kind, a)
    ref = H.reference_step(p, terms=H.step_terms(p, jets=good))
    assert ref["ok"]
    for name, jets in bad.items():
        if name.startswith("cost"):
            rd_good = good[0] / ref["model_cost_change"]
            rd_bad = jets[0] / ref["model_cost_change"]
            assert abs(rd_bad - rd_good) >= MARGIN * 1e-9 * abs(rd_good), name
            continue
        wrong = H.reference_step(p, terms=H.step_terms(p, jets=jets))
        assert wrong["ok"], name
        e = H.step_errors(p, ref, H.reference_candidate(p, wrong))
        assert e["backward"] >= MARGIN * TAU_B32, (name, e["backward"])
        print(f"[robust step] {kind} {name}: backward error {e['backward']:.1e} = {e['backward'] / TAU_B32:.0f} x TAU_B32")


def test_loss_arguments_are_checked_before_the_device():
    L = lib.lib()
    p = synth.make_problem(2, 4, 5).normalised()
    cp = lib.c_problem(p)
    o = lib.default_options(False)
    s = lib.CSummary()
    d = np.zeros(4096)
    dp = lib.dptr(d)
    valid = C.c_int(0)
    bad = [(7, 1.0), (-1, 1.0), (lib.LOSS_HUBER, 0.0), (lib.LOSS_HUBER, -1.0), (lib.LOSS_CAUCHY, float("nan")),
           (lib.LOSS_SOFT_L1, float("inf"))]
    calls = [
        lambda k, a: L.tscm_solve_robust(C.byref(cp), C.byref(o), k, a, C.byref(s)),
        lambda k, a: L.tscm_eval_normal_equations_robust(C.byref(cp), 0, C.byref(o), k, a, dp, dp, dp, dp, dp, dp),
        lambda k, a: L.tscm_eval_step_robust(C.byref(cp), 0, C.byref(o), k, a, dp, dp, dp, C.byref(valid), C.byref(s)),
        lambda k, a: L.tscm_solver_set_loss(None, k, a),
    ]
    for f in calls:
        for k, a in bad:
            assert f(k, a) == -1, (k, a)           # TSCM_E_INVALID
    if L.tscm_device_count() == 0:
        for f in calls[:3]:
            for k in (lib.LOSS_HUBER, lib.LOSS_SOFT_L1, lib.LOSS_CAUCHY):
                assert f(k, 1.0) == -2             # TSCM_E_NO_DEVICE: the arguments were fine
        with pytest.raises(lib.TscmError) as e:
            api.calibrate(p, loss=("huber", 1.0))
        assert e.value.code == -2
    with pytest.raises(ValueError):
        lib.loss_args(("tukey", 1.0))
